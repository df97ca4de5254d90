// Mixed-size uint8 frames in, with an antialiased downscale: prpe_frame_ingest
// (csrc/ingest.hip) for a batch whose frames each have their own size, strides and region, and with
// torch's triangle filter on every axis that shrinks.
//
// prpe_frame_ingest_multi — a HOST table of B frames -> the interior [B, H, W, 4] of the stem's
//   buffer. The table travels in the kernel arguments, at most 32 frames (1.8 KB) per launch; there
//   is no upload and no workspace. One kernel serves both filters and both kinds of axis:
//     two-tap axis (filter 0, or scale <= 1): prpe_frame_ingest's coordinates, weight and lerp;
//     antialias axis (filter 1, scale > 1):   a window of up to 2 * scale + 1 normalised weights.
//   One 128-thread workgroup per (frame, 8 output rows, 128 output columns), one output column per
//   thread. The weights are formed once per workgroup, in fp64, rounded to fp32 and kept in LDS:
//   each thread its own column's ([tap][thread], conflict-free), threads 0..7 the rows' (read as a
//   broadcast). The workgroup then walks the source rows its 8 output rows need, in ascending order
//   and each row ONCE: a thread forms the row's horizontal value h for its column (3 channels) and
//   adds w_y * (h - h_first) into the accumulators of the at most three output rows whose windows
//   hold that row (h_first: the h of the output row's first source row; include/prpe.h) -- so the vertical overlap of the windows costs registers, not source reads; only the rows
//   shared by two strips are read twice ((8 + 1) / 8). Horizontally a source byte is wanted by two
//   neighbouring lanes of the same wave: those are single-byte loads of the same cache lines, as in
//   prpe_frame_ingest, and wider loads would again need an alignment the strided source does not
//   promise. The order of every sum is fixed by the output pixel alone (taps ascending, rows
//   ascending), so a frame's bytes do not depend on B, its index, its chunk or its neighbours.
// Products, then adds, never an fma: contraction is off for the whole file.
#pragma clang fp contract(off)
#include "common.h"

namespace {

constexpr int IM_THREADS = 128;                 // output columns per workgroup, one per thread
constexpr int IM_ROWS = 8;                      // output rows per workgroup
constexpr int IM_CHUNK = 32;                    // frames per launch
constexpr int IM_MAX_SCALE = 32;
constexpr int IM_MAX_TAPS = 2 * IM_MAX_SCALE + 2;
constexpr int MAX_DIM = 1 << 24;

struct MultiK {
  prpe_ingest_src s[IM_CHUNK];
  float* y; int H, W; int64_t ysn, ysh, ysw;   // float elements, each a multiple of 4
  float a[3], b[3], fill[3];
  int swap_rb, filter;
  int tx, ty;                                   // LDS taps per column / per row (0: no such axis in this launch)
  float* y_amax;
};

// the window of output index o on an antialias axis: source indices [lo, lo + n)
__device__ __forceinline__ void aa_window(double scale, int o, int size, int cap, double& centre, int& lo, int& n) {
  centre = scale * ((double)o + 0.5);
  long long a = (long long)(centre - scale + 0.5), b = (long long)(centre + scale + 0.5);
  a = a > 0 ? a : 0;
  b = b < size ? b : size;
  lo = (int)a;
  n = (int)(b - a) < cap ? (int)(b - a) : cap;  // cap >= every window (the host sizes it); keeps LDS in bounds
}

// w[k * stride] = (float)(t_k / sum t), t_k = max(0, 1 - |(lo + k - centre + 0.5) * (1 / scale)|)
__device__ __forceinline__ void aa_weights(double scale, double centre, int lo, int n, float* w, int stride) {
  const double inv = 1.0 / scale;
  double sum = 0.0;
  for (int k = 0; k < n; ++k) {
    const double x = fabs(((double)(lo + k) - centre + 0.5) * inv);
    sum += x < 1.0 ? 1.0 - x : 0.0;
  }
  for (int k = 0; k < n; ++k) {
    const double x = fabs(((double)(lo + k) - centre + 0.5) * inv);
    w[(int64_t)k * stride] = (float)((x < 1.0 ? 1.0 - x : 0.0) / sum);
  }
}

// prpe_frame_ingest's tap pair of output index o: a, b (b == a only where the weight is 0)
__device__ __forceinline__ void two_tap(double scale, int o, int size, int& a, int& b, float& frac) {
  // clamped into the source before the conversion to int: in bounds for any argument
  const double s = fmin(fmax(((double)o + 0.5) * scale - 0.5, 0.0), (double)(size - 1));
  const double f = floor(s);
  frac = (float)(s - f);
  a = (int)f;
  b = a + 1 < size ? a + 1 : a;
}

__global__ __launch_bounds__(IM_THREADS, 3) void frame_ingest_multi_kernel(MultiK p) {
  extern __shared__ float lds[];                // wx [tx][IM_THREADS], wy [IM_ROWS][ty], wmax [IM_THREADS / 64]
  float* wx = lds + threadIdx.x;
  float* wy = lds + p.tx * IM_THREADS;
  float* wmax = wy + IM_ROWS * p.ty;
  const int ctiles = (p.W + IM_THREADS - 1) / IM_THREADS;
  const int bpf = ctiles * ((p.H + IM_ROWS - 1) / IM_ROWS);     // workgroups per frame
  const int n = blockIdx.x / bpf, rem = blockIdx.x - n * bpf;
  const int i0 = (rem / ctiles) * IM_ROWS, j = (rem % ctiles) * IM_THREADS + threadIdx.x;
  const uint8_t* base = p.s[n].ptr;
  const int Hs = p.s[n].h, Ws = p.s[n].w, top = p.s[n].top, left = p.s[n].left, nh = p.s[n].nh, nw = p.s[n].nw;
  const int64_t ssh = p.s[n].sh, ssw = p.s[n].sw, ssc = p.s[n].sc;
  const bool aax = p.filter && Ws > nw, aay = p.filter && Hs > nh;
  const double kx = (double)Ws / (double)nw, ky = (double)Hs / (double)nh;
  int64_t oc[3];
  float fv[3];
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    oc[c] = (int64_t)(p.swap_rb ? 2 - c : c) * ssc;
    fv[c] = p.fill[c] * p.a[c] + p.b[c];
  }
  const float fmx = fmaxf(fmaxf(fabsf(fv[0]), fabsf(fv[1])), fabsf(fv[2]));

  // this thread's column
  const bool col_in = j < p.W && (unsigned)(j - left) < (unsigned)nw;
  int xa = 0, xb = 0, nx = 0;
  float ax = 0.f;
  if (col_in) {
    if (aax) {
      double centre;
      aa_window(kx, j - left, Ws, p.tx, centre, xa, nx);
      aa_weights(kx, centre, xa, nx, wx, IM_THREADS);
    } else {
      two_tap(kx, j - left, Ws, xa, xb, ax);
    }
  }
  // the strip's rows: source rows [ylo, yhi) each (two-tap: ya and, where it differs, yb)
  int ylo[IM_ROWS], yhi[IM_ROWS];
  float ay[IM_ROWS];
  int rlo = MAX_DIM, rhi = 0;
#pragma unroll
  for (int d = 0; d < IM_ROWS; ++d) {
    const int i = i0 + d;
    ylo[d] = yhi[d] = 0;
    ay[d] = 0.f;
    if (i < p.H && (unsigned)(i - top) < (unsigned)nh) {
      if (aay) {
        double centre;
        int cnt;
        aa_window(ky, i - top, Hs, p.ty, centre, ylo[d], cnt);
        yhi[d] = ylo[d] + cnt;
        if (threadIdx.x == d) aa_weights(ky, centre, ylo[d], cnt, wy + d * p.ty, 1);
      } else {
        int yb;
        two_tap(ky, i - top, Hs, ylo[d], yb, ay[d]);
        yhi[d] = yb + 1;
      }
      rlo = ylo[d] < rlo ? ylo[d] : rlo;
      rhi = yhi[d] > rhi ? yhi[d] : rhi;
    }
  }
  __syncthreads();

  // Every weighted sum is taken as the first tap plus the weighted DIFFERENCES from it, the form of
  // prpe_frame_ingest's lerp v0 + ax * (v1 - v0) carried to n taps: a constant window gives the
  // constant exactly, whatever the fp32 weights sum to.
  float ref[IM_ROWS][3], acc[IM_ROWS][3];        // per output row: h of its first source row, sum of w * (h - ref)
#pragma unroll
  for (int d = 0; d < IM_ROWS; ++d)
#pragma unroll
    for (int c = 0; c < 3; ++c) ref[d][c] = acc[d][c] = 0.f;
  for (int r = rlo; r < rhi; ++r) {
    bool used = false;
#pragma unroll
    for (int d = 0; d < IM_ROWS; ++d) used |= r >= ylo[d] && r < yhi[d];
    if (!used || !col_in) continue;              // a row between two-tap pairs; a column outside the region
    const uint8_t* row = base + (int64_t)r * ssh;
    float h[3];
    if (aax) {
      const uint8_t* px = row + (int64_t)xa * ssw;
      float v0[3], s[3];
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        v0[c] = (float)px[oc[c]];
        s[c] = 0.f;
      }
      px += ssw;
      for (int k = 1; k < nx; ++k, px += ssw) {
        const float w = wx[k * IM_THREADS];
#pragma unroll
        for (int c = 0; c < 3; ++c) s[c] = s[c] + w * ((float)px[oc[c]] - v0[c]);
      }
#pragma unroll
      for (int c = 0; c < 3; ++c) h[c] = v0[c] + s[c];
    } else {
      const uint8_t* pa = row + (int64_t)xa * ssw;
      const uint8_t* pb = row + (int64_t)xb * ssw;
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        const float v0 = (float)pa[oc[c]], v1 = (float)pb[oc[c]];
        h[c] = v0 + ax * (v1 - v0);
      }
    }
#pragma unroll
    for (int d = 0; d < IM_ROWS; ++d) {
      if (r >= ylo[d] && r < yhi[d]) {
        if (r == ylo[d]) {
#pragma unroll
          for (int c = 0; c < 3; ++c) ref[d][c] = h[c];
        } else {                                 // two-tap: the one term ay * (u - t), added to 0.f
          const float w = aay ? wy[d * p.ty + (r - ylo[d])] : ay[d];
#pragma unroll
          for (int c = 0; c < 3; ++c) acc[d][c] = acc[d][c] + w * (h[c] - ref[d][c]);
        }
      }
    }
  }

  float m = 0.f;
  if (j < p.W) {
    float* yo = p.y + (int64_t)n * p.ysn + (int64_t)i0 * p.ysh + (int64_t)j * p.ysw;
#pragma unroll
    for (int d = 0; d < IM_ROWS; ++d) {
      if (i0 + d >= p.H) break;
      f32x4 o = {fv[0], fv[1], fv[2], 0.f};
      float om = fmx;
      if (col_in && yhi[d] > ylo[d]) {
        om = 0.f;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
          const float v = (ref[d][c] + acc[d][c]) * p.a[c] + p.b[c];
          o[c] = v;
          om = fmaxf(om, fabsf(v));
        }
      }
      m = fmaxf(m, om);
      *reinterpret_cast<f32x4*>(yo + (int64_t)d * p.ysh) = o;
    }
  }
  if (!p.y_amax) return;
  m = warp_max(m);
  if ((threadIdx.x & 63) == 0) wmax[threadIdx.x >> 6] = m;
  __syncthreads();
  if (threadIdx.x == 0) {
    m = fmaxf(wmax[0], wmax[1]);
    if (m > 0.f) atomicMax(reinterpret_cast<unsigned*>(p.y_amax + n), __float_as_uint(m));
  }
}

bool src_ok(const prpe_ingest_src& s, const prpe_view* y, int filter) {
  if (!s.ptr || s.h < 1 || s.w < 1 || s.h > MAX_DIM || s.w > MAX_DIM) return false;
  if (s.nh < 1 || s.nw < 1 || s.top < 0 || s.left < 0 || (int64_t)s.top + s.nh > y->h ||
      (int64_t)s.left + s.nw > y->w)
    return false;
  if (filter && ((int64_t)s.h > (int64_t)IM_MAX_SCALE * s.nh || (int64_t)s.w > (int64_t)IM_MAX_SCALE * s.nw))
    return false;
  return true;
}

// LDS taps that hold every window of an antialias axis: a window spans at most 2 * scale + 1 indices
int taps_for(int size, int nout) {
  if (size <= nout) return 0;
  const int t = (int)((2LL * size + nout - 1) / nout) + 2;
  return t < IM_MAX_TAPS ? t : IM_MAX_TAPS;
}

}  // namespace

extern "C" int prpe_frame_ingest_multi(const prpe_ingest_src* srcs, int32_t B, const prpe_view* y, int32_t filter,
                                       const float* a, const float* b, const float* fill, int32_t swap_rb,
                                       float* y_amax, void* stream) {
  if (!srcs || B < 1 || !view_ok(y) || !a || !b || !fill) return PRPE_EINVAL;
  if (B != y->n || (filter != 0 && filter != 1)) return PRPE_EINVAL;
  if (y->c != 4 || y->sc != 1 || y->sw % 4 || y->sh % 4 || y->sn % 4 || (uintptr_t)y->ptr % 16) return PRPE_EINVAL;
  const int64_t bpf = (int64_t)((y->w + IM_THREADS - 1) / IM_THREADS) * ((y->h + IM_ROWS - 1) / IM_ROWS);
  if (bpf * IM_CHUNK >= (1LL << 31)) return PRPE_EINVAL;
  for (int n = 0; n < B; ++n)
    if (!src_ok(srcs[n], y, filter)) return PRPE_EINVAL;
  for (int c0 = 0; c0 < B; c0 += IM_CHUNK) {
    const int nc = B - c0 < IM_CHUNK ? B - c0 : IM_CHUNK;
    MultiK p{};
    for (int n = 0; n < nc; ++n) {
      p.s[n] = srcs[c0 + n];
      if (filter) {
        const int tx = taps_for(p.s[n].w, p.s[n].nw), ty = taps_for(p.s[n].h, p.s[n].nh);
        p.tx = tx > p.tx ? tx : p.tx;
        p.ty = ty > p.ty ? ty : p.ty;
      }
    }
    p.y = y->ptr + (int64_t)c0 * y->sn; p.H = y->h; p.W = y->w; p.ysn = y->sn; p.ysh = y->sh; p.ysw = y->sw;
    for (int c = 0; c < 3; ++c) { p.a[c] = a[c]; p.b[c] = b[c]; p.fill[c] = fill[c]; }
    p.swap_rb = swap_rb ? 1 : 0;
    p.filter = filter;
    p.y_amax = y_amax ? y_amax + c0 : nullptr;
    const size_t lds = sizeof(float) * ((size_t)p.tx * IM_THREADS + (size_t)IM_ROWS * p.ty + IM_THREADS / 64);
    hipLaunchKernelGGL(frame_ingest_multi_kernel, dim3((unsigned)(bpf * nc)), dim3(IM_THREADS), lds,
                       as_stream(stream), p);
    const int st = launch_status();
    if (st) return st;
  }
  return 0;
}
