// uint8 frames in, model-ready fp32 out: the stage in front of the first conv.
//
// prpe_frame_ingest   — source uint8 [B, Hs, Ws, 3] at any element strides (HWC batches, NCHW
//   through permute, slices) -> the interior [B, H, W, 4] of the stem's zero-bordered NHWC4
//   buffer: bilinear resize into the region (top, left, nh, nw), fill outside it, per-channel
//   affine, channel 3 = 0, one 16-B store per pixel, the border never addressed. One 256-thread
//   workgroup per (frame, 8 output rows); a thread walks the columns tid, tid + 256, ..., so its
//   source column and x weight are formed once per column and the row coordinate is wave-uniform.
//   Per-frame max|y|: reduced over the workgroup, ONE atomicMax per workgroup (a workgroup never
//   spans two frames; copy_pad_kernel's scheme, csrc/pointwise.hip).
// prpe_crop_resize_u8 — prpe_crop_resize (csrc/topdown.hip) reading uint8 frames: the same launch
//   shape, window arithmetic, clamp and zero taps, written out a second time here so that the fp32
//   kernel stays as it is (tests/test_gpu_ingest.py holds the two to the same bits), then the
//   per-channel affine on every pixel of a filled slot.
//
// Loads: a pixel's taps are single bytes (12 per pixel: 4 taps x 3 channels). Neighbouring lanes
// read neighbouring bytes of the same cache lines, every source byte is fetched from HBM once,
// and the kernel's traffic is the 16 B it stores per pixel against at most 3 B it reads; wider
// loads would need an alignment the strided source does not promise (§5c has the timings).
// Coordinates in fp64, weights rounded to fp32 once, two fp32 lerps v00 + ax (v01 - v00), then
// raw * a + b as a multiply and an add: contraction is off for the whole file.
#pragma clang fp contract(off)
#include "common.h"

namespace {

constexpr int ING_THREADS = 256;
constexpr int ING_ROWS = 8;                    // output rows per workgroup
constexpr int CROP_H = 256, CROP_W = 192;      // as csrc/topdown.hip: the ViTPose input
constexpr int CROP_PAD = 2;
constexpr int BUF_H = CROP_H + 2 * CROP_PAD, BUF_W = CROP_W + 2 * CROP_PAD;
constexpr int CR_ROWS = 8;
constexpr int MAX_DIM = 1 << 24;

struct U8Frames { const uint8_t* ptr; int B, H, W; int64_t sn, sh, sw, sc; };

struct IngK {
  U8Frames s;
  float* y; int H, W; int64_t ysn, ysh, ysw;   // float elements, each a multiple of 4
  int top, left, nh, nw;
  float a[3], b[3], fill[3];
  int swap_rb;
  float* y_amax;
};

__global__ __launch_bounds__(ING_THREADS) void frame_ingest_kernel(IngK p) {
  __shared__ float wmax[ING_THREADS / 64];
  const int bpf = (p.H + ING_ROWS - 1) / ING_ROWS;              // workgroups per frame
  const int n = blockIdx.x / bpf, i0 = (blockIdx.x - n * bpf) * ING_ROWS;
  const int rows = p.H - i0 < ING_ROWS ? p.H - i0 : ING_ROWS;
  const uint8_t* base = p.s.ptr + (int64_t)n * p.s.sn;
  float* ybase = p.y + (int64_t)n * p.ysn + (int64_t)i0 * p.ysh;
  const double kx = (double)p.s.W / (double)p.nw, ky = (double)p.s.H / (double)p.nh;
  const double xmax = (double)(p.s.W - 1), ymax = (double)(p.s.H - 1);
  int64_t oc[3];
  float fv[3];
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    oc[c] = (int64_t)(p.swap_rb ? 2 - c : c) * p.s.sc;
    fv[c] = p.fill[c] * p.a[c] + p.b[c];
  }
  const float fmx = fmaxf(fmaxf(fabsf(fv[0]), fabsf(fv[1])), fabsf(fv[2]));
  float m = 0.f;
  for (int j = threadIdx.x; j < p.W; j += ING_THREADS) {
    const bool col_in = (unsigned)(j - p.left) < (unsigned)p.nw;
    // clamped into the source before the conversion to int: in bounds for any argument
    const double sx = fmin(fmax(((double)(j - p.left) + 0.5) * kx - 0.5, 0.0), xmax);
    const double fx = floor(sx);
    const float ax = (float)(sx - fx);
    const int xa = (int)fx, xb = xa + 1 < p.s.W ? xa + 1 : xa;  // xb == xa only where ax == 0
    const int64_t oa = (int64_t)xa * p.s.sw, ob = (int64_t)xb * p.s.sw;
    float* yo = ybase + (int64_t)j * p.ysw;
    for (int r = 0; r < rows; ++r) {
      const int i = i0 + r;
      f32x4 o = {fv[0], fv[1], fv[2], 0.f};
      float om = fmx;
      if (col_in && (unsigned)(i - p.top) < (unsigned)p.nh) {
        const double sy = fmin(fmax(((double)(i - p.top) + 0.5) * ky - 0.5, 0.0), ymax);
        const double fy = floor(sy);
        const float ay = (float)(sy - fy);
        const int ya = (int)fy, yb = ya + 1 < p.s.H ? ya + 1 : ya;
        const uint8_t* ra = base + (int64_t)ya * p.s.sh;
        const uint8_t* rb = base + (int64_t)yb * p.s.sh;
        om = 0.f;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
          const float v00 = (float)ra[oa + oc[c]], v01 = (float)ra[ob + oc[c]];
          const float v10 = (float)rb[oa + oc[c]], v11 = (float)rb[ob + oc[c]];
          const float t = v00 + ax * (v01 - v00), u = v10 + ax * (v11 - v10);
          const float v = (t + ay * (u - t)) * p.a[c] + p.b[c];
          o[c] = v;
          om = fmaxf(om, fabsf(v));
        }
      }
      m = fmaxf(m, om);
      *reinterpret_cast<f32x4*>(yo + (int64_t)r * p.ysh) = o;
    }
  }
  if (!p.y_amax) return;
  m = warp_max(m);
  if ((threadIdx.x & 63) == 0) wmax[threadIdx.x >> 6] = m;
  __syncthreads();
  if (threadIdx.x == 0) {
    m = fmaxf(fmaxf(wmax[0], wmax[1]), fmaxf(wmax[2], wmax[3]));
    if (m > 0.f) atomicMax(reinterpret_cast<unsigned*>(p.y_amax + n), __float_as_uint(m));
  }
}

struct ResU8K {
  U8Frames s;
  const float* meta; const int* n_crops; int max_crops;
  float a[3], b[3];
  int swap_rb;
  float* out;
};

// crop_resize_kernel of csrc/topdown.hip, statement for statement, on uint8 taps
__global__ __launch_bounds__(CROP_W) void crop_resize_u8_kernel(ResU8K p) {
  const int slot = blockIdx.x / (CROP_H / CR_ROWS);
  const int i0 = (blockIdx.x % (CROP_H / CR_ROWS)) * CR_ROWS;
  const int j = threadIdx.x;
  f32x4* orow = reinterpret_cast<f32x4*>(p.out) + ((int64_t)slot * BUF_H + CROP_PAD + i0) * BUF_W + CROP_PAD + j;
  int n = *p.n_crops;
  n = n < p.max_crops ? n : p.max_crops;
  const float* m = p.meta + (int64_t)slot * 8;
  const int f = slot < n ? __float_as_int(m[0]) : -1;
  if ((unsigned)f >= (unsigned)p.s.B) {            // empty slot (or a frame index that is none): zeros
#pragma unroll
    for (int r = 0; r < CR_ROWS; ++r) orow[(int64_t)r * BUF_W] = f32x4{0.f, 0.f, 0.f, 0.f};
    return;
  }
  const double x0 = m[2], y0 = m[3], w = m[4], h = m[5];
  const double sx = fmin(fmax(x0 + (j + 0.5) * (w / CROP_W) - 0.5, -2.0), (double)p.s.W + 1.0);
  const double fx = floor(sx);
  const float ax = (float)(sx - fx);
  const int xa = (int)fx, xb = xa + 1;
  const bool ina = (unsigned)xa < (unsigned)p.s.W, inb = (unsigned)xb < (unsigned)p.s.W;
  const uint8_t* base = p.s.ptr + (int64_t)f * p.s.sn;
  const int64_t oa = (int64_t)(ina ? xa : 0) * p.s.sw, ob = (int64_t)(inb ? xb : 0) * p.s.sw;
#pragma unroll 4
  for (int r = 0; r < CR_ROWS; ++r) {
    const double sy = fmin(fmax(y0 + (i0 + r + 0.5) * (h / CROP_H) - 0.5, -2.0), (double)p.s.H + 1.0);
    const double fy = floor(sy);
    const float ay = (float)(sy - fy);
    const int ya = (int)fy, yb = ya + 1;
    const bool rowa = (unsigned)ya < (unsigned)p.s.H, rowb = (unsigned)yb < (unsigned)p.s.H;
    const uint8_t* ra = base + (int64_t)(rowa ? ya : 0) * p.s.sh;
    const uint8_t* rb = base + (int64_t)(rowb ? yb : 0) * p.s.sh;
    float v[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const int64_t oc = (int64_t)(p.swap_rb ? 2 - c : c) * p.s.sc;
      const float v00 = rowa && ina ? (float)ra[oa + oc] : 0.f, v01 = rowa && inb ? (float)ra[ob + oc] : 0.f;
      const float v10 = rowb && ina ? (float)rb[oa + oc] : 0.f, v11 = rowb && inb ? (float)rb[ob + oc] : 0.f;
      const float top = v00 + ax * (v01 - v00), bot = v10 + ax * (v11 - v10);
      v[c] = (top + ay * (bot - top)) * p.a[c] + p.b[c];
    }
    orow[(int64_t)r * BUF_W] = f32x4{v[0], v[1], v[2], 0.f};
  }
}

bool frames_ok(const prpe_view_u8* f) {
  return f && f->ptr && f->c == 3 && f->n > 0 && f->h > 0 && f->w > 0 && f->h <= MAX_DIM && f->w <= MAX_DIM;
}

U8Frames frames_of(const prpe_view_u8* f) { return U8Frames{f->ptr, f->n, f->h, f->w, f->sn, f->sh, f->sw, f->sc}; }

}  // namespace

extern "C" int prpe_frame_ingest(const prpe_view_u8* frames, const prpe_view* y, int32_t top, int32_t left,
                                 int32_t nh, int32_t nw, const float* a, const float* b, const float* fill,
                                 int32_t swap_rb, float* y_amax, void* stream) {
  if (!frames_ok(frames) || !view_ok(y) || !a || !b || !fill) return PRPE_EINVAL;
  if (frames->n != y->n) return PRPE_EINVAL;
  if (y->c != 4 || y->sc != 1 || y->sw % 4 || y->sh % 4 || y->sn % 4 || (uintptr_t)y->ptr % 16) return PRPE_EINVAL;
  if (nh < 1 || nw < 1 || top < 0 || left < 0 || (int64_t)top + nh > y->h || (int64_t)left + nw > y->w)
    return PRPE_EINVAL;
  const int64_t blocks = (int64_t)y->n * ((y->h + ING_ROWS - 1) / ING_ROWS);
  if (blocks >= (1LL << 31)) return PRPE_EINVAL;
  IngK p{};
  p.s = frames_of(frames);
  p.y = y->ptr; p.H = y->h; p.W = y->w; p.ysn = y->sn; p.ysh = y->sh; p.ysw = y->sw;
  p.top = top; p.left = left; p.nh = nh; p.nw = nw;
  for (int c = 0; c < 3; ++c) { p.a[c] = a[c]; p.b[c] = b[c]; p.fill[c] = fill[c]; }
  p.swap_rb = swap_rb ? 1 : 0;
  p.y_amax = y_amax;
  hipLaunchKernelGGL(frame_ingest_kernel, dim3((unsigned)blocks), dim3(ING_THREADS), 0, as_stream(stream), p);
  return launch_status();
}

extern "C" int prpe_crop_resize_u8(const prpe_view_u8* frames, const float* crop_meta, const int32_t* n_crops,
                                   int32_t max_crops, const float* a, const float* b, int32_t swap_rb,
                                   float* crops, void* stream) {
  if (!frames_ok(frames) || !crop_meta || !n_crops || !crops || !a || !b) return PRPE_EINVAL;
  if (max_crops <= 0 || (int64_t)max_crops * (CROP_H / CR_ROWS) >= (1LL << 31)) return PRPE_EINVAL;
  if ((uintptr_t)crops % 16) return PRPE_EINVAL;
  ResU8K p{};
  p.s = frames_of(frames);
  p.meta = crop_meta; p.n_crops = n_crops; p.max_crops = max_crops; p.out = crops;
  for (int c = 0; c < 3; ++c) { p.a[c] = a[c]; p.b[c] = b[c]; }
  p.swap_rb = swap_rb ? 1 : 0;
  hipLaunchKernelGGL(crop_resize_u8_kernel, dim3((unsigned)(max_crops * (CROP_H / CR_ROWS))), dim3(CROP_W), 0,
                     as_stream(stream), p);
  return launch_status();
}
