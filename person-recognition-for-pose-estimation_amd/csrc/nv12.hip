// NV12 frames in: what a hardware video decoder hands over -- a luma plane, a
// half-resolution plane of interleaved (U, V) pairs, a row pitch wider than the picture -- read by
// the stages that gather the taps anyway, so that no RGB copy of the frames ever exists.
//
// The conversion is one integer rule (include/prpe.h): chroma replicated, pixel (i, j) takes the
// pair (i >> 1, j >> 1); R, G, B = clamp((cy (Y - y_off) + chroma term + 128) >> 8, 0, 255) with the
// three chroma terms crv E, -cgu D - cgv E, cbu D formed once per pair. A converted tap is a uint8
// value, so every fused kernel below has the bits of its _u8 twin (csrc/ingest.hip, csrc/roi.hip,
// csrc/facealign.hip) run on the frames prpe_nv12_to_rgb writes: the twins' statements are written
// out again here with the tap load replaced, and the twins stay as they are.
//
// prpe_nv12_to_rgb       — the unfused route. A thread owns 2 rows x 8 pixels: its 4 chroma pairs
//   arrive in one 8-byte load and are turned into their three terms once for the four pixels each
//   covers, each luma row is one 8-byte load, each output row three 8-byte stores (24 B). A lane's
//   neighbour owns the next 8 pixels, so a wave reads 512 B of each luma row and writes 1536 B of
//   each output row, contiguous. The 8-byte paths need 8-byte aligned planes and pitches (a
//   decoder's are); otherwise, and for the last partial block of a row, bytes and pairs one by one.
//   Nothing between w and the pitch is loaded: a wide load is taken only for a full block.
// prpe_frame_ingest_nv12 — prpe_frame_ingest's launch and statements. The row pair (ya, yb) is
//   wave-uniform, so when both rows share a chroma row (ya even, or the clamped last row) the two
//   pairs of the second row are neither loaded nor converted again: a uniform branch. The two x
//   taps differ per lane; both pairs are always loaded (the same 2 bytes when xa is even).
// prpe_crop_resize_nv12, prpe_roi_resize_nv12, prpe_roi_warp_nv12 — the crop stages; a tap outside
//   the frame is raw 0 in all three channels and is never loaded, as in the twins.
#pragma clang fp contract(off)
#include "roi.h"

namespace {

using namespace roi;

constexpr int ING_THREADS = 256;               // as csrc/ingest.hip
constexpr int ING_ROWS = 8;
constexpr int CROP_H = 256, CROP_W = 192;      // as csrc/topdown.hip: the ViTPose input
constexpr int CROP_PAD = 2;
constexpr int BUF_H = CROP_H + 2 * CROP_PAD, BUF_W = CROP_W + 2 * CROP_PAD;
constexpr int CR_ROWS = 8;
constexpr int CVT_PIX = 8;                     // pixels per thread and row of nv12_to_rgb
constexpr int CVT_COLS = 64, CVT_PAIRS = 4;    // a workgroup: 64 blocks of 8 pixels x 4 row pairs
constexpr int CVT_THREADS = CVT_COLS * CVT_PAIRS;

struct NvSrc {
  const uint8_t* y; const uint8_t* uv;
  int B, H, W;
  int64_t ysn, ysh, uvsn, uvsh;                // bytes
  int y_off, cy, crv, cgu, cgv, cbu;
};

// the three chroma terms of one (U, V) pair, the rounding constant included
struct Chroma { int r, g, b; };

__device__ __forceinline__ Chroma chroma_of(const NvSrc& s, unsigned pair) {
  const int D = (int)(pair & 0xffu) - 128, E = (int)(pair >> 8 & 0xffu) - 128;
  return Chroma{s.crv * E + 128, 128 - s.cgu * D - s.cgv * E, s.cbu * D + 128};
}
// the pair that covers column x of the chroma row uvrow: one aligned 16-bit load
__device__ __forceinline__ Chroma chroma_at(const NvSrc& s, const uint8_t* uvrow, int x) {
  return chroma_of(s, *reinterpret_cast<const uint16_t*>(uvrow + (int64_t)(x >> 1) * 2));
}
__device__ __forceinline__ int clamp8(int v) {
  v >>= 8;                                     // arithmetic: floor for a negative numerator
  return v < 0 ? 0 : (v > 255 ? 255 : v);
}
__device__ __forceinline__ void rgb_of(const NvSrc& s, int Y, const Chroma& c, int (&v)[3]) {
  const int l = s.cy * (Y - s.y_off);
  v[0] = clamp8(l + c.r);
  v[1] = clamp8(l + c.g);
  v[2] = clamp8(l + c.b);
}

// ---------------------------------------------------------------- prpe_nv12_to_rgb
struct CvtK {
  NvSrc s;
  uint8_t* out; int64_t osn, osh;
  int swap_rb, wide_in, wide_out;
  int cbw, rpn, bx, by;                        // blocks of 8 pixels per row, row pairs, workgroups per axis
};

__global__ __launch_bounds__(CVT_THREADS) void nv12_to_rgb_kernel(CvtK p) {
  const int per = p.bx * p.by;
  const int n = blockIdx.x / per, rem = blockIdx.x - n * per;
  const int byi = rem / p.bx, bxi = rem - byi * p.bx;
  const int cb = bxi * CVT_COLS + (threadIdx.x & (CVT_COLS - 1));
  const int rp = byi * CVT_PAIRS + (threadIdx.x >> 6);         // wave-uniform
  if (cb >= p.cbw || rp >= p.rpn) return;
  const int x0 = cb * CVT_PIX, y0 = rp * 2;
  const int cols = p.s.W - x0 < CVT_PIX ? p.s.W - x0 : CVT_PIX;
  const bool two = y0 + 1 < p.s.H;
  const uint8_t* l0 = p.s.y + (int64_t)n * p.s.ysn + (int64_t)y0 * p.s.ysh + x0;
  const uint8_t* l1 = l0 + p.s.ysh;
  const uint8_t* uv = p.s.uv + (int64_t)n * p.s.uvsn + (int64_t)rp * p.s.uvsh + x0;   // pair x0 / 2 at byte x0
  const bool full = cols == CVT_PIX;
  unsigned long long luma[2] = {0ull, 0ull}, cw = 0ull;
  if (full && p.wide_in) {
    luma[0] = *reinterpret_cast<const unsigned long long*>(l0);
    if (two) luma[1] = *reinterpret_cast<const unsigned long long*>(l1);
    cw = *reinterpret_cast<const unsigned long long*>(uv);
  } else {
#pragma unroll
    for (int q = 0; q < CVT_PIX; ++q) {
      if (q < cols) {
        luma[0] |= (unsigned long long)l0[q] << (8 * q);
        if (two) luma[1] |= (unsigned long long)l1[q] << (8 * q);
        if (!(q & 1)) cw |= (unsigned long long)*reinterpret_cast<const uint16_t*>(uv + q) << (8 * q);
      }
    }
  }
  Chroma ch[CVT_PIX / 2];
#pragma unroll
  for (int k = 0; k < CVT_PIX / 2; ++k) ch[k] = chroma_of(p.s, (unsigned)(cw >> (16 * k)) & 0xffffu);
  uint8_t* o = p.out + (int64_t)n * p.osn + (int64_t)y0 * p.osh + (int64_t)x0 * 3;
#pragma unroll
  for (int r = 0; r < 2; ++r) {
    if (r == 1 && !two) break;
    unsigned long long w[3] = {0ull, 0ull, 0ull};
    uint8_t* orow = o + (int64_t)r * p.osh;
#pragma unroll
    for (int q = 0; q < CVT_PIX; ++q) {
      int v[3];
      rgb_of(p.s, (int)(luma[r] >> (8 * q) & 0xffu), ch[q >> 1], v);
      if (p.swap_rb) { const int t = v[0]; v[0] = v[2]; v[2] = t; }
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        const int byte = q * 3 + c;
        w[byte >> 3] |= (unsigned long long)(unsigned)v[c] << (8 * (byte & 7));
      }
    }
    if (full && p.wide_out) {
#pragma unroll
      for (int k = 0; k < 3; ++k) reinterpret_cast<unsigned long long*>(orow)[k] = w[k];
    } else {
#pragma unroll
      for (int byte = 0; byte < CVT_PIX * 3; ++byte)
        if (byte < cols * 3) orow[byte] = (uint8_t)(w[byte >> 3] >> (8 * (byte & 7)));
    }
  }
}

// ---------------------------------------------------------------- prpe_frame_ingest_nv12
struct IngNvK {
  NvSrc s;
  float* y; int H, W; int64_t ysn, ysh, ysw;   // float elements, each a multiple of 4
  int top, left, nh, nw;
  float a[3], b[3], fill[3];
  float* y_amax;
};

// frame_ingest_kernel of csrc/ingest.hip, statement for statement, on converted taps
__global__ __launch_bounds__(ING_THREADS) void frame_ingest_nv12_kernel(IngNvK p) {
  __shared__ float wmax[ING_THREADS / 64];
  const int bpf = (p.H + ING_ROWS - 1) / ING_ROWS;              // workgroups per frame
  const int n = blockIdx.x / bpf, i0 = (blockIdx.x - n * bpf) * ING_ROWS;
  const int rows = p.H - i0 < ING_ROWS ? p.H - i0 : ING_ROWS;
  const uint8_t* lbase = p.s.y + (int64_t)n * p.s.ysn;
  const uint8_t* cbase = p.s.uv + (int64_t)n * p.s.uvsn;
  float* ybase = p.y + (int64_t)n * p.ysn + (int64_t)i0 * p.ysh;
  const double kx = (double)p.s.W / (double)p.nw, ky = (double)p.s.H / (double)p.nh;
  const double xmax = (double)(p.s.W - 1), ymax = (double)(p.s.H - 1);
  float fv[3];
#pragma unroll
  for (int c = 0; c < 3; ++c) fv[c] = p.fill[c] * p.a[c] + p.b[c];
  const float fmx = fmaxf(fmaxf(fabsf(fv[0]), fabsf(fv[1])), fabsf(fv[2]));
  float m = 0.f;
  for (int j = threadIdx.x; j < p.W; j += ING_THREADS) {
    const bool col_in = (unsigned)(j - p.left) < (unsigned)p.nw;
    // clamped into the source before the conversion to int: in bounds for any argument
    const double sx = fmin(fmax(((double)(j - p.left) + 0.5) * kx - 0.5, 0.0), xmax);
    const double fx = floor(sx);
    const float ax = (float)(sx - fx);
    const int xa = (int)fx, xb = xa + 1 < p.s.W ? xa + 1 : xa;  // xb == xa only where ax == 0
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
        const uint8_t* ra = lbase + (int64_t)ya * p.s.ysh;
        const uint8_t* rb = lbase + (int64_t)yb * p.s.ysh;
        const uint8_t* ua = cbase + (int64_t)(ya >> 1) * p.s.uvsh;
        const Chroma ca0 = chroma_at(p.s, ua, xa), ca1 = chroma_at(p.s, ua, xb);
        Chroma cb0 = ca0, cb1 = ca1;
        if ((yb >> 1) != (ya >> 1)) {                           // the same for the whole wave
          const uint8_t* ub = cbase + (int64_t)(yb >> 1) * p.s.uvsh;
          cb0 = chroma_at(p.s, ub, xa);
          cb1 = chroma_at(p.s, ub, xb);
        }
        int t00[3], t01[3], t10[3], t11[3];
        rgb_of(p.s, ra[xa], ca0, t00);
        rgb_of(p.s, ra[xb], ca1, t01);
        rgb_of(p.s, rb[xa], cb0, t10);
        rgb_of(p.s, rb[xb], cb1, t11);
        om = 0.f;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
          const float v00 = (float)t00[c], v01 = (float)t01[c];
          const float v10 = (float)t10[c], v11 = (float)t11[c];
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

// ---------------------------------------------------------------- the crop stages
// one tap of a crop stage: raw 0 in all three channels outside the frame, never loaded there
// (x and the rows are already 0 where the tap is outside: the twins' clamp)
__device__ __forceinline__ void tap_rgb(const NvSrc& s, const uint8_t* lrow, const uint8_t* crow, int x, bool in,
                                        float (&v)[3]) {
  v[0] = v[1] = v[2] = 0.f;
  if (in) {
    int t[3];
    rgb_of(s, lrow[x], chroma_at(s, crow, x), t);
    v[0] = (float)t[0]; v[1] = (float)t[1]; v[2] = (float)t[2];
  }
}

// the luma and chroma rows of frame f the two row taps read (row 0 where a tap is outside)
struct Rows { const uint8_t *la, *lb, *ca, *cb; };
__device__ __forceinline__ Rows rows_of(const NvSrc& s, int f, int ya, bool rowa, int yb, bool rowb) {
  const uint8_t* l = s.y + (int64_t)f * s.ysn;
  const uint8_t* c = s.uv + (int64_t)f * s.uvsn;
  const int ia = rowa ? ya : 0, ib = rowb ? yb : 0;
  return Rows{l + (int64_t)ia * s.ysh, l + (int64_t)ib * s.ysh, c + (int64_t)(ia >> 1) * s.uvsh,
              c + (int64_t)(ib >> 1) * s.uvsh};
}

struct CropNvK {
  NvSrc s;
  const float* meta; const int* n_crops; int max_crops;
  float a[3], b[3];
  float* out;
};

// crop_resize_u8_kernel of csrc/ingest.hip, statement for statement, on converted taps
__global__ __launch_bounds__(CROP_W) void crop_resize_nv12_kernel(CropNvK p) {
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
  const int oa = ina ? xa : 0, ob = inb ? xb : 0;
#pragma unroll 4
  for (int r = 0; r < CR_ROWS; ++r) {
    const double sy = fmin(fmax(y0 + (i0 + r + 0.5) * (h / CROP_H) - 0.5, -2.0), (double)p.s.H + 1.0);
    const double fy = floor(sy);
    const float ay = (float)(sy - fy);
    const int ya = (int)fy, yb = ya + 1;
    const bool rowa = (unsigned)ya < (unsigned)p.s.H, rowb = (unsigned)yb < (unsigned)p.s.H;
    const Rows rw = rows_of(p.s, f, ya, rowa, yb, rowb);
    float v00[3], v01[3], v10[3], v11[3];
    tap_rgb(p.s, rw.la, rw.ca, oa, rowa && ina, v00);
    tap_rgb(p.s, rw.la, rw.ca, ob, rowa && inb, v01);
    tap_rgb(p.s, rw.lb, rw.cb, oa, rowb && ina, v10);
    tap_rgb(p.s, rw.lb, rw.cb, ob, rowb && inb, v11);
    float v[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const float top = v00[c] + ax * (v01[c] - v00[c]), bot = v10[c] + ax * (v11[c] - v10[c]);
      v[c] = (top + ay * (bot - top)) * p.a[c] + p.b[c];
    }
    orow[(int64_t)r * BUF_W] = f32x4{v[0], v[1], v[2], 0.f};
  }
}

// ResK<uint8_t> carries the list, the output and the affine (src and its strides stay unused):
// roi::resize_block and roi::resize_amax then apply as they are
struct RoiNvK {
  ResK<uint8_t> r;
  NvSrc s;
};

// roi::resize_pixel on converted taps: blend per channel, the affine, the 16-B store
__device__ __forceinline__ float nv_pixel(const RoiNvK& p, const Rows& rw, int oa, int ob, const Tap& tx, const Tap& ty,
                                          float* yo, float mx) {
  float v00[3], v01[3], v10[3], v11[3];
  tap_rgb(p.s, rw.la, rw.ca, oa, ty.ina && tx.ina, v00);
  tap_rgb(p.s, rw.la, rw.ca, ob, ty.ina && tx.inb, v01);
  tap_rgb(p.s, rw.lb, rw.cb, oa, ty.inb && tx.ina, v10);
  tap_rgb(p.s, rw.lb, rw.cb, ob, ty.inb && tx.inb, v11);
  float v[3];
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const float top = v00[c] + tx.a * (v01[c] - v00[c]), bot = v10[c] + tx.a * (v11[c] - v10[c]);
    v[c] = top + ty.a * (bot - top);
    v[c] = v[c] * p.r.a[c] + p.r.b[c];
    mx = fmaxf(mx, fabsf(v[c]));
  }
  *reinterpret_cast<f32x4*>(yo) = f32x4{v[0], v[1], v[2], 0.f};
  return mx;
}

// roi::resize_window on converted taps
__device__ __forceinline__ float nv_window(const RoiNvK& p, const ResBlock& k) {
  const double x0 = k.m[2], y0 = k.m[3], w = k.m[4], h = k.m[5];
  float mx = 0.f;
  for (int j = threadIdx.x; j < p.r.ow; j += RR_THREADS) {
    const Tap tx = tap(x0, w, j, p.r.ow, p.s.W);
    const int oa = tx.ina ? tx.ia : 0, ob = tx.inb ? tx.ib : 0;
    float* yo = k.ybase + (int64_t)j * p.r.ysw;
#pragma unroll 4
    for (int r = 0; r < k.rows; ++r) {
      const Tap ty = tap(y0, h, k.i0 + r, p.r.oh, p.s.H);
      const Rows rw = rows_of(p.s, k.f, ty.ia, ty.ina, ty.ib, ty.inb);
      mx = nv_pixel(p, rw, oa, ob, tx, ty, yo + (int64_t)r * p.r.ysh, mx);
    }
  }
  return mx;
}

// warp_rows of csrc/facealign.hip on converted taps
__device__ __forceinline__ float nv_warp_rows(const RoiNvK& p, const ResBlock& k, const float* wr) {
  const double a = wr[2], b = wr[3], tx = wr[4], c = wr[5], d = wr[6], ty = wr[7];
  float mx = 0.f;
  for (int j = threadIdx.x; j < p.r.ow; j += RR_THREADS) {
    const double xc = a * (j + 0.5) + tx, yc = c * (j + 0.5) + ty;      // the column's part
    float* yo = k.ybase + (int64_t)j * p.r.ysw;
#pragma unroll 4
    for (int r = 0; r < k.rows; ++r) {
      const double v = (k.i0 + r) + 0.5;
      const Tap sx = tap_at(xc + b * v - 0.5, p.s.W), sy = tap_at(yc + d * v - 0.5, p.s.H);
      const int oa = sx.ina ? sx.ia : 0, ob = sx.inb ? sx.ib : 0;
      const Rows rw = rows_of(p.s, k.f, sy.ia, sy.ina, sy.ib, sy.inb);
      mx = nv_pixel(p, rw, oa, ob, sx, sy, yo + (int64_t)r * p.r.ysh, mx);
    }
  }
  return mx;
}

__global__ __launch_bounds__(RR_THREADS) void roi_resize_nv12_kernel(RoiNvK p) {
  __shared__ float wmax[RR_THREADS / 64];
  ResBlock k;
  if (!resize_block(p.r, k)) return;
  resize_amax(p.r, k.slot, nv_window(p, k), wmax);
}

__global__ __launch_bounds__(RR_THREADS) void roi_warp_nv12_kernel(RoiNvK p) {
  __shared__ float wmax[RR_THREADS / 64];
  ResBlock k;
  if (!resize_block(p.r, k)) return;
  const float* wr = p.r.warp + (int64_t)k.slot * 8;
  const float mx = __float_as_int(wr[0]) == 1 ? nv_warp_rows(p, k, wr) : nv_window(p, k);
  resize_amax(p.r, k.slot, mx, wmax);
}

// ---------------------------------------------------------------- host side
// the planes and the coefficients of a call, or false when it is refused
bool nv_args(NvSrc& s, const prpe_nv12* f, const int32_t* coef) {
  if (!f || !coef || !f->y || !f->uv) return false;
  if (f->n < 1 || f->h < 1 || f->w < 1 || f->h > MAX_DIM || f->w > MAX_DIM) return false;
  if (f->y_sh < f->w || f->uv_sh < 2 * (int64_t)((f->w + 1) / 2)) return false;
  if ((uintptr_t)f->uv % 2 || f->uv_sn % 2 || f->uv_sh % 2) return false;
  if (coef[0] < 0 || coef[0] > 255) return false;
  for (int k = 1; k < 6; ++k)
    if (coef[k] < 0 || coef[k] > 4096) return false;
  s.y = f->y; s.uv = f->uv; s.B = f->n; s.H = f->h; s.W = f->w;
  s.ysn = f->y_sn; s.ysh = f->y_sh; s.uvsn = f->uv_sn; s.uvsh = f->uv_sh;
  s.y_off = coef[0]; s.cy = coef[1]; s.crv = coef[2]; s.cgu = coef[3]; s.cgv = coef[4]; s.cbu = coef[5];
  return true;
}

// the list, the output and the grid of a roi stage through roi::resize_args (a stand-in view of
// the luma plane carries the frame count and sides to its checks)
bool roi_nv_args(RoiNvK& p, const prpe_nv12* f, const int32_t* coef, const float* crop_meta, const int32_t* n_crops,
                 int32_t max_crops, const float* a, const float* b, const prpe_view* y, float* y_amax,
                 int64_t& blocks) {
  if (!a || !b || !nv_args(p.s, f, coef)) return false;
  const prpe_view_u8 lum{f->y, f->n, f->h, f->w, 3, f->y_sn, f->y_sh, 1, 0};
  if (!resize_args(p.r, &lum, crop_meta, n_crops, max_crops, y, y_amax, blocks)) return false;
  p.r.src = nullptr;
  for (int c = 0; c < 3; ++c) { p.r.a[c] = a[c]; p.r.b[c] = b[c]; }
  return true;
}

}  // namespace

extern "C" int prpe_nv12_to_rgb(const prpe_nv12* src, const int32_t* coef, int32_t swap_rb, uint8_t* out, int64_t osn,
                                int64_t osh, void* stream) {
  CvtK p{};
  if (!out || !nv_args(p.s, src, coef)) return PRPE_EINVAL;
  if (osh < 3 * (int64_t)src->w) return PRPE_EINVAL;
  p.out = out; p.osn = osn; p.osh = osh;
  p.swap_rb = swap_rb ? 1 : 0;
  p.wide_in = !((uintptr_t)src->y % 8 || src->y_sn % 8 || src->y_sh % 8 || (uintptr_t)src->uv % 8 || src->uv_sn % 8 ||
                src->uv_sh % 8);
  p.wide_out = !((uintptr_t)out % 8 || osn % 8 || osh % 8);
  p.cbw = (src->w + CVT_PIX - 1) / CVT_PIX;
  p.rpn = (src->h + 1) / 2;
  p.bx = (p.cbw + CVT_COLS - 1) / CVT_COLS;
  p.by = (p.rpn + CVT_PAIRS - 1) / CVT_PAIRS;
  const int64_t blocks = (int64_t)src->n * p.bx * p.by;
  if (blocks >= (1LL << 31)) return PRPE_EINVAL;
  hipLaunchKernelGGL(nv12_to_rgb_kernel, dim3((unsigned)blocks), dim3(CVT_THREADS), 0, as_stream(stream), p);
  return launch_status();
}

extern "C" int prpe_frame_ingest_nv12(const prpe_nv12* src, const int32_t* coef, const prpe_view* y, int32_t top,
                                      int32_t left, int32_t nh, int32_t nw, const float* a, const float* b,
                                      const float* fill, float* y_amax, void* stream) {
  IngNvK p{};
  if (!nv_args(p.s, src, coef) || !view_ok(y) || !a || !b || !fill) return PRPE_EINVAL;
  if (src->n != y->n) return PRPE_EINVAL;
  if (y->c != 4 || y->sc != 1 || y->sw % 4 || y->sh % 4 || y->sn % 4 || (uintptr_t)y->ptr % 16) return PRPE_EINVAL;
  if (nh < 1 || nw < 1 || top < 0 || left < 0 || (int64_t)top + nh > y->h || (int64_t)left + nw > y->w)
    return PRPE_EINVAL;
  const int64_t blocks = (int64_t)y->n * ((y->h + ING_ROWS - 1) / ING_ROWS);
  if (blocks >= (1LL << 31)) return PRPE_EINVAL;
  p.y = y->ptr; p.H = y->h; p.W = y->w; p.ysn = y->sn; p.ysh = y->sh; p.ysw = y->sw;
  p.top = top; p.left = left; p.nh = nh; p.nw = nw;
  for (int c = 0; c < 3; ++c) { p.a[c] = a[c]; p.b[c] = b[c]; p.fill[c] = fill[c]; }
  p.y_amax = y_amax;
  hipLaunchKernelGGL(frame_ingest_nv12_kernel, dim3((unsigned)blocks), dim3(ING_THREADS), 0, as_stream(stream), p);
  return launch_status();
}

extern "C" int prpe_crop_resize_nv12(const prpe_nv12* src, const int32_t* coef, const float* crop_meta,
                                     const int32_t* n_crops, int32_t max_crops, const float* a, const float* b,
                                     float* crops, void* stream) {
  CropNvK p{};
  if (!nv_args(p.s, src, coef) || !crop_meta || !n_crops || !crops || !a || !b) return PRPE_EINVAL;
  if (max_crops <= 0 || (int64_t)max_crops * (CROP_H / CR_ROWS) >= (1LL << 31)) return PRPE_EINVAL;
  if ((uintptr_t)crops % 16) return PRPE_EINVAL;
  p.meta = crop_meta; p.n_crops = n_crops; p.max_crops = max_crops; p.out = crops;
  for (int c = 0; c < 3; ++c) { p.a[c] = a[c]; p.b[c] = b[c]; }
  hipLaunchKernelGGL(crop_resize_nv12_kernel, dim3((unsigned)(max_crops * (CROP_H / CR_ROWS))), dim3(CROP_W), 0,
                     as_stream(stream), p);
  return launch_status();
}

extern "C" int prpe_roi_resize_nv12(const prpe_nv12* src, const int32_t* coef, const float* crop_meta,
                                    const int32_t* n_crops, int32_t max_crops, const prpe_view* y, const float* a,
                                    const float* b, float* y_amax, void* stream) {
  RoiNvK p{};
  int64_t blocks;
  if (!roi_nv_args(p, src, coef, crop_meta, n_crops, max_crops, a, b, y, y_amax, blocks)) return PRPE_EINVAL;
  hipLaunchKernelGGL(roi_resize_nv12_kernel, dim3((unsigned)blocks), dim3(RR_THREADS), 0, as_stream(stream), p);
  return launch_status();
}

extern "C" int prpe_roi_warp_nv12(const prpe_nv12* src, const int32_t* coef, const float* crop_meta,
                                  const int32_t* n_crops, int32_t max_crops, const float* warp, const prpe_view* y,
                                  const float* a, const float* b, float* y_amax, void* stream) {
  RoiNvK p{};
  int64_t blocks;
  if (!warp || !roi_nv_args(p, src, coef, crop_meta, n_crops, max_crops, a, b, y, y_amax, blocks)) return PRPE_EINVAL;
  p.r.warp = warp;
  hipLaunchKernelGGL(roi_warp_nv12_kernel, dim3((unsigned)blocks), dim3(RR_THREADS), 0, as_stream(stream), p);
  return launch_status();
}
