// Device code shared by the kernels of csrc/roi.hip: csrc/topdown.hip's crop list
// rule and bilinear tap arithmetic with the output size as a parameter. The statements and their
// order are topdown.hip's (fp32 window with contraction off; fp64 sample coordinates, one fp32
// rounding per weight), so that at 256 x 192 the results have prpe_crop_select's and
// prpe_crop_resize's bits; topdown.hip itself keeps its own text.
#pragma once
#pragma clang fp contract(off)
#include <type_traits>
#include "common.h"

namespace roi {

constexpr int SEL_THREADS = 256;
constexpr int MAX_DIM = 1 << 24;               // frame sides stay exact in fp32
constexpr int MAX_OUT = 4096;                  // largest output side

__device__ __forceinline__ bool finitef(float v) { return fabsf(v) <= 3.402823466e38f; }   // false for NaN

struct SelK {
  const float* dets; const int* counts; int B, max_det;
  float thr, min_size, sx, sy, pad; int per_frame, max_crops;
  int out_h, out_w;
  float* meta; int* n_crops; int* status;
};

// the window of one detection row, or false when the row is skipped (crop_window of topdown.hip,
// the aspect from the output size)
__device__ __forceinline__ bool window(const SelK& p, const float* d, float& x0, float& y0, float& w, float& h) {
  const float x1 = d[0] * p.sx, y1 = d[1] * p.sy, x2 = d[2] * p.sx, y2 = d[3] * p.sy;
  if (!(finitef(x1) && finitef(y1) && finitef(x2) && finitef(y2))) return false;
  w = x2 - x1;
  h = y2 - y1;
  if (!(w >= p.min_size) || !(h >= p.min_size)) return false;
  const float cx = (x1 + x2) * 0.5f, cy = (y1 + y2) * 0.5f;
  const float a = (float)p.out_w / (float)p.out_h;
  if (w > a * h) h = w / a; else w = h * a;
  w *= p.pad;
  h *= p.pad;
  x0 = cx - 0.5f * w;
  y0 = cy - 0.5f * h;
  return finitef(w) && finitef(h) && finitef(x0) && finitef(y0);
}

// rows of frame b in the candidate prefix: the first rows with score >= thr, at most per_frame
__device__ __forceinline__ int prefix(const SelK& p, int b) {
  int c = p.counts[b];
  c = c < p.max_det ? c : p.max_det;
  c = c < p.per_frame ? c : p.per_frame;
  int n = 0;
  while (n < c && p.dets[((int64_t)b * p.max_det + n) * 6 + 4] >= p.thr) ++n;
  return n;
}

// One axis of a sample: the source index pair, the weight and which taps lie inside [0, size).
// Coordinates past the frame by more than a pixel are clamped there: every tap is outside either
// way (zero), and the conversion to int stays defined for any window (NaN -> -2).
struct Tap {
  float a; int ia, ib; bool ina, inb;
};
// the taps about the sample coordinate s (pixel k's centre at k; not yet clamped)
__device__ __forceinline__ Tap tap_at(double s, int size) {
  s = fmin(fmax(s, -2.0), (double)size + 1.0);
  const double f = floor(s);
  Tap t;
  t.a = (float)(s - f);
  t.ia = (int)f;
  t.ib = t.ia + 1;
  t.ina = (unsigned)t.ia < (unsigned)size;
  t.inb = (unsigned)t.ib < (unsigned)size;
  return t;
}
__device__ __forceinline__ Tap tap(double origin, double extent, int idx, int out, int size) {
  return tap_at(origin + (idx + 0.5) * (extent / out) - 0.5, size);
}

__device__ __forceinline__ float raw(float v) { return v; }
__device__ __forceinline__ float raw(uint8_t v) { return (float)v; }

// two fp32 lerps v00 + ax (v01 - v00); a tap outside the frame is 0 and is never loaded
template <typename T>
__device__ __forceinline__ float blend(const T* ra, const T* rb, int64_t oa, int64_t ob, const Tap& x, const Tap& y) {
  const float v00 = y.ina && x.ina ? raw(ra[oa]) : 0.f, v01 = y.ina && x.inb ? raw(ra[ob]) : 0.f;
  const float v10 = y.inb && x.ina ? raw(rb[oa]) : 0.f, v11 = y.inb && x.inb ? raw(rb[ob]) : 0.f;
  const float top = v00 + x.a * (v01 - v00), bot = v10 + x.a * (v11 - v10);
  return top + y.a * (bot - top);
}

// ---- the resample workgroup of prpe_roi_resize(_u8) and prpe_roi_warp(_u8) (csrc/facealign.hip):
// one 128-thread workgroup per (slot, 8 output rows)
constexpr int RR_THREADS = 128;
constexpr int RR_ROWS = 8;                     // output rows per workgroup

template <typename T>
struct ResK {
  const T* src; int B, H, W; int64_t sn, sh, sw, sc;
  const float* meta; const int* n_crops; int max_crops;
  float* y; int oh, ow; int64_t ysn, ysh, ysw;   // float elements, each a multiple of 4
  float a[3], b[3];                              // uint8 frames only
  int swap_rb;
  float* y_amax;
  const float* warp;                             // prpe_roi_warp only: [max_crops][8]
};

// what a workgroup works on: its slot, its rows [i0, i0 + rows), their first output element and
// the slot's frame
struct ResBlock {
  int slot, i0, rows, f;
  float* ybase;
  const float* m;
};

// false: the slot is empty (or its frame index is none) and the workgroup's rows are now zeros;
// the whole workgroup returns and y_amax stays as it is
template <typename T>
__device__ __forceinline__ bool resize_block(const ResK<T>& p, ResBlock& k) {
  const int bps = (p.oh + RR_ROWS - 1) / RR_ROWS;               // workgroups per slot
  k.slot = blockIdx.x / bps;
  k.i0 = (blockIdx.x - k.slot * bps) * RR_ROWS;
  k.rows = p.oh - k.i0 < RR_ROWS ? p.oh - k.i0 : RR_ROWS;
  k.ybase = p.y + (int64_t)k.slot * p.ysn + (int64_t)k.i0 * p.ysh;
  int n = *p.n_crops;
  n = n < p.max_crops ? n : p.max_crops;
  k.m = p.meta + (int64_t)k.slot * 8;
  k.f = k.slot < n ? __float_as_int(k.m[0]) : -1;
  if ((unsigned)k.f < (unsigned)p.B) return true;
  for (int j = threadIdx.x; j < p.ow; j += RR_THREADS)
    for (int r = 0; r < k.rows; ++r)
      *reinterpret_cast<f32x4*>(k.ybase + (int64_t)r * p.ysh + (int64_t)j * p.ysw) = f32x4{0.f, 0.f, 0.f, 0.f};
  return false;
}

// source channel offsets of the three output channels
template <typename T>
__device__ __forceinline__ void channel_offsets(const ResK<T>& p, int64_t (&oc)[3]) {
  constexpr bool U8 = std::is_same<T, uint8_t>::value;
#pragma unroll
  for (int c = 0; c < 3; ++c) oc[c] = (int64_t)(U8 && p.swap_rb ? 2 - c : c) * p.sc;
}

// one output pixel from its taps: three channels blended, the uint8 affine, the 16-B store;
// returns mx raised to the pixel's max|v|
template <typename T>
__device__ __forceinline__ float resize_pixel(const ResK<T>& p, const T* ra, const T* rb, const int64_t (&oc)[3],
                                              int64_t oa, int64_t ob, const Tap& tx, const Tap& ty, float* yo,
                                              float mx) {
  constexpr bool U8 = std::is_same<T, uint8_t>::value;
  float v[3];
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    v[c] = blend(ra + oc[c], rb + oc[c], oa, ob, tx, ty);
    if constexpr (U8) v[c] = v[c] * p.a[c] + p.b[c];
    mx = fmaxf(mx, fabsf(v[c]));
  }
  *reinterpret_cast<f32x4*>(yo) = f32x4{v[0], v[1], v[2], 0.f};
  return mx;
}

// the workgroup's rows of the slot's window in crop_meta: a thread owns the columns tid,
// tid + 128, ...; returns the thread's max|v|
template <typename T>
__device__ __forceinline__ float resize_window(const ResK<T>& p, const ResBlock& k) {
  const double x0 = k.m[2], y0 = k.m[3], w = k.m[4], h = k.m[5];
  const T* base = p.src + (int64_t)k.f * p.sn;
  int64_t oc[3];
  channel_offsets(p, oc);
  float mx = 0.f;
  for (int j = threadIdx.x; j < p.ow; j += RR_THREADS) {
    const Tap tx = tap(x0, w, j, p.ow, p.W);
    const int64_t oa = (int64_t)(tx.ina ? tx.ia : 0) * p.sw, ob = (int64_t)(tx.inb ? tx.ib : 0) * p.sw;
    float* yo = k.ybase + (int64_t)j * p.ysw;
#pragma unroll 4
    for (int r = 0; r < k.rows; ++r) {
      const Tap ty = tap(y0, h, k.i0 + r, p.oh, p.H);
      const T* ra = base + (int64_t)(ty.ina ? ty.ia : 0) * p.sh;
      const T* rb = base + (int64_t)(ty.inb ? ty.ib : 0) * p.sh;
      mx = resize_pixel(p, ra, rb, oc, oa, ob, tx, ty, yo + (int64_t)r * p.ysh, mx);
    }
  }
  return mx;
}

// the slot's max|y|: one atomicMax on the bit pattern per workgroup (wmax: RR_THREADS / 64 floats of LDS)
template <typename T>
__device__ __forceinline__ void resize_amax(const ResK<T>& p, int slot, float mx, float* wmax) {
  if (!p.y_amax) return;
  mx = warp_max(mx);
  if ((threadIdx.x & 63) == 0) wmax[threadIdx.x >> 6] = mx;
  __syncthreads();
  if (threadIdx.x == 0) {
    mx = fmaxf(wmax[0], wmax[1]);
    if (mx > 0.f) atomicMax(reinterpret_cast<unsigned*>(p.y_amax + slot), __float_as_uint(mx));
  }
}

// ---- host side: the argument checks and the launch shape the four entry points share
static inline bool y_ok(const prpe_view* y, int32_t max_crops) {
  return view_ok(y) && y->n == max_crops && y->c == 4 && y->sc == 1 && y->sw % 4 == 0 && y->sh % 4 == 0 &&
         y->sn % 4 == 0 && (uintptr_t)y->ptr % 16 == 0 && y->h <= MAX_OUT && y->w <= MAX_OUT;
}

// frames, list and output of a ResK, or false when the call is refused; blocks: the grid
template <typename T, typename V>
static inline bool resize_args(ResK<T>& p, const V* frames, const float* crop_meta, const int32_t* n_crops,
                               int32_t max_crops, const prpe_view* y, float* y_amax, int64_t& blocks) {
  if (!frames || !frames->ptr || !crop_meta || !n_crops) return false;
  if (frames->c != 3 || frames->n <= 0 || frames->h <= 0 || frames->w <= 0) return false;
  if (frames->h > MAX_DIM || frames->w > MAX_DIM) return false;
  if (max_crops <= 0 || !y_ok(y, max_crops)) return false;
  blocks = (int64_t)max_crops * ((y->h + RR_ROWS - 1) / RR_ROWS);
  if (blocks >= (1LL << 31)) return false;
  p.src = frames->ptr; p.B = frames->n; p.H = frames->h; p.W = frames->w;
  p.sn = frames->sn; p.sh = frames->sh; p.sw = frames->sw; p.sc = frames->sc;
  p.meta = crop_meta; p.n_crops = n_crops; p.max_crops = max_crops;
  p.y = y->ptr; p.oh = y->h; p.ow = y->w; p.ysn = y->sn; p.ysh = y->sh; p.ysw = y->sw;
  p.y_amax = y_amax;
  return true;
}

}  // namespace roi
