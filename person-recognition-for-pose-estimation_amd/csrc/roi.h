// The resample workgroup of prpe_roi_resize and prpe_roi_warp for every frame
// source of csrc/frames.h: the kernels of csrc/roi.hip, csrc/facealign.hip and csrc/nv12.hip are
// instantiations of the two templates below. The tap arithmetic and the blend are frames.h's, so at
// 256 x 192 prpe_roi_resize has prpe_crop_resize's bits.
#pragma once
#pragma clang fp contract(off)
#include "frames.h"

namespace roi {

using namespace fsrc;

constexpr int MAX_OUT = 4096;                  // largest output side
constexpr int RR_THREADS = 128;                // one workgroup per (slot, 8 output rows)
constexpr int RR_ROWS = 8;                     // output rows per workgroup

template <typename S>
struct ResK {
  S s;
  const float* meta; const int* n_crops; int max_crops;
  float* y; int oh, ow; int64_t ysn, ysh, ysw;   // float elements, each a multiple of 4
  float a[3], b[3];                              // sources with the affine only
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
template <typename S>
__device__ __forceinline__ bool resize_block(const ResK<S>& p, ResBlock& k) {
  const int bps = (p.oh + RR_ROWS - 1) / RR_ROWS;               // workgroups per slot
  k.slot = blockIdx.x / bps;
  k.i0 = (blockIdx.x - k.slot * bps) * RR_ROWS;
  k.rows = p.oh - k.i0 < RR_ROWS ? p.oh - k.i0 : RR_ROWS;
  k.ybase = p.y + (int64_t)k.slot * p.ysn + (int64_t)k.i0 * p.ysh;
  int n = *p.n_crops;
  n = n < p.max_crops ? n : p.max_crops;
  k.m = p.meta + (int64_t)k.slot * 8;
  k.f = k.slot < n ? __float_as_int(k.m[0]) : -1;
  if ((unsigned)k.f < (unsigned)p.s.B) return true;
  for (int j = threadIdx.x; j < p.ow; j += RR_THREADS)
    for (int r = 0; r < k.rows; ++r)
      *reinterpret_cast<f32x4*>(k.ybase + (int64_t)r * p.ysh + (int64_t)j * p.ysw) = f32x4{0.f, 0.f, 0.f, 0.f};
  return false;
}

// one output pixel from its taps: the sample, the 16-B store; returns mx raised to the pixel's max|v|
template <typename S>
__device__ __forceinline__ float resize_pixel(const ResK<S>& p, const ResBlock& k, const typename S::Cols& cols,
                                              const Tap& tx, const Tap& ty, float* yo, float mx) {
  const f32x4 o = sample(p.s, p.s.rows(k.f, ty), cols, tx, ty, p.a, p.b);
  *reinterpret_cast<f32x4*>(yo) = o;
  return fmaxf(mx, amax3(o));
}

// the workgroup's rows of the slot's window in crop_meta: a thread owns the columns tid,
// tid + 128, ..., so a column's taps are formed once per thread and a row's once per row; returns
// the thread's max|v|
template <typename S>
__device__ __forceinline__ float resize_window(const ResK<S>& p, const ResBlock& k) {
  const double x0 = k.m[2], y0 = k.m[3], w = k.m[4], h = k.m[5];
  float mx = 0.f;
  for (int j = threadIdx.x; j < p.ow; j += RR_THREADS) {
    const Tap tx = tap(x0, w, j, p.ow, p.s.W);
    const typename S::Cols cols = p.s.cols(tx);
    float* yo = k.ybase + (int64_t)j * p.ysw;
#pragma unroll 4
    for (int r = 0; r < k.rows; ++r)
      mx = resize_pixel(p, k, cols, tx, tap(y0, h, k.i0 + r, p.oh, p.s.H), yo + (int64_t)r * p.ysh, mx);
  }
  return mx;
}

// the workgroup's rows along the affine map of the slot's warp row: both tap pairs change per
// pixel, so the column part of each coordinate is formed once per thread and the row part once per
// row; returns the thread's max|v|
template <typename S>
__device__ __forceinline__ float warp_rows(const ResK<S>& p, const ResBlock& k, const float* wr) {
  const double a = wr[2], b = wr[3], tx = wr[4], c = wr[5], d = wr[6], ty = wr[7];
  float mx = 0.f;
  for (int j = threadIdx.x; j < p.ow; j += RR_THREADS) {
    const double xc = a * (j + 0.5) + tx, yc = c * (j + 0.5) + ty;      // the column's part
    float* yo = k.ybase + (int64_t)j * p.ysw;
#pragma unroll 4
    for (int r = 0; r < k.rows; ++r) {
      const double v = (k.i0 + r) + 0.5;
      const Tap sx = tap_at(xc + b * v - 0.5, p.s.W), sy = tap_at(yc + d * v - 0.5, p.s.H);
      mx = resize_pixel(p, k, p.s.cols(sx), sx, sy, yo + (int64_t)r * p.ysh, mx);
    }
  }
  return mx;
}

template <typename S>
__global__ __launch_bounds__(RR_THREADS) void roi_resize_kernel(ResK<S> p) {
  __shared__ float wmax[RR_THREADS / 64];
  ResBlock k;
  if (!resize_block(p, k)) return;
  const float mx = resize_window(p, k);
  if (p.y_amax) block_amax<RR_THREADS>(p.y_amax + k.slot, mx, wmax);
}

// a slot whose warp row is flagged samples along the row's map, every other slot its window; the
// flag is uniform across the workgroup
template <typename S>
__global__ __launch_bounds__(RR_THREADS) void roi_warp_kernel(ResK<S> p) {
  __shared__ float wmax[RR_THREADS / 64];
  ResBlock k;
  if (!resize_block(p, k)) return;
  const float* wr = p.warp + (int64_t)k.slot * 8;
  const float mx = __float_as_int(wr[0]) == 1 ? warp_rows(p, k, wr) : resize_window(p, k);
  if (p.y_amax) block_amax<RR_THREADS>(p.y_amax + k.slot, mx, wmax);
}

// ---- host side: the checks and the launches every entry point shares; p.s is set. warp: null for
// prpe_roi_resize, which launches roi_resize_kernel; a, b: sources with the affine only
template <bool WARP, typename S>
static inline int resize_run(ResK<S>& p, const float* crop_meta, const int32_t* n_crops, int32_t max_crops,
                             const float* warp, const float* a, const float* b, const prpe_view* y, float* y_amax,
                             void* stream) {
  if (!crop_meta || !n_crops || (WARP && !warp) || (S::AFFINE && (!a || !b))) return PRPE_EINVAL;
  if (max_crops <= 0 || !nhwc4_ok(y) || y->n != max_crops || y->h > MAX_OUT || y->w > MAX_OUT) return PRPE_EINVAL;
  const int64_t blocks = (int64_t)max_crops * ((y->h + RR_ROWS - 1) / RR_ROWS);
  if (blocks >= (1LL << 31)) return PRPE_EINVAL;
  p.meta = crop_meta; p.n_crops = n_crops; p.max_crops = max_crops; p.warp = warp;
  p.y = y->ptr; p.oh = y->h; p.ow = y->w; p.ysn = y->sn; p.ysh = y->sh; p.ysw = y->sw;
  p.y_amax = y_amax;
  if (S::AFFINE)
    for (int c = 0; c < 3; ++c) { p.a[c] = a[c]; p.b[c] = b[c]; }
  if constexpr (WARP) {
    hipLaunchKernelGGL(roi_warp_kernel<S>, dim3((unsigned)blocks), dim3(RR_THREADS), 0, as_stream(stream), p);
  } else {
    hipLaunchKernelGGL(roi_resize_kernel<S>, dim3((unsigned)blocks), dim3(RR_THREADS), 0, as_stream(stream), p);
  }
  return launch_status();
}

}  // namespace roi
