// Device code shared by the kernels of csrc/roi.hip: csrc/topdown.hip's crop list
// rule and bilinear tap arithmetic with the output size as a parameter. The statements and their
// order are topdown.hip's (fp32 window with contraction off; fp64 sample coordinates, one fp32
// rounding per weight), so that at 256 x 192 the results have prpe_crop_select's and
// prpe_crop_resize's bits; topdown.hip itself keeps its own text.
#pragma once
#pragma clang fp contract(off)
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
__device__ __forceinline__ Tap tap(double origin, double extent, int idx, int out, int size) {
  const double s = fmin(fmax(origin + (idx + 0.5) * (extent / out) - 0.5, -2.0), (double)size + 1.0);
  const double f = floor(s);
  Tap t;
  t.a = (float)(s - f);
  t.ia = (int)f;
  t.ib = t.ia + 1;
  t.ina = (unsigned)t.ia < (unsigned)size;
  t.inb = (unsigned)t.ib < (unsigned)size;
  return t;
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

}  // namespace roi
