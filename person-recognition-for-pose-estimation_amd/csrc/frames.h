// Frame sources, and the two fixed-shape stages that read them.
//
// Every stage that reads frames is a bilinear resample, and every one is written once, as a
// template on its frame source S (but for the fp32 crop_resize, csrc/topdown.hip, which keeps a
// kernel of its own for its speed). A source is a small device-side type that knows where the frames
// lie and what a tap is worth:
//   S::AFFINE          whether the per-channel v * a + b follows the blend (raw uint8 values: yes)
//   int B, H, W        frames and their sides
//   S::Cols cols(x)    where the two columns of the x taps lie (formed once per output column)
//   S::Rows rows(f, y) where the two rows of the y taps lie in frame f (x, y: a Tap or an EdgeTap)
//   S::Taps taps(r, c, x, y) the sample's four taps; its channel(k) gives channel k of each, raw,
//                      as floats (a Quad); a tap outside the frame is 0 and is never loaded
// The sources: ViewSrc<float> (an fp32 view), ViewSrc<uint8_t> (a uint8 view, with swap_rb) and
// NvSrc (NV12 planes, csrc/nv12.hip). The four taps are asked for at once so that a source may share
// work between them (NvSrc: one chroma row under both taps). A new format is a new source type and
// one thin entry point per stage; no stage changes.
//
// Coordinates are fp64, each weight is rounded to fp32 once, the blend is two fp32 lerps
// v00 + ax (v01 - v00), then * a + b as a multiply and an add: contraction is off.
#pragma once
#pragma clang fp contract(off)
#include <type_traits>
#include "common.h"

namespace fsrc {

constexpr int MAX_DIM = 1 << 24;               // frame sides stay exact in fp32
constexpr int CROP_H = 256, CROP_W = 192;      // the ViTPose input (arch.VIT_IMG)
constexpr int CROP_PAD = 2;                    // the patch conv's padding = the buffer's border
constexpr int BUF_H = CROP_H + 2 * CROP_PAD, BUF_W = CROP_W + 2 * CROP_PAD;
constexpr int CR_ROWS = 8;                     // output rows per crop_resize workgroup
constexpr int ING_THREADS = 256;
constexpr int ING_ROWS = 8;                    // output rows per frame_ingest workgroup

__device__ __forceinline__ bool finitef(float v) { return fabsf(v) <= 3.402823466e38f; }   // false for NaN

// One axis of a sample: the source index pair, the weight and which taps lie inside [0, size).
struct Tap {
  float a; int ia, ib; bool ina, inb;
};
// The taps about the sample coordinate s (pixel k's centre at k), zero outside the frame (the crop
// stages). Coordinates past the frame by more than a pixel are clamped there: every tap is outside
// either way (zero), and the conversion to int stays defined for any window (NaN -> -2).
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
// The taps about s clamped into the frame before the conversion to int (frame_ingest): both are
// inside for any argument, which the type says at compile time, and ib == ia only where a == 0.
struct EdgeTap {
  float a; int ia, ib;
  static constexpr bool ina = true, inb = true;
};
__device__ __forceinline__ EdgeTap tap_edge(double s, int size) {
  s = fmin(fmax(s, 0.0), (double)(size - 1));
  const double f = floor(s);
  const int ia = (int)f;
  return EdgeTap{(float)(s - f), ia, ia + 1 < size ? ia + 1 : ia};
}

// One channel of a sample's four taps, raw, as floats: v(row)(column)
struct Quad { float v00, v01, v10, v11; };

// A strided view [B, H, W, 3] of T = float or uint8_t, strides in elements. 12 gathered loads per
// pixel; the column offsets are the caller's, formed once per column, not once per channel.
template <typename T>
struct ViewSrc {
  static constexpr bool AFFINE = std::is_same<T, uint8_t>::value;
  const T* ptr; int B, H, W; int64_t sn, sh, sw, sc;
  int swap_rb;                                 // uint8 only: channel c reads source channel 2 - c
  struct Cols { int64_t a, b; };
  struct Rows { const T *a, *b; };
  template <typename TX>
  __device__ __forceinline__ Cols cols(const TX& x) const {
    return Cols{(int64_t)(x.ina ? x.ia : 0) * sw, (int64_t)(x.inb ? x.ib : 0) * sw};
  }
  template <typename TY>
  __device__ __forceinline__ Rows rows(int f, const TY& y) const {
    const T* base = ptr + (int64_t)f * sn;
    return Rows{base + (int64_t)(y.ina ? y.ia : 0) * sh, base + (int64_t)(y.inb ? y.ib : 0) * sh};
  }
  // a view's taps are independent loads: each channel's four are taken when it is asked for
  struct Taps {
    Rows r; Cols c; bool m00, m01, m10, m11; int64_t sc; bool swap;
    __device__ __forceinline__ Quad channel(int k) const {
      const int64_t oc = (int64_t)(swap ? 2 - k : k) * sc;
      return Quad{m00 ? (float)r.a[c.a + oc] : 0.f, m01 ? (float)r.a[c.b + oc] : 0.f,
                  m10 ? (float)r.b[c.a + oc] : 0.f, m11 ? (float)r.b[c.b + oc] : 0.f};
    }
  };
  template <typename TX, typename TY>
  __device__ __forceinline__ Taps taps(const Rows& r, const Cols& c, const TX& x, const TY& y) const {
    return Taps{r, c, y.ina && x.ina, y.ina && x.inb, y.inb && x.ina, y.inb && x.inb, sc, AFFINE && swap_rb};
  }
};

// One channel of an output pixel: the two fp32 lerps v00 + ax (v01 - v00), then, for a source
// with the affine, * a + b as a multiply and an add.
template <bool AFFINE>
__device__ __forceinline__ float blend(const Quad& q, float ax, float ay, float a, float b) {
  const float top = q.v00 + ax * (q.v01 - q.v00), bot = q.v10 + ax * (q.v11 - q.v10);
  const float v = top + ay * (bot - top);
  return AFFINE ? v * a + b : v;
}
// One output pixel: the four taps, each channel blended; channel 3 is 0.
template <typename S, typename TX, typename TY>
__device__ __forceinline__ f32x4 sample(const S& s, const typename S::Rows& r, const typename S::Cols& c, const TX& x,
                                        const TY& y, const float (&a)[3], const float (&b)[3]) {
  const typename S::Taps t = s.taps(r, c, x, y);
  float v[3];
#pragma unroll
  for (int k = 0; k < 3; ++k) v[k] = blend<S::AFFINE>(t.channel(k), x.a, y.a, a[k], b[k]);
  return f32x4{v[0], v[1], v[2], 0.f};
}
__device__ __forceinline__ float amax3(f32x4 v) { return fmaxf(fmaxf(fabsf(v[0]), fabsf(v[1])), fabsf(v[2])); }

// *slot raised to the workgroup's max of m: one atomicMax on the bit pattern per workgroup (a
// workgroup never spans two slots; wmax: THREADS / 64 floats of LDS)
template <int THREADS>
__device__ __forceinline__ void block_amax(float* slot, float m, float* wmax) {
  m = warp_max(m);
  if ((threadIdx.x & 63) == 0) wmax[threadIdx.x >> 6] = m;
  __syncthreads();
  if (threadIdx.x == 0) {
#pragma unroll
    for (int w = 1; w < THREADS / 64; ++w) m = fmaxf(m, wmax[w]);
    if (m > 0.f) atomicMax(reinterpret_cast<unsigned*>(slot), __float_as_uint(m));
  }
}

// ---------------------------------------------------------------- frame_ingest
template <typename S>
struct IngK {
  S s;
  float* y; int H, W; int64_t ysn, ysh, ysw;   // float elements, each a multiple of 4
  int top, left, nh, nw;
  float a[3], b[3], fill[3];
  float* y_amax;
};

// One 256-thread workgroup per (frame, 8 output rows); a thread walks the columns tid, tid + 256,
// ..., so its x taps are formed once per column and the row's taps are wave-uniform.
template <typename S>
__global__ __launch_bounds__(ING_THREADS) void frame_ingest_kernel(IngK<S> p) {
  __shared__ float wmax[ING_THREADS / 64];
  const int bpf = (p.H + ING_ROWS - 1) / ING_ROWS;              // workgroups per frame
  const int n = blockIdx.x / bpf, i0 = (blockIdx.x - n * bpf) * ING_ROWS;
  const int rows = p.H - i0 < ING_ROWS ? p.H - i0 : ING_ROWS;
  float* ybase = p.y + (int64_t)n * p.ysn + (int64_t)i0 * p.ysh;
  const double kx = (double)p.s.W / (double)p.nw, ky = (double)p.s.H / (double)p.nh;
  float fv[3];
#pragma unroll
  for (int c = 0; c < 3; ++c) fv[c] = p.fill[c] * p.a[c] + p.b[c];
  const f32x4 fill = {fv[0], fv[1], fv[2], 0.f};
  const float fmx = amax3(fill);
  float m = 0.f;
  for (int j = threadIdx.x; j < p.W; j += ING_THREADS) {
    const bool col_in = (unsigned)(j - p.left) < (unsigned)p.nw;
    const EdgeTap tx = tap_edge(((double)(j - p.left) + 0.5) * kx - 0.5, p.s.W);
    const typename S::Cols cols = p.s.cols(tx);
    float* yo = ybase + (int64_t)j * p.ysw;
    for (int r = 0; r < rows; ++r) {
      const int i = i0 + r;
      f32x4 o = fill;
      float om = fmx;
      if (col_in && (unsigned)(i - p.top) < (unsigned)p.nh) {
        const EdgeTap ty = tap_edge(((double)(i - p.top) + 0.5) * ky - 0.5, p.s.H);
        o = sample(p.s, p.s.rows(n, ty), cols, tx, ty, p.a, p.b);
        om = amax3(o);
      }
      m = fmaxf(m, om);
      *reinterpret_cast<f32x4*>(yo + (int64_t)r * p.ysh) = o;
    }
  }
  if (p.y_amax) block_amax<ING_THREADS>(p.y_amax + n, m, wmax);
}

// ---------------------------------------------------------------- crop_resize
template <typename S>
struct CropK {
  S s;
  const float* meta; const int* n_crops; int max_crops;
  float a[3], b[3];                              // sources with the affine only
  float* out;
};

// One 192-thread workgroup per (slot, 8 output rows) of the fixed 256 x 192 crop; a thread owns one
// output column, so its x taps and the window are formed once and the row's taps are wave-uniform.
template <typename S>
__global__ __launch_bounds__(CROP_W) void crop_resize_kernel(CropK<S> p) {
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
  const Tap tx = tap(x0, w, j, CROP_W, p.s.W);
  const typename S::Cols cols = p.s.cols(tx);
#pragma unroll 4
  for (int r = 0; r < CR_ROWS; ++r) {
    const Tap ty = tap(y0, h, i0 + r, CROP_H, p.s.H);
    // sample()'s two lines, in the kernel's own body: behind a call the compiler emits this blend
    // as packed fp32 operations, and the uint8 crop of 1080p frames measured 0.3 % slower than the
    // separate kernel it replaces (DESIGN.md §5m has the table)
    const typename S::Taps t = p.s.taps(p.s.rows(f, ty), cols, tx, ty);
    float v[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) v[k] = blend<S::AFFINE>(t.channel(k), tx.a, ty.a, p.a[k], p.b[k]);
    orow[(int64_t)r * BUF_W] = f32x4{v[0], v[1], v[2], 0.f};
  }
}

// ---------------------------------------------------------------- host side
// the frames of a view as a source, or false when the call is refused
template <typename T, typename V>
static inline bool view_src(ViewSrc<T>& s, const V* f, int32_t swap_rb) {
  if (!f || !f->ptr || f->c != 3 || f->n <= 0 || f->h <= 0 || f->w <= 0 || f->h > MAX_DIM || f->w > MAX_DIM)
    return false;
  s = ViewSrc<T>{f->ptr, f->n, f->h, f->w, f->sn, f->sh, f->sw, f->sc, swap_rb ? 1 : 0};
  return true;
}

// y as an NHWC4 interior that takes one aligned 16-B store per pixel
static inline bool nhwc4_ok(const prpe_view* y) {
  return view_ok(y) && y->c == 4 && y->sc == 1 && y->sw % 4 == 0 && y->sh % 4 == 0 && y->sn % 4 == 0 &&
         (uintptr_t)y->ptr % 16 == 0;
}

// the checks and the launch every frame_ingest entry point shares; p.s is set
template <typename S>
static inline int frame_ingest_run(IngK<S>& p, const prpe_view* y, int32_t top, int32_t left, int32_t nh, int32_t nw,
                                   const float* a, const float* b, const float* fill, float* y_amax, void* stream) {
  if (!nhwc4_ok(y) || !a || !b || !fill || p.s.B != y->n) return PRPE_EINVAL;
  if (nh < 1 || nw < 1 || top < 0 || left < 0 || (int64_t)top + nh > y->h || (int64_t)left + nw > y->w)
    return PRPE_EINVAL;
  const int64_t blocks = (int64_t)y->n * ((y->h + ING_ROWS - 1) / ING_ROWS);
  if (blocks >= (1LL << 31)) return PRPE_EINVAL;
  p.y = y->ptr; p.H = y->h; p.W = y->w; p.ysn = y->sn; p.ysh = y->sh; p.ysw = y->sw;
  p.top = top; p.left = left; p.nh = nh; p.nw = nw;
  for (int c = 0; c < 3; ++c) { p.a[c] = a[c]; p.b[c] = b[c]; p.fill[c] = fill[c]; }
  p.y_amax = y_amax;
  hipLaunchKernelGGL(frame_ingest_kernel<S>, dim3((unsigned)blocks), dim3(ING_THREADS), 0, as_stream(stream), p);
  return launch_status();
}

// the same for crop_resize (a, b: sources with the affine only)
template <typename S>
static inline int crop_resize_run(CropK<S>& p, const float* crop_meta, const int32_t* n_crops, int32_t max_crops,
                                  const float* a, const float* b, float* crops, void* stream) {
  if (!crop_meta || !n_crops || !crops || (S::AFFINE && (!a || !b))) return PRPE_EINVAL;
  if (max_crops <= 0 || (int64_t)max_crops * (CROP_H / CR_ROWS) >= (1LL << 31)) return PRPE_EINVAL;
  if ((uintptr_t)crops % 16) return PRPE_EINVAL;
  p.meta = crop_meta; p.n_crops = n_crops; p.max_crops = max_crops; p.out = crops;
  if (S::AFFINE)
    for (int c = 0; c < 3; ++c) { p.a[c] = a[c]; p.b[c] = b[c]; }
  hipLaunchKernelGGL(crop_resize_kernel<S>, dim3((unsigned)(max_crops * (CROP_H / CR_ROWS))), dim3(CROP_W), 0,
                     as_stream(stream), p);
  return launch_status();
}

}  // namespace fsrc
