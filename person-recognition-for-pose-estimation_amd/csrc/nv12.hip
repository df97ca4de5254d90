// NV12 frames in: what a hardware video decoder hands over -- a luma plane, a
// half-resolution plane of interleaved (U, V) pairs, a row pitch wider than the picture -- read by
// the stages that gather the taps anyway, so that no RGB copy of the frames ever exists.
//
// The conversion is one integer rule (include/prpe.h): chroma replicated, pixel (i, j) takes the
// pair (i >> 1, j >> 1); R, G, B = clamp((cy (Y - y_off) + chroma term + 128) >> 8, 0, 255) with the
// three chroma terms crv E, -cgu D - cgv E, cbu D formed once per pair. A converted tap is a uint8
// value, so every fused stage has the bits of its _u8 twin (csrc/ingest.hip, csrc/roi.hip,
// csrc/facealign.hip) run on the frames prpe_nv12_to_rgb writes: both are the same kernel template
// (csrc/frames.h, csrc/roi.h), here instantiated on the NV12 frame source NvSrc.
//
// prpe_nv12_to_rgb       — the unfused route. A thread owns 2 rows x 8 pixels: its 4 chroma pairs
//   arrive in one 8-byte load and are turned into their three terms once for the four pixels each
//   covers, each luma row is one 8-byte load, each output row three 8-byte stores (24 B). A lane's
//   neighbour owns the next 8 pixels, so a wave reads 512 B of each luma row and writes 1536 B of
//   each output row, contiguous. The 8-byte paths need 8-byte aligned planes and pitches (a
//   decoder's are); otherwise, and for the last partial block of a row, bytes and pairs one by one.
//   Nothing between w and the pitch is loaded: a wide load is taken only for a full block.
// NvSrc                  — a tap is a luma byte and the (U, V) pair over it, converted. The four taps
//   of a sample come at once: in frame_ingest, whose row pair (ya, yb) is wave-uniform and inside
//   the frame, the two pairs of the second row are neither loaded nor converted again when both
//   rows share a chroma row (ya even, or the clamped last row): a uniform branch. The two x taps
//   differ per lane; both pairs are always loaded (the same 2 bytes when xa is even). In the crop
//   stages a tap outside the frame is raw 0 in all three channels and is never loaded, as for the
//   view sources.
#pragma clang fp contract(off)
#include "roi.h"

namespace {

using namespace roi;

constexpr int CVT_PIX = 8;                     // pixels per thread and row of nv12_to_rgb
constexpr int CVT_COLS = 64, CVT_PAIRS = 4;    // a workgroup: 64 blocks of 8 pixels x 4 row pairs
constexpr int CVT_THREADS = CVT_COLS * CVT_PAIRS;

// the NV12 frame source (csrc/frames.h)
struct NvSrc {
  static constexpr bool AFFINE = true;
  const uint8_t* y; const uint8_t* uv;
  int B, H, W;
  int64_t ysn, ysh, uvsn, uvsh;                // bytes
  int y_off, cy, crv, cgu, cgv, cbu;
  struct Cols { int a, b; };
  struct Taps {                                // converted when made: a pair serves three channels
    float v[4][3];
    __device__ __forceinline__ Quad channel(int k) const { return Quad{v[0][k], v[1][k], v[2][k], v[3][k]}; }
  };
  struct Rows { const uint8_t *la, *lb, *ca, *cb; };   // luma and chroma rows (row 0 where a tap is outside)
  template <typename TX>
  __device__ __forceinline__ Cols cols(const TX& x) const { return Cols{x.ina ? x.ia : 0, x.inb ? x.ib : 0}; }
  template <typename TY>
  __device__ __forceinline__ Rows rows(int f, const TY& t) const {
    const uint8_t* l = y + (int64_t)f * ysn;
    const uint8_t* c = uv + (int64_t)f * uvsn;
    const int ia = t.ina ? t.ia : 0, ib = t.inb ? t.ib : 0;
    return Rows{l + (int64_t)ia * ysh, l + (int64_t)ib * ysh, c + (int64_t)(ia >> 1) * uvsh,
                c + (int64_t)(ib >> 1) * uvsh};
  }
  template <typename TX, typename TY>
  __device__ __forceinline__ Taps taps(const Rows& r, const Cols& c, const TX& x, const TY& t) const;
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

// ---------------------------------------------------------------- NvSrc::taps
// a luma byte and its pair's terms, converted
__device__ __forceinline__ void rgb_f(const NvSrc& s, int Y, const Chroma& k, float (&v)[3]) {
  int t[3];
  rgb_of(s, Y, k, t);
  v[0] = (float)t[0]; v[1] = (float)t[1]; v[2] = (float)t[2];
}
// one tap of a crop stage: raw 0 in all three channels outside the frame, never loaded there
__device__ __forceinline__ void tap_rgb(const NvSrc& s, const uint8_t* lrow, const uint8_t* crow, int x, bool in,
                                        float (&v)[3]) {
  v[0] = v[1] = v[2] = 0.f;
  if (in) rgb_f(s, lrow[x], chroma_at(s, crow, x), v);
}

template <typename TX, typename TY>
__device__ __forceinline__ NvSrc::Taps NvSrc::taps(const Rows& r, const Cols& c, const TX& x, const TY& t) const {
  Taps q;
  if constexpr (std::is_same<TX, EdgeTap>::value && std::is_same<TY, EdgeTap>::value) {
    // frame_ingest: every tap is inside and the row pair is wave-uniform, so when both rows lie
    // under one chroma row the second row's pairs are neither loaded nor converted again
    const Chroma a0 = chroma_at(*this, r.ca, c.a), a1 = chroma_at(*this, r.ca, c.b);
    Chroma b0 = a0, b1 = a1;
    if (r.cb != r.ca) {                          // equal pointers: the same pairs (uv_sh >= 2)
      b0 = chroma_at(*this, r.cb, c.a);
      b1 = chroma_at(*this, r.cb, c.b);
    }
    rgb_f(*this, r.la[c.a], a0, q.v[0]);
    rgb_f(*this, r.la[c.b], a1, q.v[1]);
    rgb_f(*this, r.lb[c.a], b0, q.v[2]);
    rgb_f(*this, r.lb[c.b], b1, q.v[3]);
  } else {
    tap_rgb(*this, r.la, r.ca, c.a, t.ina && x.ina, q.v[0]);
    tap_rgb(*this, r.la, r.ca, c.b, t.ina && x.inb, q.v[1]);
    tap_rgb(*this, r.lb, r.cb, c.a, t.inb && x.ina, q.v[2]);
    tap_rgb(*this, r.lb, r.cb, c.b, t.inb && x.inb, q.v[3]);
  }
  return q;
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
  IngK<NvSrc> p{};
  if (!nv_args(p.s, src, coef)) return PRPE_EINVAL;
  return frame_ingest_run(p, y, top, left, nh, nw, a, b, fill, y_amax, stream);
}

extern "C" int prpe_crop_resize_nv12(const prpe_nv12* src, const int32_t* coef, const float* crop_meta,
                                     const int32_t* n_crops, int32_t max_crops, const float* a, const float* b,
                                     float* crops, void* stream) {
  CropK<NvSrc> p{};
  if (!nv_args(p.s, src, coef)) return PRPE_EINVAL;
  return crop_resize_run(p, crop_meta, n_crops, max_crops, a, b, crops, stream);
}

extern "C" int prpe_roi_resize_nv12(const prpe_nv12* src, const int32_t* coef, const float* crop_meta,
                                    const int32_t* n_crops, int32_t max_crops, const prpe_view* y, const float* a,
                                    const float* b, float* y_amax, void* stream) {
  ResK<NvSrc> p{};
  if (!nv_args(p.s, src, coef)) return PRPE_EINVAL;
  return resize_run<false>(p, crop_meta, n_crops, max_crops, nullptr, a, b, y, y_amax, stream);
}

extern "C" int prpe_roi_warp_nv12(const prpe_nv12* src, const int32_t* coef, const float* crop_meta,
                                  const int32_t* n_crops, int32_t max_crops, const float* warp, const prpe_view* y,
                                  const float* a, const float* b, float* y_amax, void* stream) {
  ResK<NvSrc> p{};
  if (!nv_args(p.s, src, coef)) return PRPE_EINVAL;
  return resize_run<true>(p, crop_meta, n_crops, max_crops, warp, a, b, y, y_amax, stream);
}
