// Top-down pose, the stage between the person detector and ViTPose:
//
// prpe_crop_select    — padded NMS output -> a compact crop list in (frame, row) order: the select
//   kernel of csrc/roi.hip at the output size 256 x 192 (prpe_roi_select describes it).
// prpe_crop_resize    — the hot kernel: bilinear resample of each window to 256x192 straight into
//   the zero-bordered NHWC4 buffer the ViTPose patch embedding reads (prpe_crop_resize_u8,
//   csrc/ingest.hip, and prpe_crop_resize_nv12, csrc/nv12.hip, are crop_resize_kernel of
//   csrc/frames.h on their sources, with this launch shape and these statements). One
//   192-thread workgroup per (slot, 8 output rows); a thread owns one output column, so its source
//   column, x weight and the window are computed once and the row coordinate is wave-uniform.
//   Every row is one contiguous 3-KiB run of 16-B stores (channel 3 is stored as the 0 it already
//   holds); the border is never addressed. Source coordinates are formed in fp64 (4 operations
//   per thread and per row: free beside the 16-B store and 12 gathered loads per pixel), so the
//   weights carry one fp32 rounding; the blend itself is two fp32 lerps, v00 + ax (v01 - v00),
//   which return c exactly where all four taps are c.
// prpe_crop_keypoints — soft-argmax coordinates in [0,1] of the crop -> frame pixels.
#pragma clang fp contract(off)
#include "frames.h"

namespace {

using namespace fsrc;

// prpe_crop_resize keeps a kernel of its own: fsrc::crop_resize_kernel<ViewSrc<float>> has the
// same loop, instruction for instruction, but ran 1.8 % slower on 1080p frames, so
// the fp32 stage stays on this text. The statements are tap(), ViewSrc::taps and blend() of
// csrc/frames.h written out; tests/test_gpu_ingest.py holds it to the uint8 instantiation's bits.
struct CropF32K {
  const float* src; int B, H, W; int64_t sn, sh, sw, sc;
  const float* meta; const int* n_crops; int max_crops;
  float* out;
};

__global__ __launch_bounds__(CROP_W) void crop_resize_f32_kernel(CropF32K p) {
  const int slot = blockIdx.x / (CROP_H / CR_ROWS);
  const int i0 = (blockIdx.x % (CROP_H / CR_ROWS)) * CR_ROWS;
  const int j = threadIdx.x;
  f32x4* orow = reinterpret_cast<f32x4*>(p.out) + ((int64_t)slot * BUF_H + CROP_PAD + i0) * BUF_W + CROP_PAD + j;
  int n = *p.n_crops;
  n = n < p.max_crops ? n : p.max_crops;
  const float* m = p.meta + (int64_t)slot * 8;
  const int f = slot < n ? __float_as_int(m[0]) : -1;
  if ((unsigned)f >= (unsigned)p.B) {              // empty slot (or a frame index that is none): zeros
#pragma unroll
    for (int r = 0; r < CR_ROWS; ++r) orow[(int64_t)r * BUF_W] = f32x4{0.f, 0.f, 0.f, 0.f};
    return;
  }
  const double x0 = m[2], y0 = m[3], w = m[4], h = m[5];
  // coordinates past the frame by more than a pixel are clamped there: every tap is outside either
  // way (zero), and the conversion to int stays defined for any window (NaN -> -2)
  const double sx = fmin(fmax(x0 + (j + 0.5) * (w / CROP_W) - 0.5, -2.0), (double)p.W + 1.0);
  const double fx = floor(sx);
  const float ax = (float)(sx - fx);
  const int xa = (int)fx, xb = xa + 1;
  const bool ina = (unsigned)xa < (unsigned)p.W, inb = (unsigned)xb < (unsigned)p.W;
  const float* base = p.src + (int64_t)f * p.sn;
  const int64_t oa = (int64_t)(ina ? xa : 0) * p.sw, ob = (int64_t)(inb ? xb : 0) * p.sw;
#pragma unroll 4
  for (int r = 0; r < CR_ROWS; ++r) {
    const double sy = fmin(fmax(y0 + (i0 + r + 0.5) * (h / CROP_H) - 0.5, -2.0), (double)p.H + 1.0);
    const double fy = floor(sy);
    const float ay = (float)(sy - fy);
    const int ya = (int)fy, yb = ya + 1;
    const bool rowa = (unsigned)ya < (unsigned)p.H, rowb = (unsigned)yb < (unsigned)p.H;
    const float* ra = base + (int64_t)(rowa ? ya : 0) * p.sh;
    const float* rb = base + (int64_t)(rowb ? yb : 0) * p.sh;
    float v[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const int64_t oc = (int64_t)c * p.sc;
      const float v00 = rowa && ina ? ra[oa + oc] : 0.f, v01 = rowa && inb ? ra[ob + oc] : 0.f;
      const float v10 = rowb && ina ? rb[oa + oc] : 0.f, v11 = rowb && inb ? rb[ob + oc] : 0.f;
      const float top = v00 + ax * (v01 - v00), bot = v10 + ax * (v11 - v10);
      v[c] = top + ay * (bot - top);
    }
    orow[(int64_t)r * BUF_W] = f32x4{v[0], v[1], v[2], 0.f};
  }
}

struct KptK {
  const float* coords; const float* scores; int n, K;
  const float* meta; const int* n_crops; int max_crops;
  float* kpts;
};

__global__ __launch_bounds__(256) void crop_keypoints_kernel(KptK p) {
  const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (t >= (int64_t)p.max_crops * p.K) return;
  const int slot = (int)(t / p.K);
  int n = *p.n_crops;
  n = n < p.max_crops ? n : p.max_crops;
  n = n < p.n ? n : p.n;
  float x = 0.f, y = 0.f, s = 0.f;
  if (slot < n) {
    const float* m = p.meta + (int64_t)slot * 8;
    x = m[2] + p.coords[t * 2] * m[4];              // a product, then a sum: two roundings
    y = m[3] + p.coords[t * 2 + 1] * m[5];
    s = p.scores[t];
  }
  float* o = p.kpts + t * 3;
  o[0] = x; o[1] = y; o[2] = s;
}

}  // namespace

extern "C" int prpe_crop_select(const float* dets, const int32_t* counts, int32_t B, int32_t max_det, float score_thr,
                                int32_t max_per_frame, float min_size, float box_scale_x, float box_scale_y,
                                int32_t H, int32_t W, float pad, int32_t max_crops, float* crop_meta,
                                int32_t* n_crops, int32_t* status, void* stream) {
  // the one select kernel (csrc/roi.hip), the window's aspect from the fixed output size; every
  // refusal is prpe_roi_select's (its output-size check always passes here), now and later
  return prpe_roi_select(dets, counts, B, max_det, score_thr, max_per_frame, min_size, box_scale_x, box_scale_y, H, W,
                         pad, CROP_H, CROP_W, max_crops, crop_meta, n_crops, status, stream);
}

extern "C" int prpe_crop_resize(const prpe_view* frames, const float* crop_meta, const int32_t* n_crops,
                                int32_t max_crops, float* crops, void* stream) {
  ViewSrc<float> v;
  if (!view_src(v, frames, 0) || !crop_meta || !n_crops || !crops) return PRPE_EINVAL;
  if (max_crops <= 0 || (int64_t)max_crops * (CROP_H / CR_ROWS) >= (1LL << 31)) return PRPE_EINVAL;
  if ((uintptr_t)crops % 16) return PRPE_EINVAL;
  CropF32K p{};
  p.src = v.ptr; p.B = v.B; p.H = v.H; p.W = v.W; p.sn = v.sn; p.sh = v.sh; p.sw = v.sw; p.sc = v.sc;
  p.meta = crop_meta; p.n_crops = n_crops; p.max_crops = max_crops; p.out = crops;
  hipLaunchKernelGGL(crop_resize_f32_kernel, dim3((unsigned)(max_crops * (CROP_H / CR_ROWS))), dim3(CROP_W), 0,
                     as_stream(stream), p);
  return launch_status();
}

extern "C" int prpe_crop_keypoints(const float* coords, const float* scores, int32_t n, int32_t K,
                                   const float* crop_meta, const int32_t* n_crops, int32_t max_crops, float* kpts,
                                   void* stream) {
  if (!coords || !scores || !crop_meta || !n_crops || !kpts) return PRPE_EINVAL;
  if (n <= 0 || K <= 0 || max_crops <= 0 || n > max_crops) return PRPE_EINVAL;
  const int64_t total = (int64_t)max_crops * K;
  if (total >= (1LL << 31) - 256) return PRPE_EINVAL;
  KptK p{};
  p.coords = coords; p.scores = scores; p.n = n; p.K = K;
  p.meta = crop_meta; p.n_crops = n_crops; p.max_crops = max_crops; p.kpts = kpts;
  hipLaunchKernelGGL(crop_keypoints_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, as_stream(stream), p);
  return launch_status();
}
