// Face crops registered to the skeleton's eyes and nose:
//
// prpe_face_align_fit — one thread per person slot: the closed-form least-squares similarity (no
//   reflection) that takes the ArcFace template's eye and nose positions, scaled to the output
//   size, onto the person's COCO keypoints 2, 1, 0 (right eye, left eye, nose), in fp64, from
//   template to frame so nothing is inverted. The six coefficients go to the matched face's row of
//   ``warp`` when the gates hold; the match is one-to-one, so no two threads write one row.
// prpe_roi_warp(_u8) — prpe_roi_resize(_u8)'s launch, stores and max|y|. A slot whose warp row is
//   flagged samples the frame along the row's affine map instead of the window of crop_meta
//   (roi_warp_kernel, csrc/roi.h: one instantiation per frame source; the NV12 entry point is in
//   csrc/nv12.hip).
#pragma clang fp contract(off)
#include "roi.h"

namespace {

using namespace roi;

// the ArcFace positions of the viewer's-left eye, the viewer's-right eye and the nose in a
// 112 x 112 crop, paired with COCO keypoints 2 (right eye), 1 (left eye), 0 (nose)
constexpr double TPL = 112.0;
__device__ const double TPL_X[3] = {38.2946, 73.5318, 56.0252};
__device__ const double TPL_Y[3] = {51.6963, 51.5014, 71.7366};
__device__ const int TPL_KP[3] = {2, 1, 0};

struct FitK {
  const float* meta_f; const int* n_f; int max_f;
  const int* n_p; int max_p; const float* kpts; int K;
  const int* person_face;
  int oh, ow; float kp_thr, lo, hi;
  float* warp;
};

__global__ __launch_bounds__(64) void face_align_fit_kernel(FitK p) {
  const int s = blockIdx.x * 64 + threadIdx.x;
  int n_p = *p.n_p, n_f = *p.n_f;
  n_p = n_p < p.max_p ? n_p : p.max_p;
  n_f = n_f < p.max_f ? n_f : p.max_f;
  if (s >= n_p) return;
  const int fs = p.person_face[s];
  if (fs < 0 || fs >= n_f) return;
  double qx[3], qy[3], px[3], py[3];
  const double kx = (double)p.ow / TPL, ky = (double)p.oh / TPL;
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    const float* kp = p.kpts + ((int64_t)s * p.K + TPL_KP[i]) * 3;
    if (!(kp[2] >= p.kp_thr) || !finitef(kp[0]) || !finitef(kp[1])) return;
    px[i] = kp[0]; py[i] = kp[1];
    qx[i] = TPL_X[i] * kx; qy[i] = TPL_Y[i] * ky;
  }
  const double qmx = (qx[0] + qx[1] + qx[2]) / 3.0, qmy = (qy[0] + qy[1] + qy[2]) / 3.0;
  const double pmx = (px[0] + px[1] + px[2]) / 3.0, pmy = (py[0] + py[1] + py[2]) / 3.0;
  double D = 0.0, dot = 0.0, cross = 0.0;
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    const double ux = qx[i] - qmx, uy = qy[i] - qmy, vx = px[i] - pmx, vy = py[i] - pmy;
    D = D + (ux * ux + uy * uy);
    dot = dot + (ux * vx + uy * vy);
    cross = cross + (ux * vy - uy * vx);
  }
  const double a = dot / D, c = cross / D;
  const double tx = pmx - (a * qmx - c * qmy), ty = pmy - (c * qmx + a * qmy);
  // the stored values; the gates are taken on them, as prpe_roi_warp will read them
  const float af = (float)a, bf = (float)-c, txf = (float)tx, cf = (float)c, df = (float)a, tyf = (float)ty;
  if (!(finitef(af) && finitef(cf) && finitef(txf) && finitef(tyf))) return;
  const float* m = p.meta_f + (int64_t)fs * 8;
  const float x0 = m[2], y0 = m[3], w = m[4], h = m[5];
  const float size = (float)(sqrt((double)af * af + (double)cf * cf) * (double)p.ow);      // the crop's width in frame pixels
  if (!((double)p.lo * w <= (double)size && (double)size <= (double)p.hi * w)) return;
  const double u = 0.5 * p.ow, v = 0.5 * p.oh;
  const float cx = (float)(((double)af * u + (double)bf * v) + (double)txf);
  const float cy = (float)(((double)cf * u + (double)df * v) + (double)tyf);
  if (!(cx >= x0 && cx <= x0 + w && cy >= y0 && cy <= y0 + h)) return;
  float* o = p.warp + (int64_t)fs * 8;
  o[0] = __int_as_float(1); o[1] = __int_as_float(s);
  o[2] = af; o[3] = bf; o[4] = txf; o[5] = cf; o[6] = df; o[7] = tyf;
}

}  // namespace

extern "C" int prpe_face_align_fit(const float* crop_meta_f, const int32_t* n_f, int32_t max_f, const int32_t* n_p,
                                   int32_t max_p, const float* keypoints, int32_t K, const int32_t* person_face,
                                   int32_t out_h, int32_t out_w, float kp_thr, float scale_lo, float scale_hi,
                                   float* warp, void* stream) {
  if (!crop_meta_f || !n_f || !n_p || !keypoints || !person_face || !warp) return PRPE_EINVAL;
  if (max_f <= 0 || max_p <= 0 || K < 3 || out_h <= 0 || out_w <= 0 || out_h > MAX_OUT || out_w > MAX_OUT)
    return PRPE_EINVAL;
  if (kp_thr != kp_thr || !(scale_lo > 0.f) || !(scale_lo <= scale_hi)) return PRPE_EINVAL;
  if ((int64_t)max_p * K >= (1LL << 31) / 3) return PRPE_EINVAL;
  FitK p{};
  p.meta_f = crop_meta_f; p.n_f = n_f; p.max_f = max_f; p.n_p = n_p; p.max_p = max_p;
  p.kpts = keypoints; p.K = K; p.person_face = person_face;
  p.oh = out_h; p.ow = out_w; p.kp_thr = kp_thr; p.lo = scale_lo; p.hi = scale_hi; p.warp = warp;
  hipLaunchKernelGGL(face_align_fit_kernel, dim3((unsigned)((max_p + 63) / 64)), dim3(64), 0, as_stream(stream), p);
  return launch_status();
}

extern "C" int prpe_roi_warp(const prpe_view* frames, const float* crop_meta, const int32_t* n_crops,
                             int32_t max_crops, const float* warp, const prpe_view* y, float* y_amax, void* stream) {
  ResK<ViewSrc<float>> p{};
  if (!view_src(p.s, frames, 0)) return PRPE_EINVAL;
  return resize_run<true>(p, crop_meta, n_crops, max_crops, warp, nullptr, nullptr, y, y_amax, stream);
}

extern "C" int prpe_roi_warp_u8(const prpe_view_u8* frames, const float* crop_meta, const int32_t* n_crops,
                                int32_t max_crops, const float* warp, const float* a, const float* b,
                                int32_t swap_rb, const prpe_view* y, float* y_amax, void* stream) {
  ResK<ViewSrc<uint8_t>> p{};
  if (!view_src(p.s, frames, swap_rb)) return PRPE_EINVAL;
  return resize_run<true>(p, crop_meta, n_crops, max_crops, warp, a, b, y, y_amax, stream);
}
