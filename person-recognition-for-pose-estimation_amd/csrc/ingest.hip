// uint8 frames in, model-ready fp32 out: the stage in front of the first conv.
//
// prpe_frame_ingest   — source uint8 [B, Hs, Ws, 3] at any element strides (HWC batches, NCHW
//   through permute, slices) -> the interior [B, H, W, 4] of the stem's zero-bordered NHWC4
//   buffer: bilinear resize into the region (top, left, nh, nw), fill outside it, per-channel
//   affine, channel 3 = 0, one 16-B store per pixel, the border never addressed. The kernel is
//   frame_ingest_kernel of csrc/frames.h on the uint8 view source (prpe_frame_ingest_nv12,
//   csrc/nv12.hip, is the same kernel on NV12 planes). Per-frame max|y|: reduced over the
//   workgroup, ONE atomicMax per workgroup (a workgroup never spans two frames; copy_pad_kernel's
//   scheme, csrc/pointwise.hip).
// prpe_crop_resize_u8 — prpe_crop_resize (csrc/topdown.hip) reading uint8 frames: the same kernel
//   template on the uint8 view source, so the window arithmetic, clamp and zero taps are the same
//   statements, then the per-channel affine on every pixel of a filled slot.
//
// Loads: a pixel's taps are single bytes (12 per pixel: 4 taps x 3 channels). Neighbouring lanes
// read neighbouring bytes of the same cache lines, every source byte is fetched from HBM once,
// and the kernel's traffic is the 16 B it stores per pixel against at most 3 B it reads; wider
// loads would need an alignment the strided source does not promise (§5c has the timings).
#pragma clang fp contract(off)
#include "frames.h"

using namespace fsrc;

extern "C" int prpe_frame_ingest(const prpe_view_u8* frames, const prpe_view* y, int32_t top, int32_t left,
                                 int32_t nh, int32_t nw, const float* a, const float* b, const float* fill,
                                 int32_t swap_rb, float* y_amax, void* stream) {
  IngK<ViewSrc<uint8_t>> p{};
  if (!view_src(p.s, frames, swap_rb)) return PRPE_EINVAL;
  return frame_ingest_run(p, y, top, left, nh, nw, a, b, fill, y_amax, stream);
}

extern "C" int prpe_crop_resize_u8(const prpe_view_u8* frames, const float* crop_meta, const int32_t* n_crops,
                                   int32_t max_crops, const float* a, const float* b, int32_t swap_rb,
                                   float* crops, void* stream) {
  CropK<ViewSrc<uint8_t>> p{};
  if (!view_src(p.s, frames, swap_rb)) return PRPE_EINVAL;
  return crop_resize_run(p, crop_meta, n_crops, max_crops, a, b, crops, stream);
}
