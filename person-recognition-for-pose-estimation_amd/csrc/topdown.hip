// Top-down pose, the stage between the person detector and ViTPose:
//
// prpe_crop_select    — padded NMS output -> a compact crop list in (frame, row) order. ONE
//   256-thread workgroup: each thread counts the rows its frame contributes, a block prefix sum
//   over the frames (in chunks of 256) assigns the slots, so the list is the same on every run
//   (no atomics). Window arithmetic in fp32 with contraction off: the host restatement
//   (tests/test_topdown_host.py) gives the same bits.
// prpe_crop_resize    — the hot kernel: bilinear resample of each window to 256x192 straight into
//   the zero-bordered NHWC4 buffer the ViTPose patch embedding reads. One 192-thread workgroup per
//   (slot, 8 output rows); a thread owns one output column, so its source column, x weight and the
//   window are computed once and the row coordinate is wave-uniform. Every row is one contiguous
//   3-KiB run of 16-B stores (channel 3 is stored as the 0 it already holds); the border is never
//   addressed. Source coordinates are formed in fp64 (4 operations per thread and per row: free
//   beside the 16-B store and 12 gathered loads per pixel), so the weights carry one fp32
//   rounding; the blend itself is two fp32 lerps, v00 + ax (v01 - v00), which return c exactly
//   where all four taps are c.
// prpe_crop_keypoints — soft-argmax coordinates in [0,1] of the crop -> frame pixels.
#pragma clang fp contract(off)
#include "common.h"

namespace {

constexpr int CROP_H = 256, CROP_W = 192;      // the ViTPose input (arch.VIT_IMG)
constexpr int CROP_PAD = 2;                    // the patch conv's padding = the buffer's border
constexpr int BUF_H = CROP_H + 2 * CROP_PAD, BUF_W = CROP_W + 2 * CROP_PAD;
constexpr int CR_ROWS = 8;                     // output rows per workgroup
constexpr int SEL_THREADS = 256;
constexpr int MAX_DIM = 1 << 24;               // frame sides stay exact in fp32

__device__ __forceinline__ bool finitef(float v) { return fabsf(v) <= 3.402823466e38f; }   // false for NaN

struct SelK {
  const float* dets; const int* counts; int B, max_det;
  float thr, min_size, sx, sy, pad; int per_frame, max_crops;
  float* meta; int* n_crops; int* status;
};

// the window of detection row r of frame b, or false when the row is skipped
__device__ __forceinline__ bool crop_window(const SelK& p, const float* d, float& x0, float& y0, float& w, float& h) {
  const float x1 = d[0] * p.sx, y1 = d[1] * p.sy, x2 = d[2] * p.sx, y2 = d[3] * p.sy;
  if (!(finitef(x1) && finitef(y1) && finitef(x2) && finitef(y2))) return false;
  w = x2 - x1;
  h = y2 - y1;
  if (!(w >= p.min_size) || !(h >= p.min_size)) return false;
  const float cx = (x1 + x2) * 0.5f, cy = (y1 + y2) * 0.5f;
  const float a = (float)CROP_W / (float)CROP_H;
  if (w > a * h) h = w / a; else w = h * a;
  w *= p.pad;
  h *= p.pad;
  x0 = cx - 0.5f * w;
  y0 = cy - 0.5f * h;
  return finitef(w) && finitef(h) && finitef(x0) && finitef(y0);
}

// rows of frame b in the candidate prefix: the first rows with score >= thr, at most per_frame
__device__ __forceinline__ int crop_prefix(const SelK& p, int b) {
  int c = p.counts[b];
  c = c < p.max_det ? c : p.max_det;
  c = c < p.per_frame ? c : p.per_frame;
  int n = 0;
  while (n < c && p.dets[((int64_t)b * p.max_det + n) * 6 + 4] >= p.thr) ++n;
  return n;
}

__global__ __launch_bounds__(SEL_THREADS) void crop_select_kernel(SelK p) {
  __shared__ int scan[SEL_THREADS];
  __shared__ int base_s, flags_s;
  const int tid = threadIdx.x;
  if (tid == 0) { base_s = 0; flags_s = 0; }
  __syncthreads();
  for (int b0 = 0; b0 < p.B; b0 += SEL_THREADS) {
    const int b = b0 + tid;
    int pre = 0, cnt = 0;
    if (b < p.B) {
      if (p.counts[b] < 0) atomicOr(&flags_s, 1);          // NMS candidate overflow: nothing from b
      else pre = crop_prefix(p, b);
      float x0, y0, w, h;
      for (int r = 0; r < pre; ++r) cnt += crop_window(p, p.dets + ((int64_t)b * p.max_det + r) * 6, x0, y0, w, h);
    }
    scan[tid] = cnt;
    __syncthreads();
    for (int o = 1; o < SEL_THREADS; o <<= 1) {            // inclusive Hillis-Steele scan
      const int t = tid >= o ? scan[tid - o] : 0;
      __syncthreads();
      scan[tid] += t;
      __syncthreads();
    }
    const int base = base_s;
    int slot = base + scan[tid] - cnt;
    for (int r = 0; r < pre; ++r) {
      const float* d = p.dets + ((int64_t)b * p.max_det + r) * 6;
      float x0, y0, w, h;
      if (!crop_window(p, d, x0, y0, w, h)) continue;
      if (slot < p.max_crops) {
        float* m = p.meta + (int64_t)slot * 8;
        m[0] = __int_as_float(b); m[1] = __int_as_float(r);
        m[2] = x0; m[3] = y0; m[4] = w; m[5] = h; m[6] = d[4]; m[7] = 0.f;
      }
      ++slot;
    }
    __syncthreads();
    if (tid == SEL_THREADS - 1) base_s = base + scan[tid];
    __syncthreads();
  }
  const int total = base_s;
  const int n = total < p.max_crops ? total : p.max_crops;
  for (int s = n + tid; s < p.max_crops; s += SEL_THREADS) {
    float* m = p.meta + (int64_t)s * 8;
    m[0] = __int_as_float(-1);
#pragma unroll
    for (int q = 1; q < 8; ++q) m[q] = 0.f;
  }
  if (tid == 0) {
    *p.n_crops = n;
    *p.status = flags_s | (total > p.max_crops ? 2 : 0);
  }
}

struct ResK {
  const float* src; int B, H, W; int64_t sn, sh, sw, sc;
  const float* meta; const int* n_crops; int max_crops;
  float* out;
};

__global__ __launch_bounds__(CROP_W) void crop_resize_kernel(ResK p) {
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
  if (!dets || !counts || !crop_meta || !n_crops || !status) return PRPE_EINVAL;
  if (B <= 0 || max_det <= 0 || max_per_frame <= 0 || max_crops <= 0) return PRPE_EINVAL;
  if (H <= 0 || W <= 0 || H > MAX_DIM || W > MAX_DIM) return PRPE_EINVAL;
  if (!(pad > 0.f) || !(box_scale_x > 0.f) || !(box_scale_y > 0.f) || !(min_size >= 0.f)) return PRPE_EINVAL;
  if (!(fabsf(pad) <= 3.402823466e38f && fabsf(box_scale_x) <= 3.402823466e38f &&
        fabsf(box_scale_y) <= 3.402823466e38f) || score_thr != score_thr)
    return PRPE_EINVAL;
  if ((int64_t)B * max_det >= (1LL << 31)) return PRPE_EINVAL;
  SelK p{};
  p.dets = dets; p.counts = counts; p.B = B; p.max_det = max_det;
  p.thr = score_thr; p.min_size = min_size; p.sx = box_scale_x; p.sy = box_scale_y; p.pad = pad;
  p.per_frame = max_per_frame; p.max_crops = max_crops;
  p.meta = crop_meta; p.n_crops = n_crops; p.status = status;
  hipLaunchKernelGGL(crop_select_kernel, dim3(1), dim3(SEL_THREADS), 0, as_stream(stream), p);
  return launch_status();
}

extern "C" int prpe_crop_resize(const prpe_view* frames, const float* crop_meta, const int32_t* n_crops,
                                int32_t max_crops, float* crops, void* stream) {
  if (!frames || !frames->ptr || !crop_meta || !n_crops || !crops) return PRPE_EINVAL;
  if (frames->c != 3 || frames->n <= 0 || frames->h <= 0 || frames->w <= 0) return PRPE_EINVAL;
  if (frames->h > MAX_DIM || frames->w > MAX_DIM) return PRPE_EINVAL;
  if (max_crops <= 0 || (int64_t)max_crops * (CROP_H / CR_ROWS) >= (1LL << 31)) return PRPE_EINVAL;
  if ((uintptr_t)crops % 16) return PRPE_EINVAL;
  ResK p{};
  p.src = frames->ptr; p.B = frames->n; p.H = frames->h; p.W = frames->w;
  p.sn = frames->sn; p.sh = frames->sh; p.sw = frames->sw; p.sc = frames->sc;
  p.meta = crop_meta; p.n_crops = n_crops; p.max_crops = max_crops; p.out = crops;
  hipLaunchKernelGGL(crop_resize_kernel, dim3((unsigned)(max_crops * (CROP_H / CR_ROWS))), dim3(CROP_W), 0,
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
