// Per-face identification, the stages between the face detector and the trunk, and the join of
// identities to skeletons:
//
// prpe_roi_select     — padded NMS output -> a compact crop list in (frame, row) order, the window's
//   aspect taken from the output size (prpe_crop_select, csrc/topdown.hip, is this at 256 x 192).
//   ONE 256-thread workgroup: each thread counts the rows its frame contributes, a block prefix
//   sum over the frames (in chunks of 256) assigns the slots, so the list is the same on every
//   run (no atomics). Window arithmetic in fp32 with contraction off: the host restatement
//   (tests/test_topdown_host.py) gives the same bits.
// prpe_roi_resize(_u8) — the hot kernel: bilinear resample of each window to the out_h x out_w
//   interior of any zero-bordered NHWC4 buffer (the stem's, at 112 x 112), one 16-B store per
//   pixel, with the slot's max|y| for the precision-3 stem. One 128-thread workgroup per
//   (slot, 8 output rows); a thread owns the output columns tid, tid + 128, ..., so a column's
//   source index, weight and bounds are formed once per thread and a row's once per row; the
//   window is the same for the whole workgroup. At 112 columns the two waves store 1 KiB and 768 B,
//   contiguous. The workgroup is csrc/roi.h's, one instantiation per frame source (csrc/frames.h);
//   the NV12 entry points are in csrc/nv12.hip.
// prpe_face_person_match — one wavefront per frame: head point per person, centre per face, the
//   32 x 32 cost matrix in registers (lane = face f and persons (lane >> 5) + 2 t), greedy
//   one-to-one assignment by a wave-wide minimum of (cost, person, face) keys. No workspace, no
//   atomics.
#pragma clang fp contract(off)
#include "roi.h"

namespace {

using namespace roi;

constexpr int MATCH_MAX = 32;                  // persons / faces per frame the match takes
constexpr int SEL_THREADS = 256;

struct SelK {
  const float* dets; const int* counts; int B, max_det;
  float thr, min_size, sx, sy, pad; int per_frame, max_crops;
  int out_h, out_w;
  float* meta; int* n_crops; int* status;
};

// the window of one detection row, or false when the row is skipped
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

__global__ __launch_bounds__(SEL_THREADS) void roi_select_kernel(SelK p) {
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
      else pre = prefix(p, b);
      float x0, y0, w, h;
      for (int r = 0; r < pre; ++r) cnt += window(p, p.dets + ((int64_t)b * p.max_det + r) * 6, x0, y0, w, h);
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
      if (!window(p, d, x0, y0, w, h)) continue;
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

struct MatchK {
  const float* meta_p; const int* n_p; int max_p; const float* kpts; int K;
  const float* meta_f; const int* n_f; int max_f; const int64_t* ident; const float* score;
  float kp_thr; int head_kpts, B;
  int* face_slot; int64_t* out_ident; float* out_score; int* status;
};

__device__ __forceinline__ void match_none(const MatchK& p, int s) {
  p.face_slot[s] = -1;
  p.out_ident[s] = -1;
  p.out_score[s] = -INFINITY;
}

// the slots of ``meta`` [0, n) whose frame is b, in ascending order: the first MATCH_MAX of them
// into idx, the count returned (every lane gets it)
__device__ __forceinline__ int match_collect(const float* meta, int n, int b, int* idx) {
  const int lane = threadIdx.x;
  int cnt = 0;
  for (int s0 = 0; s0 < n; s0 += 64) {
    const int s = s0 + lane;
    const bool mine = s < n && __float_as_int(meta[(int64_t)s * 8]) == b;
    const unsigned long long mask = __ballot(mine);
    const int pos = cnt + __popcll(mask & ((1ull << lane) - 1ull));
    if (mine && pos < MATCH_MAX) idx[pos] = s;
    cnt += __popcll(mask);
  }
  return cnt;
}

__global__ __launch_bounds__(64) void face_person_match_kernel(MatchK p) {
  __shared__ int idx_p[MATCH_MAX], idx_f[MATCH_MAX], got[MATCH_MAX];
  __shared__ float px0[MATCH_MAX], py0[MATCH_MAX], px1[MATCH_MAX], py1[MATCH_MAX], hx[MATCH_MAX], hy[MATCH_MAX];
  __shared__ float fx[MATCH_MAX], fy[MATCH_MAX];
  const int b = blockIdx.x, lane = threadIdx.x;
  int n_p = *p.n_p, n_f = *p.n_f;
  n_p = n_p < 0 ? 0 : (n_p < p.max_p ? n_p : p.max_p);
  n_f = n_f < 0 ? 0 : (n_f < p.max_f ? n_f : p.max_f);
  if (b == 0) {
    // person slots no frame owns (at or past n_p, or a frame index outside [0, B)): no match
    for (int s = lane; s < p.max_p; s += 64)
      if (s >= n_p || (unsigned)__float_as_int(p.meta_p[(int64_t)s * 8]) >= (unsigned)p.B) match_none(p, s);
  }
  const int np = match_collect(p.meta_p, n_p, b, idx_p);
  const int nf = match_collect(p.meta_f, n_f, b, idx_f);
  if (np > MATCH_MAX || nf > MATCH_MAX) {          // past the limit: the frame gets no matches
    for (int s = lane; s < n_p; s += 64)
      if (__float_as_int(p.meta_p[(int64_t)s * 8]) == b) match_none(p, s);
    if (lane == 0) p.status[b] = 1;
    return;
  }
  if (lane == 0) p.status[b] = 0;
  __syncthreads();
  if (lane < np) {
    const int s = idx_p[lane];
    const float* m = p.meta_p + (int64_t)s * 8;
    const float x0 = m[2], y0 = m[3], w = m[4], h = m[5];
    float sx = 0.f, sy = 0.f;
    int cnt = 0;
    for (int k = 0; k < p.head_kpts; ++k) {
      const float* kp = p.kpts + ((int64_t)s * p.K + k) * 3;
      if (kp[2] >= p.kp_thr) { sx += kp[0]; sy += kp[1]; ++cnt; }
    }
    px0[lane] = x0; py0[lane] = y0; px1[lane] = x0 + w; py1[lane] = y0 + h;
    hx[lane] = cnt ? sx / (float)cnt : x0 + 0.5f * w;
    hy[lane] = cnt ? sy / (float)cnt : y0 + 0.25f * h;
    got[lane] = -1;
  }
  if (lane < nf) {
    const float* m = p.meta_f + (int64_t)idx_f[lane] * 8;
    fx[lane] = m[2] + 0.5f * m[4];
    fy[lane] = m[3] + 0.5f * m[5];
  }
  __syncthreads();
  // lane owns face fi and the persons (lane >> 5) + 2 t: keys (cost bits, person, face), ~0 where
  // the pair is not eligible; a finite cost is >= +0, so its bit pattern orders as the value does
  const int fi = lane & 31;
  unsigned long long key[MATCH_MAX / 2];
#pragma unroll
  for (int t = 0; t < MATCH_MAX / 2; ++t) {
    const int pi = (lane >> 5) + 2 * t;
    key[t] = ~0ull;
    if (pi < np && fi < nf) {
      const float cx = fx[fi], cy = fy[fi];
      const float dx = hx[pi] - cx, dy = hy[pi] - cy;
      const float cost = dx * dx + dy * dy;
      if (cx >= px0[pi] && cx <= px1[pi] && cy >= py0[pi] && cy <= py1[pi] && finitef(cost))
        key[t] = (unsigned long long)__float_as_uint(cost) << 32 | (unsigned)(pi << 8 | fi);
    }
  }
  unsigned pm = 0, fm = 0;                         // matched persons / faces (the same in every lane)
  const int rounds = np < nf ? np : nf;
  for (int it = 0; it < rounds; ++it) {
    unsigned long long best = ~0ull;
    if (!(fm >> fi & 1u)) {
#pragma unroll
      for (int t = 0; t < MATCH_MAX / 2; ++t) {
        const int pi = (lane >> 5) + 2 * t;
        if (!(pm >> pi & 1u) && key[t] < best) best = key[t];
      }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      const unsigned long long other = __shfl_xor(best, o, 64);
      best = other < best ? other : best;
    }
    if (best == ~0ull) break;                      // no eligible pair is left
    const int pi = (int)(best >> 8 & 0xff), fj = (int)(best & 0xff);
    pm |= 1u << pi;
    fm |= 1u << fj;
    if (lane == 0) got[pi] = fj;
  }
  __syncthreads();
  if (lane < np) {
    const int s = idx_p[lane], fj = got[lane];
    if (fj < 0) {
      match_none(p, s);
    } else {
      const int fs = idx_f[fj];
      p.face_slot[s] = fs;
      p.out_ident[s] = p.ident[fs];
      p.out_score[s] = p.score[fs];
    }
  }
}

}  // namespace

extern "C" int prpe_roi_select(const float* dets, const int32_t* counts, int32_t B, int32_t max_det, float score_thr,
                               int32_t max_per_frame, float min_size, float box_scale_x, float box_scale_y,
                               int32_t H, int32_t W, float pad, int32_t out_h, int32_t out_w, int32_t max_crops,
                               float* crop_meta, int32_t* n_crops, int32_t* status, void* stream) {
  if (!dets || !counts || !crop_meta || !n_crops || !status) return PRPE_EINVAL;
  if (B <= 0 || max_det <= 0 || max_per_frame <= 0 || max_crops <= 0) return PRPE_EINVAL;
  if (H <= 0 || W <= 0 || H > MAX_DIM || W > MAX_DIM) return PRPE_EINVAL;
  if (out_h <= 0 || out_w <= 0 || out_h > MAX_OUT || out_w > MAX_OUT) return PRPE_EINVAL;
  if (!(pad > 0.f) || !(box_scale_x > 0.f) || !(box_scale_y > 0.f) || !(min_size >= 0.f)) return PRPE_EINVAL;
  if (!(fabsf(pad) <= 3.402823466e38f && fabsf(box_scale_x) <= 3.402823466e38f &&
        fabsf(box_scale_y) <= 3.402823466e38f) || score_thr != score_thr)
    return PRPE_EINVAL;
  if ((int64_t)B * max_det >= (1LL << 31)) return PRPE_EINVAL;
  SelK p{};
  p.dets = dets; p.counts = counts; p.B = B; p.max_det = max_det;
  p.thr = score_thr; p.min_size = min_size; p.sx = box_scale_x; p.sy = box_scale_y; p.pad = pad;
  p.per_frame = max_per_frame; p.max_crops = max_crops; p.out_h = out_h; p.out_w = out_w;
  p.meta = crop_meta; p.n_crops = n_crops; p.status = status;
  hipLaunchKernelGGL(roi_select_kernel, dim3(1), dim3(SEL_THREADS), 0, as_stream(stream), p);
  return launch_status();
}

extern "C" int prpe_roi_resize(const prpe_view* frames, const float* crop_meta, const int32_t* n_crops,
                               int32_t max_crops, const prpe_view* y, float* y_amax, void* stream) {
  ResK<ViewSrc<float>> p{};
  if (!view_src(p.s, frames, 0)) return PRPE_EINVAL;
  return resize_run<false>(p, crop_meta, n_crops, max_crops, nullptr, nullptr, nullptr, y, y_amax, stream);
}

extern "C" int prpe_roi_resize_u8(const prpe_view_u8* frames, const float* crop_meta, const int32_t* n_crops,
                                  int32_t max_crops, const float* a, const float* b, int32_t swap_rb,
                                  const prpe_view* y, float* y_amax, void* stream) {
  ResK<ViewSrc<uint8_t>> p{};
  if (!view_src(p.s, frames, swap_rb)) return PRPE_EINVAL;
  return resize_run<false>(p, crop_meta, n_crops, max_crops, nullptr, a, b, y, y_amax, stream);
}

extern "C" int prpe_face_person_match(const float* crop_meta_p, const int32_t* n_p, int32_t max_p,
                                      const float* keypoints, int32_t K, const float* crop_meta_f,
                                      const int32_t* n_f, int32_t max_f, const int64_t* ident, const float* score,
                                      float kp_thr, int32_t head_kpts, int32_t B, int32_t* face_slot,
                                      int64_t* person_ident, float* person_score, int32_t* status, void* stream) {
  if (!crop_meta_p || !n_p || !keypoints || !crop_meta_f || !n_f || !ident || !score) return PRPE_EINVAL;
  if (!face_slot || !person_ident || !person_score || !status) return PRPE_EINVAL;
  if (max_p <= 0 || max_f <= 0 || B <= 0 || K <= 0 || head_kpts <= 0 || head_kpts > K) return PRPE_EINVAL;
  if (kp_thr != kp_thr || (int64_t)max_p * K >= (1LL << 31) / 3) return PRPE_EINVAL;
  MatchK p{};
  p.meta_p = crop_meta_p; p.n_p = n_p; p.max_p = max_p; p.kpts = keypoints; p.K = K;
  p.meta_f = crop_meta_f; p.n_f = n_f; p.max_f = max_f; p.ident = ident; p.score = score;
  p.kp_thr = kp_thr; p.head_kpts = head_kpts; p.B = B;
  p.face_slot = face_slot; p.out_ident = person_ident; p.out_score = person_score; p.status = status;
  hipLaunchKernelGGL(face_person_match_kernel, dim3((unsigned)B), dim3(64), 0, as_stream(stream), p);
  return launch_status();
}
