// Pose validation step after the model (PoseEstimationModule.validation_step,
// training/lightning/pose_estimation/module.py:451-570).
//   pose_eval_kernel    : one 256-thread workgroup per (frame, keypoint). One read of the
//                         prediction (heat, or the flip-test average formed in registers with
//                         flip_average_kernel's indexing) feeds three results:
//                           - the target of _generate_target_heatmap (:298-380) rebuilt per pixel
//                             from the keypoints (never stored unless target_out is given),
//                           - JointsMSELoss's per-keypoint term (:76-88),
//                           - softargmax_kernel's coords / scores / argmax (same arithmetic and
//                             reduction order: bit-identical to prpe_softargmax on the average).
//                         Up to 16 pixels per thread (H*W <= 4096, ViTPose's 64x48 = 12) stay in
//                         registers between the passes; a larger map re-reads the prediction and
//                         recomputes the Gaussians (same values: the bits do not depend on it).
//   pose_ohkm_kernel    : OHKM (:92-107): per frame the sum of the topk largest per-keypoint
//                         losses, then over frames in a fixed order. No atomics.
//   pose_records_kernel : the COCO record loop (:505-561), one wavefront per image; a record's slot
//                         is the counter plus the counts of the images before it, which every
//                         workgroup sums itself (B*N bytes from L2), so the order is (image,
//                         instance) without a workspace. pose_records_count_kernel then advances
//                         the counter. The host's keep flags travel as a bitmask in the kernel
//                         arguments (no upload): 8192 images per launch pair, more in turn.
// FP contraction is off in this file: every product and sum rounds as the reference's does.
#pragma clang fp contract(off)
#include "common.h"

namespace {

constexpr int PE_MAX_K = 64;
constexpr int PE_MAX_N = 256;     // instances per frame: one setup thread each
constexpr int PE_THREADS = 256;
constexpr int PE_PER = 16;        // pixels per thread held in registers (H*W <= 4096)

struct PoseEvalK {
  const float* heat; const float* flip; float* avg_out;
  const float* kp; const float* areas; const float* boxes;
  float* per_kp; float* coords; float* scores; int* argmax; float* target_out; float* weights_out;
  int B, N, K, H, W, mode;
  float sigma;
  int partner[PE_MAX_K];
  float kpw[PE_MAX_K];
};

template <bool REG>
__global__ __launch_bounds__(PE_THREADS) void pose_eval_kernel(PoseEvalK p) {
  const int bk = blockIdx.x;
  const int b = bk / p.K, k = bk % p.K;
  const int W = p.W, HW = p.H * p.W;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  __shared__ float s_mx[PE_MAX_N], s_my[PE_MAX_N], s_den[PE_MAX_N];
  __shared__ int s_act[PE_MAX_N];
  __shared__ float rm[4], rw[4], rs[4][3];
  __shared__ int ri[4];
  __shared__ double rg[4], rl[4];

  // ---- instances of frame b: centre, 2 sigma_n^2, whether it draws keypoint k, its weight
  float wc = 0.f;
  if (tid < p.N) {
    const float* kpn = p.kp + ((int64_t)b * p.N + tid) * p.K * 3;
    bool any = false;
    for (int j = 0; j < p.K; ++j) any |= kpn[j * 3 + 2] > 0.f;
    const float vis = kpn[k * 3 + 2];
    if (any) wc = vis == 2.f ? 1.f : 0.5f;        // a skipped instance adds no weight (:348-350)
    const float mx = kpn[k * 3] * (float)W - 0.5f, my = kpn[k * 3 + 1] * (float)p.H - 0.5f;
    s_mx[tid] = mx;
    s_my[tid] = my;
    float sg = p.sigma;
    if (p.areas) {
      float w = sqrtf(p.areas[(int64_t)b * p.N + tid]) / 96.f;
      w = w < 0.5f ? 0.5f : (w > 2.f ? 2.f : w);
      sg = p.sigma * w;
    }
    const float den = 2.f * (sg * sg);
    s_den[tid] = den;
    // 1: draws keypoint k. The reference multiplies the Gaussian of a keypoint it does not draw by
    // a mask of 0 (:361-363), and NaN * 0 is NaN: a processed instance with a NaN sigma (a
    // negative area) or a NaN centre wipes the map of such a keypoint too. 2: masked, but the
    // Gaussian may not be a number (anything but a finite centre over a finite positive 2 sigma^2)
    const bool plain = den > 0.f && den <= 3.402823466e38f && fabsf(mx) <= 3.402823466e38f &&
                       fabsf(my) <= 3.402823466e38f;
    s_act[tid] = !any ? 0 : (vis > 0.f ? 1 : (plain ? 0 : 2));
  }
  wc = warp_max(wc);
  if (lane == 0) rw[wave] = wc;

  // ---- the prediction: heat, or the flip-test average (flip_average_kernel's indexing)
  const float* src = p.heat + (int64_t)bk * HW;
  const float* fs = nullptr;
  if (p.flip) {
    int b2 = b, k2 = k;
    const int pk = p.partner[k];
    if (pk >= 0) {
      if (p.mode == 0) b2 = p.B - 1 - b;
      else k2 = pk;
    }
    fs = p.flip + ((int64_t)b2 * p.K + k2) * HW;
  }
  float* avg = p.avg_out ? p.avg_out + (int64_t)bk * HW : nullptr;
  auto load_pred = [&](int i) {
    float v = src[i];
    if (fs) {
      const int h = i / W, w = i - h * W;
      v = (v + fs[h * W + (W - 1 - w)]) * 0.5f;
    }
    return v;
  };
  // pred again after the first pass (large maps only): avg_out may alias heat, so read what
  // this thread stored there
  auto reload_pred = [&](int i) { return avg ? avg[i] : load_pred(i); };
  __syncthreads();                                  // s_* and rw are written
  auto gauss = [&](int i) {
    const float fx = (float)(i % W), fy = (float)(i / W);
    float t = 0.f;
    for (int n = 0; n < p.N; ++n) {
      if (!s_act[n]) continue;
      const float dx = fx - s_mx[n], dy = fy - s_my[n];
      float g = expf(-(dx * dx + dy * dy) / s_den[n]);
      if (s_act[n] == 2) g *= 0.f;                  // the mask of a keypoint that is not drawn: 0, or NaN
      if (g > t || g != g) t = g;                   // torch.maximum: NaN propagates
    }
    return t;
  };

  // ---- pass 1: load, argmax (softargmax_kernel's order), unnormalised target and its sum
  float v[PE_PER], g[PE_PER];
  float m = -INFINITY;
  int mi = 0x7fffffff;
  double gs = 0.0;
  if constexpr (REG) {
#pragma unroll
    for (int j = 0; j < PE_PER; ++j) {
      const int i = tid + j * PE_THREADS;
      v[j] = 0.f; g[j] = 0.f;
      if (i < HW) {
        v[j] = load_pred(i);
        if (avg) avg[i] = v[j];
        if (v[j] > m || (v[j] == m && i < mi)) { m = v[j]; mi = i; }
        g[j] = gauss(i);
        gs += (double)g[j];
      }
    }
  } else {
    for (int i = tid; i < HW; i += PE_THREADS) {
      const float x = load_pred(i);
      if (avg) avg[i] = x;
      if (x > m || (x == m && i < mi)) { m = x; mi = i; }
      gs += (double)gauss(i);
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const float om = __shfl_xor(m, o, 64);
    const int oi = __shfl_xor(mi, o, 64);
    if (om > m || (om == m && oi < mi)) { m = om; mi = oi; }
  }
  gs = warp_sum_d(gs);
  if (lane == 0) { rm[wave] = m; ri[wave] = mi; rg[wave] = gs; }
  __syncthreads();
  m = rm[0]; mi = ri[0];
  for (int w = 1; w < 4; ++w)
    if (rm[w] > m || (rm[w] == m && ri[w] < mi)) { m = rm[w]; mi = ri[w]; }
  // heatmaps / (heatmaps.sum((2, 3)) + 1e-8) (:375): the sum is exact to fp32 rounding here
  const float den = (float)((rg[0] + rg[1]) + (rg[2] + rg[3])) + 1e-8f;

  // ---- pass 2: soft-argmax sums (softargmax_kernel's arithmetic) and the squared error
  float se = 0.f, sx = 0.f, sy = 0.f;
  double ls = 0.0;
  float* tout = p.target_out ? p.target_out + (int64_t)bk * HW : nullptr;
  auto accumulate = [&](int i, float x, float gi) {
    const float e = expf(x - m);
    se += e;
    sx += e * (float)(i % W);
    sy += e * (float)(i / W);
    float t = gi / den;
    t = t > 0.005f ? t : 0.f;                       // :378 (a NaN becomes 0 there too)
    if (tout) tout[i] = t;
    const double d = (double)x - (double)t;
    ls += d * d;
  };
  if constexpr (REG) {
#pragma unroll
    for (int j = 0; j < PE_PER; ++j) {
      const int i = tid + j * PE_THREADS;
      if (i < HW) accumulate(i, v[j], g[j]);
    }
  } else {
    for (int i = tid; i < HW; i += PE_THREADS) accumulate(i, reload_pred(i), gauss(i));
  }
  se = warp_sum(se); sx = warp_sum(sx); sy = warp_sum(sy);
  ls = warp_sum_d(ls);
  if (lane == 0) { rs[wave][0] = se; rs[wave][1] = sx; rs[wave][2] = sy; rl[wave] = ls; }
  __syncthreads();
  if (tid == 0) {
    const float S = (rs[0][0] + rs[1][0]) + (rs[2][0] + rs[3][0]);
    const float X = (rs[0][1] + rs[1][1]) + (rs[2][1] + rs[3][1]);
    const float Y = (rs[0][2] + rs[1][2]) + (rs[2][2] + rs[3][2]);
    const float cx = (X / S + 0.5f) / (float)W;
    const float cy = (Y / S + 0.5f) / (float)p.H;
    float sc = 1.f / S;   // max prob = exp(0)/sum
    if (p.boxes) {
      const float* bx = p.boxes + (int64_t)b * p.N * 4;       // boxes[:, 0] (:501)
      const float area = (bx[2] - bx[0]) * (bx[3] - bx[1]);
      float w = sqrtf(area) / 96.f;
      w = w < 0.5f ? 0.5f : (w > 2.f ? 2.f : w);
      sc = sc * w;
    }
    p.coords[(int64_t)bk * 2] = cx;
    p.coords[(int64_t)bk * 2 + 1] = cy;
    p.scores[bk] = sc;
    if (p.argmax) p.argmax[bk] = mi;
    const float wgt = fmaxf(fmaxf(rw[0], rw[1]), fmaxf(rw[2], rw[3]));
    if (p.weights_out) p.weights_out[bk] = wgt;
    const double mse = ((rl[0] + rl[1]) + (rl[2] + rl[3])) / (double)HW;
    p.per_kp[bk] = (float)(mse * (double)wgt * (double)p.kpw[k]);
  }
}

// torch.topk's order: NaN above every number
__device__ __forceinline__ bool topk_before(float a, int ia, float c, int ic) {
  const bool an = a != a, cn = c != c;
  if (an || cn) return an && (!cn || ia < ic);
  return a > c || (a == c && ia < ic);
}

// loss[0] = sum_b (sum of the topk largest of per_kp[b, :K]) / (B * topk). Wave w takes frames
// w, w+4, ...: lane k ranks its value among the K (ties by index), the selected ones are summed
// by the wave's fixed tree in double; lane 0 adds the frames in order, thread 0 the four waves.
__global__ __launch_bounds__(256) void pose_ohkm_kernel(const float* per_kp, int B, int K, int topk, float* loss) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  __shared__ double red[4];
  double acc = 0.0;
  for (int b = wave; b < B; b += 4) {
    const float x = lane < K ? per_kp[(int64_t)b * K + lane] : 0.f;
    int rank = 0;
    for (int j = 0; j < K; ++j) {
      const float y = __shfl(x, j, 64);
      rank += (j != lane && topk_before(y, j, x, lane)) ? 1 : 0;
    }
    acc += warp_sum_d((lane < K && rank < topk) ? (double)x : 0.0);
  }
  if (lane == 0) red[wave] = acc;
  __syncthreads();
  if (threadIdx.x == 0) loss[0] = (float)(((red[0] + red[1]) + (red[2] + red[3])) / ((double)B * (double)topk));
}

constexpr int PR_CHUNK = 8192;    // images per launch: their keep flags as 256 words of kernel arguments

// all pointers and slot_base are those of the launch's first image; B = images of the launch
struct PoseRecK {
  const float* coords; const float* scores; const float* boxes; const float* areas;
  const uint8_t* masks; const uint8_t* crowd;
  unsigned keep[PR_CHUNK / 32];
  int B, N, K, slot_base;
  double thresh;
  unsigned long long* counter;
  float* kpts; float* meta;
  int64_t cap;
};

// instances image j tries: range(masks[j].sum()) (:516)
__device__ __forceinline__ int rec_limit(const PoseRecK& p, int j) {
  if (!((p.keep[j >> 5] >> (j & 31)) & 1u)) return 0;
  const uint8_t* mk = p.masks + (int64_t)j * p.N;
  int lim = 0;
  for (int n = 0; n < p.N; ++n) lim += mk[n] != 0;
  return lim;
}
// records image j appends: those of them that are no crowd (:517)
__device__ __forceinline__ int rec_count(const PoseRecK& p, int j) {
  const int lim = rec_limit(p, j);
  const uint8_t* cr = p.crowd + (int64_t)j * p.N;
  int c = 0;
  for (int n = 0; n < lim; ++n) c += cr[n] == 0;
  return c;
}
__device__ __forceinline__ int warp_sum_i(int v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// one wavefront per image; lane k is keypoint k
__global__ __launch_bounds__(64) void pose_records_kernel(PoseRecK p) {
  const int b = blockIdx.x, lane = threadIdx.x;
  const int lim = rec_limit(p, b);
  if (lim == 0) return;
  int64_t before = 0;
  for (int j0 = 0; j0 < b; j0 += 64) {
    const int j = j0 + lane;
    before += warp_sum_i(j < b ? rec_count(p, j) : 0);
  }
  int64_t r = (int64_t)*p.counter + before;
  const bool has_k = lane < p.K;
  const float kx = has_k ? p.coords[((int64_t)b * p.K + lane) * 2] : 0.f;
  const float ky = has_k ? p.coords[((int64_t)b * p.K + lane) * 2 + 1] : 0.f;
  const float sc = has_k ? p.scores[(int64_t)b * p.K + lane] : 0.f;
  const float vis = (double)sc > p.thresh ? 2.f : 1.f;       // score.item() > keypoint_thresh (:545)
  const float mean = (float)(warp_sum_d(has_k ? (double)sc : 0.0) / (double)p.K);
  for (int n = 0; n < lim; ++n) {
    if (p.crowd[(int64_t)b * p.N + n]) continue;
    if (r < p.cap) {
      const float* bx = p.boxes + ((int64_t)b * p.N + n) * 4;
      const float x1 = bx[0], y1 = bx[1], x2 = bx[2], y2 = bx[3];
      if (has_k) {
        float* o = p.kpts + (r * p.K + lane) * 3;
        o[0] = kx * (x2 - x1) + x1;                 // two roundings (:543-544); contraction is off
        o[1] = ky * (y2 - y1) + y1;
        o[2] = vis;
      }
      if (lane < 8) {
        float mv;
        switch (lane) {
          case 0: mv = __int_as_float(p.slot_base + b); break;
          case 1: mv = __int_as_float(n); break;
          case 2: mv = mean; break;
          case 3: mv = x1; break;
          case 4: mv = y1; break;
          case 5: mv = x2; break;
          case 6: mv = y2; break;
          default: mv = p.areas[(int64_t)b * p.N + n]; break;
        }
        p.meta[r * 8 + lane] = mv;
      }
    }
    ++r;
  }
}

// counter += records of the batch (after pose_records_kernel in stream order: every workgroup
// of it read the old value)
__global__ __launch_bounds__(256) void pose_records_count_kernel(PoseRecK p) {
  __shared__ int red[4];
  int c = 0;
  for (int j = threadIdx.x; j < p.B; j += 256) c += rec_count(p, j);
  c = warp_sum_i(c);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = c;
  __syncthreads();
  if (threadIdx.x == 0) *p.counter += (unsigned long long)(red[0] + red[1] + red[2] + red[3]);
}

}  // namespace

extern "C" int prpe_pose_eval_loss(const float* heat, const float* heat_flipped, const int32_t* partner, int32_t mode,
                                   float* avg_out, int32_t B, int32_t K, int32_t H, int32_t W,
                                   const float* keypoints, const float* areas, const float* boxes, int32_t N,
                                   float sigma, const float* kp_weights, int32_t topk, float* per_kp, float* loss,
                                   float* coords, float* scores, int32_t* argmax, float* target_out,
                                   float* weights_out, void* stream) {
  if (!heat || !keypoints || !kp_weights || !per_kp || !loss || !coords || !scores) return PRPE_EINVAL;
  if (B <= 0 || K <= 0 || K > PE_MAX_K || H <= 0 || W <= 0 || N < 1 || N > PE_MAX_N) return PRPE_EINVAL;
  if (topk < 1 || topk > K) return PRPE_EINVAL;
  if (mode != 0 && mode != 1) return PRPE_EINVAL;
  const int64_t HW = (int64_t)H * W;
  if (HW >= (1LL << 31) || (int64_t)B * K >= (1LL << 31)) return PRPE_EINVAL;
  if (avg_out) {
    if (!heat_flipped) return PRPE_EINVAL;
    // the flipped map is read at other (b, k, w) than the one a workgroup writes
    const uintptr_t bytes = (uintptr_t)B * K * HW * 4, a = (uintptr_t)avg_out, f = (uintptr_t)heat_flipped;
    if (spans_overlap(a, a + bytes, f, f + bytes)) return PRPE_EINVAL;
    // in place (avg_out == heat) a workgroup overwrites only what it has read; shifted against
    // heat it would overwrite another workgroup's input
    const uintptr_t h = (uintptr_t)heat;
    if (a != h && spans_overlap(a, a + bytes, h, h + bytes)) return PRPE_EINVAL;
  }
  PoseEvalK p{};
  p.heat = heat; p.flip = heat_flipped; p.avg_out = avg_out;
  p.kp = keypoints; p.areas = areas; p.boxes = boxes;
  p.per_kp = per_kp; p.coords = coords; p.scores = scores; p.argmax = argmax;
  p.target_out = target_out; p.weights_out = weights_out;
  p.B = B; p.N = N; p.K = K; p.H = H; p.W = W; p.mode = mode; p.sigma = sigma;
  for (int k = 0; k < K; ++k) {
    const int q = (heat_flipped && partner) ? partner[k] : -1;
    if (q >= K) return PRPE_EINVAL;
    p.partner[k] = q;
    p.kpw[k] = kp_weights[k];
  }
  hipStream_t st = as_stream(stream);
  if (HW <= PE_PER * PE_THREADS)
    hipLaunchKernelGGL(pose_eval_kernel<true>, dim3((unsigned)(B * K)), dim3(PE_THREADS), 0, st, p);
  else
    hipLaunchKernelGGL(pose_eval_kernel<false>, dim3((unsigned)(B * K)), dim3(PE_THREADS), 0, st, p);
  const int rc = launch_status();
  if (rc) return rc;
  hipLaunchKernelGGL(pose_ohkm_kernel, dim3(1), dim3(256), 0, st, (const float*)per_kp, B, K, topk, loss);
  return launch_status();
}

extern "C" int prpe_pose_coco_records(const float* coords, const float* scores, const float* boxes,
                                      const float* areas, const uint8_t* masks, const uint8_t* is_crowd,
                                      const uint8_t* keep, int32_t B, int32_t N, int32_t K, double keypoint_thresh,
                                      int32_t slot_base, uint64_t* counter, float* rec_kpts, float* rec_meta,
                                      int64_t capacity, void* stream) {
  if (!coords || !scores || !boxes || !areas || !masks || !is_crowd || !keep || !counter || !rec_kpts || !rec_meta)
    return PRPE_EINVAL;
  if (B <= 0 || N < 1 || K <= 0 || K > PE_MAX_K || capacity < 0 || slot_base < 0) return PRPE_EINVAL;
  if ((int64_t)slot_base + B >= (1LL << 31)) return PRPE_EINVAL;
  hipStream_t st = as_stream(stream);
  // the counter a chunk's records kernel reads already counts the chunks before it (stream order)
  for (int b0 = 0; b0 < B; b0 += PR_CHUNK) {
    PoseRecK p{};
    p.B = B - b0 < PR_CHUNK ? B - b0 : PR_CHUNK;
    p.coords = coords + (int64_t)b0 * K * 2; p.scores = scores + (int64_t)b0 * K;
    p.boxes = boxes + (int64_t)b0 * N * 4; p.areas = areas + (int64_t)b0 * N;
    p.masks = masks + (int64_t)b0 * N; p.crowd = is_crowd + (int64_t)b0 * N;
    for (int j = 0; j < p.B; ++j)
      if (keep[b0 + j]) p.keep[j >> 5] |= 1u << (j & 31);
    p.N = N; p.K = K; p.slot_base = slot_base + b0; p.thresh = keypoint_thresh;
    p.counter = reinterpret_cast<unsigned long long*>(counter);
    p.kpts = rec_kpts; p.meta = rec_meta; p.cap = capacity;
    hipLaunchKernelGGL(pose_records_kernel, dim3(p.B), dim3(64), 0, st, p);
    int rc = launch_status();
    if (rc) return rc;
    hipLaunchKernelGGL(pose_records_count_kernel, dim3(1), dim3(256), 0, st, p);
    rc = launch_status();
    if (rc) return rc;
  }
  return 0;
}
