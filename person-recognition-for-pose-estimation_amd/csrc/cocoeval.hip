// Pose validation epoch end on device: COCO keypoint AP / AR. The reference's
// on_validation_epoch_end (training/lightning/pose_estimation/module.py:578-647) hands the epoch's
// records to pycocotools' COCOeval(gt, dt, 'keypoints'): evaluate(), accumulate(), summarize(). Here
// the records never leave the device:
//   coco_runs_kernel    : the run of records of every image (a PoseEvalStep epoch keeps an image id
//                         once, so an image's records are contiguous): first and last record of the
//                         run, found by the records at the run's two ends. No atomics.
//   coco_match_kernel   : evaluate(). One wavefront per image: the records ranked by score (stable,
//                         NaN last; numpy's mergesort of -score), the best 20 kept; loadRes' keypoint
//                         extent area; computeOks' [20 x G] matrix in LDS; then 30 lanes, one per
//                         (area range, OKS threshold), each walk evaluateImg's greedy loop with a
//                         64-bit mask of the matched ground truth. Results go to fixed slots
//                         [image, rank], which is COCOeval's concatenation order.
//   coco_key_kernel + rocPRIM radix sort : accumulate()'s one stable descending sort. The key is
//                         (score, slot), unique, so the order does not lean on the sort's stability.
//   coco_pr_kernel      : one wavefront per (area range, threshold): the cumulative tp / fp come from
//                         ballots, walking the sorted list from its end so that the precision
//                         envelope (a suffix maximum) is at hand when a recall threshold is crossed.
//   coco_stats_kernel   : summarize()'s ten numbers.
// All metric arithmetic is fp64 in COCOeval's operation order; contraction is off in this file.
#pragma clang fp contract(off)
#include "common.h"
#include <cstring>
#include <rocprim/rocprim.hpp>

namespace {

constexpr int MD = PRPE_COCO_MAX_DETS;      // 20
constexpr int MG = PRPE_COCO_MAX_GT;        // 64
constexpr int NT = PRPE_COCO_IOU_THRS;      // 10
constexpr int NR = PRPE_COCO_REC_THRS;      // 101
constexpr int NA = PRPE_COCO_AREAS;         // 3
constexpr int NP = NA * NT;                 // (area, threshold) pairs
constexpr int MAX_K = 64;
constexpr int SC_MAX = 1024;                // scores of an image's records held in LDS up to this many
constexpr unsigned long long EMPTY = 1ull << 63;
constexpr double EPS = 2.220446049250313e-16;   // np.spacing(1) = 2^-52

__device__ __forceinline__ int64_t record_count(const unsigned long long* counter, int64_t n_max) {
  if (!counter) return n_max;
  const unsigned long long c = *counter;
  return c < (unsigned long long)n_max ? (int64_t)c : n_max;
}

__global__ __launch_bounds__(256) void coco_runs_kernel(const float* meta, const unsigned long long* counter,
                                                        int64_t n_max, const int32_t* slot_to_img, int slots, int I,
                                                        int32_t* det_range) {
  const int64_t n = record_count(counter, n_max);
  const int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (r >= n) return;
  auto img_of = [&](int64_t q) {
    const int s = __float_as_int(meta[q * 8]);
    if (s < 0 || s >= slots) return -1;
    const int im = slot_to_img[s];
    return (im < 0 || im >= I) ? -1 : im;
  };
  const int cur = img_of(r);
  if (cur < 0) return;
  if (r == 0 || img_of(r - 1) != cur) det_range[2 * cur] = (int32_t)r;
  if (r == n - 1 || img_of(r + 1) != cur) det_range[2 * cur + 1] = (int32_t)(r + 1);
}

struct CocoMatchK {
  const float* kpts; const float* meta; const unsigned long long* counter; int64_t n_max;
  const int32_t* det_range;
  const int32_t* gt_start; const double* gt_kpts; const double* gt_bbox; const double* gt_area;
  const uint8_t* gt_crowd; const uint8_t* gt_ignore;
  int I, G, K;
  double var[MAX_K];                    // (2 sigma)^2
  double thr[NT];
  double rng[2 * NA];
  float* dt_score; unsigned long long* dt_bits; int32_t* dt_rec; int32_t* npig; double* oks_out;
};

// numpy's stable argsort of -score: record e comes before record d
__device__ __forceinline__ bool score_before(float se, int e, float sd, int d) {
  const bool en = se != se, dn = sd != sd;
  if (en || dn) return dn && (!en || e < d);
  return se > sd || (se == sd && e < d);
}

__global__ __launch_bounds__(64) void coco_match_kernel(CocoMatchK p) {
  const int img = blockIdx.x, lane = threadIdx.x;
  __shared__ double s_oks[MD * MG];
  __shared__ float s_score[SC_MAX];
  __shared__ int s_kept[MD];
  __shared__ double s_darea[MD];
  __shared__ unsigned s_m[NP], s_i[NP];
  __shared__ double s_thr[NT], s_rng[2 * NA];

  const int64_t n = record_count(p.counter, p.n_max);
  int64_t d0 = p.det_range[2 * img], d1 = p.det_range[2 * img + 1];
  if (d0 < 0 || d1 > n || d1 < d0) d0 = d1 = 0;
  const int D = (int)(d1 - d0);
  int gs = p.gt_start[img], G = p.gt_start[img + 1] - gs;
  if (gs < 0 || G < 0 || G > MG || (int64_t)gs + G > p.G) G = 0;
  const int Dk = D < MD ? D : MD;
  const int K = p.K;

#pragma unroll
  for (int q = 0; q < NT; ++q)
    if (lane == q) s_thr[q] = p.thr[q];
#pragma unroll
  for (int q = 0; q < 2 * NA; ++q)
    if (lane == q) s_rng[q] = p.rng[q];

  // ---- a. the records by descending score, the first 20
  const bool cached = D <= SC_MAX;
  if (cached)
    for (int e = lane; e < D; e += 64) s_score[e] = p.meta[(d0 + e) * 8 + 2];
  if (lane < MD) s_kept[lane] = -1;
  __syncthreads();
  auto score = [&](int e) { return cached ? s_score[e] : p.meta[(d0 + e) * 8 + 2]; };
  for (int d = lane; d < D; d += 64) {
    const float sd = score(d);
    int rank = 0;
    for (int e = 0; e < D && rank < MD; ++e) rank += (e != d && score_before(score(e), e, sd, d)) ? 1 : 0;
    if (rank < MD) s_kept[rank] = d;
  }
  __syncthreads();

  // loadRes: a detection's area is the extent of its keypoints (np.min / np.max: a NaN stays)
  if (lane < Dk) {
    const float* kp = p.kpts + (d0 + s_kept[lane]) * K * 3;
    double x0 = (double)kp[0], x1 = x0, y0 = (double)kp[1], y1 = y0;
    for (int k = 1; k < K; ++k) {
      const double x = (double)kp[k * 3], y = (double)kp[k * 3 + 1];
      if (x < x0 || x != x) x0 = x;
      if (x > x1 || x != x) x1 = x;
      if (y < y0 || y != y) y0 = y;
      if (y > y1 || y != y) y1 = y;
    }
    s_darea[lane] = (x1 - x0) * (y1 - y0);
  }

  // ---- b. computeOks: row = detection by rank, column = the image's ground truth in table order
  for (int pq = lane; pq < Dk * G; pq += 64) {
    const int i = pq / G, j = pq - i * G;
    const double* gk = p.gt_kpts + (int64_t)(gs + j) * K * 3;
    const float* dk = p.kpts + (d0 + s_kept[i]) * K * 3;
    int k1 = 0;
    for (int k = 0; k < K; ++k) k1 += gk[k * 3 + 2] > 0.0 ? 1 : 0;
    const double* bb = p.gt_bbox + (int64_t)(gs + j) * 4;
    const double bx0 = bb[0] - bb[2], bx1 = bb[0] + bb[2] * 2.0;
    const double by0 = bb[1] - bb[3], by1 = bb[1] + bb[3] * 2.0;
    const double den = p.gt_area[gs + j] + EPS;
    double sum = 0.0;
    for (int k = 0; k < K; ++k) {
      const double xd = (double)dk[k * 3], yd = (double)dk[k * 3 + 1];
      double dx, dy;
      if (k1 > 0) {
        dx = xd - gk[k * 3];
        dy = yd - gk[k * 3 + 1];
      } else {
        // np.maximum(0, v): a NaN stays
        auto pos = [](double v) { return (v > 0.0 || v != v) ? v : 0.0; };
        dx = pos(bx0 - xd) + pos(xd - bx1);
        dy = pos(by0 - yd) + pos(yd - by1);
      }
      const double e = (dx * dx + dy * dy) / p.var[k] / den / 2.0;
      if (k1 == 0 || gk[k * 3 + 2] > 0.0) sum += exp(-e);
    }
    s_oks[i * MG + j] = sum / (double)(k1 > 0 ? k1 : K);
  }
  __syncthreads();

  // ---- c. evaluateImg: lane = (area range, threshold)
  if (lane < NP) {
    const int a = lane / NT, t = lane - a * NT;
    const double lo = s_rng[2 * a], hi = s_rng[2 * a + 1];
    unsigned long long ign = 0, crowd = 0;
    for (int j = 0; j < G; ++j) {
      const double ar = p.gt_area[gs + j];
      if (p.gt_ignore[gs + j] || ar < lo || ar > hi) ign |= 1ull << j;
      if (p.gt_crowd[gs + j]) crowd |= 1ull << j;
    }
    const double t0 = s_thr[t] < 1.0 - 1e-10 ? s_thr[t] : 1.0 - 1e-10;
    unsigned long long gtm = 0;
    unsigned dm = 0, di = 0;
    for (int i = 0; i < Dk; ++i) {
      double iou = t0;
      int m = -1;
      // the ground truth in stable order of its ignore flag; reaching an ignored one with a
      // match among the others ends the walk (the `break`)
      for (int pass = 0; pass < 2 && !(pass == 1 && m >= 0); ++pass) {
        for (int j = 0; j < G; ++j) {
          if ((int)((ign >> j) & 1) != pass) continue;
          if (((gtm >> j) & 1) && !((crowd >> j) & 1)) continue;
          const double o = s_oks[i * MG + j];
          if (o < iou) continue;
          iou = o;
          m = j;
        }
      }
      if (m >= 0) {
        dm |= 1u << i;
        if ((ign >> m) & 1) di |= 1u << i;
        gtm |= 1ull << m;
      } else {
        const double da = s_darea[i];
        if (da < lo || da > hi) di |= 1u << i;
      }
    }
    s_m[lane] = dm;
    s_i[lane] = di;
    if (t == 0) p.npig[img * NA + a] = G - __popcll(ign);
  }
  __syncthreads();

  // ---- d. the image's 20 slots
  if (lane < MD) {
    unsigned long long w = 0;
    for (int q = 0; q < NP; ++q) {
      w |= (unsigned long long)((s_m[q] >> lane) & 1u) << q;
      w |= (unsigned long long)((s_i[q] >> lane) & 1u) << (NP + q);
    }
    const bool has = lane < Dk;
    const int64_t o = (int64_t)img * MD + lane;
    p.dt_bits[o] = has ? w : EMPTY;
    p.dt_score[o] = has ? score(s_kept[lane]) : 0.f;
    p.dt_rec[o] = has ? (int32_t)(d0 + s_kept[lane]) : -1;
  }
  if (p.oks_out) {
    double* oo = p.oks_out + (int64_t)img * MD * MG;
    for (int q = lane; q < MD * MG; q += 64) {
      const int i = q / MG, j = q - i * MG;
      oo[q] = (i < Dk && j < G) ? s_oks[q] : -1.0;
    }
  }
}

// key of slot q: the high word ascends as the score descends (-0 as +0; empty slots and NaN
// last), the low word is the slot, so equal scores stay in slot order
__global__ __launch_bounds__(256) void coco_key_kernel(const float* dt_score, const unsigned long long* dt_bits,
                                                       int M, unsigned long long* keys) {
  const int q = blockIdx.x * 256 + threadIdx.x;
  if (q >= M) return;
  float s = dt_score[q];
  if (s == 0.f) s = 0.f;
  const unsigned u = __float_as_uint(s);
  const unsigned ord = (u & 0x80000000u) ? ~u : (u | 0x80000000u);
  const unsigned hi = ((dt_bits[q] & EMPTY) || s != s) ? 0xffffffffu : ~ord;
  keys[q] = ((unsigned long long)hi << 32) | (unsigned)q;
}

struct CocoPrK {
  const unsigned long long* keys;       // sorted
  const unsigned long long* dt_bits;
  const int32_t* npig;
  int I, M;
  double rec[NR];
  double* precision; double* recall;
};

__device__ __forceinline__ int warp_sum_int(int v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// one wavefront per (area range a, threshold t)
__global__ __launch_bounds__(64) void coco_pr_kernel(CocoPrK p) {
  const int pair = blockIdx.x, lane = threadIdx.x;
  const int a = pair / NT, t = pair - a * NT;
  __shared__ double s_rec[NR];
#pragma unroll
  for (int q = 0; q < NR; ++q)
    if (lane == (q & 63)) s_rec[q] = p.rec[q];
  int np = 0;
  for (int i = lane; i < p.I; i += 64) np += p.npig[i * NA + a];
  np = warp_sum_int(np);
  __syncthreads();
  auto prec_at = [&](int r) -> double& { return p.precision[((int64_t)t * NR + r) * NA + a]; };
  if (np == 0) {                        // no ground truth to find: the pair stays -1
    for (int r = lane; r < NR; r += 64) prec_at(r) = -1.0;
    if (lane == 0) p.recall[t * NA + a] = -1.0;
    return;
  }
  const unsigned long long mbit = 1ull << pair, ibit = 1ull << (NP + pair);
  auto flags = [&](int q, bool& tp, bool& fp) {
    const unsigned long long w = q < p.M ? p.dt_bits[(unsigned)p.keys[q]] : EMPTY;
    const bool live = !(w & EMPTY) && !(w & ibit);
    tp = live && (w & mbit);
    fp = live && !(w & mbit);
  };
  int tp_tot = 0, fp_tot = 0;
  for (int q = lane; q < p.M; q += 64) {
    bool tp, fp;
    flags(q, tp, fp);
    tp_tot += tp;
    fp_tot += fp;
  }
  tp_tot = warp_sum_int(tp_tot);
  fp_tot = warp_sum_int(fp_tot);
  const double npd = (double)np;
  // thresholds at or below x (they ascend)
  auto count_le = [&](double x) {
    int lo = 0, hi = NR;
    while (lo < hi) {
      const int mid = (lo + hi) >> 1;
      if (s_rec[mid] <= x) lo = mid + 1;
      else hi = mid;
    }
    return lo;
  };
  // from the end: tp_i, fp_i are the cumulative counts at entry i, smax the running envelope
  int tp_end = tp_tot, fp_end = fp_tot;
  double smax = 0.0;                    // every precision is >= 0
  const unsigned long long above = lane == 63 ? 0ull : ~0ull << (lane + 1);
  for (int c = (p.M + 63) / 64 - 1; c >= 0; --c) {
    const int q = c * 64 + lane;
    bool tp, fp;
    flags(q, tp, fp);
    const unsigned long long bt = __ballot(tp), bf = __ballot(fp);
    if (bt == 0 && bf == 0 && c > 0) continue;      // nothing counted here: no threshold is crossed
    const int tpi = tp_end - __popcll(bt & above), fpi = fp_end - __popcll(bf & above);
    const double tpd = (double)tpi, fpd = (double)fpi;
    double pr = tpd / (fpd + tpd + EPS);
    if (q >= p.M) pr = 0.0;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const double v = __shfl_down(pr, o, 64);
      if (lane + o < 64 && v > pr) pr = v;
    }
    if (smax > pr) pr = smax;
    smax = __shfl(pr, 0, 64);
    if (q < p.M && (tp || q == 0)) {
      // the first entry whose recall reaches a threshold gives that threshold its precision
      const int r0 = q == 0 ? 0 : count_le((double)(tpi - (tp ? 1 : 0)) / npd);
      const double rc = tpd / npd;
      for (int r = r0; r < NR && s_rec[r] <= rc; ++r) prec_at(r) = pr;
    }
    tp_end -= __popcll(bt);
    fp_end -= __popcll(bf);
  }
  const double rc_last = (double)tp_tot / npd;
  for (int r = count_le(rc_last) + lane; r < NR; r += 64) prec_at(r) = 0.0;
  if (lane == 0) p.recall[t * NA + a] = rc_last;
}

// summarize() for keypoints: lane s is stats[s]; mean of the entries > -1, in index order
__global__ __launch_bounds__(64) void coco_stats_kernel(const double* precision, const double* recall, double* stats) {
  const int s = threadIdx.x;
  if (s >= 10) return;
  const bool ap = s < 5;
  const int kind = s % 5;               // all, iou .5, iou .75, medium, large
  const int t0 = kind == 1 ? 0 : (kind == 2 ? 5 : 0), t1 = kind == 1 ? 1 : (kind == 2 ? 6 : NT);
  const int a = kind == 3 ? 1 : (kind == 4 ? 2 : 0);
  double sum = 0.0;
  int cnt = 0;
  for (int t = t0; t < t1; ++t) {
    if (ap) {
      for (int r = 0; r < NR; ++r) {
        const double v = precision[(t * NR + r) * NA + a];
        if (v > -1.0) { sum += v; ++cnt; }
      }
    } else {
      const double v = recall[t * NA + a];
      if (v > -1.0) { sum += v; ++cnt; }
    }
  }
  stats[s] = cnt == 0 ? -1.0 : sum / (double)cnt;
}

inline size_t align256(size_t v) { return (v + 255) & ~(size_t)255; }

size_t key_sort_temp_bytes(size_t m) {
  size_t bytes = 0;
  if (rocprim::radix_sort_keys((void*)nullptr, bytes, (const unsigned long long*)nullptr,
                               (unsigned long long*)nullptr, m) != hipSuccess)
    return 0;
  return bytes;
}

}  // namespace

extern "C" int64_t prpe_coco_kp_match_workspace_bytes(int32_t I) {
  return I > 0 ? (int64_t)align256((size_t)I * 2 * sizeof(int32_t)) : 0;
}

extern "C" int prpe_coco_kp_match(const float* rec_kpts, const float* rec_meta, const uint64_t* counter,
                                  int64_t n_max, const int32_t* slot_to_img, int32_t slots,
                                  const int32_t* gt_start, const double* gt_kpts, const double* gt_bbox,
                                  const double* gt_area, const uint8_t* gt_iscrowd, const uint8_t* gt_ignore,
                                  int32_t I, int32_t G, int32_t max_gt, int32_t K, const double* sigmas,
                                  const double* iou_thrs, const double* area_rngs, float* dt_score,
                                  uint64_t* dt_bits, int32_t* dt_rec, int32_t* npig, double* oks_out,
                                  void* workspace, int64_t workspace_bytes, void* stream) {
  if (!gt_start || !sigmas || !iou_thrs || !area_rngs || !dt_score || !dt_bits || !dt_rec || !npig || !workspace)
    return PRPE_EINVAL;
  if (I < 1 || (int64_t)I * MD >= (1LL << 31) || K < 1 || K > MAX_K || G < 0 || max_gt < 0 || max_gt > MG ||
      n_max < 0 || n_max >= (1LL << 31) || slots < 0 || workspace_bytes < prpe_coco_kp_match_workspace_bytes(I))
    return PRPE_EINVAL;
  if (n_max > 0 && (!rec_kpts || !rec_meta || !slot_to_img || slots < 1)) return PRPE_EINVAL;
  if (G > 0 && (!gt_kpts || !gt_bbox || !gt_area || !gt_iscrowd || !gt_ignore)) return PRPE_EINVAL;
  CocoMatchK p{};
  for (int k = 0; k < K; ++k) {
    if (!(sigmas[k] > 0.0) || !(sigmas[k] <= 1.79769313486231570e308)) return PRPE_EINVAL;
    p.var[k] = (sigmas[k] * 2.0) * (sigmas[k] * 2.0);
  }
  for (int t = 0; t < NT; ++t) {
    if (iou_thrs[t] != iou_thrs[t]) return PRPE_EINVAL;
    p.thr[t] = iou_thrs[t];
  }
  for (int q = 0; q < 2 * NA; ++q) {
    if (area_rngs[q] != area_rngs[q]) return PRPE_EINVAL;
    p.rng[q] = area_rngs[q];
  }
  hipStream_t st = as_stream(stream);
  int32_t* det_range = static_cast<int32_t*>(workspace);
  if (hipMemsetAsync(det_range, 0, (size_t)I * 2 * sizeof(int32_t), st) != hipSuccess) return launch_status();
  const unsigned long long* cnt = reinterpret_cast<const unsigned long long*>(counter);
  if (n_max > 0) {
    hipLaunchKernelGGL(coco_runs_kernel, dim3((unsigned)((n_max + 255) / 256)), dim3(256), 0, st, rec_meta, cnt,
                       n_max, slot_to_img, slots, I, det_range);
    const int rc = launch_status();
    if (rc) return rc;
  }
  p.kpts = rec_kpts; p.meta = rec_meta; p.counter = cnt; p.n_max = n_max; p.det_range = det_range;
  p.gt_start = gt_start; p.gt_kpts = gt_kpts; p.gt_bbox = gt_bbox; p.gt_area = gt_area;
  p.gt_crowd = gt_iscrowd; p.gt_ignore = gt_ignore;
  p.I = I; p.G = G; p.K = K;
  p.dt_score = dt_score; p.dt_bits = reinterpret_cast<unsigned long long*>(dt_bits); p.dt_rec = dt_rec;
  p.npig = npig; p.oks_out = oks_out;
  hipLaunchKernelGGL(coco_match_kernel, dim3((unsigned)I), dim3(64), 0, st, p);
  return launch_status();
}

extern "C" int64_t prpe_coco_kp_accumulate_workspace_bytes(int32_t I) {
  if (I < 1 || (int64_t)I * MD >= (1LL << 31)) return 0;
  const size_t m = (size_t)I * MD;
  return (int64_t)(2 * align256(m * 8) + align256(key_sort_temp_bytes(m)));
}

extern "C" int prpe_coco_kp_accumulate(const float* dt_score, const uint64_t* dt_bits, const int32_t* npig,
                                       int32_t I, const double* rec_thrs, double* precision, double* recall,
                                       double* stats, void* workspace, int64_t workspace_bytes, void* stream) {
  if (!dt_score || !dt_bits || !npig || !rec_thrs || !precision || !recall || !stats || !workspace) return PRPE_EINVAL;
  if (I < 1 || (int64_t)I * MD >= (1LL << 31) || workspace_bytes < prpe_coco_kp_accumulate_workspace_bytes(I))
    return PRPE_EINVAL;
  CocoPrK p{};
  for (int r = 0; r < NR; ++r) {
    if (rec_thrs[r] != rec_thrs[r] || (r > 0 && !(rec_thrs[r] > rec_thrs[r - 1]))) return PRPE_EINVAL;
    p.rec[r] = rec_thrs[r];
  }
  const int M = I * MD;
  hipStream_t st = as_stream(stream);
  char* w = static_cast<char*>(workspace);
  unsigned long long* keys_in = reinterpret_cast<unsigned long long*>(w); w += align256((size_t)M * 8);
  unsigned long long* keys_out = reinterpret_cast<unsigned long long*>(w); w += align256((size_t)M * 8);
  size_t tb = key_sort_temp_bytes((size_t)M);
  const unsigned long long* bits = reinterpret_cast<const unsigned long long*>(dt_bits);
  hipLaunchKernelGGL(coco_key_kernel, dim3((unsigned)((M + 255) / 256)), dim3(256), 0, st, dt_score, bits, M, keys_in);
  int rc = launch_status();
  if (rc) return rc;
  if (rocprim::radix_sort_keys((void*)w, tb, (const unsigned long long*)keys_in, keys_out, (size_t)M, 0, 64, st) !=
      hipSuccess)
    return launch_status();
  p.keys = keys_out; p.dt_bits = bits; p.npig = npig; p.I = I; p.M = M;
  p.precision = precision; p.recall = recall;
  hipLaunchKernelGGL(coco_pr_kernel, dim3(NP), dim3(64), 0, st, p);
  rc = launch_status();
  if (rc) return rc;
  hipLaunchKernelGGL(coco_stats_kernel, dim3(1), dim3(64), 0, st, (const double*)precision, (const double*)recall,
                     stats);
  return launch_status();
}
