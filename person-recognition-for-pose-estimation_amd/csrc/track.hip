// Tracking persons across frames (include/prpe.h, prpe_track_update).
//
// One wavefront per stream. It loads the stream's 32-slot track table into LDS once, finds its
// frames in frame_stream with a ballot over 64 frames at a time, and for each of them in
// ascending order: collects the frame's person slots (ballot and popcount, as
// face_person_match_kernel), stages them in LDS, forms the 32 x 32 keys in registers (lane =
// person lane & 31 and tracks (lane >> 5) + 2 t), runs the greedy rounds on a wave-wide minimum,
// then updates, ages and opens tracks in LDS. The state goes back to memory once, after the last
// frame. No workspace, no atomics; a sequential chain of B frames is B dependent steps of one
// wave, so the time of a launch is the latency of its longest stream.
#pragma clang fp contract(off)
#include "common.h"

namespace {

constexpr int TRK = 32;                        // track slots per stream, persons per frame
constexpr int TRK_MAX_K = 64;

__device__ __forceinline__ bool finitef(float v) { return fabsf(v) <= 3.402823466e38f; }   // false for NaN

struct TrackK {
  const float* meta_p; const int* n_p; int max_p; const float* kpts; int K;
  const int64_t* ident; const float* score; const int* frame_stream; int B, S;
  int mode; float gate, kp_thr; int min_common; float new_thr; int max_age;
  float* trk_meta; float* trk_kpts; int64_t* trk_ident; float* trk_iscore; int* next_id;
  int* out_id; int* out_hits; int64_t* out_ident; float* out_iscore; int* status;
  float k2[TRK_MAX_K];
};

__device__ __forceinline__ void track_none(const TrackK& p, int s) {
  p.out_id[s] = -1;
  p.out_hits[s] = 0;
  p.out_ident[s] = -1;
  p.out_iscore[s] = -INFINITY;
}

// (cost, track, person) as one unsigned key that orders as (cost as a number, track, person):
// -0 becomes +0, then the usual sign flip makes the bit pattern monotonic over all finite floats.
// A finite cost never gives the all-ones key.
__device__ __forceinline__ unsigned long long track_key(float c, int ti, int di) {
  if (c == 0.f) c = 0.f;
  unsigned u = __float_as_uint(c);
  u ^= (u >> 31) ? 0xffffffffu : 0x80000000u;
  return (unsigned long long)u << 32 | (unsigned)(ti << 8 | di);
}

__global__ __launch_bounds__(64) void track_update_kernel(TrackK p) {
  extern __shared__ float kp_lds[];            // tk [32][K][3] then dk [32][K][3]
  __shared__ int t_id[TRK], t_age[TRK], t_hits[TRK];
  __shared__ float t_x0[TRK], t_y0[TRK], t_w[TRK], t_h[TRK], t_sc[TRK], t_isc[TRK];
  __shared__ int64_t t_ident[TRK];
  __shared__ int idx_p[TRK], got[TRK], cand[TRK];
  __shared__ float d_x0[TRK], d_y0[TRK], d_w[TRK], d_h[TRK], d_sc[TRK], d_isc[TRK];
  __shared__ int64_t d_ident[TRK];
  __shared__ float k2s[TRK_MAX_K];
  const int s = blockIdx.x, lane = threadIdx.x;
  const int K3 = p.K * 3;
  float* tk = kp_lds;
  float* dk = kp_lds + TRK * K3;
  int n_p = *p.n_p;
  n_p = n_p < 0 ? 0 : (n_p < p.max_p ? n_p : p.max_p);
  const unsigned long long below = (1ull << lane) - 1ull;

  if (s == 0) {
    // what no stream owns: slots at or past n_p, slots of no frame, persons and status of the
    // frames that are not tracked
    for (int q = lane; q < p.max_p; q += 64) {
      const int f = q < n_p ? __float_as_int(p.meta_p[(int64_t)q * 8]) : -1;
      if ((unsigned)f >= (unsigned)p.B || (unsigned)p.frame_stream[f] >= (unsigned)p.S) track_none(p, q);
    }
    for (int64_t b = lane; b < p.B; b += 64)
      if ((unsigned)p.frame_stream[b] >= (unsigned)p.S) p.status[b] = 0;
  }

  // the stream's state -> LDS
  const int64_t row0 = (int64_t)s * TRK;
  if (lane < TRK) {
    const float* m = p.trk_meta + (row0 + lane) * 8;
    t_id[lane] = __float_as_int(m[0]); t_age[lane] = __float_as_int(m[1]); t_hits[lane] = __float_as_int(m[2]);
    t_x0[lane] = m[3]; t_y0[lane] = m[4]; t_w[lane] = m[5]; t_h[lane] = m[6]; t_sc[lane] = m[7];
    t_ident[lane] = p.trk_ident[row0 + lane];
    t_isc[lane] = p.trk_iscore[row0 + lane];
  }
  if (lane < p.K) k2s[lane] = p.k2[lane];
  for (int i = lane; i < TRK * K3; i += 64) tk[i] = p.trk_kpts[row0 * K3 + i];
  unsigned next = (unsigned)p.next_id[s];
  __syncthreads();

  const int di = lane & 31, half = lane >> 5;
  for (int64_t b0 = 0; b0 < p.B; b0 += 64) {
    unsigned long long mine = __ballot(b0 + lane < p.B && p.frame_stream[b0 + lane < p.B ? b0 + lane : 0] == s);
    while (mine) {
      const int b = (int)b0 + __builtin_ctzll(mine);
      mine &= mine - 1;

      // the frame's person slots, ascending
      int np = 0;
      for (int s0 = 0; s0 < n_p; s0 += 64) {
        const int q = s0 + lane;
        const bool in = q < n_p && __float_as_int(p.meta_p[(int64_t)q * 8]) == b;
        const unsigned long long mask = __ballot(in);
        const int pos = np + __popcll(mask & below);
        if (in && pos < TRK) idx_p[pos] = q;
        np += __popcll(mask);
      }
      if (np > TRK) {                                // past the limit: the frame is skipped whole
        for (int q = lane; q < n_p; q += 64)
          if (__float_as_int(p.meta_p[(int64_t)q * 8]) == b) track_none(p, q);
        if (lane == 0) p.status[b] = 1;
        __syncthreads();
        continue;
      }
      __syncthreads();
      if (lane < np) {
        const int q = idx_p[lane];
        const float* m = p.meta_p + (int64_t)q * 8;
        d_x0[lane] = m[2]; d_y0[lane] = m[3]; d_w[lane] = m[4]; d_h[lane] = m[5]; d_sc[lane] = m[6];
        const int64_t id = p.ident[q];
        const float sc = p.score[q];
        const bool carries = id >= 0 && finitef(sc);
        d_ident[lane] = carries ? id : -1;
        d_isc[lane] = carries ? sc : -INFINITY;
      }
      if (lane < TRK) got[lane] = -1;
      for (int i = lane; i < np * K3; i += 64) {
        const int d = i / K3;
        dk[i] = p.kpts[(int64_t)idx_p[d] * K3 + (i - d * K3)];
      }
      __syncthreads();
      const unsigned live = (unsigned)__ballot(lane < TRK && t_id[lane] >= 0);

      // keys: lane owns person di and the tracks half + 2 t; ~0 where the pair is not eligible
      unsigned long long key[TRK / 2];
      if (p.mode == 0) {
        const float bx0 = d_x0[di], by0 = d_y0[di], bw = d_w[di], bh = d_h[di];
        const float bx1 = bx0 + bw, by1 = by0 + bh, barea = bw * bh;
#pragma unroll
        for (int t = 0; t < TRK / 2; ++t) {
          const int ti = half + 2 * t;
          key[t] = ~0ull;
          if (di < np && (live >> ti & 1u)) {
            const float ax0 = t_x0[ti], ay0 = t_y0[ti], aw = t_w[ti], ah = t_h[ti];
            const float ax1 = ax0 + aw, ay1 = ay0 + ah;
            float ix = (bx1 < ax1 ? bx1 : ax1) - (bx0 > ax0 ? bx0 : ax0);
            float iy = (by1 < ay1 ? by1 : ay1) - (by0 > ay0 ? by0 : ay0);
            ix = ix < 0.f ? 0.f : ix;
            iy = iy < 0.f ? 0.f : iy;
            const float inter = ix * iy;
            const float uni = aw * ah + barea - inter;
            const float c = 1.f - inter / uni;
            if (finitef(c) && c <= p.gate) key[t] = track_key(c, ti, di);
          }
        }
      } else {
        float sum[TRK / 2], den[TRK / 2];
        int cnt[TRK / 2];
#pragma unroll
        for (int t = 0; t < TRK / 2; ++t) {
          const int ti = half + 2 * t;
          sum[t] = 0.f;
          cnt[t] = 0;
          den[t] = t_w[ti] * t_h[ti];
        }
        for (int k = 0; k < p.K; ++k) {
          const float* dp = dk + (di * p.K + k) * 3;
          const float px = dp[0], py = dp[1];
          const bool dok = di < np && dp[2] >= p.kp_thr;
          const float kk = k2s[k];
#pragma unroll
          for (int t = 0; t < TRK / 2; ++t) {
            if (!(live >> (2 * t) & 3u)) continue;     // neither of the two tracks is live (uniform)
            const float* tp = tk + ((half + 2 * t) * p.K + k) * 3;
            if (dok && tp[2] >= p.kp_thr) {
              const float dx = px - tp[0], dy = py - tp[1];
              sum[t] = sum[t] + (dx * dx + dy * dy) / (den[t] * kk);
              ++cnt[t];
            }
          }
        }
#pragma unroll
        for (int t = 0; t < TRK / 2; ++t) {
          const int ti = half + 2 * t;
          key[t] = ~0ull;
          if (di < np && (live >> ti & 1u) && cnt[t] >= p.min_common) {
            const float c = sum[t] / (float)cnt[t];
            if (finitef(c) && c <= p.gate) key[t] = track_key(c, ti, di);
          }
        }
      }

      // greedy rounds; tm / dm: matched tracks / persons, the same in every lane
      unsigned tm = 0, dm = 0;
      for (int it = 0; it < np; ++it) {
        unsigned long long best = ~0ull;
        if (!(dm >> di & 1u)) {
#pragma unroll
          for (int t = 0; t < TRK / 2; ++t)
            if (!(tm >> (half + 2 * t) & 1u) && key[t] < best) best = key[t];
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
          const unsigned long long other = __shfl_xor(best, o, 64);
          best = other < best ? other : best;
        }
        if (best == ~0ull) break;                    // no eligible pair is left
        const int ti = (int)(best >> 8 & 0xff), dj = (int)(best & 0xff);
        tm |= 1u << ti;
        dm |= 1u << dj;
        if (lane == 0) got[dj] = ti;
      }
      __syncthreads();

      // matched tracks take their person (one person per track: no two lanes write one slot)
      if (lane < np && got[lane] >= 0) {
        const int ti = got[lane];
        t_x0[ti] = d_x0[lane]; t_y0[ti] = d_y0[lane]; t_w[ti] = d_w[lane]; t_h[ti] = d_h[lane]; t_sc[ti] = d_sc[lane];
        t_age[ti] = 0;
        t_hits[ti] += 1;
        const int64_t id = d_ident[lane];
        const float sc = d_isc[lane];
        if (id >= 0) {
          if (id == t_ident[ti]) {
            t_isc[ti] = sc > t_isc[ti] ? sc : t_isc[ti];
          } else if (sc > t_isc[ti]) {
            t_ident[ti] = id;
            t_isc[ti] = sc;
          }
        }
      }
      // the others age, and go when they are too old
      if (lane < TRK && (live >> lane & 1u) && !(tm >> lane & 1u)) {
        const int a = t_age[lane] + 1;
        t_age[lane] = a;
        if (a > p.max_age) { t_id[lane] = -1; t_ident[lane] = -1; t_isc[lane] = -INFINITY; }
      }
      __syncthreads();
      // new tracks: the r-th candidate person takes the r-th free slot
      const bool isfree = lane < TRK && t_id[lane] < 0;
      const bool iscand = lane < np && got[lane] < 0 && d_sc[lane] >= p.new_thr;
      const unsigned long long fmask = __ballot(isfree), cmask = __ballot(iscand);
      const int nfree = __popcll(fmask), ncand = __popcll(cmask);
      if (iscand) cand[__popcll(cmask & below)] = lane;
      __syncthreads();
      if (isfree) {
        const int r = __popcll(fmask & below);
        if (r < ncand) {
          const int d = cand[r];
          t_id[lane] = (int)(next + (unsigned)r);
          t_age[lane] = 0;
          t_hits[lane] = 1;
          t_x0[lane] = d_x0[d]; t_y0[lane] = d_y0[d]; t_w[lane] = d_w[d]; t_h[lane] = d_h[d]; t_sc[lane] = d_sc[d];
          t_ident[lane] = d_ident[d];
          t_isc[lane] = d_isc[d];
          got[d] = lane;
        }
      }
      next += (unsigned)(ncand < nfree ? ncand : nfree);
      __syncthreads();
      // keypoints of every person that has a track now, and the frame's outputs
      for (int i = lane; i < np * K3; i += 64) {
        const int d = i / K3, ti = got[d];
        if (ti >= 0) tk[ti * K3 + (i - d * K3)] = dk[i];
      }
      if (lane < np) {
        const int q = idx_p[lane], ti = got[lane];
        if (ti < 0) {
          track_none(p, q);
        } else {
          p.out_id[q] = t_id[ti];
          p.out_hits[q] = t_hits[ti];
          p.out_ident[q] = t_ident[ti];
          p.out_iscore[q] = t_isc[ti];
        }
      }
      if (lane == 0) p.status[b] = ncand > nfree ? 2 : 0;
      __syncthreads();
    }
  }

  // the state back to memory, once
  if (lane < TRK) {
    float* m = p.trk_meta + (row0 + lane) * 8;
    m[0] = __int_as_float(t_id[lane]); m[1] = __int_as_float(t_age[lane]); m[2] = __int_as_float(t_hits[lane]);
    m[3] = t_x0[lane]; m[4] = t_y0[lane]; m[5] = t_w[lane]; m[6] = t_h[lane]; m[7] = t_sc[lane];
    p.trk_ident[row0 + lane] = t_ident[lane];
    p.trk_iscore[row0 + lane] = t_isc[lane];
  }
  for (int i = lane; i < TRK * K3; i += 64) p.trk_kpts[row0 * K3 + i] = tk[i];
  if (lane == 0) p.next_id[s] = (int)next;
}

}  // namespace

extern "C" int prpe_track_update(const float* crop_meta_p, const int32_t* n_p, int32_t max_p, const float* keypoints,
                                 int32_t K, const int64_t* person_ident, const float* person_score,
                                 const int32_t* frame_stream, int32_t B, int32_t S, int32_t mode, float gate,
                                 float kp_thr, int32_t min_common, const float* k2, float new_thr, int32_t max_age,
                                 float* trk_meta, float* trk_kpts, int64_t* trk_ident, float* trk_iscore,
                                 int32_t* next_id, int32_t* track_id, int32_t* track_hits, int64_t* track_ident,
                                 float* track_iscore, int32_t* status, void* stream) {
  if (!crop_meta_p || !n_p || !keypoints || !person_ident || !person_score || !frame_stream || !k2) return PRPE_EINVAL;
  if (!trk_meta || !trk_kpts || !trk_ident || !trk_iscore || !next_id) return PRPE_EINVAL;
  if (!track_id || !track_hits || !track_ident || !track_iscore || !status) return PRPE_EINVAL;
  if (B <= 0 || S <= 0 || K <= 0 || max_p <= 0 || K > TRK_MAX_K) return PRPE_EINVAL;
  if ((int64_t)max_p * K >= (1LL << 31) / 3) return PRPE_EINVAL;
  if (mode != 0 && mode != 1) return PRPE_EINVAL;
  if (gate != gate || kp_thr != kp_thr || new_thr != new_thr) return PRPE_EINVAL;
  if (min_common < 1 || min_common > K || max_age < 0) return PRPE_EINVAL;
  TrackK p{};
  for (int k = 0; k < K; ++k) {
    if (!(k2[k] > 0.f) || !(k2[k] <= 3.402823466e38f)) return PRPE_EINVAL;
    p.k2[k] = k2[k];
  }
  p.meta_p = crop_meta_p; p.n_p = n_p; p.max_p = max_p; p.kpts = keypoints; p.K = K;
  p.ident = person_ident; p.score = person_score; p.frame_stream = frame_stream; p.B = B; p.S = S;
  p.mode = mode; p.gate = gate; p.kp_thr = kp_thr; p.min_common = min_common; p.new_thr = new_thr;
  p.max_age = max_age;
  p.trk_meta = trk_meta; p.trk_kpts = trk_kpts; p.trk_ident = trk_ident; p.trk_iscore = trk_iscore;
  p.next_id = next_id;
  p.out_id = track_id; p.out_hits = track_hits; p.out_ident = track_ident; p.out_iscore = track_iscore;
  p.status = status;
  const size_t lds = (size_t)2 * TRK * K * 3 * sizeof(float);
  hipLaunchKernelGGL(track_update_kernel, dim3((unsigned)S), dim3(64), lds, as_stream(stream), p);
  return launch_status();
}
