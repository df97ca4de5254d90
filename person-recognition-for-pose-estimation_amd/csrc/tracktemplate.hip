// Track-level face templates (include/prpe.h, prpe_track_template_update and
// prpe_track_template_assign): the embeddings of a track's faces summed in fixed point, the sums of
// the tracks that changed handed to the gallery search as query rows, and the search's answer
// taken back into the state and out to the persons.
//
// update, launch 1 (tmpl_accumulate_kernel): one workgroup of 256 threads per (stream, slot); a
// thread owns columns tid and tid + 256 of the slot's sum, two int64 in registers. The workgroup
// walks the person list once, 256 slots at a time: a ballot per wave and a prefix over the four
// waves put the slot's candidates into LDS in list order; one wave per candidate tests its norm
// and its whole row (a ballot over the row's elements) before anything is added; a second ordered
// compaction keeps the candidates that contribute, cut at 2^20 faces; then every thread adds its
// two columns of four rows at a time. The state row goes back once. dirty_pos takes 0 / -1.
// update, launch 2 (tmpl_queries_kernel): one workgroup per stream counts the dirty slots before
// its own (the sign of dirty_pos, which this launch never changes: see below), numbers its own,
// converts their sums into query rows and zeroes its share of the rows past the list.
// assign, one launch: a thread per list position and per person slot.
// No atomics, no workspace, vector stores only.
#pragma clang fp contract(off)
#include "common.h"

namespace {

constexpr int TT = 32;                         // template slots per stream (the tracker's track slots)
constexpr int TT_THREADS = 256;
constexpr int TT_MAX_FACES = 1 << 20;          // faces a template sums at most
constexpr int TT_MAX_STREAMS = 4096;           // every workgroup of tmpl_queries_kernel reads all S * 32 flags
constexpr float TT_SCALE = 16777216.f;         // 2^24
constexpr float TT_MAX_NORM = 32768.f;         // 2^15

__device__ __forceinline__ bool finitef(float v) { return fabsf(v) <= 3.402823466e38f; }   // false for NaN

struct TmplK {
  const float* meta_p; const int* n_p; int max_p; const int* track_id; const int* person_face;
  const float* emb; int64_t lde; const float* norms; const int* n_f; int max_f; int D;
  const int* frame_stream; int B, S; const float* trk_meta; int mode; float min_norm;
  int* owner; int64_t* sum; int* n; int64_t* ident; float* score;
  int* dirty_rows; int* n_dirty; int* dirty_pos; float* queries; int max_q;
};

// The rank of this thread among the threads of the workgroup with `in` set, in thread order, and
// their number. Two barriers; wcnt may be reused as soon as it returns.
__device__ __forceinline__ int wg_rank(bool in, int* wcnt, int& total) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const unsigned long long mask = __ballot(in);
  if (lane == 0) wcnt[wave] = __popcll(mask);
  __syncthreads();
  int base = 0, tot = 0;
#pragma unroll
  for (int w = 0; w < TT_THREADS / 64; ++w) {
    const int c = wcnt[w];
    base += w < wave ? c : 0;
    tot += c;
  }
  total = tot;
  __syncthreads();
  return base + __popcll(mask & ((1ull << lane) - 1ull));
}

__global__ __launch_bounds__(TT_THREADS) void tmpl_accumulate_kernel(TmplK p) {
  __shared__ int cand_f[TT_THREADS], take_f[TT_THREADS], cand_ok[TT_THREADS], wcnt[TT_THREADS / 64];
  __shared__ float cand_w[TT_THREADS], take_w[TT_THREADS];
  const int64_t g = blockIdx.x;                // s * 32 + j
  const int s = (int)(g / TT);
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int d0 = tid, d1 = tid + TT_THREADS;
  const bool has0 = d0 < p.D, has1 = d1 < p.D;
  int64_t* srow = p.sum + g * p.D;
  const int id = __float_as_int(p.trk_meta[g * 8]);
  if (id < 0) {                                // a free slot: the template is forgotten
    if (has0) srow[d0] = 0;
    if (has1) srow[d1] = 0;
    if (tid == 0) {
      p.owner[g] = -1; p.n[g] = 0; p.ident[g] = -1; p.score[g] = -INFINITY;
      p.dirty_pos[g] = -1;
    }
    return;
  }
  const bool clear = p.owner[g] != id;         // the slot was reused
  int n = clear ? 0 : p.n[g];
  const int n_before = n;
  int64_t acc0 = !clear && has0 ? srow[d0] : 0, acc1 = !clear && has1 ? srow[d1] : 0;
  int n_p = *p.n_p, n_f = *p.n_f;
  n_p = n_p < 0 ? 0 : (n_p < p.max_p ? n_p : p.max_p);
  n_f = n_f < 0 ? 0 : (n_f < p.max_f ? n_f : p.max_f);

  for (int c0 = 0; c0 < n_p; c0 += TT_THREADS) {     // one walk of the person list
    const int q = c0 + tid;                    // c0 + 255 <= n_p + 254: max_p is at most 2^30
    int f = -1;
    if (q < n_p && p.track_id[q] == id) {
      const int b = __float_as_int(p.meta_p[(int64_t)q * 8]);
      if ((unsigned)b < (unsigned)p.B && p.frame_stream[b] == s) f = p.person_face[q];
    }
    const bool in = (unsigned)f < (unsigned)n_f;
    int total;
    const int pos = wg_rank(in, wcnt, total);
    if (total == 0) continue;                  // the same in every thread
    if (in) cand_f[pos] = f;
    __syncthreads();
    // a wave per candidate: the norm and every element of the row, before anything is added
    for (int c = wave; c < total; c += TT_THREADS / 64) {
      const int fc = cand_f[c];
      const float nv = p.norms[fc];
      bool ok = finitef(nv) && nv >= p.min_norm && nv < TT_MAX_NORM;
      if (ok) {
        const float* row = p.emb + (int64_t)fc * p.lde;
        bool bad = false;
        for (int d = lane; d < p.D; d += 64) bad |= !finitef(row[d]);
        ok = __ballot(bad) == 0ull;
      }
      if (lane == 0) { cand_ok[c] = ok; cand_w[c] = p.mode == 0 ? nv : 1.f; }
    }
    __syncthreads();
    // the candidates that contribute, in list order, up to 2^20 faces in all
    const bool ok = tid < total && cand_ok[tid];
    int n_ok;
    const int pos2 = wg_rank(ok, wcnt, n_ok);
    const int room = TT_MAX_FACES - n;
    const int ntake = n_ok < room ? n_ok : room;
    if (ok && pos2 < ntake) { take_f[pos2] = cand_f[tid]; take_w[pos2] = cand_w[tid]; }
    __syncthreads();
    for (int c = 0; c < ntake; c += 4) {
      float w[4], v0[4], v1[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int cc = c + u < ntake ? c + u : ntake - 1;
        const float* row = p.emb + (int64_t)take_f[cc] * p.lde;
        w[u] = take_w[cc];
        v0[u] = has0 ? row[d0] : 0.f;
        v1[u] = has1 ? row[d1] : 0.f;
      }
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        if (c + u < ntake) {
          acc0 += llrintf((w[u] * v0[u]) * TT_SCALE);
          acc1 += llrintf((w[u] * v1[u]) * TT_SCALE);
        }
      }
    }
    n += ntake;
  }

  const bool dirty = n > n_before;
  if (clear || dirty) {
    if (has0) srow[d0] = acc0;
    if (has1) srow[d1] = acc1;
    if (tid == 0) {
      p.n[g] = n;
      if (clear) { p.owner[g] = id; p.ident[g] = -1; p.score[g] = -INFINITY; }
    }
  }
  if (tid == 0) p.dirty_pos[g] = dirty ? 0 : -1;
}

// dirty_pos holds 0 (dirty) or -1 from the launch before. This launch replaces a 0 by the slot's
// position in the list, which is never negative, and leaves a -1: the test `>= 0` that the counting
// reads has one answer whether another workgroup has numbered the slot yet or not.
__global__ __launch_bounds__(TT_THREADS) void tmpl_queries_kernel(TmplK p) {
  __shared__ int part[2][TT_THREADS / 64];
  const int s = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int64_t row0 = (int64_t)s * TT, slots = (int64_t)p.S * TT;
  int before = 0, total = 0;
  for (int64_t i = tid; i < slots; i += TT_THREADS) {
    const int d = p.dirty_pos[i] >= 0;
    total += d;
    before += i < row0 ? d : 0;
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    total += __shfl_xor(total, o, 64);
    before += __shfl_xor(before, o, 64);
  }
  if (lane == 0) { part[0][wave] = total; part[1][wave] = before; }
  __syncthreads();
  total = before = 0;
#pragma unroll
  for (int w = 0; w < TT_THREADS / 64; ++w) { total += part[0][w]; before += part[1][w]; }
  const int n_dirty = total < p.max_q ? total : p.max_q;       // the list holds max_q rows
  if (s == 0 && tid == 0) *p.n_dirty = n_dirty;

  // the stream's own slots (every wave forms the same mask; wave 0 writes)
  const bool mine = lane < TT && p.dirty_pos[row0 + (lane < TT ? lane : 0)] >= 0;
  unsigned long long mask = __ballot(mine);
  const int pos = before + __popcll(mask & ((1ull << lane) - 1ull));
  __syncthreads();                             // every read of this stream's row by this workgroup is done
  if (wave == 0 && mine) {
    p.dirty_pos[row0 + lane] = pos;            // a position at or past max_q: dirty, but in no list
    if (pos < p.max_q) p.dirty_rows[pos] = (int)(row0 + lane);
  }
  int r = before;
  while (mask) {
    const int j = __builtin_ctzll(mask);
    mask &= mask - 1;
    if (r < p.max_q) {
      const int64_t* srow = p.sum + (row0 + j) * p.D;
      float* qrow = p.queries + (int64_t)r * p.D;
      for (int d = tid; d < p.D; d += TT_THREADS) qrow[d] = (float)((double)srow[d] * 5.9604644775390625e-08);   // 2^-24
    }
    ++r;
  }
  // the rows past the list, dealt out over the streams
  for (int64_t z = (int64_t)n_dirty + s; z < p.max_q; z += p.S) {
    float* qrow = p.queries + z * p.D;
    for (int d = tid; d < p.D; d += TT_THREADS) qrow[d] = 0.f;
    if (tid == 0) p.dirty_rows[z] = -1;
  }
}

struct AssignK {
  const float* meta_p; const int* n_p; int max_p; const int* track_id; const int* frame_stream; int B, S;
  const float* trk_meta; const int64_t* ident; const float* score; const int* n_dirty; const int* dirty_rows;
  const int* dirty_pos; int max_q; const int* n; int64_t* t_ident; float* t_score;
  int64_t* out_ident; float* out_score; int* out_faces;
};

// A thread with i < n_dirty writes the state of list row i; a thread with i < max_p serves person
// slot i, reading the state of slots that are in no list and the search's answer for the others.
__global__ __launch_bounds__(TT_THREADS) void tmpl_assign_kernel(AssignK p) {
  const int64_t i = (int64_t)blockIdx.x * TT_THREADS + threadIdx.x;
  int n_dirty = *p.n_dirty;
  n_dirty = n_dirty < 0 ? 0 : (n_dirty < p.max_q ? n_dirty : p.max_q);
  const int64_t slots = (int64_t)p.S * TT;
  if (i < n_dirty) {
    const int g = p.dirty_rows[i];
    if ((unsigned)g < (unsigned)slots && p.dirty_pos[g] == (int)i) {
      p.t_ident[g] = p.ident[i];
      p.t_score[g] = p.score[i];
    }
  }
  if (i >= p.max_p) return;
  int n_p = *p.n_p;
  n_p = n_p < 0 ? 0 : (n_p < p.max_p ? n_p : p.max_p);
  int64_t o_ident = -1;
  float o_score = -INFINITY;
  int o_faces = 0;
  const int id = i < n_p ? p.track_id[i] : -1;
  if (id >= 0) {
    const int b = __float_as_int(p.meta_p[i * 8]);
    const int s = (unsigned)b < (unsigned)p.B ? p.frame_stream[b] : -1;
    if ((unsigned)s < (unsigned)p.S) {
      int j = -1;
      for (int t = TT - 1; t >= 0; --t)
        if (__float_as_int(p.trk_meta[((int64_t)s * TT + t) * 8]) == id) j = t;
      if (j >= 0) {
        const int64_t g = (int64_t)s * TT + j;
        const int r = p.dirty_pos[g];
        const bool listed = r >= 0 && r < n_dirty && p.dirty_rows[r] == (int)g;
        o_ident = listed ? p.ident[r] : p.t_ident[g];
        o_score = listed ? p.score[r] : p.t_score[g];
        o_faces = p.n[g];
      }
    }
  }
  p.out_ident[i] = o_ident;
  p.out_score[i] = o_score;
  p.out_faces[i] = o_faces;
}

}  // namespace

extern "C" int prpe_track_template_update(const float* crop_meta_p, const int32_t* n_p, int32_t max_p,
                                          const int32_t* track_id, const int32_t* person_face,
                                          const float* embeddings, int64_t emb_row_stride, const float* norms,
                                          const int32_t* n_f, int32_t max_f, int32_t D, const int32_t* frame_stream,
                                          int32_t B, int32_t S, const float* trk_meta, int32_t weight_mode,
                                          float min_norm, int32_t* tmpl_owner, int64_t* tmpl_sum, int32_t* tmpl_n,
                                          int64_t* tmpl_ident, float* tmpl_score, int32_t* dirty_rows,
                                          int32_t* n_dirty, int32_t* dirty_pos, float* queries, int32_t max_q,
                                          void* stream) {
  if (!crop_meta_p || !n_p || !track_id || !person_face || !embeddings || !norms || !n_f || !frame_stream) return PRPE_EINVAL;
  if (!trk_meta || !tmpl_owner || !tmpl_sum || !tmpl_n || !tmpl_ident || !tmpl_score) return PRPE_EINVAL;
  if (!dirty_rows || !n_dirty || !dirty_pos || !queries) return PRPE_EINVAL;
  if (B < 1 || S < 1 || max_p < 1 || max_f < 1 || S > TT_MAX_STREAMS || max_p > (1 << 30)) return PRPE_EINVAL;
  if (D < 32 || D > 2 * TT_THREADS || D % 32) return PRPE_EINVAL;
  if (emb_row_stride < D) return PRPE_EINVAL;
  const int64_t slots = (int64_t)S * TT;
  if (max_q < (slots < max_f ? slots : max_f)) return PRPE_EINVAL;
  if (weight_mode != 0 && weight_mode != 1) return PRPE_EINVAL;
  if (min_norm != min_norm) return PRPE_EINVAL;
  TmplK p{};
  p.meta_p = crop_meta_p; p.n_p = n_p; p.max_p = max_p; p.track_id = track_id; p.person_face = person_face;
  p.emb = embeddings; p.lde = emb_row_stride; p.norms = norms; p.n_f = n_f; p.max_f = max_f; p.D = D;
  p.frame_stream = frame_stream; p.B = B; p.S = S; p.trk_meta = trk_meta; p.mode = weight_mode; p.min_norm = min_norm;
  p.owner = tmpl_owner; p.sum = tmpl_sum; p.n = tmpl_n; p.ident = tmpl_ident; p.score = tmpl_score;
  p.dirty_rows = dirty_rows; p.n_dirty = n_dirty; p.dirty_pos = dirty_pos; p.queries = queries; p.max_q = max_q;
  hipLaunchKernelGGL(tmpl_accumulate_kernel, dim3((unsigned)slots), dim3(TT_THREADS), 0, as_stream(stream), p);
  hipLaunchKernelGGL(tmpl_queries_kernel, dim3((unsigned)S), dim3(TT_THREADS), 0, as_stream(stream), p);
  return launch_status();
}

extern "C" int prpe_track_template_assign(const float* crop_meta_p, const int32_t* n_p, int32_t max_p,
                                          const int32_t* track_id, const int32_t* frame_stream, int32_t B, int32_t S,
                                          const float* trk_meta, const int64_t* ident, const float* score,
                                          const int32_t* n_dirty, const int32_t* dirty_rows, const int32_t* dirty_pos,
                                          int32_t max_q, const int32_t* tmpl_n, int64_t* tmpl_ident, float* tmpl_score,
                                          int64_t* template_ident, float* template_score, int32_t* template_faces,
                                          void* stream) {
  if (!crop_meta_p || !n_p || !track_id || !frame_stream || !trk_meta || !ident || !score) return PRPE_EINVAL;
  if (!n_dirty || !dirty_rows || !dirty_pos || !tmpl_n || !tmpl_ident || !tmpl_score) return PRPE_EINVAL;
  if (!template_ident || !template_score || !template_faces) return PRPE_EINVAL;
  if (B < 1 || S < 1 || max_p < 1 || max_q < 1 || S > TT_MAX_STREAMS || max_p > (1 << 30)) return PRPE_EINVAL;
  AssignK p{};
  p.meta_p = crop_meta_p; p.n_p = n_p; p.max_p = max_p; p.track_id = track_id; p.frame_stream = frame_stream;
  p.B = B; p.S = S; p.trk_meta = trk_meta; p.ident = ident; p.score = score; p.n_dirty = n_dirty;
  p.dirty_rows = dirty_rows; p.dirty_pos = dirty_pos; p.max_q = max_q; p.n = tmpl_n; p.t_ident = tmpl_ident;
  p.t_score = tmpl_score; p.out_ident = template_ident; p.out_score = template_score; p.out_faces = template_faces;
  const int64_t threads = max_p > max_q ? max_p : max_q;
  hipLaunchKernelGGL(tmpl_assign_kernel, dim3((unsigned)((threads + TT_THREADS - 1) / TT_THREADS)), dim3(TT_THREADS), 0,
                     as_stream(stream), p);
  return launch_status();
}
