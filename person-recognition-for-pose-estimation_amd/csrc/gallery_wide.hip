// Wide-batch gallery search: prpe_gallery_topk's output, bit for bit, for many
// queries per call. A bf16 MFMA pass over the gallery finds, per query, a set of rows that
// provably contains the exact top-k; only those are scored with the exact fp32 chain of §5d.
//
// prpe_gallery_topk_wide, five launches, no host read, no atomics:
//   0. gallery.hip's normalise kernel writes the queries as fp32 (the exact route's bits) and as
//      bf16 (round to nearest even) into the workspace;
//   1. filter: gallery.hip's streaming walk on v_mfma_f32_16x16x32_bf16. A 4-wave workgroup holds 64
//      bf16 queries in LDS in fragment order (64 KB; with the lists 80 KB, two workgroups per CU)
//      and walks one chunk of gallery rows; a wave takes 16 fp32 rows per step straight from global
//      memory, rounds them to bf16 in registers, and keeps per query a sorted list of the L = 8
//      best coarse scores plus the largest coarse score it ever dropped. A non-finite coarse score
//      orders as +inf. The chunk's lists are merged per query into [chunk][Q][L] and the dropped
//      maximum into spill [chunk][Q]. One writer per list, as in gallery_topk_kernel;
//   2. rescore: one wave per query. t = the k-th largest finite coarse score of its lists,
//      bar = t - 2 eps(D). The entries at or above the bar (the +inf ones included) are the
//      candidates; the query is certified when they number at most C = 64 and every chunk either
//      dropped nothing or dropped only scores below the bar. A certified query's candidates are
//      scored with the exact chain (the same v_mfma_f32_16x16x4_f32 sequence as
//      gallery_topk_kernel: gallery row as A, query as B, four residue accumulators) and the best
//      k finite ones written in the total order. An uncertified query writes only its flag;
//   3. compact: one wave lists the flagged queries in ascending order and counts them;
//   4. gallery.hip's listed variants of the exact kernels finish exactly those queries.
#pragma clang fp contract(off)
#include "gallery.h"

namespace {

constexpr int GW_QT = 4;                 // 16-query MFMA tiles per workgroup
constexpr int GW_QB = GW_QT * 16;        // queries resident in LDS
constexpr int GW_L = 8;                  // list length per (chunk, query)
constexpr int GW_C = 64;                 // candidates the exact pass takes per query
constexpr int GW_PF = 4;                 // 32-column steps per register buffer (128 columns)
static_assert(GW_L == GL_KMAX, "the lists reuse gallery.h's 8-entry selection");

// ------------------------------------------------------------------------- launch 1: filter
struct FilterK {
  const __bf16* qbf;      // normalised queries, bf16 [Q][D]
  const float* gal;       // normalised gallery [>= G][D]
  const uint8_t* valid;   // [G] or NULL
  Ent* lists;             // [nchunks][Q][L]
  float* spill;           // [nchunks][Q]
  int Q, D, G, chunk, nqb;
};

template <bool FULL>
__global__ __launch_bounds__(GL_NW * 64) void gallery_filter_kernel(FilterK p) {
  constexpr int QS_BYTES = GW_QB * GL_DMAX * 2;
  __shared__ __attribute__((aligned(16))) unsigned char lds[QS_BYTES + GL_NW * GW_QB * GW_L * (int)sizeof(Ent)];
  bf16x8* qs = reinterpret_cast<bf16x8*>(lds);
  Ent* lists = reinterpret_cast<Ent*>(lds + QS_BYTES);

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int r = lane & 15, g = lane >> 4;
  const int qb0 = ((int)blockIdx.x % p.nqb) * GW_QB;
  const int c = (int)blockIdx.x / p.nqb;
  const int D = p.D, G = p.G;
  const int nsteps = D >> 5;

  // the query block in fragment order: step st of tile t is 64 lanes x 8 bf16, lane (g, r) holding
  // columns 32 st + 8 g + (0..7) of query 16 t + r (rows past Q are zeros, never written out)
  const int d8 = D >> 3;
  for (int i = tid; i < GW_QB * d8; i += GL_NW * 64) {
    const int ql = i / d8, col = (i - ql * d8) * 8;
    const int q = qb0 + ql;
    bf16x8 v = {0, 0, 0, 0, 0, 0, 0, 0};
    if (q < p.Q) v = *reinterpret_cast<const bf16x8*>(p.qbf + (int64_t)q * D + col);
    const int t = ql >> 4, st = col >> 5, gg = (col >> 3) & 3;
    qs[(t * nsteps + st) * 64 + gg * 16 + (ql & 15)] = v;
  }
  for (int i = tid; i < GL_NW * GW_QB * GW_L; i += GL_NW * 64) lists[i] = Ent{-INFINITY, GL_EMPTY};
  __syncthreads();

  Ent* mylists = lists + wave * GW_QB * GW_L;
  const int r0 = c * p.chunk;
  const int r1 = r0 + min(p.chunk, G - r0);   // r0 < G (wide_plan)
  const int ngroups = (nsteps + GW_PF - 1) / GW_PF;

  // 4 steps of one 16-row tile: lane (g, r) reads columns 32 st + 8 g + (0..7) of row base + r.
  // Rows past G - 1 and steps past the last re-read valid memory (their products are not used)
  auto load = [&](f32x4 (&dst)[GW_PF][2], int base, int grp) {
    const int row = min(base + r, G - 1);
    const float* src = p.gal + (int64_t)row * D + g * 8;
#pragma unroll
    for (int s = 0; s < GW_PF; ++s) {
      const int st = FULL ? grp * GW_PF + s : min(grp * GW_PF + s, nsteps - 1);
      dst[s][0] = *reinterpret_cast<const f32x4*>(src + st * 32);
      dst[s][1] = *reinterpret_cast<const f32x4*>(src + st * 32 + 4);
    }
  };

  f32x4 cur[GW_PF][2], nxt[GW_PF][2];
  f32x4 acc[GW_QT];
  float dropped[GW_QT];   // the largest coarse score of query 16 t + r that this lane saw dropped
#pragma unroll
  for (int t = 0; t < GW_QT; ++t) {
    acc[t] = f32x4{0.f, 0.f, 0.f, 0.f};
    dropped[t] = -INFINITY;
  }
  uint8_t vb[4] = {1, 1, 1, 1};   // valid bytes of rows base + 4 g + (0..3), fetched at the tile's first group
  int base = r0 + wave * GL_TILE, grp = 0;
  if (base < r1) load(cur, base, 0);
  while (base < r1) {
    int nb = base, ng = grp + 1;
    if (ng == ngroups) { ng = 0; nb = base + GL_STEP_ROWS; }
    if (grp == 0 && p.valid) {
#pragma unroll
      for (int j = 0; j < 4; ++j) vb[j] = p.valid[min(base + g * 4 + j, G - 1)];
    }
    load(nxt, nb, ng);
#pragma unroll
    for (int s = 0; s < GW_PF; ++s) {
      const int st = grp * GW_PF + s;
      if (FULL || st < nsteps) {
        bf16x8 a;
#pragma unroll
        for (int i = 0; i < 8; ++i) a[i] = (__bf16)cur[s][i >> 2][i & 3];
#pragma unroll
        for (int t = 0; t < GW_QT; ++t)
          acc[t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, qs[(t * nsteps + st) * 64 + lane], acc[t], 0, 0, 0);
      }
    }
    if (ng == 0) {
      bool ok[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) ok[j] = base + g * 4 + j < G && vb[j];
#pragma unroll
      for (int t = 0; t < GW_QT; ++t) {
        // m[j] = coarse score of query 16 t + r against row base + 4 g + j: +inf when it is not
        // finite, -inf (which no present row has) when the row is absent
        float m[4];
        const int ql = t * 16 + r;
        const Ent last = mylists[ql * GW_L + GW_L - 1];
        bool pass = false;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const float v = acc[t][j];
          m[j] = ok[j] ? (gl_finite(v) ? v : INFINITY) : -INFINITY;
          pass |= ok[j] && gl_better(m[j], base + g * 4 + j, last.s, last.r);
        }
        if (__any(pass)) {
          // lane q (< 16) owns query q's list; the other lanes' candidates come by shuffle
#pragma unroll
          for (int gg = 0; gg < 4; ++gg) {
#pragma unroll
            for (int j = 0; j < 4; ++j) {
              const float cs = __shfl(m[j], gg * 16 + r, 64);
              const int row = base + gg * 4 + j;
              if (lane < 16 && cs > -INFINITY) {
                Ent* L = mylists + ql * GW_L;
                if (gl_better(cs, row, L[GW_L - 1].s, L[GW_L - 1].r)) {
                  dropped[t] = fmaxf(dropped[t], L[GW_L - 1].s);   // -inf while the list is not full
                  int i = GW_L - 1;
                  while (i > 0 && gl_better(cs, row, L[i - 1].s, L[i - 1].r)) { L[i] = L[i - 1]; --i; }
                  L[i] = Ent{cs, row};
                } else {
                  dropped[t] = fmaxf(dropped[t], cs);
                }
              }
            }
          }
        } else {
          dropped[t] = fmaxf(fmaxf(dropped[t], fmaxf(m[0], m[1])), fmaxf(m[2], m[3]));
        }
        acc[t] = f32x4{0.f, 0.f, 0.f, 0.f};
      }
    }
#pragma unroll
    for (int s = 0; s < GW_PF; ++s) { cur[s][0] = nxt[s][0]; cur[s][1] = nxt[s][1]; }
    base = nb;
    grp = ng;
  }
  __syncthreads();

  // the waves' dropped maxima per query, over the query area (no wave reads it any more)
  float* dm = reinterpret_cast<float*>(lds);   // [GL_NW][GW_QB]
#pragma unroll
  for (int t = 0; t < GW_QT; ++t) {
    float v = dropped[t];
    v = fmaxf(v, __shfl_xor(v, 16, 64));
    v = fmaxf(v, __shfl_xor(v, 32, 64));
    if (lane < 16) dm[wave * GW_QB + t * 16 + r] = v;
  }
  __syncthreads();

  // the chunk's list of query ql: the best L of the waves' lists; what the merge leaves behind is
  // dropped as well
  for (int ql = wave; ql < GW_QB; ql += GL_NW) {
    const int q = qb0 + ql;
    if (q >= p.Q) break;
    Local loc;
    loc.clear();
    if (lane < GL_NW * GW_L) {
      const Ent e = lists[((lane / GW_L) * GW_QB + ql) * GW_L + lane % GW_L];
      loc.push(e.s, e.r);
    }
    Ent* out = p.lists + ((int64_t)c * p.Q + q) * GW_L;
    for (int i = 0; i < GW_L; ++i) {
      const Ent e = wave_take_best(loc);
      if (lane == 0) out[i] = e;
    }
    float left = loc.s[0];   // -inf once the lane's entry is taken
    if (lane < GL_NW) left = fmaxf(left, dm[lane * GW_QB + ql]);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) left = fmaxf(left, __shfl_xor(left, o, 64));
    if (lane == 0) p.spill[(int64_t)c * p.Q + q] = left;
  }
}

// ------------------------------------------------------------------------- launch 2: certificate, exact re-score
struct RescoreK {
  const Ent* lists; const float* spill; int nchunks, Q, D, k;
  float eps2;             // 2 eps(D)
  const float* qn; const float* gal;
  float* scores; int* rows;
  const int64_t* labels; float threshold; int64_t* ident;
  uint8_t* flag;          // [Q]: 1 = not certified
  uint8_t* route;         // the caller's copy of flag, or NULL
};

__global__ __launch_bounds__(64) void gallery_rescore_kernel(RescoreK p) {
  __shared__ int cand[GW_C];
  __shared__ float exact[GW_C];
  const int q = blockIdx.x, lane = threadIdx.x;
  const int r = lane & 15, g = lane >> 4;
  const int k = p.k, D = p.D;
  const int n = p.nchunks * GW_L;   // nchunks <= 2^24 (wide_plan)
  auto entry = [&](int j) { return p.lists[((int64_t)(j / GW_L) * p.Q + q) * GW_L + j % GW_L]; };

  // t: the k-th largest finite coarse score (a non-finite one bounds nothing; it is a candidate anyway)
  Local loc;
  loc.clear();
  for (int j0 = lane; j0 < n; j0 += 4 * 64) {
    Ent e[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) e[u] = j0 + u * 64 < n ? entry(j0 + u * 64) : Ent{-INFINITY, GL_EMPTY};
#pragma unroll
    for (int u = 0; u < 4; ++u)
      if (e[u].r != GL_EMPTY && e[u].s < INFINITY) loc.push(e[u].s, e[u].r);
  }
  float t = -INFINITY;
  for (int i = 0; i < k; ++i) {
    const Ent e = wave_take_best(loc);
    if (i == k - 1 && e.r != GL_EMPTY) t = e.s;
  }
  const float bar = t - p.eps2;

  // the candidates, in list order
  int ncand = 0;
  for (int j0 = 0; j0 < n; j0 += 64) {
    const int j = j0 + lane;
    Ent e{-INFINITY, GL_EMPTY};
    if (j < n) e = entry(j);
    const bool is = e.r != GL_EMPTY && e.s >= bar;
    const unsigned long long mask = __ballot(is);
    const int pos = ncand + __popcll(mask & ((1ull << lane) - 1ull));
    if (is && pos < GW_C) cand[pos] = e.r;
    ncand += __popcll(mask);
  }
  bool bad = false;
  for (int ch = lane; ch < p.nchunks; ch += 64) {
    const float sp = p.spill[(int64_t)ch * p.Q + q];
    bad |= !(sp == -INFINITY || sp < bar);   // nothing dropped, or only below the bar
  }
  const bool certified = ncand <= GW_C && !__any(bad);
  if (lane == 0) {
    p.flag[q] = certified ? 0 : 1;
    if (p.route) p.route[q] = certified ? 0 : 1;
  }
  if (!certified) return;
  __syncthreads();

  // gallery_topk_kernel's chain on 16 candidates at a time: A = candidate row tt * 16 + r, B = the
  // query in every column; lane (g, r) holds columns 16 st + 4 g + (0..3) of both
  const float* b = p.qn + (int64_t)q * D + g * 4;
  const int nsteps = D >> 4;
  for (int tt = 0; tt * 16 < ncand; ++tt) {
    const int row = cand[min(tt * 16 + r, ncand - 1)];
    const float* a = p.gal + (int64_t)row * D + g * 4;
    f32x4 acc[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) acc[e] = f32x4{0.f, 0.f, 0.f, 0.f};
    for (int st = 0; st < nsteps; ++st) {
      const f32x4 av = *reinterpret_cast<const f32x4*>(a + st * 16);
      const f32x4 bv = *reinterpret_cast<const f32x4*>(b + st * 16);
#pragma unroll
      for (int e = 0; e < 4; ++e) acc[e] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[e], bv[e], acc[e], 0, 0, 0);
    }
    const f32x4 sc = (acc[0] + acc[1]) + (acc[2] + acc[3]);   // sc[j]: candidate tt * 16 + 4 g + j
    if (r == 0) {
#pragma unroll
      for (int j = 0; j < 4; ++j) exact[tt * 16 + g * 4 + j] = sc[j];
    }
  }
  __syncthreads();

  float s = -INFINITY;
  int rw = GL_EMPTY;
  if (lane < ncand && gl_finite(exact[lane])) { s = exact[lane]; rw = cand[lane]; }
  for (int i = 0; i < k; ++i) {
    float bs = s;
    int br = rw;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      const float os = __shfl_xor(bs, o, 64);
      const int orow = __shfl_xor(br, o, 64);
      if (gl_better(os, orow, bs, br)) { bs = os; br = orow; }
    }
    if (br != GL_EMPTY && rw == br) { s = -INFINITY; rw = GL_EMPTY; }
    if (lane == 0) {
      const bool hit = br != GL_EMPTY;
      p.scores[(int64_t)q * k + i] = hit ? bs : -INFINITY;
      p.rows[(int64_t)q * k + i] = hit ? br : -1;
      if (i == 0 && p.ident) p.ident[q] = (hit && bs >= p.threshold) ? p.labels[br] : (int64_t)-1;
    }
  }
}

// ------------------------------------------------------------------------- launch 3: the fallback list
// one wave: the flagged queries in ascending order (a ballot scan; no atomic append)
__global__ __launch_bounds__(64) void gallery_compact_kernel(const uint8_t* flag, int Q, int* list, int* count) {
  const int lane = threadIdx.x;
  int n = 0;
  for (int q0 = 0; q0 < Q; q0 += 64) {
    const int q = q0 + lane;
    const bool f = q < Q && flag[q];
    const unsigned long long mask = __ballot(f);
    if (f) list[n + __popcll(mask & ((1ull << lane) - 1ull))] = q;
    n += __popcll(mask);
  }
  if (lane == 0) *count = n;
}

// ------------------------------------------------------------------------- host
// query blocks, rows per chunk (a multiple of 64) and chunks of the filter: at least 64 chunks where
// the gallery has them, so that the 8-entry lists rarely overflow, and 512 workgroups or more
struct WidePlan { int nqb, chunk, nchunks; };
inline WidePlan wide_plan(int Q, int G) {
  WidePlan pl;
  pl.nqb = (Q + GW_QB - 1) / GW_QB;
  const int tiles = (G + GL_STEP_ROWS - 1) / GL_STEP_ROWS;
  const int target = 512 / pl.nqb > 64 ? 512 / pl.nqb : 64;
  const int tpc = (tiles + target - 1) / target;
  pl.chunk = tpc * GL_STEP_ROWS;
  pl.nchunks = (tiles + tpc - 1) / tpc;
  return pl;
}

struct WideLayout { int64_t qn, part, qbf, lists, spill, flag, list, count, total; };
inline WideLayout wide_layout(int Q, int G, int k) {
  const WidePlan wp = wide_plan(Q, G);
  const Plan lp = gallery_plan_listed(Q, G);
  WideLayout w;
  int64_t o = 0;
  w.qn = o;    o += align256((int64_t)Q * GL_DMAX * 4);
  w.part = o;  o += align256((int64_t)lp.nchunks * Q * k * (int64_t)sizeof(Ent));
  w.qbf = o;   o += align256((int64_t)Q * GL_DMAX * 2);
  w.lists = o; o += align256((int64_t)wp.nchunks * Q * GW_L * (int64_t)sizeof(Ent));
  w.spill = o; o += align256((int64_t)wp.nchunks * Q * 4);
  w.flag = o;  o += align256(Q);
  w.list = o;  o += align256((int64_t)Q * 4);
  w.count = o; o += 256;
  w.total = o;
  return w;
}

}  // namespace

extern "C" int64_t prpe_gallery_topk_wide_workspace_bytes(int32_t Q, int32_t G, int32_t k) {
  if (Q < 1 || G < 1 || G > GL_GMAX || k < 1 || k > GL_KMAX) return PRPE_EINVAL;
  return wide_layout(Q, G, k).total;
}

extern "C" int prpe_gallery_topk_wide(const float* queries, int64_t q_row_stride, int32_t Q, int32_t D,
                                      const float* gallery, int32_t G, const uint8_t* valid, int32_t k,
                                      float* scores, int32_t* rows, const int64_t* labels, float threshold,
                                      int64_t* ident, uint8_t* route, void* workspace, int64_t workspace_bytes,
                                      void* stream) {
  if (!queries || !gallery || !scores || !rows || !workspace || Q < 1 || G < 1 || G > GL_GMAX || k < 1 ||
      k > GL_KMAX || !dim_ok(D) || q_row_stride < D || (labels == nullptr) != (ident == nullptr) ||
      ((uintptr_t)gallery & 15) || ((uintptr_t)workspace & 255))
    return PRPE_EINVAL;
  if (workspace_bytes < prpe_gallery_topk_wide_workspace_bytes(Q, G, k)) return PRPE_EINVAL;
  const WidePlan wp = wide_plan(Q, G);
  const Plan lp = gallery_plan_listed(Q, G);
  if ((int64_t)wp.nqb * wp.nchunks > 0x7fffffff || (int64_t)lp.nqb * lp.nchunks > 0x7fffffff) return PRPE_EINVAL;
  const WideLayout w = wide_layout(Q, G, k);
  hipStream_t st = as_stream(stream);
  unsigned char* ws = static_cast<unsigned char*>(workspace);
  float* qn = reinterpret_cast<float*>(ws + w.qn);
  __bf16* qbf = reinterpret_cast<__bf16*>(ws + w.qbf);
  Ent* lists = reinterpret_cast<Ent*>(ws + w.lists);
  float* spill = reinterpret_cast<float*>(ws + w.spill);
  uint8_t* flag = ws + w.flag;
  int* list = reinterpret_cast<int*>(ws + w.list);
  int* count = reinterpret_cast<int*>(ws + w.count);

  int e = gallery_launch_normalise_bf16(queries, q_row_stride, Q, D, qn, qbf, st);
  if (e) return e;

  FilterK fk{qbf, gallery, valid, lists, spill, Q, D, G, wp.chunk, wp.nqb};
  const dim3 grid(wp.nqb * wp.nchunks), block(GL_NW * 64);
  if (D % (GW_PF * 32) == 0) hipLaunchKernelGGL(gallery_filter_kernel<true>, grid, block, 0, st, fk);
  else hipLaunchKernelGGL(gallery_filter_kernel<false>, grid, block, 0, st, fk);
  e = launch_status();
  if (e) return e;

  const float eps2 = 2.0f * (float)PRPE_GALLERY_WIDE_EPS(D);
  RescoreK rk{lists, spill, wp.nchunks, Q, D, k, eps2, qn, gallery, scores, rows, labels, threshold, ident, flag, route};
  hipLaunchKernelGGL(gallery_rescore_kernel, dim3(Q), dim3(64), 0, st, rk);
  e = launch_status();
  if (e) return e;

  hipLaunchKernelGGL(gallery_compact_kernel, dim3(1), dim3(64), 0, st, flag, Q, list, count);
  e = launch_status();
  if (e) return e;

  return gallery_launch_listed(qn, Q, D, gallery, G, valid, k, scores, rows, labels, threshold, ident, ws + w.part,
                               list, count, st);
}
