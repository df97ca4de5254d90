// Face identification, the stage after the AdaFace embedding:
//
// prpe_gallery_enrol — L2-normalise fp32 rows (prpe_l2norm's arithmetic, eps 1e-12) into rows
//   [row0, row0 + n) of the gallery, one wave per row. The gallery is the search kernel's operand
//   as it stands: normalised fp32 rows [capacity][D] (exact fp32 operands, D x 4 bytes per row).
// prpe_gallery_topk  — cosine top-k of Q queries against gallery rows [0, G) without the [Q, G]
//   score matrix ever reaching memory. Three launches:
//   0. the queries are normalised into the workspace (the enrol arithmetic);
//   1. a streaming fp32-input MFMA GEMM (v_mfma_f32_16x16x4_f32: every product and sum is an fp32
//      fma, so the operands are exact) whose epilogue is a running top-k. A 4-wave workgroup holds
//      a block of 16 (Q <= 16) or 64 queries in LDS in MFMA fragment order and walks one contiguous
//      chunk of gallery rows; a wave takes 16 rows per step straight from global memory into its
//      A fragments (they are used once: no LDS round trip), double-buffered in registers 128
//      columns at a time. Each wave keeps a sorted k-list per query in LDS; its k-th entry is the
//      admission bar, so after warm-up a 16 x 16 score tile costs one LDS read and four compares
//      per lane. A list is only ever written by ONE lane (lane q of the wave that owns it); the
//      candidates of the other lanes reach it through shuffles. The chunk's lists are merged per
//      query and written to the workspace as [chunk][Q][k] partial lists;
//   2. one wave per query merges the partial lists and applies labels / threshold.
//   Order: score descending, then row ascending -- a total order, so the selected set does not
//   depend on the order candidates arrive in and there are no atomics: two runs give the same bits.
//   Batch independence: a (query, row) score is (a0 + a1) + (a2 + a3), a_e the chain
//   acc = fma(g[c], q[c], acc) over the columns c with c % 4 == e in ascending order (one MFMA per
//   16-column step and e, summing c = 16 st + 4 j + e over j = 0..3), whatever tile, wave, chunk
//   or query block the pair lands in.
// The wide route (gallery_wide.hip) reuses launch 0 with a bf16 copy of the queries
// and, for the queries its filter cannot certify, launches 1 and 2 in their LIST variants.
#pragma clang fp contract(off)
#include "gallery.h"

#include <type_traits>

namespace {

// ------------------------------------------------------------------------- normalise (enrol, queries)
// prpe_l2norm's arithmetic: the squares summed in fp64 (lane-strided, then across the wave),
// norm = (float) sqrt, y = x / max(norm, eps) as an fp32 division. BF16 (the wide route's queries,
// DESIGN.md 5k): ybf receives the same values rounded to nearest even
template <bool BF16>
__global__ __launch_bounds__(256) void gallery_normalise_kernel(const float* x, int64_t ldx, int n, int D, float* y,
                                                                float* norm, __bf16* ybf) {
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= n) return;
  const int lane = threadIdx.x & 63;
  const float* xr = x + (int64_t)row * ldx;
  double s = 0.0;
  for (int c = lane; c < D; c += 64) s += (double)xr[c] * xr[c];
  const float nrm = (float)sqrt(warp_sum_d(s));
  const float den = fmaxf(nrm, GL_EPS);
  for (int c = lane; c < D; c += 64) {
    const float v = xr[c] / den;
    y[(int64_t)row * D + c] = v;
    if constexpr (BF16) ybf[(int64_t)row * D + c] = (__bf16)v;
  }
  if (norm && lane == 0) norm[row] = nrm;
}

// ------------------------------------------------------------------------- phase 1
struct TopkK {
  const float* qn;        // normalised queries [Q][D]
  const float* gal;       // normalised gallery [>= G][D]
  const uint8_t* valid;   // [G] or NULL
  Ent* part;              // [nchunks][Q][k]
  int Q, D, G, k, chunk, nqb;
};
// LIST (the wide route's fallback): the queries are list[0 .. *count), ascending
// indices into qn, whose rows are normalised already; the lists go to part[..][list[i]][..]
struct TopkKL : TopkK {
  const int* list;
  const int* count;
};

template <int QT, bool FULL, bool LIST = false>
__global__ __launch_bounds__(GL_NW * 64) void gallery_topk_kernel(std::conditional_t<LIST, TopkKL, TopkK> p) {
  constexpr int QB = QT * 16;
  constexpr int QS_BYTES = QB * GL_DMAX * 4;
  __shared__ __attribute__((aligned(16))) unsigned char lds[QS_BYTES + GL_NW * QB * GL_KMAX * (int)sizeof(Ent)];
  float* qs = reinterpret_cast<float*>(lds);
  Ent* lists = reinterpret_cast<Ent*>(lds + QS_BYTES);

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int r = lane & 15, g = lane >> 4;
  const int c = (int)blockIdx.x / p.nqb;
  // LIST: the few live query blocks are the first ones; rotated by the chunk, their workgroups
  // spread over all XCDs (workgroup i runs on XCD i % 8) instead of piling onto one
  const int qb0 = (LIST ? ((int)blockIdx.x % p.nqb + c) % p.nqb : (int)blockIdx.x % p.nqb) * QB;
  int nq = p.Q;   // queries of this launch
  if constexpr (LIST) {
    nq = *p.count;
    if (qb0 >= nq) return;
  }
  const int D = p.D, G = p.G, k = p.k;
  const int nsteps = D >> 4;

  // the query block in fragment order: step st of tile t is 64 lanes x 4 floats, lane (g, r)
  // holding columns 16 st + 4 g + (0..3) of query 16 t + r (rows past Q are zeros, never written out)
  const int d4 = D >> 2;
  for (int i = tid; i < QB * d4; i += GL_NW * 64) {
    const int ql = i / d4, col = (i - ql * d4) * 4;
    int q = qb0 + ql;
    f32x4 v = {0.f, 0.f, 0.f, 0.f};
    if (q < nq) {
      if constexpr (LIST) q = p.list[q];
      v = *reinterpret_cast<const f32x4*>(p.qn + (int64_t)q * D + col);
    }
    const int t = ql >> 4, st = col >> 4, gg = (col >> 2) & 3;
    *reinterpret_cast<f32x4*>(qs + ((t * nsteps + st) * 64 + gg * 16 + (ql & 15)) * 4) = v;
  }
  for (int i = tid; i < GL_NW * QB * GL_KMAX; i += GL_NW * 64) lists[i] = Ent{-INFINITY, GL_EMPTY};
  __syncthreads();

  Ent* mylists = lists + wave * QB * GL_KMAX;
  const int r0 = c * p.chunk;
  const int r1 = r0 + min(p.chunk, G - r0);   // r0 < G (gallery_plan); no sum past G is formed
  const int ngroups = (nsteps + GL_PF - 1) / GL_PF;

  // 8 steps of one 16-row tile: lane (g, r) reads columns 16 st + 4 g + (0..3) of row base + r.
  // Rows past G - 1 and steps past the last re-read valid memory (their products are not used)
  auto load = [&](f32x4 (&dst)[GL_PF], int base, int grp) {
    const int row = min(base + r, G - 1);
    const float* src = p.gal + (int64_t)row * D + g * 4;
#pragma unroll
    for (int s = 0; s < GL_PF; ++s) {
      const int st = FULL ? grp * GL_PF + s : min(grp * GL_PF + s, nsteps - 1);
      dst[s] = *reinterpret_cast<const f32x4*>(src + st * 16);
    }
  };

  f32x4 cur[GL_PF], nxt[GL_PF];
  // four accumulators per tile, one per column residue e = c % 4: four independent MFMA chains
  // (the 16x16x4 result is ready 40 cycles after issue, the next can issue after 32), each a
  // quarter of the sum, so the rounding of a score near 1 is that of sums near 1/4
  f32x4 acc[QT][4];
#pragma unroll
  for (int t = 0; t < QT; ++t)
#pragma unroll
    for (int e = 0; e < 4; ++e) acc[t][e] = f32x4{0.f, 0.f, 0.f, 0.f};
  int base = r0 + wave * GL_TILE, grp = 0;
  if (base < r1) load(cur, base, 0);
  while (base < r1) {
    int nb = base, ng = grp + 1;
    if (ng == ngroups) { ng = 0; nb = base + GL_STEP_ROWS; }
    load(nxt, nb, ng);
#pragma unroll
    for (int s = 0; s < GL_PF; ++s) {
      const int st = grp * GL_PF + s;
      if (FULL || st < nsteps) {
#pragma unroll
        for (int t = 0; t < QT; ++t) {
          const f32x4 b = *reinterpret_cast<const f32x4*>(qs + ((t * nsteps + st) * 64 + lane) * 4);
#pragma unroll
          for (int e = 0; e < 4; ++e)
            acc[t][e] = __builtin_amdgcn_mfma_f32_16x16x4f32(cur[s][e], b[e], acc[t][e], 0, 0, 0);
        }
      }
    }
    if (ng == 0) {
      // sc[j] = score of query 16 t + r against row base + 4 g + j
#pragma unroll
      for (int t = 0; t < QT; ++t) {
        const f32x4 sc = (acc[t][0] + acc[t][1]) + (acc[t][2] + acc[t][3]);
        const int ql = t * 16 + r;
        const Ent kth = mylists[ql * GL_KMAX + k - 1];
        bool pass = false;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const int row = base + g * 4 + j;
          pass |= row < G && gl_finite(sc[j]) && gl_better(sc[j], row, kth.s, kth.r);
        }
        if (__any(pass)) {
          // lane q (< 16) owns query q's list; the other lanes' candidates come by shuffle
#pragma unroll
          for (int gg = 0; gg < 4; ++gg) {
#pragma unroll
            for (int j = 0; j < 4; ++j) {
              const float cs = __shfl(sc[j], gg * 16 + r, 64);
              const int row = base + gg * 4 + j;
              if (lane < 16 && row < G && gl_finite(cs)) {
                Ent* L = mylists + ql * GL_KMAX;
                if (gl_better(cs, row, L[k - 1].s, L[k - 1].r) && (!p.valid || p.valid[row])) {
                  int i = k - 1;
                  while (i > 0 && gl_better(cs, row, L[i - 1].s, L[i - 1].r)) { L[i] = L[i - 1]; --i; }
                  L[i] = Ent{cs, row};
                }
              }
            }
          }
        }
#pragma unroll
        for (int e = 0; e < 4; ++e) acc[t][e] = f32x4{0.f, 0.f, 0.f, 0.f};
      }
    }
#pragma unroll
    for (int s = 0; s < GL_PF; ++s) cur[s] = nxt[s];
    base = nb;
    grp = ng;
  }
  __syncthreads();

  // the chunk's list of query ql: the best k of the waves' lists
  for (int ql = wave; ql < QB; ql += GL_NW) {
    int q = qb0 + ql;
    if (q >= nq) break;
    if constexpr (LIST) q = p.list[q];
    Local loc;
    loc.clear();
    if (lane < GL_NW * k) {
      const Ent e = lists[((lane / k) * QB + ql) * GL_KMAX + lane % k];
      loc.push(e.s, e.r);
    }
    Ent* out = p.part + ((int64_t)c * p.Q + q) * k;
    for (int i = 0; i < k; ++i) {
      const Ent e = wave_take_best(loc);
      if (lane == 0) out[i] = e;
    }
  }
}

// ------------------------------------------------------------------------- phase 2
struct MergeK {
  const Ent* part; int nchunks, Q, k;
  float* scores; int* rows;
  const int64_t* labels; float threshold; int64_t* ident;
};

struct MergeKL : MergeK {
  const int* list;
  const int* count;
};

template <bool LIST = false>
__global__ __launch_bounds__(64) void gallery_merge_kernel(std::conditional_t<LIST, MergeKL, MergeK> p) {
  int q = blockIdx.x;
  const int lane = threadIdx.x;
  if constexpr (LIST) {
    if (q >= *p.count) return;
    q = p.list[q];
  }
  const int k = p.k;
  Local loc;
  loc.clear();
  const int64_t n = (int64_t)p.nchunks * k;
  for (int64_t j = lane; j < n; j += 64) {
    const int64_t ch = j / k;
    const Ent e = p.part[(ch * p.Q + q) * k + (j - ch * k)];
    loc.push(e.s, e.r);
  }
  for (int i = 0; i < k; ++i) {
    const Ent e = wave_take_best(loc);
    if (lane == 0) {
      const bool hit = e.r != GL_EMPTY;
      p.scores[(int64_t)q * k + i] = hit ? e.s : -INFINITY;
      p.rows[(int64_t)q * k + i] = hit ? e.r : -1;
      if (i == 0 && p.ident) p.ident[q] = (hit && e.s >= p.threshold) ? p.labels[e.r] : (int64_t)-1;
    }
  }
}

}  // namespace

extern "C" int prpe_gallery_enrol(const float* x, int64_t x_row_stride, int32_t n, int32_t D, float* gallery,
                                  float* norms, int32_t capacity, int32_t row0, void* stream) {
  if (!x || !gallery || !norms || n < 1 || !dim_ok(D) || capacity < 1 || row0 < 0 ||
      (int64_t)row0 + n > capacity || x_row_stride < D || ((uintptr_t)gallery & 15))
    return PRPE_EINVAL;
  hipLaunchKernelGGL(gallery_normalise_kernel<false>, dim3((n + 3) / 4), dim3(256), 0, as_stream(stream), x,
                     x_row_stride, n, D, gallery + (int64_t)row0 * D, norms + row0, static_cast<__bf16*>(nullptr));
  return launch_status();
}

extern "C" int64_t prpe_gallery_topk_workspace_bytes(int32_t Q, int32_t G, int32_t k) {
  if (Q < 1 || G < 1 || G > GL_GMAX || k < 1 || k > GL_KMAX) return PRPE_EINVAL;
  const Plan pl = gallery_plan(Q, G);
  return align256((int64_t)Q * GL_DMAX * 4) + align256((int64_t)pl.nchunks * Q * k * (int64_t)sizeof(Ent));
}

extern "C" int prpe_gallery_topk(const float* queries, int64_t q_row_stride, int32_t Q, int32_t D,
                                 const float* gallery, int32_t G, const uint8_t* valid, int32_t k, float* scores,
                                 int32_t* rows, const int64_t* labels, float threshold, int64_t* ident,
                                 void* workspace, int64_t workspace_bytes, void* stream) {
  if (!queries || !gallery || !scores || !rows || !workspace || Q < 1 || G < 1 || G > GL_GMAX || k < 1 ||
      k > GL_KMAX || !dim_ok(D) || q_row_stride < D || (labels == nullptr) != (ident == nullptr) ||
      ((uintptr_t)gallery & 15) || ((uintptr_t)workspace & 255))
    return PRPE_EINVAL;
  if (workspace_bytes < prpe_gallery_topk_workspace_bytes(Q, G, k)) return PRPE_EINVAL;
  const Plan pl = gallery_plan(Q, G);
  if ((int64_t)pl.nqb * pl.nchunks > 0x7fffffff) return PRPE_EINVAL;
  hipStream_t st = as_stream(stream);
  float* qn = static_cast<float*>(workspace);
  Ent* part = reinterpret_cast<Ent*>(static_cast<unsigned char*>(workspace) + align256((int64_t)Q * GL_DMAX * 4));

  hipLaunchKernelGGL(gallery_normalise_kernel<false>, dim3((Q + 3) / 4), dim3(256), 0, st, queries, q_row_stride, Q,
                     D, qn, static_cast<float*>(nullptr), static_cast<__bf16*>(nullptr));
  int e = launch_status();
  if (e) return e;

  TopkK tk{qn, gallery, valid, part, Q, D, G, k, pl.chunk, pl.nqb};
  const dim3 grid(pl.nqb * pl.nchunks), block(GL_NW * 64);
  const bool full = D % (GL_PF * 16) == 0;
  if (pl.qb == 16) {
    if (full) hipLaunchKernelGGL((gallery_topk_kernel<1, true>), grid, block, 0, st, tk);
    else hipLaunchKernelGGL((gallery_topk_kernel<1, false>), grid, block, 0, st, tk);
  } else {
    if (full) hipLaunchKernelGGL((gallery_topk_kernel<4, true>), grid, block, 0, st, tk);
    else hipLaunchKernelGGL((gallery_topk_kernel<4, false>), grid, block, 0, st, tk);
  }
  e = launch_status();
  if (e) return e;

  MergeK mk{part, pl.nchunks, Q, k, scores, rows, labels, threshold, ident};
  hipLaunchKernelGGL(gallery_merge_kernel<false>, dim3(Q), dim3(64), 0, st, mk);
  return launch_status();
}

int gallery_launch_normalise_bf16(const float* queries, int64_t q_row_stride, int Q, int D, float* qn, __bf16* qbf,
                                  hipStream_t st) {
  hipLaunchKernelGGL(gallery_normalise_kernel<true>, dim3((Q + 3) / 4), dim3(256), 0, st, queries, q_row_stride, Q,
                     D, qn, static_cast<float*>(nullptr), qbf);
  return launch_status();
}

int gallery_launch_listed(const float* qn, int Q, int D, const float* gallery, int G, const uint8_t* valid, int k,
                          float* scores, int32_t* rows, const int64_t* labels, float threshold, int64_t* ident,
                          void* part, const int* list, const int* count, hipStream_t st) {
  const Plan pl = gallery_plan_listed(Q, G);
  if ((int64_t)pl.nqb * pl.nchunks > 0x7fffffff) return PRPE_EINVAL;
  TopkKL tk{{qn, gallery, valid, static_cast<Ent*>(part), Q, D, G, k, pl.chunk, pl.nqb}, list, count};
  const dim3 grid(pl.nqb * pl.nchunks), block(GL_NW * 64);
  const bool full = D % (GL_PF * 16) == 0;
  if (pl.qb == 16) {
    if (full) hipLaunchKernelGGL((gallery_topk_kernel<1, true, true>), grid, block, 0, st, tk);
    else hipLaunchKernelGGL((gallery_topk_kernel<1, false, true>), grid, block, 0, st, tk);
  } else {
    if (full) hipLaunchKernelGGL((gallery_topk_kernel<4, true, true>), grid, block, 0, st, tk);
    else hipLaunchKernelGGL((gallery_topk_kernel<4, false, true>), grid, block, 0, st, tk);
  }
  int e = launch_status();
  if (e) return e;
  MergeKL mk{{static_cast<const Ent*>(part), pl.nchunks, Q, k, scores, rows, labels, threshold, ident}, list, count};
  hipLaunchKernelGGL(gallery_merge_kernel<true>, dim3(Q), dim3(64), 0, st, mk);
  return launch_status();
}
