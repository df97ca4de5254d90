// Open-set 1:N identification evaluation: prpe_ident_best (pass 1),
// prpe_ident_rank (pass 2) and prpe_ident_finish; the semantics are stated in include/prpe.h.
//
// Both passes are the all-pairs GEMM of csrc/pairhist.hip with another epilogue. The tile product
// -- the walk over 128 x 128 score tiles (the rectangle, or the upper triangle in self mode), the
// LDS staging, the MFMA loop and the score bits, pair_hist's and gallery_topk's -- is
// csrc/pairs.h's; rows past M / N re-read the last row and are masked by their flag.
//
// A candidate of a probe is one 64-bit key, image(score) << 32 | (0xFFFFFFFF - row): a larger key
// is an earlier entry of gallery_topk's order (score descending, row ascending); 0 is "none".
// The row side of a tile serves the probes of its a rows with its b rows as candidates; in self
// mode the pairs i < j are taken and the column side serves probe j with row i as well.
// Pass 1 keeps, per probe, the largest key among the candidates of its own label (mate) and among
// the others (non): a lane reduces its 4 columns (8 rows) in registers, the 16 (4) lanes that
// share a row (column) by shuffles, the 2 (4) waves that share it by a 64-bit max in LDS, and one
// global 64-bit atomicMax per non-empty slot and tile leaves the workgroup. A max commutes.
// Pass 2 reads mate_key of the tile's probes into LDS and counts, the same way with integer adds,
// the non-mate candidates whose key is greater.
#pragma clang fp contract(off)
#include "pairs.h"

namespace {

constexpr int ID_T = pairs::T;
constexpr int ID_RANKS = PRPE_IDENT_RANKS;     // R: rank_hist has R + 1 slots
constexpr int ID_MAXBINS = 4096;
enum : uint8_t { ID_CAND = 1, ID_PROBE = 2 };

struct IdentK {
  const float* a;
  const float* b;
  int64_t lda, ldb;
  const int64_t* la;
  const int64_t* lb;
  const uint8_t* va;
  const uint8_t* vb;
  unsigned long long* mate;      // pass 2 only reads it
  unsigned long long* non;
  unsigned long long* skipped;
  int* rank;
  int M, N, D, self, tn, brow0;
  int64_t ntiles;
};

// order-preserving uint32 image of a finite float: -0 becomes +0, then csrc/track.hip's sign flip.
// No finite score gives 0
__device__ __forceinline__ unsigned id_image(float s) {
  if (s == 0.f) s = 0.f;
  const unsigned u = __float_as_uint(s);
  return u ^ ((u >> 31) ? 0xffffffffu : 0x80000000u);
}
__device__ __forceinline__ float id_score(unsigned img) {
  return __uint_as_float(img ^ ((img >> 31) ? 0x80000000u : 0xffffffffu));
}
__device__ __forceinline__ unsigned long long id_max(unsigned long long x, unsigned long long y) { return x > y ? x : y; }

// PASS 1: best mate and best non-mate. PASS 2: non-mates ahead of the best mate. SELF: p.self,
// known to the compiler, so that cross mode carries no column side
template <int PASS, bool SELF>
__global__ __launch_bounds__(pairs::NT) void ident_kernel(IdentK p) {
  __shared__ pairs::Frag frag;
  __shared__ long long lab[2][ID_T];                               // [side][slot]
  __shared__ unsigned long long lkey[2][PASS == 1 ? 2 : 1][ID_T];   // pass 1: [side][mate | non]; pass 2: mate_key
  __shared__ int lcnt[2][PASS == 2 ? ID_T : 1];                    // pass 2: the slot's count
  __shared__ uint8_t flag[2][ID_T];                                // ID_CAND | ID_PROBE

  const pairs::Lane ln;
  const int tid = ln.tid;
  const int nchunks = p.D / pairs::KC;
  constexpr bool self = SELF;
  unsigned myskip = 0;

  for (int64_t id = blockIdx.x; id < p.ntiles; id += gridDim.x) {
    int ti, tj;
    pairs::tile_of(id, p.tn, self, ti, tj);
    const int row0 = ti * ID_T, col0 = tj * ID_T;

    __syncthreads();   // the previous tile's flush has read lkey, lcnt and flag
    if (tid < 2 * ID_T) {
      const int side = tid >> 7, i = tid & (ID_T - 1);
      const int row = (side ? col0 : row0) + i;
      const int64_t* L = side ? p.lb : p.la;
      const uint8_t* V = side ? p.vb : p.va;
      long long l = -1;
      uint8_t f = 0;
      if (row < (side ? p.N : p.M) && (!V || V[row])) {
        l = L[row];
        // cross mode: the a side holds probes only, the b side candidates only
        f = (uint8_t)((self || side ? ID_CAND : 0) | ((self || !side) && l >= 0 ? ID_PROBE : 0));
      }
      lab[side][i] = l;
      flag[side][i] = f;
      if (PASS == 1) {
        lkey[side][0][i] = 0ull;
        lkey[side][1][i] = 0ull;
      } else {
        lkey[side][0][i] = (f & ID_PROBE) ? p.mate[row] : 0ull;
        lcnt[side][i] = 0;
      }
    }

    pairs::Acc acc;
    pairs::clear(acc);
    pairs::product(frag, acc, ln, p.a, p.lda, p.M, p.b, p.ldb, p.N, row0, col0, nchunks);

    long long lbj[pairs::WN];
    uint8_t fj[pairs::WN];
    unsigned long long cm[pairs::WN], cn[pairs::WN];   // column side: best keys; pass 2: cm is mate_key
    int cc[pairs::WN];                                 // pass 2: the column's count
#pragma unroll
    for (int j = 0; j < pairs::WN; ++j) {
      lbj[j] = lab[1][ln.jl(j)];
      fj[j] = flag[1][ln.jl(j)];
      cm[j] = PASS == 2 && self ? lkey[1][0][ln.jl(j)] : 0ull;
      cn[j] = 0ull;
      cc[j] = 0;
    }
#pragma unroll
    for (int i = 0; i < pairs::WM; ++i) {
      const int il = ln.il(i);
      long long lai[4];
      uint8_t fi[4];
      unsigned long long rm[4], rn[4];                 // row side, as cm, cn and cc
      int rc[4];
#pragma unroll
      for (int reg = 0; reg < 4; ++reg) {
        lai[reg] = lab[0][il + reg];
        fi[reg] = flag[0][il + reg];
        rm[reg] = PASS == 2 ? lkey[0][0][il + reg] : 0ull;
        rn[reg] = 0ull;
        rc[reg] = 0;
      }
#pragma unroll
      for (int j = 0; j < pairs::WN; ++j) {
        const f32x4 sc = pairs::score(acc, i, j);
        const int gj = col0 + ln.jl(j);
#pragma unroll
        for (int reg = 0; reg < 4; ++reg) {
          const int gi = row0 + il + reg;
          const float s = sc[reg];
          const bool pair = !self || gi < gj;
          const bool fin = pairs::finite(s), same = lai[reg] == lbj[j];
          const unsigned long long img = (unsigned long long)id_image(s) << 32;
          const bool ron = pair && (fi[reg] & ID_PROBE) && (fj[j] & ID_CAND);
          const bool con = self && pair && (fj[j] & ID_PROBE) && (fi[reg] & ID_CAND);
          const unsigned long long rkey = img | (0xFFFFFFFFu - ((unsigned)p.brow0 + (unsigned)gj));
          const unsigned long long ckey = img | (0xFFFFFFFFu - (unsigned)gi);
          if (PASS == 1) {
            myskip += (unsigned)(ron && !fin) + (unsigned)(con && !fin);
            const unsigned long long rk = ron && fin ? rkey : 0ull, ck = con && fin ? ckey : 0ull;
            rm[reg] = id_max(rm[reg], same ? rk : 0ull);
            rn[reg] = id_max(rn[reg], same ? 0ull : rk);
            cm[j] = id_max(cm[j], same ? ck : 0ull);
            cn[j] = id_max(cn[j], same ? 0ull : ck);
          } else {
            // a probe without a mate (or none at all) holds mate_key 0 and counts nothing
            rc[reg] += (int)(ron && fin && !same && rm[reg] != 0ull && rkey > rm[reg]);
            cc[j] += (int)(con && fin && !same && cm[j] != 0ull && ckey > cm[j]);
          }
        }
      }
      // the 16 lanes of equal g hold the same 4 rows
      if (PASS == 1) {
        const bool mates = __any((rm[0] | rm[1] | rm[2] | rm[3]) != 0ull);   // rare: most tiles hold no mate
#pragma unroll
        for (int reg = 0; reg < 4; ++reg) {
#pragma unroll
          for (int o = 1; o < 16; o <<= 1) {
            rn[reg] = id_max(rn[reg], __shfl_xor(rn[reg], o, 64));
            if (mates) rm[reg] = id_max(rm[reg], __shfl_xor(rm[reg], o, 64));
          }
          if (ln.r == 0) {
            if (rm[reg]) atomicMax(&lkey[0][0][il + reg], rm[reg]);
            if (rn[reg]) atomicMax(&lkey[0][1][il + reg], rn[reg]);
          }
        }
      } else {
#pragma unroll
        for (int reg = 0; reg < 4; ++reg) {
          int c = rc[reg];
#pragma unroll
          for (int o = 1; o < 16; o <<= 1) c += __shfl_xor(c, o, 64);
          if (ln.r == 0 && c) atomicAdd(&lcnt[0][il + reg], c);
        }
      }
    }
    // the 4 lanes of equal r hold the same 4 columns
    if (self) {
#pragma unroll
      for (int j = 0; j < pairs::WN; ++j) {
        const int jl = ln.jl(j);
        if (PASS == 1) {
#pragma unroll
          for (int o = 16; o < 64; o <<= 1) {
            cm[j] = id_max(cm[j], __shfl_xor(cm[j], o, 64));
            cn[j] = id_max(cn[j], __shfl_xor(cn[j], o, 64));
          }
          if (ln.g == 0) {
            if (cm[j]) atomicMax(&lkey[1][0][jl], cm[j]);
            if (cn[j]) atomicMax(&lkey[1][1][jl], cn[j]);
          }
        } else {
          int c = cc[j];
#pragma unroll
          for (int o = 16; o < 64; o <<= 1) c += __shfl_xor(c, o, 64);
          if (ln.g == 0 && c) atomicAdd(&lcnt[1][jl], c);
        }
      }
    }

    // a non-empty slot belongs to a probe, so its row lies below M
    __syncthreads();
    if (PASS == 1) {
      const int side = tid >> 8, kind = (tid >> 7) & 1, i = tid & (ID_T - 1);
      if (side == 0 || self) {
        const unsigned long long k = lkey[side][kind][i];
        if (k) atomicMax((kind ? p.non : p.mate) + (side ? col0 : row0) + i, k);
      }
    } else if (tid < 2 * ID_T) {
      const int side = tid >> 7, i = tid & (ID_T - 1);
      if (side == 0 || self) {
        const int c = lcnt[side][i];
        if (c) atomicAdd(p.rank + (side ? col0 : row0) + i, c);
      }
    }
  }
  if (PASS == 1) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) myskip += __shfl_xor(myskip, o, 64);
    if (ln.lane == 0 && myskip) atomicAdd(p.skipped, (unsigned long long)myskip);
  }
}

// ---- finish: one thread per probe; a block's bins in LDS, flushed with 64-bit atomic adds
struct FinishK {
  const int64_t* la;
  const uint8_t* va;
  const unsigned long long* mate;
  const unsigned long long* non;
  const int* rm1;                 // optional
  float* mate_score;
  int* mate_row;
  float* non_score;
  int* non_row;
  int* rank;
  unsigned long long* hist;       // [3][nbins]
  unsigned long long* rank_hist;  // [R + 1], with rm1
  unsigned long long* counts;     // [4]
  int M, nbins;
};
constexpr int ID_FIN_NT = 256;
constexpr int ID_FIN_CELLS = 3 * ID_MAXBINS + ID_RANKS + 1 + 4;

__global__ __launch_bounds__(ID_FIN_NT) void ident_finish_kernel(FinishK p) {
  __shared__ unsigned cnt[ID_FIN_CELLS];        // hist, then rank_hist, then counts: a cell grows by at most M <= 2^24
  const int tid = threadIdx.x, nbins = p.nbins;
  const int cells = 3 * nbins + ID_RANKS + 1 + 4;
  unsigned* const crank = cnt + 3 * nbins;
  unsigned* const ccount = crank + ID_RANKS + 1;
  const float h = (float)(nbins >> 1);
  for (int i = tid; i < cells; i += ID_FIN_NT) cnt[i] = 0;
  __syncthreads();
  auto bin = [&](float s) {   // prpe_pair_hist's rule
    const float t = fminf(fmaxf(floorf(s * h), -h), h - 1.f);
    return (int)t + (nbins >> 1);
  };
  for (int64_t i = (int64_t)blockIdx.x * ID_FIN_NT + tid; i < p.M; i += (int64_t)gridDim.x * ID_FIN_NT) {
    const bool probe = (!p.va || p.va[i]) && p.la[i] >= 0;
    const unsigned long long mk = probe ? p.mate[i] : 0ull, nk = probe ? p.non[i] : 0ull;
    const float ms = mk ? id_score((unsigned)(mk >> 32)) : -INFINITY;
    const float ns = nk ? id_score((unsigned)(nk >> 32)) : -INFINITY;
    int rank = 0;
    if (mk) rank = p.rm1 ? p.rm1[i] + 1 : (mk > nk ? 1 : -1);
    p.mate_score[i] = ms;
    p.mate_row[i] = mk ? (int)(0xFFFFFFFFu - (unsigned)mk) : -1;
    p.non_score[i] = ns;
    p.non_row[i] = nk ? (int)(0xFFFFFFFFu - (unsigned)nk) : -1;
    p.rank[i] = rank;
    if (!probe) {
      atomicAdd(ccount + 2, 1u);
    } else if (mk) {
      atomicAdd(ccount + 0, 1u);
      if (mk > nk) atomicAdd(cnt + bin(ms), 1u);
      else atomicAdd(cnt + nbins + bin(ns), 1u);
      // rank >= 1 when the caller zeroed rank_minus_1; the lower clamp keeps a slot inside crank if not
      if (p.rm1) atomicAdd(crank + (rank < 1 ? 1 : (rank < ID_RANKS + 1 ? rank : ID_RANKS + 1)) - 1, 1u);
    } else {
      atomicAdd(ccount + 1, 1u);
      if (nk) atomicAdd(cnt + 2 * nbins + bin(ns), 1u);
      else atomicAdd(ccount + 3, 1u);
    }
  }
  __syncthreads();
  for (int i = tid; i < cells; i += ID_FIN_NT) {
    const unsigned v = cnt[i];
    if (!v) continue;
    unsigned long long* dst = i < 3 * nbins ? p.hist + i
                              : (i < 3 * nbins + ID_RANKS + 1 ? p.rank_hist + (i - 3 * nbins)
                                                              : p.counts + (i - 3 * nbins - ID_RANKS - 1));
    atomicAdd(dst, (unsigned long long)v);
  }
}

inline bool id_nbins_ok(int nbins) {
  for (int l = 8; l <= 12; ++l)
    if (nbins == 1 << l) return true;
  return false;
}
inline bool id_al8(const void* q) { return q && !((uintptr_t)q & 7); }

// the operand checks both passes share; fills p
inline bool id_args(IdentK& p, const float* a, int64_t lda, int M, const int64_t* la, const uint8_t* va, const float* b,
                    int64_t ldb, int N, const int64_t* lb, const uint8_t* vb, int brow0, int D) {
  if (!pairs::rows_ok(a, lda, M, D) || !la) return false;
  const bool self = b == nullptr;
  if (self) {
    if (lb || vb || brow0 != 0) return false;
  } else if (!lb || !pairs::rows_ok(b, ldb, N, D) || brow0 < 0 || brow0 > INT32_MAX - N) {
    return false;
  }
  p = IdentK{};
  p.a = a;
  p.lda = lda;
  p.la = la;
  p.va = va;
  p.M = M;
  p.b = self ? a : b;
  p.ldb = self ? lda : ldb;
  p.lb = self ? la : lb;
  p.vb = self ? va : vb;
  p.N = self ? M : N;
  p.D = D;
  p.self = self ? 1 : 0;
  p.brow0 = brow0;
  const pairs::Tiles tl = pairs::tiles(p.M, p.N, self);
  p.tn = tl.tn;
  p.ntiles = tl.ntiles;
  return true;
}

}  // namespace

extern "C" int prpe_ident_best(const float* a, int64_t a_row_stride, int32_t M, const int64_t* a_labels,
                               const uint8_t* a_valid, const float* b, int64_t b_row_stride, int32_t N,
                               const int64_t* b_labels, const uint8_t* b_valid, int32_t b_row0, int32_t D,
                               uint64_t* mate_key, uint64_t* non_key, uint64_t* skipped, void* stream) {
  IdentK p;
  if (!id_al8(mate_key) || !id_al8(non_key) || !id_al8(skipped) ||
      !id_args(p, a, a_row_stride, M, a_labels, a_valid, b, b_row_stride, N, b_labels, b_valid, b_row0, D))
    return PRPE_EINVAL;
  p.mate = reinterpret_cast<unsigned long long*>(mate_key);
  p.non = reinterpret_cast<unsigned long long*>(non_key);
  p.skipped = reinterpret_cast<unsigned long long*>(skipped);
  void (*const kernel)(IdentK) = p.self ? ident_kernel<1, true> : ident_kernel<1, false>;
  hipLaunchKernelGGL(kernel, dim3(pairs::grid(p.ntiles)), dim3(pairs::NT), 0, as_stream(stream), p);
  return launch_status();
}

extern "C" int prpe_ident_rank(const float* a, int64_t a_row_stride, int32_t M, const int64_t* a_labels,
                               const uint8_t* a_valid, const float* b, int64_t b_row_stride, int32_t N,
                               const int64_t* b_labels, const uint8_t* b_valid, int32_t b_row0, int32_t D,
                               const uint64_t* mate_key, int32_t* rank_minus_1, void* stream) {
  IdentK p;
  if (!id_al8(mate_key) || !rank_minus_1 ||
      !id_args(p, a, a_row_stride, M, a_labels, a_valid, b, b_row_stride, N, b_labels, b_valid, b_row0, D))
    return PRPE_EINVAL;
  p.mate = reinterpret_cast<unsigned long long*>(const_cast<uint64_t*>(mate_key));
  p.rank = rank_minus_1;
  void (*const kernel)(IdentK) = p.self ? ident_kernel<2, true> : ident_kernel<2, false>;
  hipLaunchKernelGGL(kernel, dim3(pairs::grid(p.ntiles)), dim3(pairs::NT), 0, as_stream(stream), p);
  return launch_status();
}

extern "C" int prpe_ident_finish(int32_t M, const int64_t* a_labels, const uint8_t* a_valid, const uint64_t* mate_key,
                                 const uint64_t* non_key, const int32_t* rank_minus_1, int32_t nbins, float* mate_score,
                                 int32_t* mate_row, float* non_score, int32_t* non_row, int32_t* rank, uint64_t* hist,
                                 uint64_t* rank_hist, uint64_t* counts, void* stream) {
  if (M < 1 || M > pairs::MAXROWS || !a_labels || !id_al8(mate_key) || !id_al8(non_key) || !id_nbins_ok(nbins) ||
      !mate_score || !mate_row || !non_score || !non_row || !rank || !id_al8(hist) || !id_al8(counts) ||
      (rank_minus_1 ? !id_al8(rank_hist) : rank_hist != nullptr))
    return PRPE_EINVAL;
  FinishK p;
  p.la = a_labels;
  p.va = a_valid;
  p.mate = reinterpret_cast<const unsigned long long*>(mate_key);
  p.non = reinterpret_cast<const unsigned long long*>(non_key);
  p.rm1 = rank_minus_1;
  p.mate_score = mate_score;
  p.mate_row = mate_row;
  p.non_score = non_score;
  p.non_row = non_row;
  p.rank = rank;
  p.hist = reinterpret_cast<unsigned long long*>(hist);
  p.rank_hist = reinterpret_cast<unsigned long long*>(rank_hist);
  p.counts = reinterpret_cast<unsigned long long*>(counts);
  p.M = M;
  p.nbins = nbins;
  const int blocks = (M + ID_FIN_NT - 1) / ID_FIN_NT;
  hipLaunchKernelGGL(ident_finish_kernel, dim3(blocks < 256 ? blocks : 256), dim3(ID_FIN_NT), 0, as_stream(stream), p);
  return launch_status();
}
