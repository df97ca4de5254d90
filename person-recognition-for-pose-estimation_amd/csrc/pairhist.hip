// 1:1 face verification: prpe_pair_hist -- the scores of all pairs between two
// sets of L2-normalised fp32 rows (prpe_gallery_enrol's output), binned into a genuine and an
// impostor histogram. A GEMM whose epilogue is a histogram: the score matrix never reaches memory.
//
// Score bits: those of prpe_gallery_topk (csrc/gallery.hip). score = (a0 + a1) + (a2 + a3), a_e the
// chain acc = fma(x[c], y[c], acc) over the columns c with c % 4 == e in ascending order: one
// v_mfma_f32_16x16x4_f32 per 16-column step and e, exact fp32 operands, K walked in ascending
// 16-column steps, whatever tile, wave or workgroup the pair lands in. A product commutes, so
// score(i, j) == score(j, i).
//
// Tiling: an 8-wave workgroup takes a 128 x 128 score tile, a wave 32 x 64 of it (2 x 4 MFMA tiles,
// 4 accumulators each: 32 independent chains, 128 accumulator registers; two waves per SIMD).
// BOTH operands are reused across the tile, so both go through LDS in MFMA fragment order, 32
// columns at a time, double buffered: the next chunk is fetched into registers under the MFMAs of
// this one and stored after them; one barrier per chunk. A lane's global read (row r, columns 4 g ..) is the fragment it
// stores, so the LDS image is written and read linearly (no bank conflict on either side).
// The grid is one workgroup per CU, each walking tiles id, id + grid, ..: row-major over the
// rectangle (cross mode) or over the upper triangle of tiles (self mode; diagonal tiles mask
// i < j). Rows past M / N re-read the last row and are masked by their label.
//
// Histogram: uint32 counters in LDS, [class][bin][copy] with 4096 / nbins interleaved copies per
// bin (a lane adds to copy lane % copies: impostor scores pile up around 0, and the copies of one
// bin lie on neighbouring banks), flushed with 64-bit atomic adds to hist at the end of the walk
// and every PH_FLUSH_TILES tiles (a counter grows by at most 128 x 128 per tile). Integer adds
// commute: two runs give the same numbers.
#pragma clang fp contract(off)
#include "common.h"

namespace {

constexpr int PH_T = 128;                     // score tile of a workgroup (rows and columns)
constexpr int PH_NW = 8;                      // waves, 4 x 2, 32 x 64 scores each
constexpr int PH_NT = PH_NW * 64;
constexpr int PH_WM = 2, PH_WN = 4;           // 16-row MFMA tiles per wave: rows of a, rows of b
constexpr int PH_KC = 32;                     // columns per LDS chunk: two 16-column steps
constexpr int PH_F4 = PH_T * PH_KC / 4;       // float4 per operand and chunk
constexpr int PH_LD = PH_F4 / PH_NT;          // float4 a thread moves per operand and chunk
constexpr int PH_HIST = 4096;                 // private counters per class (nbins x copies)
constexpr unsigned PH_FLUSH_TILES = (unsigned)((1ull << 32) / (PH_T * PH_T)) - 1;
constexpr int PH_MAXROWS = 1 << 24;

struct PairK {
  const float* a;
  const float* b;
  int64_t lda, ldb;
  const int64_t* la;
  const int64_t* lb;
  const uint8_t* va;
  const uint8_t* vb;
  unsigned long long* hist;
  unsigned long long* skipped;
  int M, N, D, lbins, self, tn;
  int64_t ntiles;
};

__device__ __forceinline__ bool ph_finite(float v) { return fabsf(v) <= 3.402823466e38f; }   // false for NaN

// tile id of the upper triangle (row-major, row ti holds tj = ti .. nt - 1) -> (ti, tj)
__device__ __forceinline__ void tri_tile(int64_t id, int nt, int& ti, int& tj) {
  const double b = 2.0 * nt + 1.0;
  int64_t t = (int64_t)((b - sqrt(b * b - 8.0 * (double)id)) * 0.5);
  t = t < 0 ? 0 : (t > nt - 1 ? nt - 1 : t);
  auto off = [nt](int64_t x) { return x * nt - x * (x - 1) / 2; };
  while (t > 0 && off(t) > id) --t;
  while (t + 1 < nt && off(t + 1) <= id) ++t;
  ti = (int)t;
  tj = (int)(t + (id - off(t)));
}

__global__ __launch_bounds__(PH_NT) void pair_hist_kernel(PairK p) {
  __shared__ f32x4 frag[2][2][PH_F4];          // [buffer][operand][(tile, step, g, r)]: 64 KB
  __shared__ unsigned cnt[2 * PH_HIST];        // [class][bin][copy]: 32 KB
  __shared__ long long lab[2][PH_T];           // the tile's labels, -1: the row takes part in no pair

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int r = lane & 15, g = lane >> 4;
  const int wm = wave >> 1, wn = wave & 1;
  const int nbins = 1 << p.lbins, cshift = 12 - p.lbins, copy = lane & ((1 << cshift) - 1);
  const float h = (float)(nbins >> 1);
  const int nchunks = p.D / PH_KC;

  for (int i = tid; i < 2 * PH_HIST; i += PH_NT) cnt[i] = 0;
  unsigned since = 0, myskip = 0;

  // the private counters added to hist and cleared; every thread of the workgroup calls it
  auto flush = [&]() {
    __syncthreads();
    for (int i = tid; i < 2 * nbins; i += PH_NT) {
      unsigned* c = cnt + (i >> p.lbins) * PH_HIST + ((i & (nbins - 1)) << cshift);
      unsigned long long sum = 0;
      for (int k = 0; k < (1 << cshift); ++k) { sum += c[k]; c[k] = 0; }
      if (sum) atomicAdd(p.hist + i, sum);
    }
    unsigned sk = myskip;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) sk += __shfl_xor(sk, o, 64);
    if (lane == 0 && sk) atomicAdd(p.skipped, (unsigned long long)sk);
    myskip = 0;
    __syncthreads();
  };

  f32x4 acc[PH_WM][PH_WN][4];
#pragma unroll
  for (int i = 0; i < PH_WM; ++i)
#pragma unroll
    for (int j = 0; j < PH_WN; ++j)
#pragma unroll
      for (int e = 0; e < 4; ++e) acc[i][j][e] = f32x4{0.f, 0.f, 0.f, 0.f};

  for (int64_t id = blockIdx.x; id < p.ntiles; id += gridDim.x) {
    int ti, tj;
    if (p.self) {
      tri_tile(id, p.tn, ti, tj);
    } else {
      ti = (int)(id / p.tn);
      tj = (int)(id - (int64_t)ti * p.tn);
    }
    const int row0 = ti * PH_T, col0 = tj * PH_T;

    __syncthreads();   // the previous tile's epilogue has read lab (first tile: cnt is cleared)
    if (tid < 2 * PH_T) {
      const int side = tid >> 7, i = tid & (PH_T - 1);
      const int row = (side ? col0 : row0) + i;
      const int64_t* L = side ? p.lb : p.la;
      const uint8_t* V = side ? p.vb : p.va;
      long long l = -1;
      if (row < (side ? p.N : p.M)) {
        l = L[row];
        if (l < 0 || (V && !V[row])) l = -1;
      }
      lab[side][i] = l;
    }

    // fragment q of this thread: float4 tid + 512 q of the chunk image = MFMA tile 4 q + (wave >> 1),
    // step wave & 1, lane (g, r): columns 16 step + 4 g + (0..3) of row 16 tile + r
    const float* pa[PH_LD];
    const float* pb[PH_LD];
#pragma unroll
    for (int q = 0; q < PH_LD; ++q) {
      const int rl = 16 * (4 * q + (wave >> 1)) + r, c = 16 * (wave & 1) + 4 * g;
      pa[q] = p.a + (int64_t)min(row0 + rl, p.M - 1) * p.lda + c;
      pb[q] = p.b + (int64_t)min(col0 + rl, p.N - 1) * p.ldb + c;
    }
    f32x4 na[PH_LD], nb[PH_LD];
    auto fetch = [&](int kc) {
#pragma unroll
      for (int q = 0; q < PH_LD; ++q) {
        na[q] = *reinterpret_cast<const f32x4*>(pa[q] + kc * PH_KC);
        nb[q] = *reinterpret_cast<const f32x4*>(pb[q] + kc * PH_KC);
      }
    };
    auto stage = [&](int buf) {
#pragma unroll
      for (int q = 0; q < PH_LD; ++q) {
        frag[buf][0][tid + PH_NT * q] = na[q];
        frag[buf][1][tid + PH_NT * q] = nb[q];
      }
    };

    fetch(0);
    stage(0);
    __syncthreads();
    for (int kc = 0; kc < nchunks; ++kc) {
      const int buf = kc & 1;
      if (kc + 1 < nchunks) fetch(kc + 1);
#pragma unroll
      for (int st = 0; st < PH_KC / 16; ++st) {
        f32x4 af[PH_WM], bf[PH_WN];
#pragma unroll
        for (int i = 0; i < PH_WM; ++i) af[i] = frag[buf][0][((PH_WM * wm + i) * 2 + st) * 64 + lane];
#pragma unroll
        for (int j = 0; j < PH_WN; ++j) bf[j] = frag[buf][1][((PH_WN * wn + j) * 2 + st) * 64 + lane];
#pragma unroll
        for (int i = 0; i < PH_WM; ++i)
#pragma unroll
          for (int j = 0; j < PH_WN; ++j)
#pragma unroll
            for (int e = 0; e < 4; ++e)
              acc[i][j][e] = __builtin_amdgcn_mfma_f32_16x16x4f32(af[i][e], bf[j][e], acc[i][j][e], 0, 0, 0);
      }
      // buffer buf ^ 1 was last read before the previous barrier
      if (kc + 1 < nchunks) stage(buf ^ 1);
      __syncthreads();
    }

    // acc[i][j][.][reg] of lane (g, r): row 32 wm + 16 i + 4 g + reg of a, row 64 wn + 16 j + r of b
    long long lbj[PH_WN];
#pragma unroll
    for (int j = 0; j < PH_WN; ++j) lbj[j] = lab[1][64 * wn + 16 * j + r];
#pragma unroll
    for (int i = 0; i < PH_WM; ++i) {
      const int il = 16 * (PH_WM * wm + i) + 4 * g;
      long long lai[4];
#pragma unroll
      for (int reg = 0; reg < 4; ++reg) lai[reg] = lab[0][il + reg];
#pragma unroll
      for (int j = 0; j < PH_WN; ++j) {
        const f32x4 sc = (acc[i][j][0] + acc[i][j][1]) + (acc[i][j][2] + acc[i][j][3]);
        const int gj = col0 + 64 * wn + 16 * j + r;
#pragma unroll
        for (int reg = 0; reg < 4; ++reg) {
          const bool on = lai[reg] >= 0 && lbj[j] >= 0 && (!p.self || row0 + il + reg < gj);
          if (on) {
            const float s = sc[reg];
            if (ph_finite(s)) {
              // s * h is exact (h a power of two); the clamp before the conversion is the
              // stated clamp of the bin
              const float t = fminf(fmaxf(floorf(s * h), -h), h - 1.f);
              const int bin = (int)t + (nbins >> 1);
              const int cls = lai[reg] != lbj[j];
              atomicAdd(cnt + cls * PH_HIST + (bin << cshift) + copy, 1u);
            } else {
              ++myskip;
            }
          }
        }
#pragma unroll
        for (int e = 0; e < 4; ++e) acc[i][j][e] = f32x4{0.f, 0.f, 0.f, 0.f};
      }
    }
    if (++since == PH_FLUSH_TILES) {
      flush();
      since = 0;
    }
  }
  flush();
}

inline bool ph_dim_ok(int D) { return D >= 32 && D <= 512 && D % 32 == 0; }
inline int ph_lbins(int nbins) {
  for (int l = 8; l <= 12; ++l)
    if (nbins == 1 << l) return l;
  return -1;
}

// one workgroup per CU (the kernel's LDS admits one), each walking ntiles / grid tiles
inline int ph_grid(int64_t ntiles) {
  static const int cus = [] {
    int dev = 0, n = 0;
    if (hipGetDevice(&dev) != hipSuccess ||
        hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess)
      n = 256;
    return n > 0 ? n : 256;
  }();
  return (int)(ntiles < cus ? ntiles : cus);
}

}  // namespace

extern "C" int prpe_pair_hist(const float* a, int64_t a_row_stride, int32_t M, const int64_t* a_labels,
                              const uint8_t* a_valid, const float* b, int64_t b_row_stride, int32_t N,
                              const int64_t* b_labels, const uint8_t* b_valid, int32_t D, int32_t nbins,
                              uint64_t* hist, uint64_t* skipped, void* stream) {
  const int lbins = ph_lbins(nbins);
  if (!a || !a_labels || !hist || !skipped || M < 1 || M > PH_MAXROWS || !ph_dim_ok(D) || lbins < 0 ||
      a_row_stride < D || (a_row_stride & 3) || ((uintptr_t)a & 15))
    return PRPE_EINVAL;
  const bool self = b == nullptr;
  if (self) {
    if (b_labels || b_valid) return PRPE_EINVAL;
  } else if (!b_labels || N < 1 || N > PH_MAXROWS || b_row_stride < D || (b_row_stride & 3) ||
             ((uintptr_t)b & 15)) {
    return PRPE_EINVAL;
  }
  PairK p;
  p.a = a;
  p.lda = a_row_stride;
  p.la = a_labels;
  p.va = a_valid;
  p.M = M;
  p.b = self ? a : b;
  p.ldb = self ? a_row_stride : b_row_stride;
  p.lb = self ? a_labels : b_labels;
  p.vb = self ? a_valid : b_valid;
  p.N = self ? M : N;
  p.hist = reinterpret_cast<unsigned long long*>(hist);
  p.skipped = reinterpret_cast<unsigned long long*>(skipped);
  p.D = D;
  p.lbins = lbins;
  p.self = self ? 1 : 0;
  const int64_t tm = (p.M + PH_T - 1) / PH_T, tn = (p.N + PH_T - 1) / PH_T;
  p.tn = (int)tn;
  p.ntiles = self ? tm * (tm + 1) / 2 : tm * tn;
  hipLaunchKernelGGL(pair_hist_kernel, dim3(ph_grid(p.ntiles)), dim3(PH_NT), 0, as_stream(stream), p);
  return launch_status();
}
