// The all-pairs tile product that csrc/pairhist.hip (pair_hist_kernel) and
// csrc/facecluster.hip (pair_cluster_kernel<1|2>, §5j) share: the only copy of the tile
// constants, the walk over tiles, the double-buffered LDS staging, the MFMA loop, the score sum
// and the host-side grid and operand checks. Each kernel adds its own epilogue.
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
// this one and stored after them; one barrier per chunk. A lane's global read (row r, columns
// 4 g ..) is the fragment it stores, so the LDS image is written and read linearly (no bank
// conflict on either side). The grid is one workgroup per CU, each walking tiles id, id + grid, ..:
// row-major over the rectangle (cross mode) or over the upper triangle of tiles (self mode). Rows
// past M / N re-read the last row; the epilogue masks them.
#pragma once
#pragma clang fp contract(off)
#include "common.h"

namespace {
namespace pairs {

constexpr int T = 128;                  // score tile of a workgroup (rows and columns)
constexpr int NW = 8;                   // waves, 4 x 2, 32 x 64 scores each
constexpr int NT = NW * 64;
constexpr int WM = 2, WN = 4;           // 16-row MFMA tiles per wave: rows of a, rows of b
constexpr int KC = 32;                  // columns per LDS chunk: two 16-column steps
constexpr int F4 = T * KC / 4;          // float4 per operand and chunk
constexpr int LD = F4 / NT;             // float4 a thread moves per operand and chunk
constexpr int MAXROWS = 1 << 24;

typedef f32x4 Frag[2][2][F4];           // LDS image, [buffer][operand][(tile, step, g, r)]: 64 KB
typedef f32x4 Acc[WM][WN][4];           // a wave's accumulators, [i][j][e]

__device__ __forceinline__ bool finite(float v) { return fabsf(v) <= 3.402823466e38f; }   // false for NaN

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
// tile id -> (ti, tj): the upper triangle (self) or row-major over the rectangle, tn tiles a row
__device__ __forceinline__ void tile_of(int64_t id, int tn, bool self, int& ti, int& tj) {
  if (self) {
    tri_tile(id, tn, ti, tj);
  } else {
    ti = (int)(id / tn);
    tj = (int)(id - (int64_t)ti * tn);
  }
}

// a thread's place in the workgroup, and in the wave's 32 x 64 scores: acc[i][j][.][reg] holds the
// pair of row il(i) + reg of the tile's a side and row jl(j) of its b side
struct Lane {
  int tid, lane, wave, r, g, wm, wn;
  __device__ __forceinline__ Lane()
      : tid(threadIdx.x), lane(tid & 63), wave(tid >> 6), r(lane & 15), g(lane >> 4), wm(wave >> 1), wn(wave & 1) {}
  __device__ __forceinline__ int il(int i) const { return 16 * (WM * wm + i) + 4 * g; }
  __device__ __forceinline__ int jl(int j) const { return 64 * wn + 16 * j + r; }
};

__device__ __forceinline__ void clear(Acc& acc) {
#pragma unroll
  for (int i = 0; i < WM; ++i)
#pragma unroll
    for (int j = 0; j < WN; ++j)
#pragma unroll
      for (int e = 0; e < 4; ++e) acc[i][j][e] = f32x4{0.f, 0.f, 0.f, 0.f};
}

// acc += the tile's products over nchunks chunks of KC columns: rows row0 .. of a [M] against rows
// col0 .. of b [N] (self mode: b is a). Every thread of the workgroup calls it; it ends on a barrier
__device__ __forceinline__ void product(Frag& frag, Acc& acc, const Lane ln, const float* a, int64_t lda, int M,
                                        const float* b, int64_t ldb, int N, int row0, int col0, int nchunks) {
  // fragment q of this thread: float4 tid + 512 q of the chunk image = MFMA tile 4 q + (wave >> 1),
  // step wave & 1, lane (g, r): columns 16 step + 4 g + (0..3) of row 16 tile + r
  const float* pa[LD];
  const float* pb[LD];
#pragma unroll
  for (int q = 0; q < LD; ++q) {
    const int rl = 16 * (4 * q + (ln.wave >> 1)) + ln.r, c = 16 * (ln.wave & 1) + 4 * ln.g;
    pa[q] = a + (int64_t)min(row0 + rl, M - 1) * lda + c;
    pb[q] = b + (int64_t)min(col0 + rl, N - 1) * ldb + c;
  }
  f32x4 na[LD], nb[LD];
  auto fetch = [&](int kc) {
#pragma unroll
    for (int q = 0; q < LD; ++q) {
      na[q] = *reinterpret_cast<const f32x4*>(pa[q] + kc * KC);
      nb[q] = *reinterpret_cast<const f32x4*>(pb[q] + kc * KC);
    }
  };
  auto stage = [&](int buf) {
#pragma unroll
    for (int q = 0; q < LD; ++q) {
      frag[buf][0][ln.tid + NT * q] = na[q];
      frag[buf][1][ln.tid + NT * q] = nb[q];
    }
  };

  fetch(0);
  stage(0);
  __syncthreads();
  for (int kc = 0; kc < nchunks; ++kc) {
    const int buf = kc & 1;
    if (kc + 1 < nchunks) fetch(kc + 1);
#pragma unroll
    for (int st = 0; st < KC / 16; ++st) {
      f32x4 af[WM], bf[WN];
#pragma unroll
      for (int i = 0; i < WM; ++i) af[i] = frag[buf][0][((WM * ln.wm + i) * 2 + st) * 64 + ln.lane];
#pragma unroll
      for (int j = 0; j < WN; ++j) bf[j] = frag[buf][1][((WN * ln.wn + j) * 2 + st) * 64 + ln.lane];
#pragma unroll
      for (int i = 0; i < WM; ++i)
#pragma unroll
        for (int j = 0; j < WN; ++j)
#pragma unroll
          for (int e = 0; e < 4; ++e)
            acc[i][j][e] = __builtin_amdgcn_mfma_f32_16x16x4f32(af[i][e], bf[j][e], acc[i][j][e], 0, 0, 0);
    }
    // buffer buf ^ 1 was last read before the previous barrier
    if (kc + 1 < nchunks) stage(buf ^ 1);
    __syncthreads();
  }
}

__device__ __forceinline__ f32x4 score(const Acc& acc, int i, int j) {
  return (acc[i][j][0] + acc[i][j][1]) + (acc[i][j][2] + acc[i][j][3]);
}

// ------------------------------------------------------------------------- host
inline bool dim_ok(int D) { return D >= 32 && D <= 512 && D % 32 == 0; }
inline bool rows_ok(const float* a, int64_t lda, int N, int D) {
  return a && N >= 1 && N <= MAXROWS && dim_ok(D) && lda >= D && !(lda & 3) && !((uintptr_t)a & 15);
}

// the tiles of a launch: tn a row, ntiles in all (self: the upper triangle of tn x tn)
struct Tiles {
  int tn;
  int64_t ntiles;
};
inline Tiles tiles(int M, int N, bool self) {
  const int64_t tm = (M + T - 1) / T, tn = (N + T - 1) / T;
  return Tiles{(int)tn, self ? tm * (tm + 1) / 2 : tm * tn};
}

// one workgroup per CU (LDS or registers of every kernel of the family admit one), each walking
// ntiles / grid tiles
inline int grid(int64_t ntiles) {
  static const int cus = [] {
    int dev = 0, n = 0;
    if (hipGetDevice(&dev) != hipSuccess ||
        hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess)
      n = 256;
    return n > 0 ? n : 256;
  }();
  return (int)(ntiles < cus ? ntiles : cus);
}

}  // namespace pairs
}  // namespace
