// 1:1 face verification: prpe_pair_hist -- the scores of all pairs between two
// sets of L2-normalised fp32 rows (prpe_gallery_enrol's output), binned into a genuine and an
// impostor histogram. A GEMM whose epilogue is a histogram: the score matrix never reaches memory.
//
// The tile product -- the walk over 128 x 128 score tiles, the LDS staging, the MFMA loop and the
// score bits, which are those of prpe_gallery_topk -- is csrc/pairs.h's, shared with the DBSCAN
// passes of csrc/facecluster.hip. This file holds what is pair_hist's own: the labels of a tile's
// rows (a negative label or a zero valid byte masks a row, and so the rows past M / N, which
// re-read the last row; diagonal tiles of self mode mask i < j), the bin rule and the histogram.
//
// Histogram: uint32 counters in LDS, [class][bin][copy] with 4096 / nbins interleaved copies per
// bin (a lane adds to copy lane % copies: impostor scores pile up around 0, and the copies of one
// bin lie on neighbouring banks), flushed with 64-bit atomic adds to hist at the end of the walk
// and every PH_FLUSH_TILES tiles (a counter grows by at most 128 x 128 per tile). Integer adds
// commute: two runs give the same numbers.
#pragma clang fp contract(off)
#include "pairs.h"

namespace {

constexpr int PH_HIST = 4096;                 // private counters per class (nbins x copies)
constexpr unsigned PH_FLUSH_TILES = (unsigned)((1ull << 32) / (pairs::T * pairs::T)) - 1;

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

__global__ __launch_bounds__(pairs::NT) void pair_hist_kernel(PairK p) {
  __shared__ pairs::Frag frag;
  __shared__ unsigned cnt[2 * PH_HIST];        // [class][bin][copy]: 32 KB
  __shared__ long long lab[2][pairs::T];       // the tile's labels, -1: the row takes part in no pair

  const pairs::Lane ln;
  const int tid = ln.tid;
  const int nbins = 1 << p.lbins, cshift = 12 - p.lbins, copy = ln.lane & ((1 << cshift) - 1);
  const float h = (float)(nbins >> 1);
  const int nchunks = p.D / pairs::KC;

  for (int i = tid; i < 2 * PH_HIST; i += pairs::NT) cnt[i] = 0;
  unsigned since = 0, myskip = 0;

  // the private counters added to hist and cleared; every thread of the workgroup calls it
  auto flush = [&]() {
    __syncthreads();
    for (int i = tid; i < 2 * nbins; i += pairs::NT) {
      unsigned* c = cnt + (i >> p.lbins) * PH_HIST + ((i & (nbins - 1)) << cshift);
      unsigned long long sum = 0;
      for (int k = 0; k < (1 << cshift); ++k) { sum += c[k]; c[k] = 0; }
      if (sum) atomicAdd(p.hist + i, sum);
    }
    unsigned sk = myskip;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) sk += __shfl_xor(sk, o, 64);
    if (ln.lane == 0 && sk) atomicAdd(p.skipped, (unsigned long long)sk);
    myskip = 0;
    __syncthreads();
  };

  for (int64_t id = blockIdx.x; id < p.ntiles; id += gridDim.x) {
    int ti, tj;
    pairs::tile_of(id, p.tn, p.self, ti, tj);
    const int row0 = ti * pairs::T, col0 = tj * pairs::T;

    __syncthreads();   // the previous tile's epilogue has read lab (first tile: cnt is cleared)
    if (tid < 2 * pairs::T) {
      const int side = tid >> 7, i = tid & (pairs::T - 1);
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

    pairs::Acc acc;
    pairs::clear(acc);
    pairs::product(frag, acc, ln, p.a, p.lda, p.M, p.b, p.ldb, p.N, row0, col0, nchunks);

    long long lbj[pairs::WN];
#pragma unroll
    for (int j = 0; j < pairs::WN; ++j) lbj[j] = lab[1][ln.jl(j)];
#pragma unroll
    for (int i = 0; i < pairs::WM; ++i) {
      const int il = ln.il(i);
      long long lai[4];
#pragma unroll
      for (int reg = 0; reg < 4; ++reg) lai[reg] = lab[0][il + reg];
#pragma unroll
      for (int j = 0; j < pairs::WN; ++j) {
        const f32x4 sc = pairs::score(acc, i, j);
        const int gj = col0 + ln.jl(j);
#pragma unroll
        for (int reg = 0; reg < 4; ++reg) {
          const bool on = lai[reg] >= 0 && lbj[j] >= 0 && (!p.self || row0 + il + reg < gj);
          if (on) {
            const float s = sc[reg];
            if (pairs::finite(s)) {
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
      }
    }
    if (++since == PH_FLUSH_TILES) {
      flush();
      since = 0;
    }
  }
  flush();
}

inline int ph_lbins(int nbins) {
  for (int l = 8; l <= 12; ++l)
    if (nbins == 1 << l) return l;
  return -1;
}

}  // namespace

extern "C" int prpe_pair_hist(const float* a, int64_t a_row_stride, int32_t M, const int64_t* a_labels,
                              const uint8_t* a_valid, const float* b, int64_t b_row_stride, int32_t N,
                              const int64_t* b_labels, const uint8_t* b_valid, int32_t D, int32_t nbins,
                              uint64_t* hist, uint64_t* skipped, void* stream) {
  const int lbins = ph_lbins(nbins);
  if (!pairs::rows_ok(a, a_row_stride, M, D) || !a_labels || !hist || !skipped || lbins < 0) return PRPE_EINVAL;
  const bool self = b == nullptr;
  if (self) {
    if (b_labels || b_valid) return PRPE_EINVAL;
  } else if (!b_labels || !pairs::rows_ok(b, b_row_stride, N, D)) {
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
  const pairs::Tiles tl = pairs::tiles(p.M, p.N, self);
  p.tn = tl.tn;
  p.ntiles = tl.ntiles;
  hipLaunchKernelGGL(pair_hist_kernel, dim3(pairs::grid(p.ntiles)), dim3(pairs::NT), 0, as_stream(stream), p);
  return launch_status();
}
