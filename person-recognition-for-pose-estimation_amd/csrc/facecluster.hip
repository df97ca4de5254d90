// Clustering of unlabelled face embeddings: DBSCAN over cosine similarity on the
// rows a gallery stores, self mode. prpe_pair_degree (pass 1), prpe_pair_link (pass 2),
// prpe_cluster_finish and prpe_cluster_centroids; the semantics are stated in include/prpe.h.
//
// Both passes are the all-pairs GEMM of csrc/pairhist.hip with another epilogue. The tile product
// -- the walk over the upper triangle of 128 x 128 score tiles, the LDS staging, the MFMA loop and
// the score bits, pair_hist's and gallery_topk's -- is csrc/pairs.h's, the one copy both files
// compile; rows past N re-read the last row and are masked by their flag.
//
// Pass 1 counts the accepted pairs i < j of a tile into 128 + 128 LDS counters (a lane sums its
// own scores of one row / one column in registers first) and adds the non-zero ones to degree:
// one global integer atomic per row and tile, none per pair.
// Pass 2 reads degree for the tile's 256 rows into LDS flags and links: core-core pairs in a
// tile-local union-find over the tile's row slots, flushed with at most one global union per slot
// that is not its local root; core-border pairs by a 64-bit max of (score image, lowest row first)
// in LDS, flushed with one global 64-bit atomicMax per non-empty slot.
//
// Union-find, LDS and global alike: parent[x] <= x and a parent only decreases. A union finds both
// roots and hooks the higher under the lower by a compare-and-swap on the root's own slot; a lost
// CAS finds again. find shortens the path it walks with atomicMin (the new parent is an ancestor,
// hence lower). No locks; no thread waits for another: every step lowers an index or loses a CAS
// to a thread that won one. A root is never hooked under a higher row, so a component's root ends
// as its lowest row, whatever the order of arrival. Global parent is read with agent-scope relaxed
// atomic loads and written by agent-scope atomics only.
#pragma clang fp contract(off)
#include "pairs.h"

namespace {

constexpr int FC_T = pairs::T;
constexpr int FC_SLOTS = 2 * FC_T;            // row slots of a tile: the row side, then the column side

enum : uint8_t { FC_OUT = 0, FC_OTHER = 1, FC_CORE = 2 };   // LDS flags of pass 2

struct ClusterK {
  const float* a;
  int64_t lda;
  const uint8_t* valid;
  int* degree;
  int* parent;
  unsigned long long* best;
  float thr;
  int N, D, tn, min_samples;
  int64_t ntiles;
};

// order-preserving uint32 image of a finite float (-0 is +0 here: a sum of fmas from +0 never is -0)
__device__ __forceinline__ unsigned fc_image(float s) {
  const unsigned u = __float_as_uint(s + 0.f);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

// ---- union-find, SCOPE the memory scope of the relaxed loads: the workgroup's for a tile's LDS
// parents, the agent's for the global ones
constexpr int FC_LDS = __HIP_MEMORY_SCOPE_WORKGROUP, FC_GLB = __HIP_MEMORY_SCOPE_AGENT;
template <int SCOPE>
__device__ __forceinline__ int uf_find(int* par, int x) {
  for (;;) {
    const int p = __hip_atomic_load(par + x, __ATOMIC_RELAXED, SCOPE);
    if (p == x) return x;
    const int gp = __hip_atomic_load(par + p, __ATOMIC_RELAXED, SCOPE);
    if (gp != p) atomicMin(par + x, gp);
    x = p;
  }
}
template <int SCOPE>
__device__ __forceinline__ void uf_union(int* par, int x, int y) {
  for (;;) {
    x = uf_find<SCOPE>(par, x);
    y = uf_find<SCOPE>(par, y);
    if (x == y) return;
    const int hi = x > y ? x : y, lo = x > y ? y : x;
    if (atomicCAS(par + hi, hi, lo) == hi) return;
  }
}

// PASS 1: degree. PASS 2: link.
template <int PASS>
__global__ __launch_bounds__(pairs::NT) void pair_cluster_kernel(ClusterK p) {
  __shared__ pairs::Frag frag;
  __shared__ unsigned long long lbest[PASS == 2 ? FC_SLOTS : 1];   // pass 2: the best core neighbour of a slot
  __shared__ int word[FC_SLOTS];               // pass 1: the slot's count; pass 2: its local parent
  __shared__ uint8_t flag[FC_SLOTS];           // pass 1: takes part; pass 2: FC_OUT / FC_OTHER / FC_CORE

  const pairs::Lane ln;
  const int tid = ln.tid;
  const int nchunks = p.D / pairs::KC;

  for (int64_t id = blockIdx.x; id < p.ntiles; id += gridDim.x) {
    int ti, tj;
    pairs::tile_of(id, p.tn, true, ti, tj);
    const int row0 = ti * FC_T, col0 = tj * FC_T;
    const bool diag = ti == tj;

    __syncthreads();   // the previous tile's flush has read word, flag and lbest
    if (tid < FC_SLOTS) {
      const int row = (tid < FC_T ? row0 : col0 - FC_T) + tid;
      uint8_t f = FC_OUT;
      if (row < p.N && (!p.valid || p.valid[row])) {
        f = FC_OTHER;
        if (PASS == 2 && p.degree[row] + 1 >= p.min_samples) f = FC_CORE;
      }
      flag[tid] = f;
      word[tid] = PASS == 2 ? tid : 0;
      if (PASS == 2) lbest[tid] = 0ull;
    }

    pairs::Acc acc;
    pairs::clear(acc);
    pairs::product(frag, acc, ln, p.a, p.lda, p.N, p.a, p.lda, p.N, row0, col0, nchunks);

    // in a diagonal tile the two sides are the same rows: the column side then takes the row
    // side's slots
    const int cbase = diag ? 0 : FC_T;
    uint8_t fj[pairs::WN];
    int colcnt[pairs::WN];
#pragma unroll
    for (int j = 0; j < pairs::WN; ++j) {
      fj[j] = flag[FC_T + ln.jl(j)];
      colcnt[j] = 0;
    }
#pragma unroll
    for (int i = 0; i < pairs::WM; ++i) {
      const int il = ln.il(i);
      uint8_t fi[4];
      int rowcnt[4];
#pragma unroll
      for (int reg = 0; reg < 4; ++reg) {
        fi[reg] = flag[il + reg];
        rowcnt[reg] = 0;
      }
#pragma unroll
      for (int j = 0; j < pairs::WN; ++j) {
        const f32x4 sc = pairs::score(acc, i, j);
        const int jl = ln.jl(j);
#pragma unroll
        for (int reg = 0; reg < 4; ++reg) {
          const float s = sc[reg];
          const bool on = fi[reg] != FC_OUT && fj[j] != FC_OUT && row0 + il + reg < col0 + jl &&
                          pairs::finite(s) && s >= p.thr;
          if (PASS == 1) {
            rowcnt[reg] += on;
            colcnt[j] += on;
          } else if (on) {
            const bool ci = fi[reg] == FC_CORE, cj = fj[j] == FC_CORE;
            if (ci && cj) {
              uf_union<FC_LDS>(word, il + reg, cbase + jl);
            } else if (ci) {
              atomicMax(lbest + cbase + jl,
                        (unsigned long long)fc_image(s) << 32 | (0xFFFFFFFFu - (unsigned)(row0 + il + reg)));
            } else if (cj) {
              atomicMax(lbest + il + reg,
                        (unsigned long long)fc_image(s) << 32 | (0xFFFFFFFFu - (unsigned)(col0 + jl)));
            }
          }
        }
      }
      if (PASS == 1) {
#pragma unroll
        for (int reg = 0; reg < 4; ++reg)
          if (rowcnt[reg]) atomicAdd(word + il + reg, rowcnt[reg]);
      }
    }
    if (PASS == 1) {
#pragma unroll
      for (int j = 0; j < pairs::WN; ++j)
        if (colcnt[j]) atomicAdd(word + FC_T + ln.jl(j), colcnt[j]);
    }

    __syncthreads();
    if (tid < FC_SLOTS && flag[tid] != FC_OUT) {
      const int row = (tid < FC_T ? row0 : col0 - FC_T) + tid;
      if (PASS == 1) {
        if (word[tid]) atomicAdd(p.degree + row, word[tid]);
      } else {
        const int lr = uf_find<FC_LDS>(word, tid);
        if (lr != tid) uf_union<FC_GLB>(p.parent, row, (lr < FC_T ? row0 : col0 - FC_T) + lr);
        const unsigned long long b = lbest[tid];
        if (b) atomicMax(p.best + row, b);
      }
    }
  }
}

__global__ void fc_zero_degree_kernel(int* degree, int N) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < N) degree[i] = 0;
}
__global__ void fc_init_kernel(int* parent, unsigned long long* best, int N) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < N) {
    parent[i] = i;
    best[i] = 0ull;
  }
}

// one thread per row: flatten root, classify kind (parent and best are complete: another launch wrote them)
__global__ void fc_classify_kernel(int N, const uint8_t* valid, int min_samples, const int* degree, const int* parent,
                                   const unsigned long long* best, int* root, uint8_t* kind) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= N) return;
  int k = 0, x = -1;
  if (!valid || valid[i]) {
    if (degree[i] + 1 >= min_samples) {
      k = 3;
      x = i;
    } else {
      const unsigned long long b = best[i];
      k = b ? 2 : 1;
      if (b) x = (int)(0xFFFFFFFFu - (unsigned)b);
    }
  }
  if (x >= 0)
    while (parent[x] != x) x = parent[x];
  root[i] = x;
  kind[i] = (uint8_t)k;
}

// one workgroup: a chunked scan over "row is its own root and core" gives the compact ids in
// ascending root order (written at the root rows) and n_clusters; sizes[0 .. min(C, max)) zeroed
constexpr int FC_SCAN_NT = 1024, FC_SCAN_PER = 8;
__global__ __launch_bounds__(FC_SCAN_NT) void fc_compact_kernel(int N, const int* root, const uint8_t* kind, int* cluster,
                                                                int* n_clusters, int max_clusters, int* sizes) {
  __shared__ int wsum[FC_SCAN_NT / 64];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  int base = 0;
  for (int64_t start = 0; start < N; start += FC_SCAN_NT * FC_SCAN_PER) {
    const int64_t i0 = start + (int64_t)tid * FC_SCAN_PER;
    bool f[FC_SCAN_PER];
    int cnt = 0;
#pragma unroll
    for (int e = 0; e < FC_SCAN_PER; ++e) {
      const int64_t i = i0 + e;
      f[e] = i < N && kind[i] == 3 && root[i] == (int)i;
      cnt += f[e];
    }
    int inc = cnt;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const int t = __shfl_up(inc, o, 64);
      if (lane >= o) inc += t;
    }
    if (lane == 63) wsum[wave] = inc;
    __syncthreads();
    int woff = 0, total = 0;
#pragma unroll
    for (int w = 0; w < FC_SCAN_NT / 64; ++w) {
      const int v = wsum[w];
      woff += w < wave ? v : 0;
      total += v;
    }
    int idx = base + woff + inc - cnt;
#pragma unroll
    for (int e = 0; e < FC_SCAN_PER; ++e)
      if (f[e]) cluster[i0 + e] = idx++;
    base += total;
    __syncthreads();
  }
  if (tid == 0) n_clusters[0] = base;
  const int lim = base < max_clusters ? base : max_clusters;
  for (int i = tid; i < lim; i += FC_SCAN_NT) sizes[i] = 0;
}

// one thread per row: the id of the row's root; sizes by integer atomics
__global__ void fc_assign_kernel(int N, const int* root, int* cluster, int max_clusters, int* sizes) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= N) return;
  const int x = root[i];
  if (x < 0) {
    cluster[i] = -1;
    return;
  }
  const int c = cluster[x];          // a root row's id is fc_compact_kernel's and is not written here
  if (x != i) cluster[i] = c;
  if (c < max_clusters) atomicAdd(sizes + c, 1);
}

// ---- centroids
constexpr int FC_SUM_NT = 256, FC_SUM_ROWS = 16;   // rows a wave walks
__global__ void fc_zero_sums_kernel(const int* n_clusters, int max_clusters, int D, long long* sums) {
  const int c = n_clusters[0];
  const int64_t lim = (int64_t)(c < max_clusters ? c : max_clusters) * D;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < lim; i += (int64_t)gridDim.x * blockDim.x)
    sums[i] = 0;
}
// a wave takes FC_SUM_ROWS consecutive rows, a lane the columns lane, lane + 64, ..: runs of equal
// cluster are added in registers and leave as 64 contiguous int64 atomic adds per instruction
__global__ __launch_bounds__(FC_SUM_NT) void fc_sums_kernel(const float* a, int64_t lda, int N, int D, const int* cluster,
                                                             int max_clusters, long long* sums) {
  const int lane = threadIdx.x & 63;
  const int64_t r0 = ((int64_t)blockIdx.x * (FC_SUM_NT / 64) + (threadIdx.x >> 6)) * FC_SUM_ROWS;
  long long acc[8];
#pragma unroll
  for (int q = 0; q < 8; ++q) acc[q] = 0;
  int cur = -1;
  auto flush = [&]() {
    if (cur < 0) return;
#pragma unroll
    for (int q = 0; q < 8; ++q) {
      const int col = lane + 64 * q;
      if (col < D) atomicAdd(reinterpret_cast<unsigned long long*>(sums + (int64_t)cur * D + col), (unsigned long long)acc[q]);
      acc[q] = 0;
    }
  };
  for (int64_t row = r0; row < r0 + FC_SUM_ROWS && row < N; ++row) {
    int c = cluster[row];
    if (c < 0 || c >= max_clusters) c = -1;
    if (c != cur) {
      flush();
      cur = c;
    }
    if (c >= 0) {
#pragma unroll
      for (int q = 0; q < 8; ++q) {
        const int col = lane + 64 * q;
        if (col < D) acc[q] += llrintf(a[row * lda + col] * 4294967296.f);
      }
    }
  }
  flush();
}
__global__ void fc_centroids_kernel(const int* n_clusters, int max_clusters, int D, const long long* sums, float* centroids) {
  const int c = n_clusters[0];
  const int64_t lim = (int64_t)(c < max_clusters ? c : max_clusters) * D;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < lim; i += (int64_t)gridDim.x * blockDim.x)
    centroids[i] = (float)((double)sums[i] * (1.0 / 4294967296.0));
}

inline int64_t fc_ws_bytes(int N) { return (((int64_t)N * 12) + 255) & ~(int64_t)255; }
inline bool fc_ws_ok(const void* ws, int64_t bytes, int N) { return ws && !((uintptr_t)ws & 255) && bytes >= fc_ws_bytes(N); }
inline unsigned long long* fc_best(void* ws) { return reinterpret_cast<unsigned long long*>(ws); }
inline int* fc_parent(void* ws, int N) { return reinterpret_cast<int*>(fc_best(ws) + N); }
inline unsigned fc_blocks(int64_t n, int per) { return (unsigned)((n + per - 1) / per); }

inline ClusterK fc_args(const float* a, int64_t lda, int N, const uint8_t* valid, int D, float thr) {
  ClusterK p{};
  p.a = a;
  p.lda = lda;
  p.valid = valid;
  p.N = N;
  p.D = D;
  p.thr = thr;
  const pairs::Tiles tl = pairs::tiles(N, N, true);
  p.tn = tl.tn;
  p.ntiles = tl.ntiles;
  return p;
}

}  // namespace

extern "C" int64_t prpe_face_cluster_workspace_bytes(int32_t N) {
  if (N < 1 || N > pairs::MAXROWS) return PRPE_EINVAL;
  return fc_ws_bytes(N);
}

extern "C" int prpe_pair_degree(const float* a, int64_t a_row_stride, int32_t N, const uint8_t* valid, int32_t D,
                                float threshold, int32_t* degree, void* stream) {
  if (!pairs::rows_ok(a, a_row_stride, N, D) || !isfinite(threshold) || !degree) return PRPE_EINVAL;
  ClusterK p = fc_args(a, a_row_stride, N, valid, D, threshold);
  p.degree = degree;
  hipLaunchKernelGGL(fc_zero_degree_kernel, dim3(fc_blocks(N, 256)), dim3(256), 0, as_stream(stream), degree, N);
  hipLaunchKernelGGL(pair_cluster_kernel<1>, dim3(pairs::grid(p.ntiles)), dim3(pairs::NT), 0, as_stream(stream), p);
  return launch_status();
}

extern "C" int prpe_pair_link(const float* a, int64_t a_row_stride, int32_t N, const uint8_t* valid, int32_t D,
                              float threshold, int32_t min_samples, const int32_t* degree, void* workspace,
                              int64_t workspace_bytes, void* stream) {
  if (!pairs::rows_ok(a, a_row_stride, N, D) || !isfinite(threshold) || min_samples < 1 || !degree ||
      !fc_ws_ok(workspace, workspace_bytes, N))
    return PRPE_EINVAL;
  ClusterK p = fc_args(a, a_row_stride, N, valid, D, threshold);
  p.degree = const_cast<int*>(degree);
  p.min_samples = min_samples;
  p.best = fc_best(workspace);
  p.parent = fc_parent(workspace, N);
  hipLaunchKernelGGL(fc_init_kernel, dim3(fc_blocks(N, 256)), dim3(256), 0, as_stream(stream), p.parent, p.best, N);
  hipLaunchKernelGGL(pair_cluster_kernel<2>, dim3(pairs::grid(p.ntiles)), dim3(pairs::NT), 0, as_stream(stream), p);
  return launch_status();
}

extern "C" int prpe_cluster_finish(int32_t N, const uint8_t* valid, int32_t min_samples, const int32_t* degree,
                                   const void* workspace, int64_t workspace_bytes, int32_t* root, uint8_t* kind,
                                   int32_t* cluster, int32_t* n_clusters, int32_t max_clusters, int32_t* sizes,
                                   void* stream) {
  if (N < 1 || N > pairs::MAXROWS || min_samples < 1 || !degree || !fc_ws_ok(workspace, workspace_bytes, N) || !root ||
      !kind || !cluster || !n_clusters || max_clusters < 1 || !sizes)
    return PRPE_EINVAL;
  void* ws = const_cast<void*>(workspace);
  hipLaunchKernelGGL(fc_classify_kernel, dim3(fc_blocks(N, 256)), dim3(256), 0, as_stream(stream), N, valid, min_samples,
                     degree, fc_parent(ws, N), fc_best(ws), root, kind);
  hipLaunchKernelGGL(fc_compact_kernel, dim3(1), dim3(FC_SCAN_NT), 0, as_stream(stream), N, root, kind, cluster,
                     n_clusters, max_clusters, sizes);
  hipLaunchKernelGGL(fc_assign_kernel, dim3(fc_blocks(N, 256)), dim3(256), 0, as_stream(stream), N, root, cluster,
                     max_clusters, sizes);
  return launch_status();
}

extern "C" int prpe_cluster_centroids(const float* a, int64_t a_row_stride, int32_t N, int32_t D, const int32_t* cluster,
                                      const int32_t* n_clusters, int32_t max_clusters, int64_t* sums, float* centroids,
                                      void* stream) {
  if (!pairs::rows_ok(a, a_row_stride, N, D) || !cluster || !n_clusters || max_clusters < 1 || !sums || !centroids)
    return PRPE_EINVAL;
  const int64_t cells = (int64_t)max_clusters * D;
  const unsigned grid = (unsigned)(cells < 2048 * 256 ? (cells + 255) / 256 : 2048);
  long long* s = reinterpret_cast<long long*>(sums);
  hipLaunchKernelGGL(fc_zero_sums_kernel, dim3(grid), dim3(256), 0, as_stream(stream), n_clusters, max_clusters, D, s);
  hipLaunchKernelGGL(fc_sums_kernel, dim3(fc_blocks(N, (FC_SUM_NT / 64) * FC_SUM_ROWS)), dim3(FC_SUM_NT), 0,
                     as_stream(stream), a, a_row_stride, N, D, cluster, max_clusters, s);
  hipLaunchKernelGGL(fc_centroids_kernel, dim3(grid), dim3(256), 0, as_stream(stream), n_clusters, max_clusters, D, s,
                     centroids);
  return launch_status();
}
