// What csrc/gallery.hip (the exact search) and csrc/gallery_wide.hip (the bf16 filter in front of
// it) share: the entry type, the total order, the wave-wide selection, the launch
// plan, and the two launches of gallery.hip that the wide route reuses.
#pragma once
#include "common.h"

namespace {

constexpr int GL_NW = 4;            // waves per workgroup
constexpr int GL_TILE = 16;         // gallery rows per wave step (one MFMA tile)
constexpr int GL_STEP_ROWS = GL_NW * GL_TILE;
constexpr int GL_KMAX = 8;
constexpr int GL_DMAX = 512;
constexpr int GL_PF = 8;            // 16-column steps per register buffer (128 columns)
constexpr int GL_EMPTY = 0x7fffffff;   // row of an empty slot inside the kernels (-1 in the output)
constexpr float GL_EPS = 1e-12f;    // F.normalize

struct Ent { float s; int r; };

__device__ __forceinline__ bool gl_finite(float v) { return fabsf(v) <= 3.402823466e38f; }   // false for NaN
// the total order: score descending, then row ascending
__device__ __forceinline__ bool gl_better(float s, int r, float s2, int r2) { return s > s2 || (s == s2 && r < r2); }

// ------------------------------------------------------------------------- wave-wide selection
// a lane's sorted list of up to 8 entries, in registers (every index static)
struct Local {
  float s[GL_KMAX];
  int r[GL_KMAX];
  __device__ __forceinline__ void clear() {
#pragma unroll
    for (int j = 0; j < GL_KMAX; ++j) { s[j] = -INFINITY; r[j] = GL_EMPTY; }
  }
  __device__ __forceinline__ void push(float es, int er) {
    if (!gl_better(es, er, s[GL_KMAX - 1], r[GL_KMAX - 1])) return;
    s[GL_KMAX - 1] = es;
    r[GL_KMAX - 1] = er;
#pragma unroll
    for (int j = GL_KMAX - 1; j > 0; --j) {
      if (gl_better(s[j], r[j], s[j - 1], r[j - 1])) {
        const float ts = s[j]; s[j] = s[j - 1]; s[j - 1] = ts;
        const int tr = r[j]; r[j] = r[j - 1]; r[j - 1] = tr;
      }
    }
  }
  __device__ __forceinline__ void pop() {
#pragma unroll
    for (int j = 0; j < GL_KMAX - 1; ++j) { s[j] = s[j + 1]; r[j] = r[j + 1]; }
    s[GL_KMAX - 1] = -INFINITY;
    r[GL_KMAX - 1] = GL_EMPTY;
  }
};

// the best head of the wave's 64 local lists, removed from its list; every lane returns it.
// Rows are unique across the lists (empty slots apart), so exactly one lane pops.
__device__ __forceinline__ Ent wave_take_best(Local& loc) {
  float bs = loc.s[0];
  int br = loc.r[0];
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const float os = __shfl_xor(bs, o, 64);
    const int orow = __shfl_xor(br, o, 64);
    if (gl_better(os, orow, bs, br)) { bs = os; br = orow; }
  }
  if (br != GL_EMPTY && loc.r[0] == br) loc.pop();
  return Ent{bs, br};
}

// ------------------------------------------------------------------------- host
inline int64_t align256(int64_t v) { return (v + 255) & ~(int64_t)255; }
inline bool dim_ok(int D) { return D >= 32 && D <= GL_DMAX && D % 32 == 0; }
constexpr int GL_GMAX = 0x7fffffff - 4096;

// query block width, query blocks, rows per chunk (a multiple of 64) and chunks: enough
// workgroups to fill the chip a few times over, each with a long contiguous walk at large G
struct Plan { int qb, nqb, chunk, nchunks; };
inline Plan gallery_plan(int Q, int G) {
  Plan pl;
  pl.qb = Q <= 16 ? 16 : 64;
  pl.nqb = (Q + pl.qb - 1) / pl.qb;
  const int tiles = (G + GL_STEP_ROWS - 1) / GL_STEP_ROWS;
  const int target = Q <= 16 ? 1024 : (512 / pl.nqb > 1 ? 512 / pl.nqb : 1);
  const int tpc = (tiles + target - 1) / target;
  pl.chunk = tpc * GL_STEP_ROWS;
  pl.nchunks = (tiles + tpc - 1) / tpc;
  return pl;
}
// the listed launch (the wide route's fallback): the number of listed queries is known on the
// device only, and one live query block must still fill the chip, so the chunks are those of a
// single query block whatever Q
inline Plan gallery_plan_listed(int Q, int G) {
  Plan pl;
  pl.qb = Q <= 16 ? 16 : 64;
  pl.nqb = (Q + pl.qb - 1) / pl.qb;
  const int tiles = (G + GL_STEP_ROWS - 1) / GL_STEP_ROWS;
  const int target = Q <= 16 ? 1024 : 256;
  const int tpc = (tiles + target - 1) / target;
  pl.chunk = tpc * GL_STEP_ROWS;
  pl.nchunks = (tiles + tpc - 1) / tpc;
  return pl;
}

}  // namespace

// gallery.hip's launches behind prpe_gallery_topk_wide (not part of the C ABI)
#define GL_INTERNAL __attribute__((visibility("hidden")))
// launch 0 of prpe_gallery_topk (the same bits in qn), and qbf = RNE bf16 of those bits, [Q][D]
GL_INTERNAL int gallery_launch_normalise_bf16(const float* queries, int64_t q_row_stride, int Q, int D, float* qn,
                                              __bf16* qbf, hipStream_t st);
// launches 1 and 2 of prpe_gallery_topk for the queries list[0 .. *count) only (ascending query
// indices, both on the device), their rows already normalised in qn; part as in prpe_gallery_topk.
// Sized for count = Q; the workgroups past *count return at entry.
GL_INTERNAL int gallery_launch_listed(const float* qn, int Q, int D, const float* gallery, int G,
                                      const uint8_t* valid, int k, float* scores, int32_t* rows,
                                      const int64_t* labels, float threshold, int64_t* ident, void* part,
                                      const int* list, const int* count, hipStream_t st);
