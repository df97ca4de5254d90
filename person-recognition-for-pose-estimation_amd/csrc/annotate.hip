// Annotated frames out (include/prpe.h, prpe_annotate_nv12 / prpe_annotate_u8):
// skeletons, boxes and face redaction painted in place into the surface that goes to the encoder.
//
// Two launches, both a function of the inputs alone.
//
// build — one wavefront per person slot and one per (face slot, block row). A person's wave turns
//   the window, the limbs and the keypoints into integer primitives (the only floating point of the
//   feature: q = rintf(v * s)), a lane per primitive, and reduces their bounding boxes to the
//   person's. A face's waves write the face's window, mode and block side, and for mode 1 the means
//   of one row of pixelation blocks each. Everything goes into the caller's table:
//     frame [E]      int32, -1: the owner draws nothing       (E = max_p + max_f, persons first)
//     box   [E][4]   the owner's bounding box (a face: its unclipped window)
//     meta  [E][4]   person: (colour, 0, 0, 0); face: (colour, mode, block side, 0)
//     prim  [max_p][PP][4]  PP = 1 + n_limbs + K: the window, the limbs (a, b), the discs (c, c);
//                    x0 == VOID: not drawn
// paint — one workgroup per (frame, super-tile of 2 x 2 tiles). It scans the owners' frame words a
//   chunk of 256 at a time, keeps those of its frame whose box meets the super-tile (ballot and
//   popcount, as track.hip and roi.hip), expands the kept persons into their primitives, culls
//   those against the super-tile into an LDS list of at most 256 and consumes the list before the
//   next chunk is formed: it cannot overflow, however many primitives fall on one tile. A thread
//   owns a strip of 8 x 2 pixels in each of the 4 tiles and keeps the best (layer, slot) key of
//   each of its 64 pixels in registers across the chunks. A workgroup that kept nothing ends
//   without a load or a store of a picture byte; a strip with no key set neither loads nor stores.
//   A full 8-pixel luma row is one 8-byte store (read first when only part of it is painted) where
//   the plane and its pitches are 8-byte aligned; bytes otherwise. A strip's 4 chroma pairs follow
//   the keys of its even row's even pixels.
#pragma clang fp contract(off)
#include <limits.h>
#include "common.h"

namespace {

constexpr int AN_THREADS = 256;
constexpr int STRIP_W = 8, STRIP_H = 2;        // pixels a thread owns in a tile
constexpr int TILE_W = 64, TILE_H = 64;        // 8 x 32 strips
constexpr int SUPER_X = 2, SUPER_Y = 2;        // tiles per super-tile
constexpr int SUPER_W = TILE_W * SUPER_X, SUPER_H = TILE_H * SUPER_Y;
constexpr int NTILE = SUPER_X * SUPER_Y, NPIX = STRIP_W * STRIP_H;
constexpr int CHUNK = AN_THREADS;              // LDS list entries: one candidate per thread
constexpr int AN_MAX_SIDE = 16384, Q_MIN = -4096, Q_MAX = 20479;
constexpr int AN_MAX_LIMBS = 32, AN_MAX_K = 64, AN_MAX_R = 16, AN_BLOCKS = 17, AN_MAX_SLOTS = 1 << 20;
constexpr int VOID = INT_MIN;
constexpr unsigned SLOT_MASK = 0x0fffffffu;    // key = (layer + 1) << 28 | (SLOT_MASK - slot): larger wins
enum { L_FACE = 0, L_BOX = 1, L_LIMB = 2, L_DISC = 3 };
enum { KIND_RECT = 0, KIND_OUTLINE = 1, KIND_ROUND = 2 };

static_assert(TILE_W / STRIP_W * (TILE_H / STRIP_H) == AN_THREADS, "a thread per strip");

// the surface: NV12 (p0 = luma, p1 = chroma pairs) or packed uint8 (p0, any strides)
struct Surf {
  uint8_t* p0; uint8_t* p1;
  int B, H, W;
  int64_t sn0, sh0, sn1, sh1, sw, sc;          // bytes
  int wide;                                    // NV12: 8-byte paths are legal
};

__device__ __forceinline__ int4 ld4(const int* p) { return *reinterpret_cast<const int4*>(p); }

// q = rintf(v * s), or false when the product is not finite or q is outside [Q_MIN, Q_MAX]
__device__ __forceinline__ bool quant(float v, float s, int& q) {
  const float t = v * s;
  const float r = rintf(t);
  if (!(r >= (float)Q_MIN && r <= (float)Q_MAX)) return false;       // NaN and inf fail here too
  q = (int)r;
  return true;
}
__device__ __forceinline__ bool window_of(const float* m, float sx, float sy, int4& w) {
  const bool a = quant(m[2], sx, w.x), b = quant(m[3], sy, w.y);
  const bool c = quant(m[2] + m[4], sx, w.z), d = quant(m[3] + m[5], sy, w.w);
  return a && b && c && d;
}
__device__ __forceinline__ int wave_min(int v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = min(v, __shfl_xor(v, o, 64));
  return v;
}
__device__ __forceinline__ int wave_max(int v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = max(v, __shfl_xor(v, o, 64));
  return v;
}
__device__ __forceinline__ unsigned wave_add(unsigned v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
// a list's count clamped into [0, cap]; a list of capacity 0 has no count to read
__device__ __forceinline__ int clamp_count(const int* n, int cap) {
  if (cap <= 0) return 0;
  const int v = *n;
  return v < 0 ? 0 : (v < cap ? v : cap);
}
__device__ __forceinline__ int wrap(int v, int n) {
  const int r = v % n;
  return r < 0 ? r + n : r;
}

// ---------------------------------------------------------------- build
struct BuildK {
  Surf s;
  const float* meta_p; const int* n_p; int max_p;
  const float* kpts; int K; const int* pcol;
  const float* meta_f; const int* n_f; int max_f;
  const int* fmode; const int* fcol;
  int n_colours, n_limbs, PP, Ea;
  int box_t, limb_r, kp_r, cell;
  float kp_thr, sx, sy;
  int* table; uint8_t* means;
  unsigned char limbs[2 * AN_MAX_LIMBS];
};

__device__ __forceinline__ bool kp_of(const BuildK& p, int e, int j, int& x, int& y) {
  const float* k = p.kpts + ((int64_t)e * p.K + j) * 3;
  if (!(k[2] >= p.kp_thr)) return false;                              // a NaN score does not count
  const bool a = quant(k[0], p.sx, x), b = quant(k[1], p.sy, y);
  return a && b;
}

__device__ void build_person(const BuildK& p, int e, int lane) {
  const int np = clamp_count(p.n_p, p.max_p);
  const float* m = p.meta_p + (int64_t)e * 8;
  const int frame = e < np ? __float_as_int(m[0]) : -1;
  const int col = p.pcol[e];
  const bool draw = e < np && (unsigned)frame < (unsigned)p.s.B && col >= 0;
  int bx0 = INT_MAX, by0 = INT_MAX, bx1 = INT_MIN, by1 = INT_MIN;
  int* prim = p.table + (int64_t)9 * p.Ea + (int64_t)e * p.PP * 4;
  for (int k = lane; k < p.PP; k += 64) {
    int4 q = {VOID, 0, 0, 0};
    int r = 0;
    if (draw) {
      if (k == 0) {
        int4 w;
        if (p.box_t > 0 && window_of(m, p.sx, p.sy, w) && w.z > w.x && w.w > w.y) q = w;
      } else if (k <= p.n_limbs) {
        int ax, ay, bx, by;
        const bool a = kp_of(p, e, p.limbs[2 * (k - 1)], ax, ay), b = kp_of(p, e, p.limbs[2 * (k - 1) + 1], bx, by);
        if (a && b) q = int4{ax, ay, bx, by};
        r = p.limb_r;
      } else {
        int x, y;
        if (kp_of(p, e, k - 1 - p.n_limbs, x, y)) q = int4{x, y, x, y};
        r = p.kp_r;
      }
    }
    *reinterpret_cast<int4*>(prim + k * 4) = q;
    if (q.x != VOID) {
      if (k == 0) {
        bx0 = min(bx0, q.x); by0 = min(by0, q.y); bx1 = max(bx1, q.z); by1 = max(by1, q.w);
      } else {
        bx0 = min(bx0, min(q.x, q.z) - r); by0 = min(by0, min(q.y, q.w) - r);
        bx1 = max(bx1, max(q.x, q.z) + r + 1); by1 = max(by1, max(q.y, q.w) + r + 1);
      }
    }
  }
  bx0 = wave_min(bx0); by0 = wave_min(by0); bx1 = wave_max(bx1); by1 = wave_max(by1);
  if (lane == 0) {
    const bool any = draw && bx1 > bx0;
    p.table[e] = any ? frame : -1;
    *reinterpret_cast<int4*>(p.table + p.Ea + (int64_t)e * 4) = int4{bx0, by0, bx1, by1};
    *reinterpret_cast<int4*>(p.table + (int64_t)5 * p.Ea + (int64_t)e * 4) = int4{draw ? wrap(col, p.n_colours) : 0, 0, 0, 0};
  }
}

template <bool NV>
__device__ void build_face(const BuildK& p, int f, int brow, int lane) {
  const int nf = clamp_count(p.n_f, p.max_f);
  const float* m = p.meta_f + (int64_t)f * 8;
  const int frame = f < nf ? __float_as_int(m[0]) : -1;
  const int mode = p.fmode[f];
  int4 w = {0, 0, 0, 0};
  bool draw = f < nf && (unsigned)frame < (unsigned)p.s.B && (mode == 1 || mode == 2);
  draw = draw && window_of(m, p.sx, p.sy, w) && w.z > w.x && w.w > w.y;
  const int side = max(w.z - w.x, w.w - w.y);
  const int c = max(p.cell, 2 * ((side + 31) / 32));
  const int e = p.max_p + f;
  if (brow == 0 && lane == 0) {
    p.table[e] = draw ? frame : -1;
    *reinterpret_cast<int4*>(p.table + p.Ea + (int64_t)e * 4) = w;
    *reinterpret_cast<int4*>(p.table + (int64_t)5 * p.Ea + (int64_t)e * 4) =
        int4{draw ? wrap(p.fcol[f], p.n_colours) : 0, mode, c, 0};
  }
  if (!draw || mode != 1) return;
  // the means of block row brow: blocks anchored at the window's corner rounded down to even
  const int ax = w.x & ~1, ay = w.y & ~1;
  const int ys = ay + brow * c;
  if (ys >= w.w) return;
  const int ya = max(ys, 0), yb = min(ys + c, p.s.H);
  if (ya >= yb) return;
  const uint8_t* base0 = p.s.p0 + (int64_t)frame * p.s.sn0;
  const uint8_t* base1 = NV ? p.s.p1 + (int64_t)frame * p.s.sn1 : nullptr;
  for (int bcol = 0; bcol < AN_BLOCKS; ++bcol) {
    const int xs = ax + bcol * c;
    if (xs >= w.z) break;
    const int xa = max(xs, 0), xb = min(xs + c, p.s.W);
    if (xa >= xb) continue;
    const int cw = xb - xa;
    int lw = 64;                                 // lanes along x: the smallest power of two >= cw, at most 64
    while ((lw >> 1) >= cw) lw >>= 1;
    const int lx = lane & (lw - 1), ly = lane / lw, rows = 64 / lw;
    unsigned s0 = 0, s1 = 0, s2 = 0, nc = 0;
    for (int y = ya + ly; y < yb; y += rows) {
      for (int x = xa + lx; x < xb; x += lw) {
        if (NV) {
          s0 += base0[(int64_t)y * p.s.sh0 + x];
          if (!((x | y) & 1)) {                  // the pair whose first luma pixel this is
            const unsigned pr = *reinterpret_cast<const uint16_t*>(base1 + (int64_t)(y >> 1) * p.s.sh1 + x);
            s1 += pr & 0xffu; s2 += pr >> 8; ++nc;
          }
        } else {
          const uint8_t* px = base0 + (int64_t)y * p.s.sh0 + (int64_t)x * p.s.sw;
          s0 += px[0]; s1 += px[p.s.sc]; s2 += px[2 * p.s.sc];
        }
      }
    }
    s0 = wave_add(s0); s1 = wave_add(s1); s2 = wave_add(s2); nc = wave_add(nc);
    if (lane == 0) {
      const unsigned n = (unsigned)cw * (unsigned)(yb - ya);
      const unsigned n12 = NV ? nc : n;
      const unsigned v0 = (s0 + n / 2) / n;
      const unsigned v1 = n12 ? (s1 + n12 / 2) / n12 : 0u, v2 = n12 ? (s2 + n12 / 2) / n12 : 0u;
      *reinterpret_cast<unsigned*>(p.means + (((int64_t)f * AN_BLOCKS + brow) * AN_BLOCKS + bcol) * 4) =
          v0 | v1 << 8 | v2 << 16;
    }
  }
}

template <bool NV>
__global__ __launch_bounds__(AN_THREADS) void annotate_build_kernel(BuildK p) {
  const int wave = blockIdx.x * (AN_THREADS / 64) + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (wave < p.max_p) {
    build_person(p, wave, lane);
  } else {
    const int r = wave - p.max_p, f = r / AN_BLOCKS;
    if (f < p.max_f) build_face<NV>(p, f, r - f * AN_BLOCKS, lane);
  }
}

// ---------------------------------------------------------------- paint
struct PaintK {
  Surf s;
  const int* n_p; int max_p;
  const int* n_f; int max_f;
  int PP, n_limbs, Ea;
  int box_t, limb_r, kp_r;
  const int* table; const uint8_t* means; const uint8_t* palette;
  int stx, sty;                                // super-tiles per axis
};

struct LPrim {
  int x0, y0, x1, y1;                          // the primitive
  int bx0, by0, bx1, by1;                      // its bounding box, [..) on both axes
  unsigned key; int kind, r2, t;
};

// the position of a kept candidate in the workgroup's list and the list's length; every thread
// calls it. The first barrier also ends every read of the list formed before.
__device__ __forceinline__ int block_compact(bool keep, int* s_cnt, int& total) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const unsigned long long mask = __ballot(keep);
  __syncthreads();
  if (lane == 0) s_cnt[wave] = __popcll(mask);
  __syncthreads();
  int base = 0;
  total = 0;
#pragma unroll
  for (int w = 0; w < AN_THREADS / 64; ++w) {
    const int c = s_cnt[w];
    base += w < wave ? c : 0;
    total += c;
  }
  return base + __popcll(mask & ((1ull << lane) - 1ull));
}

__device__ __forceinline__ bool covers(const LPrim& q, int x, int y) {
  if (q.kind == KIND_ROUND) {
    const int pax = x - q.x0, pay = y - q.y0, pbx = x - q.x1, pby = y - q.y1;
    if (pax * pax + pay * pay <= q.r2 || pbx * pbx + pby * pby <= q.r2) return true;
    const int dx = q.x1 - q.x0, dy = q.y1 - q.y0;
    const int L2 = dx * dx + dy * dy, dot = pax * dx + pay * dy;
    if (L2 == 0 || dot < 0 || dot > L2) return false;
    const int64_t cr = (int64_t)dx * pay - (int64_t)dy * pax;
    return cr * cr <= (int64_t)q.r2 * L2;
  }
  if (!(x >= q.x0 && x < q.x1 && y >= q.y0 && y < q.y1)) return false;
  if (q.kind == KIND_RECT) return true;
  return !(x >= q.x0 + q.t && x < q.x1 - q.t && y >= q.y0 + q.t && y < q.y1 - q.t);
}

// the list's primitives against a thread's strips, tile by tile
__device__ __forceinline__ void consume(const LPrim* list, int n, int X0, int Y0, int W, int H,
                                        unsigned (&key)[NTILE][NPIX]) {
  const int cx = (threadIdx.x & (TILE_W / STRIP_W - 1)) * STRIP_W, cy = (threadIdx.x / (TILE_W / STRIP_W)) * STRIP_H;
#pragma unroll
  for (int t = 0; t < NTILE; ++t) {
    const int tx = X0 + (t % SUPER_X) * TILE_W, ty = Y0 + (t / SUPER_X) * TILE_H;
    if (tx >= W || ty >= H) continue;
    const int px = tx + cx, py = ty + cy;
    for (int j = 0; j < n; ++j) {
      const LPrim& q = list[j];
      if (q.bx1 <= tx || q.bx0 >= tx + TILE_W || q.by1 <= ty || q.by0 >= ty + TILE_H) continue;   // the whole workgroup
      if (q.bx1 <= px || q.bx0 >= px + STRIP_W || q.by1 <= py || q.by0 >= py + STRIP_H) continue;
#pragma unroll
      for (int i = 0; i < NPIX; ++i)
        if (key[t][i] < q.key && covers(q, px + (i & (STRIP_W - 1)), py + i / STRIP_W)) key[t][i] = q.key;
    }
  }
}

// the three bytes a key paints at (x, y): a palette entry, or a face's block mean
__device__ __forceinline__ unsigned value_of(const PaintK& p, unsigned key, int x, int y) {
  const int layer = (int)(key >> 28) - 1, slot = (int)(SLOT_MASK - (key & SLOT_MASK));
  const int e = layer == L_FACE ? p.max_p + slot : slot;
  const int4 m = ld4(p.table + (int64_t)5 * p.Ea + (int64_t)e * 4);
  if (layer != L_FACE || m.y != 1) return reinterpret_cast<const unsigned*>(p.palette)[m.x];
  const int* w = p.table + p.Ea + (int64_t)e * 4;
  const int bx = (x - (w[0] & ~1)) / m.z, by = (y - (w[1] & ~1)) / m.z;
  return reinterpret_cast<const unsigned*>(p.means)[((int64_t)slot * AN_BLOCKS + by) * AN_BLOCKS + bx];
}

template <bool NV>
__device__ __forceinline__ void write_strip(const PaintK& p, int n, int px, int py, const unsigned (&key)[NPIX]) {
  unsigned any = 0;
#pragma unroll
  for (int i = 0; i < NPIX; ++i) any |= key[i];
  if (!any) return;
  unsigned val[NPIX];
  unsigned lastk = 0, lastv = 0;
  bool reuse = false;
#pragma unroll
  for (int i = 0; i < NPIX; ++i) {
    val[i] = 0;
    if (!key[i]) continue;
    if (!(reuse && key[i] == lastk)) {
      lastv = value_of(p, key[i], px + (i & (STRIP_W - 1)), py + i / STRIP_W);
      lastk = key[i];
      reuse = (key[i] >> 28) - 1 != L_FACE;      // a face's value may change from pixel to pixel
    }
    val[i] = lastv;
    if (!NV) {                                   // three byte stores at the view's strides
      uint8_t* q = p.s.p0 + (int64_t)n * p.s.sn0 + (int64_t)(py + i / STRIP_W) * p.s.sh0 +
                   (int64_t)(px + (i & (STRIP_W - 1))) * p.s.sw;
      q[0] = (uint8_t)lastv; q[p.s.sc] = (uint8_t)(lastv >> 8); q[2 * p.s.sc] = (uint8_t)(lastv >> 16);
    }
  }
  if (NV) {
    const bool full = px + STRIP_W <= p.s.W && p.s.wide;
#pragma unroll
    for (int r = 0; r < STRIP_H; ++r) {
      uint8_t* row = p.s.p0 + (int64_t)n * p.s.sn0 + (int64_t)(py + r) * p.s.sh0 + px;
      unsigned long long v = 0ull, mask = 0ull;
#pragma unroll
      for (int c = 0; c < STRIP_W; ++c)
        if (key[r * STRIP_W + c]) {
          v |= (unsigned long long)(val[r * STRIP_W + c] & 0xffu) << (8 * c);
          mask |= 0xffull << (8 * c);
        }
      if (!mask) continue;
      if (full) {
        unsigned long long* q = reinterpret_cast<unsigned long long*>(row);
        *q = ~mask ? (*q & ~mask) | v : v;
      } else {
#pragma unroll
        for (int c = 0; c < STRIP_W; ++c)
          if (key[r * STRIP_W + c]) row[c] = (uint8_t)(v >> (8 * c));
      }
    }
    // the pairs of the strip: pair (py / 2, px / 2 + k) follows luma pixel (py, px + 2 k)
    uint8_t* crow = p.s.p1 + (int64_t)n * p.s.sn1 + (int64_t)(py >> 1) * p.s.sh1 + px;
    unsigned long long v = 0ull, mask = 0ull;
#pragma unroll
    for (int k = 0; k < STRIP_W / 2; ++k)
      if (key[2 * k]) {
        v |= (unsigned long long)(val[2 * k] >> 8 & 0xffffu) << (16 * k);
        mask |= 0xffffull << (16 * k);
      }
    if (mask) {
      if (full) {
        unsigned long long* q = reinterpret_cast<unsigned long long*>(crow);
        *q = ~mask ? (*q & ~mask) | v : v;
      } else {
#pragma unroll
        for (int k = 0; k < STRIP_W / 2; ++k)
          if (key[2 * k]) reinterpret_cast<uint16_t*>(crow)[k] = (uint16_t)(v >> (16 * k));
      }
    }
  }
}

template <bool NV>
__global__ __launch_bounds__(AN_THREADS) void annotate_paint_kernel(PaintK p) {
  __shared__ LPrim s_prim[CHUNK];
  __shared__ int s_own[CHUNK];
  __shared__ int s_cnt[AN_THREADS / 64];
  const int per = p.stx * p.sty, tid = threadIdx.x;
  const int n = blockIdx.x / per, rem = blockIdx.x - n * per;
  const int X0 = (rem % p.stx) * SUPER_W, Y0 = (rem / p.stx) * SUPER_H;
  const int X1 = min(X0 + SUPER_W, p.s.W), Y1 = min(Y0 + SUPER_H, p.s.H);
  const int np = clamp_count(p.n_p, p.max_p), nf = clamp_count(p.n_f, p.max_f);
  const int* box = p.table + p.Ea;
  unsigned key[NTILE][NPIX];
#pragma unroll
  for (int t = 0; t < NTILE; ++t)
#pragma unroll
    for (int i = 0; i < NPIX; ++i) key[t][i] = 0u;
  bool painted = false;                          // the same in every thread

  // faces: an owner is its own primitive
  for (int e0 = 0; e0 < nf; e0 += CHUNK) {
    const int f = e0 + tid;
    bool keep = f < nf && p.table[p.max_p + f] == n;
    int4 w = {0, 0, 0, 0};
    if (keep) {
      w = ld4(box + (int64_t)(p.max_p + f) * 4);
      keep = w.x < X1 && w.z > X0 && w.y < Y1 && w.w > Y0;
    }
    int total;
    const int pos = block_compact(keep, s_cnt, total);
    if (keep) s_prim[pos] = LPrim{w.x, w.y, w.z, w.w, w.x, w.y, w.z, w.w,
                                  (unsigned)(L_FACE + 1) << 28 | (SLOT_MASK - (unsigned)f), KIND_RECT, 0, 0};
    __syncthreads();
    if (total) {
      consume(s_prim, total, X0, Y0, p.s.W, p.s.H, key);
      painted = true;
    }
  }
  // persons: the kept owners of a chunk, then their primitives a chunk at a time
  for (int e0 = 0; e0 < np; e0 += CHUNK) {
    const int e = e0 + tid;
    bool keep = e < np && p.table[e] == n;
    if (keep) {
      const int4 w = ld4(box + (int64_t)e * 4);
      keep = w.x < X1 && w.z > X0 && w.y < Y1 && w.w > Y0;
    }
    int owners;
    const int at = block_compact(keep, s_cnt, owners);
    if (keep) s_own[at] = e;
    __syncthreads();
    const int cand = owners * p.PP;
    for (int i0 = 0; i0 < cand; i0 += CHUNK) {
      const int i = i0 + tid;
      LPrim q{};
      bool hit = false;
      if (i < cand) {
        const int h = i / p.PP, k = i - h * p.PP, slot = s_own[h];
        const int4 c = ld4(p.table + (int64_t)9 * p.Ea + ((int64_t)slot * p.PP + k) * 4);
        if (c.x != VOID) {
          const int layer = k == 0 ? L_BOX : (k <= p.n_limbs ? L_LIMB : L_DISC);
          const int r = layer == L_LIMB ? p.limb_r : p.kp_r;
          q = LPrim{c.x, c.y, c.z, c.w, c.x, c.y, c.z, c.w,
                    (unsigned)(layer + 1) << 28 | (SLOT_MASK - (unsigned)slot), KIND_OUTLINE, 0, p.box_t};
          if (k > 0) {
            q.bx0 = min(c.x, c.z) - r; q.by0 = min(c.y, c.w) - r;
            q.bx1 = max(c.x, c.z) + r + 1; q.by1 = max(c.y, c.w) + r + 1;
            q.kind = KIND_ROUND; q.r2 = r * r;
          }
          hit = q.bx0 < X1 && q.bx1 > X0 && q.by0 < Y1 && q.by1 > Y0;
        }
      }
      int total;
      const int pos = block_compact(hit, s_cnt, total);
      if (hit) s_prim[pos] = q;
      __syncthreads();
      if (total) {
        consume(s_prim, total, X0, Y0, p.s.W, p.s.H, key);
        painted = true;
      }
    }
  }
  if (!painted) return;

  const int cx = (tid & (TILE_W / STRIP_W - 1)) * STRIP_W, cy = (tid / (TILE_W / STRIP_W)) * STRIP_H;
#pragma unroll
  for (int t = 0; t < NTILE; ++t) {
    const int px = X0 + (t % SUPER_X) * TILE_W + cx, py = Y0 + (t / SUPER_X) * TILE_H + cy;
#pragma unroll
    for (int i = 0; i < NPIX; ++i)
      if (px + (i & (STRIP_W - 1)) >= p.s.W || py + i / STRIP_W >= p.s.H) key[t][i] = 0u;
    write_strip<NV>(p, n, px, py, key[t]);
  }
}

// ---------------------------------------------------------------- host side
int64_t table_words(int max_p, int max_f, int K, int n_limbs) {
  const int64_t Ea = ((int64_t)max_p + max_f + 3) & ~3LL;
  return 9 * Ea + (int64_t)max_p * (1 + n_limbs + K) * 4;
}

bool sizes_ok(int32_t max_p, int32_t max_f, int32_t K, int32_t n_limbs) {
  return max_p >= 0 && max_f >= 0 && max_p <= AN_MAX_SLOTS && max_f <= AN_MAX_SLOTS && K >= 1 && K <= AN_MAX_K &&
         n_limbs >= 0 && n_limbs <= AN_MAX_LIMBS;
}

// every refusal that does not depend on the surface, and the two parameter blocks
bool args_ok(const prpe_annotate_args* a, BuildK& b, PaintK& k) {
  if (!a || !sizes_ok(a->max_p, a->max_f, a->K, a->n_limbs)) return false;
  if (a->max_p > 0 && (!a->crop_meta_p || !a->n_p || !a->keypoints || !a->person_colour)) return false;
  if (a->max_f > 0 && (!a->crop_meta_f || !a->n_f || !a->face_mode || !a->face_colour || !a->means)) return false;
  if (!a->palette || (uintptr_t)a->palette % 4 || a->n_colours < 1) return false;
  if (a->n_limbs > 0 && !a->limbs) return false;
  for (int i = 0; i < 2 * a->n_limbs; ++i)
    if (a->limbs[i] < 0 || a->limbs[i] >= a->K) return false;
  if (a->box_t < 0 || a->box_t > AN_MAX_R || a->limb_r < 0 || a->limb_r > AN_MAX_R || a->kp_r < 0 || a->kp_r > AN_MAX_R)
    return false;
  if (a->cell < 2 || a->cell > 64 || a->cell % 2) return false;
  if (!(a->sx > 0.f && a->sx < INFINITY && a->sy > 0.f && a->sy < INFINITY) || a->kp_thr != a->kp_thr) return false;
  if (a->max_p + a->max_f > 0) {
    if (!a->table || (uintptr_t)a->table % 16 ||
        a->table_bytes < 4 * table_words(a->max_p, a->max_f, a->K, a->n_limbs))
      return false;
    if (a->max_f > 0 && (uintptr_t)a->means % 4) return false;
  }
  b.meta_p = a->crop_meta_p; b.n_p = a->n_p; b.max_p = a->max_p; b.kpts = a->keypoints; b.K = a->K;
  b.pcol = a->person_colour; b.meta_f = a->crop_meta_f; b.n_f = a->n_f; b.max_f = a->max_f;
  b.fmode = a->face_mode; b.fcol = a->face_colour; b.n_colours = a->n_colours; b.n_limbs = a->n_limbs;
  b.PP = 1 + a->n_limbs + a->K;
  b.Ea = (a->max_p + a->max_f + 3) & ~3;
  b.box_t = a->box_t; b.limb_r = a->limb_r; b.kp_r = a->kp_r; b.cell = a->cell;
  b.kp_thr = a->kp_thr; b.sx = a->sx; b.sy = a->sy;
  b.table = static_cast<int*>(a->table); b.means = a->means;
  for (int i = 0; i < 2 * a->n_limbs; ++i) b.limbs[i] = (unsigned char)a->limbs[i];
  // a zero-capacity list is never dereferenced: its count reads as a capacity of 0
  k.n_p = a->n_p; k.max_p = a->max_p; k.n_f = a->n_f; k.max_f = a->max_f;
  k.PP = b.PP; k.n_limbs = a->n_limbs; k.Ea = b.Ea; k.box_t = a->box_t; k.limb_r = a->limb_r; k.kp_r = a->kp_r;
  k.table = b.table; k.means = a->means; k.palette = a->palette;
  return true;
}

template <bool NV>
int launch(const Surf& s, BuildK& b, PaintK& k, void* stream) {
  if (b.max_p + b.max_f == 0) return 0;
  k.stx = (s.W + SUPER_W - 1) / SUPER_W;
  k.sty = (s.H + SUPER_H - 1) / SUPER_H;
  const int64_t paint = (int64_t)s.B * k.stx * k.sty;
  const int64_t waves = (int64_t)b.max_p + (int64_t)b.max_f * AN_BLOCKS;
  const int64_t build = (waves + AN_THREADS / 64 - 1) / (AN_THREADS / 64);
  if (paint >= (1LL << 31) || build >= (1LL << 31)) return PRPE_EINVAL;
  b.s = s; k.s = s;
  hipLaunchKernelGGL(annotate_build_kernel<NV>, dim3((unsigned)build), dim3(AN_THREADS), 0, as_stream(stream), b);
  hipLaunchKernelGGL(annotate_paint_kernel<NV>, dim3((unsigned)paint), dim3(AN_THREADS), 0, as_stream(stream), k);
  return launch_status();
}

}  // namespace

extern "C" void prpe_annotate_geometry(int32_t* out) {
  out[0] = TILE_H; out[1] = TILE_W; out[2] = SUPER_H; out[3] = SUPER_W;
}

extern "C" int64_t prpe_annotate_table_bytes(int32_t max_p, int32_t max_f, int32_t K, int32_t n_limbs) {
  if (!sizes_ok(max_p, max_f, K, n_limbs)) return PRPE_EINVAL;
  return 4 * table_words(max_p, max_f, K, n_limbs);
}

extern "C" int prpe_annotate_nv12(const prpe_nv12* dst, const prpe_annotate_args* a, void* stream) {
  BuildK b{};
  PaintK k{};
  if (!args_ok(a, b, k)) return PRPE_EINVAL;
  if (!dst || !dst->y || !dst->uv || dst->n < 1 || dst->h < 1 || dst->w < 1 || dst->h > AN_MAX_SIDE ||
      dst->w > AN_MAX_SIDE)
    return PRPE_EINVAL;
  if (dst->y_sh < dst->w || dst->uv_sh < 2 * (int64_t)((dst->w + 1) / 2)) return PRPE_EINVAL;
  if ((uintptr_t)dst->uv % 2 || dst->uv_sn % 2 || dst->uv_sh % 2) return PRPE_EINVAL;
  Surf s{};
  s.p0 = const_cast<uint8_t*>(dst->y); s.p1 = const_cast<uint8_t*>(dst->uv);
  s.B = dst->n; s.H = dst->h; s.W = dst->w;
  s.sn0 = dst->y_sn; s.sh0 = dst->y_sh; s.sn1 = dst->uv_sn; s.sh1 = dst->uv_sh;
  s.wide = !((uintptr_t)dst->y % 8 || dst->y_sn % 8 || dst->y_sh % 8 || (uintptr_t)dst->uv % 8 || dst->uv_sn % 8 ||
             dst->uv_sh % 8);
  return launch<true>(s, b, k, stream);
}

extern "C" int prpe_annotate_u8(const prpe_view_u8* dst, const prpe_annotate_args* a, void* stream) {
  BuildK b{};
  PaintK k{};
  if (!args_ok(a, b, k)) return PRPE_EINVAL;
  if (!dst || !dst->ptr || dst->n < 1 || dst->h < 1 || dst->w < 1 || dst->c != 3 || dst->h > AN_MAX_SIDE ||
      dst->w > AN_MAX_SIDE)
    return PRPE_EINVAL;
  Surf s{};
  s.p0 = const_cast<uint8_t*>(dst->ptr);
  s.B = dst->n; s.H = dst->h; s.W = dst->w;
  s.sn0 = dst->sn; s.sh0 = dst->sh; s.sw = dst->sw; s.sc = dst->sc;
  return launch<false>(s, b, k, stream);
}
