// Triangular symmetric rank-k update on the matrix cores (reference
// El::Herk(El::LOWER, ...) at ml/krr.hpp:371/:639, ml/kernels.hpp:241/:585,
// base/distance.hpp:92/:126): the uplo triangle of
//   C <- alpha op(A) op(A)^T + beta C,
// A f32 (exact three-plane bf16 split, six plane products) or bf16 (one
// product), C f32 / f64, in a fixed summation order.
//
// Operand planes.  A block of K rows of op(A)^T is written as K-contiguous
// bf16 planes S (s x [H | M | L], each seg wide, zero past the block;
// H = rne(x), M = rne(x - H), L = rne(x - H - M)), transposing (A n x s,
// C = A^T A) or not (A s x n, C = A A^T).  bf16 A is its own H plane.
//
// Main kernel (the 256 x 256 / 8-wave / LDS-DMA / swizzle loop of
// gemm_nt.hip).  One step = one 64-wide K slice of one plane pair of one
// lower-triangle tile (tm >= tn).  The steps of ONE chunk of chunk_rows K
// rows, ordered tile-major, then pair, then slice, are cut statically into
// `workgroups` equal ranges (tile-major stream-K, as the cut blocks of
// Y = A Z in rsvd_stream.hip), one range per workgroup, one workgroup per CU,
// and every workgroup walks the same range in every chunk of the launch: the
// whole chip is on one chunk's planes at a time (200 MB at s = 4096, against
// 1 GB for a launch-long range).  The pairs go smallest products first --
// (H,L) (L,H) (H,M) (M,H) (M,M) (H,H) -- so the 2^-16 and 2^-8 terms are
// summed while the accumulator is still small and only the (H,H) pass rounds
// at the magnitude of the result (slice-major order, every pair added to an
// accumulator that already holds H H^T, measured 2.1 x the error of the
// two-product path on 200 x 64 data).
// One f32 accumulator set per (tile, chunk): when it leaves a tile or a chunk
// a workgroup widens it to f64 and adds it into a slab tile it owns
// exclusively (slab g * npw + tile - first_tile(g), at most two per workgroup
// when its range is shorter than a tile's; fragment order, so every access
// is a 512-B wave row).  The partition depends only on (s, chunk_rows,
// workgroups), so it is the same for every launch of a call and the slabs
// keep accumulating across super-chunks.  The finishing kernel sums each
// tile's slabs in ascending owner order, applies alpha / beta and stores only
// the requested triangle (the lower tile transposed for uplo U).  No atomics,
// no waits across workgroups: bit-identical from run to run.
#include "sl_common.hpp"

namespace {

typedef __attribute__((ext_vector_type(8))) __bf16 bf16x8;
typedef __attribute__((ext_vector_type(4))) float f32x4;

constexpr int BM = 256, BK = 64, NT = 512;
constexpr int OPB = BM * BK * 2;        // bytes of one operand slice (32 KB)
constexpr int STAGE = 2 * OPB;          // A + B slice (64 KB)
constexpr int TILE_E = BM * BM;         // elements of one slab tile
constexpr int MAX_WG = 4096;

__device__ __forceinline__ int swz(int r) { return (r >> 1) & 7; }

__device__ __forceinline__ void glds16(const void* g, char* lds_base) {
  __builtin_amdgcn_global_load_lds(g, (__attribute__((address_space(3))) void*)lds_base, 16, 0, 0);
}

// the static partition, shared by the main and the finishing kernel
struct Plan {
  int s, nt;            // order of C, tile rows
  int tiles;            // nt (nt + 1) / 2
  int np;               // plane pairs: 6 (f32 A) or 1 (bf16 A)
  int sc;               // K slices per chunk
  int spt;              // steps of one (tile, chunk): pairs x sc
  int G;                // workgroups
  int npw;              // slab tiles per workgroup
  int64_t W, Q;         // steps of one chunk over all tiles, and per workgroup
};

__host__ __device__ __forceinline__ int64_t plan_lo(const Plan& p, int g) {
  const int64_t v = (int64_t)g * p.Q;
  return v < p.W ? v : p.W;
}

// triangular tile index -> (tm, tn), tm >= tn, tile = tm (tm + 1) / 2 + tn
__device__ __forceinline__ void tile_rc(int tile, int* tm, int* tn) {
  int m = (int)((sqrtf(8.f * (float)tile + 1.f) - 1.f) * 0.5f);
  while ((m + 1) * (m + 2) / 2 <= tile) ++m;
  while (m * (m + 1) / 2 > tile) --m;
  *tm = m;
  *tn = tile - m * (m + 1) / 2;
}

// plane (0 H, 1 M, 2 L) of the A / B side of pair p, smallest products first:
// (H,L) (L,H) (H,M) (M,H) (M,M) (H,H)
__device__ __forceinline__ int pair_a(int p) { return p == 1 ? 2 : (p == 3 || p == 4 ? 1 : 0); }
__device__ __forceinline__ int pair_b(int p) { return p == 0 ? 2 : (p == 2 || p == 4 ? 1 : 0); }

struct Step {
  int tile, c, p, kc;       // tile, chunk, pair, slice of the chunk
  int row0, col0;
};

template <int NP>
__global__ void __launch_bounds__(NT, 1)
k_syrk_split(const bf16_t* __restrict__ P, int64_t ld, int64_t seg, Plan pl, int nsl, double* __restrict__ slabs) {
  __shared__ __attribute__((aligned(1024))) char lds[2 * STAGE];

  // workgroup b runs on XCD b % 8: give each XCD a contiguous eighth of the
  // ranges, so the workgroups sharing an L2 sit on neighbouring tiles of one
  // tile row (the same A panel, and near the same K position)
  const int b = blockIdx.x;
  const int g = (pl.G & 7) == 0 ? (b & 7) * (pl.G >> 3) + (b >> 3) : b;
  const int64_t lo = plan_lo(pl, g), hi = plan_lo(pl, g + 1);
  if (lo >= hi) return;
  const int first_tile = (int)(lo / pl.spt);
  const int nch = (nsl + pl.sc - 1) / pl.sc;     // chunks of this (maybe shorter) super-chunk
  int p_lo, kc_lo;                                // (pair, slice) of step lo in first_tile
  {
    const int r = (int)(lo - (int64_t)first_tile * pl.spt);
    p_lo = r / pl.sc;
    kc_lo = r - p_lo * pl.sc;
  }
  // a position of the full-chunk step list -> the first real step at or
  // after it: a short last chunk has holes (slices past nsl), and past hi the
  // range starts over in the next chunk; false when the chunks are used up
  auto settle = [&](Step& s) -> bool {
    while (true) {
      if (s.kc >= min(pl.sc, nsl - s.c * pl.sc)) { s.kc = 0; ++s.p; }
      if (s.p == NP) { s.p = 0; ++s.tile; }
      if (s.tile < pl.tiles && (int64_t)s.tile * pl.spt + s.p * pl.sc + s.kc < hi) return true;
      if (++s.c >= nch) return false;
      s.tile = first_tile;
      s.p = p_lo;
      s.kc = kc_lo;
    }
  };
  auto place = [&](Step& s) {
    int tm, tn;
    tile_rc(s.tile, &tm, &tn);
    s.row0 = tm * BM;
    s.col0 = tn * BM;
  };
  Step cur;
  cur.tile = first_tile;
  cur.c = 0;
  cur.p = p_lo;
  cur.kc = kc_lo;
  if (!settle(cur)) return;
  place(cur);
  // the step after s, false at the end of the last chunk's range
  auto advance = [&](Step& s) -> bool {
    const int t0 = s.tile;
    if (++s.kc == pl.sc) { s.kc = 0; ++s.p; }
    const bool more = settle(s);
    if (more && s.tile != t0) place(s);
    return more;
  };

  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int wm = w >> 2, wn = w & 3;

  // DMA: instruction i of wave w fills LDS rows (4w + i) * 8 + lane / 8, chunk
  // slot lane % 8, with the global chunk (lane % 8) ^ swz(row); rows past s
  // are clamped (never stored by the finishing kernel)
  auto issue = [&](const Step& s, int st) {
    char* base = lds + st * STAGE + w * 4 * 1024;
    const int64_t k0 = ((int64_t)s.c * pl.sc + s.kc) * BK;
    const bf16_t* pa = P + (NP == 1 ? 0 : pair_a(s.p) * seg) + k0;
    const bf16_t* pb = P + (NP == 1 ? 0 : pair_b(s.p) * seg) + k0;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int r = (4 * w + i) * 8 + (lane >> 3);
      const int c = (lane & 7) ^ swz(r);
      glds16(pa + (int64_t)min(s.row0 + r, pl.s - 1) * ld + c * 8, base + i * 1024);
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int r = (4 * w + i) * 8 + (lane >> 3);
      const int c = (lane & 7) ^ swz(r);
      glds16(pb + (int64_t)min(s.col0 + r, pl.s - 1) * ld + c * 8, base + OPB + i * 1024);
    }
  };

  f32x4 acc[8][4];
#pragma unroll
  for (int i = 0; i < 8; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

  const int fr = lane & 15, fq = lane >> 4;
  auto read_frags = [&](int st, int kh, bf16x8 (&a)[8], bf16x8 (&bb)[4]) {
    const char* sA = lds + st * STAGE;
    const char* sB = sA + OPB;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const int r = wm * 128 + i * 16 + fr;
      a[i] = *(const bf16x8*)(sA + r * 128 + (((4 * kh + fq) ^ swz(r)) << 4));
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int r = wn * 64 + j * 16 + fr;
      bb[j] = *(const bf16x8*)(sB + r * 128 + (((4 * kh + fq) ^ swz(r)) << 4));
    }
  };
  auto mfmas = [&](const bf16x8 (&a)[8], const bf16x8 (&bb)[4]) {
#pragma unroll
    for (int i = 0; i < 8; ++i)
#pragma unroll
      for (int j = 0; j < 4; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[i], bb[j], acc[i][j], 0, 0, 0);
  };
  // f32 accumulators -> += into this workgroup's f64 slab of `tile`, fragment
  // order: element ((w * 32 + i * 4 + j) * 4 + e) * 64 + lane
  auto flush = [&](int tile) {
    double* sl = slabs + ((int64_t)g * pl.npw + (tile - first_tile)) * TILE_E + w * (TILE_E / 8) + lane;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      double v[16];
#pragma unroll
      for (int q = 0; q < 16; ++q) v[q] = sl[(i * 16 + q) * 64];
#pragma unroll
      for (int q = 0; q < 16; ++q) sl[(i * 16 + q) * 64] = v[q] + (double)acc[i][q >> 2][q & 3];
#pragma unroll
      for (int j = 0; j < 4; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
    }
  };

  // One step = one 64-wide K slice of one plane pair.  As in gemm_nt.hip the
  // DMA of the next step is issued right after the barrier that opens this
  // one, the second K-half's MFMAs are deferred under the next step's first
  // fragment reads, and there is one counted wait + one raw s_barrier per
  // step; the deferred half is drained early when the step closes a (tile,
  // chunk) so the accumulators can be flushed.
  Step nxt = cur;
  bool has_nxt = advance(nxt);
  bf16x8 a0[8], b0[4], a1[8], b1[4];
  issue(cur, 0);
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __builtin_amdgcn_s_barrier();
  __builtin_amdgcn_sched_barrier(0);
  int st = 0;
  bool pend = false;
  while (true) {
    if (has_nxt) issue(nxt, st ^ 1);
    read_frags(st, 0, a0, b0);
    __builtin_amdgcn_s_setprio(1);
    if (pend) mfmas(a1, b1);
    read_frags(st, 1, a1, b1);
    mfmas(a0, b0);
    const bool last = !has_nxt || nxt.tile != cur.tile || nxt.c != cur.c;
    if (last) mfmas(a1, b1);
    pend = !last;
    __builtin_amdgcn_s_setprio(0);
    // step + 1 landed (this wave's DMA), everyone done reading stage st
    asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    __builtin_amdgcn_sched_barrier(0);
    if (last) flush(cur.tile);
    if (!has_nxt) break;
    cur = nxt;
    has_nxt = advance(nxt);
    st ^= 1;
  }
}

// C's uplo triangle <- alpha * (sum of the tile's slabs, ascending owner) + beta * C
template <typename CT>
__global__ void __launch_bounds__(256)
k_syrk_finish(const double* __restrict__ slabs, Plan pl, CT* __restrict__ C, int64_t ldc, int upper, double alpha,
              double beta) {
  const int tile = blockIdx.x;
  int tm, tn;
  tile_rc(tile, &tm, &tn);
  const int ga = (int)(((int64_t)tile * pl.spt) / pl.Q);
  const int gb = (int)(((int64_t)(tile + 1) * pl.spt - 1) / pl.Q);
  for (int x = blockIdx.y * 256 + threadIdx.x; x < TILE_E; x += gridDim.y * 256) {
    const int w = x >> 13, blk = (x >> 8) & 31, e = (x >> 6) & 3, lane = x & 63;
    const int row = tm * BM + (w >> 2) * 128 + (blk >> 2) * 16 + 4 * (lane >> 4) + e;
    const int col = tn * BM + (w & 3) * 64 + (blk & 3) * 16 + (lane & 15);
    if (row >= pl.s || col > row) continue;
    double sum = 0.0;
    for (int g = ga; g <= gb; ++g) {
      const int ft = (int)(plan_lo(pl, g) / pl.spt);
      sum += slabs[((int64_t)g * pl.npw + (tile - ft)) * TILE_E + x];
    }
    CT* p = upper ? C + (int64_t)col * ldc + row : C + (int64_t)row * ldc + col;
    double v = alpha * sum;
    if (beta != 0.0) v += beta * (double)*p;
    *p = (CT)v;
  }
}

// bf16 pair (x0, x1) -> the packed hardware RNE word and the two rounded values
__device__ __forceinline__ uint32_t rne_pair(float x0, float x1, float* r0, float* r1) {
  typedef __attribute__((ext_vector_type(2))) __bf16 bf16x2_t;
  const bf16x2_t q = __builtin_convertvector((__attribute__((ext_vector_type(2))) float){x0, x1}, bf16x2_t);
  const uint32_t p = __builtin_bit_cast(uint32_t, q);
  *r0 = bf16_to_f((bf16_t)(p & 0xffffu));
  *r1 = bf16_to_f((bf16_t)(p >> 16));
  return p;
}

// Transposing three-plane split: X (w x m, ldx) -> S (m x [H | M | L], row
// stride ld), zero for w <= k < 64 ceil(w / 64).  64 x 64 tiles through LDS,
// as k_split3_t of gemm_nt.hip but without the duplicated segments.
__global__ void __launch_bounds__(256)
k_planes_t(const float* __restrict__ X, int w, int m, int64_t ldx, bf16_t* __restrict__ S, int64_t seg, int64_t ld,
           int nsl) {
  __shared__ float tile[64][65];
  const int c0 = blockIdx.x * 64;
  const int t = threadIdx.x;
  const int cc = t >> 2, q = t & 3;
  const int c = c0 + cc;
  // the K blocks of this column strip, gridDim.y apart (nsl may exceed the grid's y limit)
  for (int kb = blockIdx.y; kb < nsl; kb += gridDim.y) {
    const int k0 = kb * 64;
    {
      float v[16];
#pragma unroll
      for (int i = 0; i < 16; ++i) {
        const int e = t + 256 * i, k = k0 + (e >> 6), cx = c0 + (e & 63);
        v[i] = X[(int64_t)(k < w ? k : w - 1) * ldx + (cx < m ? cx : m - 1)];
      }
#pragma unroll
      for (int i = 0; i < 16; ++i) {
        const int e = t + 256 * i, kk = e >> 6, ce = e & 63;
        tile[kk][ce] = (k0 + kk < w && c0 + ce < m) ? v[i] : 0.f;
      }
    }
    __syncthreads();
    if (c < m) {
      uint32_t h[8], md[8], l[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) {
        const float x0 = tile[16 * q + 2 * u][cc], x1 = tile[16 * q + 2 * u + 1][cc];
        float h0, h1, m0, m1, d0, d1;
        h[u] = rne_pair(x0, x1, &h0, &h1);
        const float r0 = x0 - h0, r1 = x1 - h1;
        md[u] = rne_pair(r0, r1, &m0, &m1);
        l[u] = rne_pair(r0 - m0, r1 - m1, &d0, &d1);
      }
      bf16_t* row = S + (int64_t)c * ld + k0 + 16 * q;
      auto put = [&](int sg, const uint32_t* v) {
        uint4* p = (uint4*)(row + (int64_t)sg * seg);
        p[0] = make_uint4(v[0], v[1], v[2], v[3]);
        p[1] = make_uint4(v[4], v[5], v[6], v[7]);
      };
      put(0, h);
      put(1, md);
      put(2, l);
    }
    __syncthreads();   // the tile is rewritten by the next K block
  }
}

// Non-transposing three-plane split: K columns [0, w) of A (m x *, lda; already
// K-contiguous) -> S (m x [H | M | L]), zero for w <= k < kpad
__global__ void __launch_bounds__(256)
k_planes_n(const float* __restrict__ A, int w, int m, int64_t lda, bf16_t* __restrict__ S, int64_t seg, int64_t ld,
           int kpad) {
  const int64_t per_row = kpad / 4;
  const int64_t total = (int64_t)m * per_row;
  for (int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; t < total; t += (int64_t)gridDim.x * blockDim.x) {
    const int64_t r = t / per_row;
    const int k = (int)(t - r * per_row) * 4;
    float x[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) x[e] = A[r * lda + (k + e < w ? k + e : w - 1)];
#pragma unroll
    for (int e = 0; e < 4; ++e) x[e] = k + e < w ? x[e] : 0.f;
    float h0, h1, h2, h3, m0, m1, m2, m3, d;
    const uint32_t ha = rne_pair(x[0], x[1], &h0, &h1), hb = rne_pair(x[2], x[3], &h2, &h3);
    const float r0 = x[0] - h0, r1 = x[1] - h1, r2 = x[2] - h2, r3 = x[3] - h3;
    const uint32_t ma = rne_pair(r0, r1, &m0, &m1), mb = rne_pair(r2, r3, &m2, &m3);
    const uint32_t la = rne_pair(r0 - m0, r1 - m1, &d, &d), lb = rne_pair(r2 - m2, r3 - m3, &d, &d);
    bf16_t* row = S + r * ld + k;
    *(uint2*)row = make_uint2(ha, hb);
    *(uint2*)(row + seg) = make_uint2(ma, mb);
    *(uint2*)(row + 2 * seg) = make_uint2(la, lb);
  }
}

int auto_workgroups() {
  static int cus = 0;
  if (cus == 0) {
    int dev = 0;
    hipDeviceProp_t prop;
    if (hipGetDevice(&dev) != hipSuccess || hipGetDeviceProperties(&prop, dev) != hipSuccess) return 256;
    cus = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
  }
  return cus;
}

// the partition of a call: false when the arguments are out of range
bool make_plan(int s, int64_t k_full, int chunk_rows, int workgroups, int np, Plan* pl) {
  if (s <= 0 || k_full <= 0 || chunk_rows <= 0 || chunk_rows % BK || workgroups > MAX_WG || (np != 1 && np != 6))
    return false;
  const int64_t nsl = (k_full + BK - 1) / BK;
  pl->s = s;
  pl->nt = (s + BM - 1) / BM;
  if (pl->nt > 8192) return false;
  pl->tiles = pl->nt * (pl->nt + 1) / 2;
  pl->np = np;
  // slices per chunk (one short chunk when k_full < chunk_rows)
  pl->sc = (int)(chunk_rows / BK < nsl ? chunk_rows / BK : nsl);
  pl->spt = pl->sc * np;
  pl->W = (int64_t)pl->tiles * pl->spt;
  // one workgroup per CU, but never more than there are steps to hand out (a
  // one-tile problem would clear 128 MB of slabs that stay zero)
  const int cus = auto_workgroups();
  pl->G = workgroups > 0 ? workgroups : (int)(pl->W < cus ? pl->W : cus);
  pl->Q = (pl->W + pl->G - 1) / pl->G;
  // a range of Q steps starting anywhere in a tile touches at most this many tiles
  const int64_t npw = (pl->Q + pl->spt - 2) / pl->spt + 1;
  pl->npw = (int)(npw < pl->tiles ? npw : pl->tiles);
  return true;
}

}  // namespace

// Workspace sizes of a call: out[0] = slab tiles (256 x 256 f64 each) the
// partition of (s, k_full, chunk_rows, workgroups, pairs) needs, out[1] = the
// workgroups it launches (workgroups <= 0: one per CU).
SL_API int sl_syrk_split_plan(int s, int64_t k_full, int chunk_rows, int workgroups, int a_dtype, int64_t* out) {
  Plan pl;
  if (!make_plan(s, k_full, chunk_rows, workgroups, a_dtype == SL_BF16 ? 1 : 6, &pl)) {
    sl_set_last_error("syrk_split_plan: needs s > 0, k_full > 0, chunk_rows % 64 == 0, workgroups <= 4096");
    return SL_ERR_INVALID;
  }
  out[0] = (int64_t)pl.G * pl.npw;
  out[1] = pl.G;
  return SL_OK;
}

// One super-chunk of C's uplo triangle <- alpha op(A) op(A)^T + beta C.
//   A: k_len K rows of the operand -- trans != 0: A is k_len x s (C = A^T A),
//      else s x k_len (C = A A^T) -- f32 (split into S) or bf16 (trans == 0
//      only, read in place: 16-B aligned rows, k_len % 64 == 0);
//   S: split workspace, s x 3 seg bf16 (f32 A), seg % 64 == 0, seg >= k_len;
//   slabs: n_slabs zero-initialised 256 x 256 f64 tiles (sl_syrk_split_plan),
//      accumulated across the super-chunks of a call; k_full is the length of
//      a full super-chunk (the caller keeps it a multiple of chunk_rows when
//      there is more than one; it is the same for every launch of a call, so
//      the partition is too), k_len <= k_full;
//   finish != 0 (last super-chunk): reduce the slabs into C (s x s, ldc, f32 /
//      f64; uplo 'L' / 'U'); beta == 0 does not read C.
SL_API int sl_syrk_split(const void* A, int a_dtype, int trans, int s, int64_t k_len, int64_t k_full, int64_t lda,
                         void* S, int64_t seg, void* slabs, int64_t n_slabs, int chunk_rows, int workgroups,
                         int finish, void* C, int c_dtype, int64_t ldc, int uplo, double alpha, double beta,
                         void* stream) {
  const int np = a_dtype == SL_BF16 ? 1 : 6;
  Plan pl;
  if ((a_dtype != SL_F32 && a_dtype != SL_BF16) || !make_plan(s, k_full, chunk_rows, workgroups, np, &pl) ||
      k_len <= 0 || k_len > k_full || !A || !slabs || n_slabs < (int64_t)pl.G * pl.npw) {
    sl_set_last_error("syrk_split: needs f32 / bf16 A, 0 < k_len <= k_full, chunk_rows % 64 == 0, slabs from "
                      "syrk_split_plan");
    return SL_ERR_INVALID;
  }
  if (finish && (!C || (c_dtype != SL_F32 && c_dtype != SL_F64) || ldc < s || (uplo != 'L' && uplo != 'U'))) {
    sl_set_last_error("syrk_split: C must be f32 / f64 with ldc >= s, uplo 'L' or 'U'");
    return SL_ERR_INVALID;
  }
  hipStream_t st = (hipStream_t)stream;
  const int nsl = (int)((k_len + BK - 1) / BK);
  const bf16_t* P;
  int64_t ld;
  if (a_dtype == SL_BF16) {
    if (trans || k_len % BK || lda % 8 || lda < k_len || ((uintptr_t)A & 15)) {
      sl_set_last_error("syrk_split: bf16 A needs trans == 0, k_len % 64 == 0, 16-B aligned rows");
      return SL_ERR_INVALID;
    }
    P = (const bf16_t*)A;
    ld = lda;
  } else {
    if (!S || seg % BK || seg < k_len || ((uintptr_t)S & 15) || lda < (trans ? s : k_len) || k_len > INT32_MAX - BK) {
      sl_set_last_error("syrk_split: f32 A needs a 16-B aligned split workspace with seg % 64 == 0, seg >= k_len");
      return SL_ERR_INVALID;
    }
    P = (const bf16_t*)S;
    ld = 3 * seg;
    if (trans) {
      dim3 grid((unsigned)((s + 63) / 64), (unsigned)(nsl < 65535 ? nsl : 65535));
      k_planes_t<<<grid, 256, 0, st>>>((const float*)A, (int)k_len, s, lda, (bf16_t*)S, seg, ld, nsl);
    } else {
      const unsigned grid = sl_grid_for((size_t)s * (size_t)(nsl * (BK / 4)), 256, 8192);
      k_planes_n<<<grid, 256, 0, st>>>((const float*)A, (int)k_len, s, lda, (bf16_t*)S, seg, ld, nsl * BK);
    }
    SL_LAUNCH_CHECK();
  }
  if (np == 6) k_syrk_split<6><<<(unsigned)pl.G, NT, 0, st>>>(P, ld, seg, pl, nsl, (double*)slabs);
  else k_syrk_split<1><<<(unsigned)pl.G, NT, 0, st>>>(P, ld, seg, pl, nsl, (double*)slabs);
  SL_LAUNCH_CHECK();
  if (finish) {
    dim3 grid((unsigned)pl.tiles, 16);
    if (c_dtype == SL_F64)
      k_syrk_finish<double><<<grid, 256, 0, st>>>((const double*)slabs, pl, (double*)C, ldc, uplo == 'U', alpha, beta);
    else
      k_syrk_finish<float><<<grid, 256, 0, st>>>((const double*)slabs, pl, (float*)C, ldc, uplo == 'U', alpha, beta);
    SL_LAUNCH_CHECK();
  }
  return SL_OK;
}
