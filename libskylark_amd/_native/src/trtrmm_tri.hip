// In-place f64 triangular-triangular product (Elemental's Trtrmm, LAPACK's LAUUM): the `uplo` triangle of a
// row-major n x n matrix A holds a triangular factor and is overwritten by the same triangle of L^T L (uplo 'L') or
// U U^T (uplo 'U').  The third stage of HPDInverse (Cholesky, TriangularInverse, Trtrmm), the reference's
// El::Inverse(*Cache[j]) of ml/BlockADMM.hpp:437: with X = L^-1 in the triangle, X^T X is the inverse of L L^T.
//
// Storage rules (the family's, see trtri_tri.hip): the strict other triangle of A and the pitch padding are never
// read or written and may hold NaN; no status word, no workspace, no allocation, no host synchronisation.
//
// Both triangles run one algorithm on a logical lower-triangular view L[i][c] in which one of the two strides is 1.
// uplo 'L' is the matrix itself (L[i][c] = A[i pitch + c]); uplo 'U' is its transposed view (L[i][c] = A[c pitch + i]:
// U^T is lower triangular and (U^T)^T U^T = U U^T).  The index reversal of trsm_tri.hip / trtri_tri.hip does not
// carry over: under i -> n - 1 - i, U U^T becomes L L^T, not L^T L.  A template flag (TV) selects the view; it
// changes two things only.  (1) How a slice of L is staged: L[k][x] runs along memory in x for the matrix itself
// (as stage_x of trtri_tri.hip) and in k for the transposed view (as stage_m), and the staging index is decoded so
// that consecutive lanes load consecutive doubles in both.  (2) Which of the two blocks of a tile feeds the MFMA's
// row operand: the accumulator's column index (lane & 15) must be the direction that runs along memory, so the
// transposed view computes the transposed tile.  The memory address of an accumulator element is then the same
// expression in both variants, and only the side of the diagonal that a diagonal tile keeps differs.  A column-major
// A is passed by the caller as the transposed row-major operand with uplo flipped.
//
// Schedule.  In 128 x 128 blocks (NB = T = 128; r, I, J are block indices) the result is
//     C[I][J] = sum over row slabs r >= I of L[r][I]^T L[r][J],      J <= I.
// LAPACK's order (step i writes row block i with K = n - i0) starts with single tiles whose K is close to n, one
// after the other.  This file takes the slab order instead: the outer loop runs over row slab r from the top, and
// every tile [I][J] with I < r adds the slab's rank-128 contribution L[r][I]^T L[r][J], so every step fills the chip
// and each element is read-modify-written once per step by its one owner.  Step r = 1 .. nblk - 1 is two launches of
// one kernel, and one closing launch ends the call:
//
//   1. update(r)  tiles [I][J], J <= I < r:  acc <- C[I][J] (loaded);  acc += L[r][I]^T L[r][J];  store.
//                 The owner of [r-1][r-1] loads nothing: it starts from masked(L11)^T masked(L11) of its own block,
//                 which still holds L[r-1][r-1], and then adds the slab (two passes of K = 128).  It is enumerated
//                 first, the longest tile of the launch.
//   2. row(r)     tiles [r][J], J < r:  acc <- 0;  acc += masked(L[r][r])^T L[r][J];  store over L[r][J].
//   3. closing    tile [nblk-1][nblk-1]:  masked(L11)^T masked(L11) over itself.
//
// Hazards, and why each launch boundary exists.  update(r) reads the slab, row block r, in every tile, so nothing in
// row block r can be written in that launch: row(r), which overwrites L[r][J], comes after it.  row(r) reads L[r][r]
// in every tile, so L[r][r] cannot be overwritten in that launch: its product is folded into update(r + 1), which
// runs after row(r) in stream order and touches row block r only through the tiles' own read-modify-write; the last
// diagonal block has no update(r + 1) and is the closing launch.  update(r + 1) cannot be merged with row(r) either:
// it overwrites L[r][r], which row(r) reads.  Within a launch every tile reads blocks that no other tile of the
// launch writes (its own, the slab, or L[r][r]), and a workgroup's own global reads are complete (staged through
// LDS behind barriers) before its stores.  2 nblk - 1 launches for n > 0, one for n <= 128.
//
// The tile is the family's (sl_tri_f64.hpp: 128 x 128, K in slices of 32 through LDS, operand and accumulator
// layout); the staging is this file's own.  K positions that fall outside the triangle (the diagonal blocks of a
// slab: k < x) or outside the matrix are staged as explicit zeros; a loaded value is never multiplied by zero.
// Diagonal output tiles load and store their triangle only, and a wave whose quadrant lies in the other triangle or
// outside the matrix issues no MFMA.  All 32 loads of a thread's staging pass are issued before the first is used,
// and the loads of slice h + 1 are in flight while slice h is multiplied.  Tiles whose blocks lie wholly inside the
// matrix and off the diagonal (all but O(nblk) of a launch) stage and store without tests; the others load without
// branches (see load_slice).
// Two things differ from the other kernels of the family, both decided by the compile log, not by a measurement against it.  (1) One
// workgroup per CU, not two: the 64 registers of the slice in flight next to the 128 accumulator registers do not
// fit 256 registers per lane (__launch_bounds__(256, 2): 233 / 264 registers spilled, 608 / 732 bytes of scratch per
// lane; still 151 / 200 spilled with no slice in flight), and they fit 512.  (2) The staging index map of the
// matrix-itself view (see px / pk).
//
// The sums have at most n terms; the order is fixed (K slices in order, four terms per MFMA, one fused multiply-add
// each): no atomics, no workgroup waits on another, every element has one writer per launch, results are
// bit-identical from run to run.  n^3 / 3 flops.
//
// Compile log (gfx950, -O3, kernel resource usage): no spills, scratch is 0 bytes per lane in both instantiations.
// k_trtrmm<false> 173 VGPRs, k_trtrmm<true> 176, each with the accumulator file (256 AGPRs reported) beside them,
// 106 SGPRs, one wave per SIMD.
//
// Measured (one MI355X, C = B B^T + n I, median of 5, ms; profiles/r7/hpdinv_ab.jsonl, benchmarks/bench_hpdinv.py):
// this kernel (uplo L) / the whole HPDInverse chain (chol_tri + trtri_tri + this) / torch.cholesky_inverse(
// torch.linalg.cholesky(C)) / torch.linalg.inv(C):
//   n = 1024   0.63 /  3.17 /  3.29 /   5.81     (15 launches)
//   n = 2048   1.33 /  6.51 /  7.61 /  22.35     (31 launches)
//   n = 4096   2.90 / 13.87 / 18.34 /  55.07     (63 launches; uplo U: 2.72 / 14.40)
//   n = 8192   9.86 / 43.29 / 81.25 / 158.01     (127 launches, 18.6 TFLOP/s of n^3 / 3)
// The chain's stages at n = 4096: Cholesky 6.57, TriangularInverse 4.40, Trtrmm 2.90 ms: with the flops of
// trtri_tri (4.46 ms in profiles/r7/trtri_tri_ab.jsonl) and none of its division chain this kernel is 1.5 times
// faster, and still ten times the 0.29 ms that n^3 / 3 flops take at the f64 matrix-core peak.  Per launch at
// n = 4096 (kernel trace, mean of 4): row(r) 30.7 us at 2 tiles to 33.2 us at 31; update(r) 53.4 us at 3 tiles,
// 55.3 at 120, 58.3 at 253, then 68.1 at 276 to 75.7 at 465 and 90.9 at 496 (more tiles than the 256 CUs); the
// closing launch 29.7 us.  The call is the sum of its launches (63 launches, 2.89 ms in the trace): a serial chain
// of tile latencies, not matrix-core work.  A tile's one pass over K = 128 is about 30 us for 13.7 us of MFMA issue
// on its one wave per SIMD (512 MFMAs of 64 cycles), and up to 256 tiles an update launch lasts as long as its one
// two-pass tile [r-1][r-1], 53 us, whatever the other tiles take.
// Not measured: two workgroups per CU with fewer loads in flight, 64 x 64 tiles or a split of K for the launches
// that do not fill the chip, a separate workgroup shape for the two-pass tile, NB = 256 slabs (half the launches),
// column-major timings, n beyond 8192, sizes that are no multiple of 128.
#include "sl_tri_f64.hpp"

namespace {

using sl_tri::T;                // block width of the schedule and edge of a tile
using sl_tri::KH;               // slab rows staged in LDS at a time
using sl_tri::LP;
using sl_tri::TILE_LDS;
using sl_tri::f64x4;
constexpr int CH = T * KH / 256;                                          // loads per thread and operand slice
constexpr int64_t MAX_PITCH = (int64_t)1 << 22;   // byte offsets inside a block fit 32 bits: (127 pitch + 127) 8 < 2^32

struct Mat {
  double* A;
  int64_t pitch, n;
};

// Every global address below is a workgroup-uniform 64-bit base plus a 32-bit byte offset that depends on the lane
// only (pitch <= MAX_PITCH keeps it below 2^32): one address register per thread serves all loads of a staging pass, so
// that they can all be in flight next to the 128 accumulator registers.
__device__ __forceinline__ const double* at(const char* base, uint32_t off) { return (const double*)(base + off); }
__device__ __forceinline__ double* at(char* base, uint32_t off) { return (double*)(base + off); }

// A thread's CH positions (x, k) of a 128 x 32 operand slice: position u is (px(tid, u), pk(tid, u)).  In both views
// 16 or 32 consecutive lanes load consecutive doubles, and a wave's 64 stores into the slice (pitch 36) fall on all
// LDS banks: it covers 16 x by 4 k for the matrix itself (x runs along memory) and 2 x by 32 k for the transposed
// view (k does).  128 consecutive x per pass, as stage_x of trtri_tri.hip has them, store with an 8-way conflict;
// that cost little here (a row launch 33.7 -> 32.3 us, the call 2.95 -> 2.90 ms at n = 4096, two separate runs).
template <bool TV> __device__ __forceinline__ constexpr int px(int tid, int u) {
  return TV ? tid / KH + (256 / KH) * u : (tid & 15) + 16 * (u & 7);
}
template <bool TV> __device__ __forceinline__ constexpr int pk(int tid, int u) {
  return TV ? tid & (KH - 1) : (tid >> 4) + 16 * (u >> 3);
}

// Slice [k0, k0 + KH) of block (R, X) of the view: t[u] = L[R0 + k0 + k][X0 + x] for this thread's CH positions;
// `voff` is the byte offset of its position 0 in a slice (see k_trtrmm).  GUARD: positions outside the matrix, and
// with `masked` (R == X, a diagonal block) those above the diagonal, are explicit zeros and are not loaded.
template <bool TV, bool GUARD>
__device__ __forceinline__ void load_slice(const Mat& m, int64_t R0, int64_t X0, int k0, bool masked, int tid,
                                           uint32_t voff, double (&t)[CH]) {
  const char* ob = (const char*)(m.A + (TV ? X0 * m.pitch + R0 : R0 * m.pitch + X0));         // the block's origin
  const char* sb = ob + (TV ? (int64_t)k0 : k0 * m.pitch) * (int64_t)sizeof(double);         // the slice's
  const int64_t kr = m.n - R0, xr = m.n - X0;
  const int klim = (int)(kr < T ? kr : T), xlim = (int)(xr < T ? xr : T);   // the block's rows / columns in the matrix
#pragma unroll
  for (int u = 0; u < CH; ++u) {
    if (GUARD) {
      // No load under a test (a guarded load is a branch with its own wait): a position that is not to be read
      // loads the nearest position of the same block that is (inside the matrix, on or below the diagonal), and a
      // select puts the explicit zero in its place.
      const int k = k0 + pk<TV>(tid, u), x = px<TV>(tid, u);
      const bool take = k < klim && x < xlim && (!masked || k >= x);
      const int kc = k < klim ? k : klim - 1;
      int xc = x < xlim ? x : xlim - 1;
      if (masked) xc = xc < kc ? xc : kc;
      const uint32_t off = ((uint32_t)(TV ? xc : kc) * (uint32_t)m.pitch + (uint32_t)(TV ? kc : xc)) *
                           (uint32_t)sizeof(double);
      const double v = *at(ob, off);
      t[u] = take ? v : 0.0;
    } else {
      // position u lies a workgroup-uniform distance from position 0
      const int dx = px<TV>(0, u), dk = pk<TV>(0, u);
      t[u] = *at(sb + (TV ? dx * m.pitch + dk : dk * m.pitch + dx) * (int64_t)sizeof(double), voff);
    }
  }
}

template <bool TV>
__device__ __forceinline__ void store_slice(double* __restrict__ P, int tid, const double (&t)[CH]) {
#pragma unroll
  for (int u = 0; u < CH; ++u) P[px<TV>(tid, u) * LP + pk<TV>(tid, u)] = t[u];
}

// acc += L[R][BM]^T L[R][BN] over the T rows of slab R (BM / BN: the blocks of the MFMA's row / column operand).
template <bool TV, bool GUARD>
__device__ __forceinline__ void slab_pass(const Mat& m, int64_t R, int64_t BM, int64_t BN, double* Ms, double* Xs,
                                          const double* pa, const double* pb, bool active, int tid,
                                          uint32_t voff, f64x4 (&acc)[4][4]) {
  double ta[CH], tb[CH];
  load_slice<TV, GUARD>(m, R * T, BM * T, 0, R == BM, tid, voff, ta);
  load_slice<TV, GUARD>(m, R * T, BN * T, 0, R == BN, tid, voff, tb);
#pragma unroll 1
  for (int h = 0; h < T / KH; ++h) {
    __syncthreads();                      // the previous slice (or pass) has been read
    store_slice<TV>(Ms, tid, ta);
    store_slice<TV>(Xs, tid, tb);
    __syncthreads();
    if (h + 1 < T / KH) {                 // in flight while this slice is multiplied
      load_slice<TV, GUARD>(m, R * T, BM * T, (h + 1) * KH, R == BM, tid, voff, ta);
      load_slice<TV, GUARD>(m, R * T, BN * T, (h + 1) * KH, R == BN, tid, voff, tb);
    }
    if (active) sl_tri::mma_slice<false>(pa, pb, acc);
  }
}

// row == 0, update(r): workgroup b owns tile [I][J], J <= I < r, enumerated from the last ([r-1][r-1]) down.
// row == 1: workgroup b owns tile [r][jb + b] and starts from zero (row(r): jb = 0; closing: jb = r).
template <bool TV>
__global__ void __launch_bounds__(256, 1)
k_trtrmm(const Mat m, const int64_t r, const int row, const int64_t jb) {
  extern __shared__ __align__(16) unsigned char smem[];
  double* Ms = (double*)smem;
  double* Xs = Ms + T * LP;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  int64_t I, J;
  if (row) {
    I = r, J = jb + blockIdx.x;
  } else {
    const int64_t t = r * (r + 1) / 2 - 1 - (int64_t)blockIdx.x;
    I = (int64_t)((sqrt(8.0 * (double)t + 1.0) - 1.0) * 0.5);
    while (I * (I + 1) / 2 > t) --I;
    while ((I + 1) * (I + 2) / 2 <= t) ++I;
    J = t - I * (I + 1) / 2;
  }
  const bool diag = I == J;
  const bool own = !row && diag && I == r - 1;    // starts from the product of its own block
  const bool load = !row && !own;
  const int64_t BM = TV ? J : I, BN = TV ? I : J;  // memory row / column block of the tile
  const int wp = wave >> 1, wq = wave & 1;
  const int fr = lane & 15, fq = lane >> 4;
  const int p0 = wp * 64 + fq, q0 = wq * 64 + fr;
  const int64_t mr = m.n - BM * T, nr = m.n - BN * T;
  const int mlim = (int)(mr < T ? mr : T), nlim = (int)(nr < T ? nr : T);   // the tile's rows / columns in the matrix
  char* cb = (char*)(m.A + BM * T * m.pitch + BN * T);
  const uint32_t coff = (uint32_t)((p0 * m.pitch + q0) * (int64_t)sizeof(double));
  const int64_t crow = m.pitch * (int64_t)sizeof(double);
  const uint32_t voff = (uint32_t)(((TV ? px<TV>(tid, 0) : pk<TV>(tid, 0)) * m.pitch +
                                    (TV ? pk<TV>(tid, 0) : px<TV>(tid, 0))) * (int64_t)sizeof(double));
  // wave-uniform: a quadrant outside the matrix or in the other triangle of a diagonal tile takes no part
  const bool active = BM * T + wp * 64 < m.n && BN * T + wq * 64 < m.n && (!diag || (TV ? wq >= wp : wq <= wp));
  const double* pa = Ms + (wp * 64 + fr) * LP + fq;
  const double* pb = Xs + (wq * 64 + fr) * LP + fq;
  // block-uniform: the whole tile is stored (off the diagonal and inside the matrix)
  const bool whole = !diag && mlim == T && nlim == T;
  f64x4 acc[4][4];
#pragma unroll
  for (int mi = 0; mi < 4; ++mi)
#pragma unroll
    for (int ni = 0; ni < 4; ++ni) acc[mi][ni] = f64x4{0.0, 0.0, 0.0, 0.0};
  if (load && active) {
    if (whole) {
#pragma unroll
      for (int mi = 0; mi < 4; ++mi)
#pragma unroll
        for (int ni = 0; ni < 4; ++ni)
#pragma unroll
          for (int g = 0; g < 4; ++g)
            acc[mi][ni][g] = *at(cb + (mi * 16 + 4 * g) * crow + ni * 16 * (int)sizeof(double), coff);
    } else {
      // as in load_slice: no load under a test, an element that is not stored loads the nearest one that is
#pragma unroll
      for (int mi = 0; mi < 4; ++mi)
#pragma unroll
        for (int ni = 0; ni < 4; ++ni)
#pragma unroll
          for (int g = 0; g < 4; ++g) {
            const int p = p0 + mi * 16 + 4 * g, q = q0 + ni * 16;
            const bool take = p < mlim && q < nlim && (!diag || (TV ? q >= p : q <= p));
            int pc = p < mlim ? p : mlim - 1, qc = q < nlim ? q : nlim - 1;
            if (diag) {
              if (TV) pc = pc < qc ? pc : qc;
              else qc = qc < pc ? qc : pc;
            }
            const double c = *at(cb, ((uint32_t)pc * (uint32_t)m.pitch + (uint32_t)qc) * (uint32_t)sizeof(double));
            acc[mi][ni][g] = take ? c : 0.0;
          }
    }
  }
#pragma unroll 1
  for (int64_t R = own ? I : r; R <= r; ++R) {
    // block-uniform: all three blocks inside the matrix and off the diagonal
    const bool full = R != I && R != J && (R + 1) * T <= m.n;
    if (full) slab_pass<TV, false>(m, R, BM, BN, Ms, Xs, pa, pb, active, tid, voff, acc);
    else slab_pass<TV, true>(m, R, BM, BN, Ms, Xs, pa, pb, active, tid, voff, acc);
  }
  if (!active) return;
  if (whole) {
#pragma unroll
    for (int mi = 0; mi < 4; ++mi)
#pragma unroll
      for (int ni = 0; ni < 4; ++ni)
#pragma unroll
        for (int g = 0; g < 4; ++g)
          *at(cb + (mi * 16 + 4 * g) * crow + ni * 16 * (int)sizeof(double), coff) = acc[mi][ni][g];
    return;
  }
#pragma unroll
  for (int mi = 0; mi < 4; ++mi)
#pragma unroll
    for (int ni = 0; ni < 4; ++ni)
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const int p = p0 + mi * 16 + 4 * g, q = q0 + ni * 16;
        if (p < mlim && q < nlim && (!diag || (TV ? q >= p : q <= p)))
          *at(cb + (mi * 16 + 4 * g) * crow + ni * 16 * (int)sizeof(double), coff) = acc[mi][ni][g];
      }
}

template <bool TV>
int run(const Mat& m, hipStream_t st) {
  SL_LDS_ATTR((k_trtrmm<TV>), TILE_LDS);
  const int64_t nblk = (m.n + T - 1) / T;
  for (int64_t r = 1; r < nblk; ++r) {
    k_trtrmm<TV><<<(unsigned)(r * (r + 1) / 2), 256, TILE_LDS, st>>>(m, r, 0, 0);
    SL_LAUNCH_CHECK();
    k_trtrmm<TV><<<(unsigned)r, 256, TILE_LDS, st>>>(m, r, 1, 0);
    SL_LAUNCH_CHECK();
  }
  k_trtrmm<TV><<<1u, 256, TILE_LDS, st>>>(m, nblk - 1, 1, nblk - 1);
  SL_LAUNCH_CHECK();
  return SL_OK;
}

}  // namespace

// The sizes at which the code changes path: the block width of the schedule and the edge of a tile (equal here).
SL_API int sl_trtrmm_tri_block(int* nb, int* tile) {
  if (nb) *nb = T;
  if (tile) *tile = T;
  return SL_OK;
}

// The `uplo` triangle of the row-major f64 n x n matrix A, row pitch `pitch` >= n (elements), 8-B aligned, is
// overwritten by that triangle of L^T L ('L') or U U^T ('U').  Ordinary launches on `stream`, no host
// synchronisation; n = 0 returns at once.
SL_API int sl_trtrmm_tri(void* A, int uplo, int64_t n, int64_t pitch, void* stream) {
  if (n < 0 || (uplo != 'L' && uplo != 'U') || (n > 0 && (!A || pitch < n || pitch > MAX_PITCH)) ||
      ((uintptr_t)A & 7)) {
    sl_set_last_error("trtrmm_tri: needs an 8-B aligned f64 A, 0 <= n <= pitch <= 2^22, uplo 'L' / 'U'");
    return SL_ERR_INVALID;
  }
  if (n == 0) return SL_OK;
  const Mat m{(double*)A, pitch, n};
  hipStream_t st = (hipStream_t)stream;
  return uplo == 'U' ? run<true>(m, st) : run<false>(m, st);
}
