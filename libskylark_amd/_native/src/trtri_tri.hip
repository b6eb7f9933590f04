// Blocked, in-place f64 triangular inverse: the `uplo` triangle of a row-major
// n x n matrix A is overwritten by the same triangle of A^-1; diag 'U' takes a
// unit diagonal.  The reference's El::TriangularInverse(El::UPPER, El::NON_UNIT,
// invA) (algorithms/regression/accelerated_linearl2_regression_solver_Elemental
// .hpp:63), the explicit R^-1 preconditioner of Blendenpik / LSRN.
//
// Storage rules: the strict other triangle of A and the pitch padding are never
// read or written, with diag 'U' neither is the diagonal.  They may all hold
// NaN.  A zero on a non-unit diagonal gives inf / NaN as in BLAS; there is no
// status word, no workspace, no host synchronisation and no allocation.
//
// Both triangles run one code path on a logical lower-triangular view L[i][c] =
// A[base + i rs + c cs] (trsm_tri.hip's trick, with signed strides): uplo 'U'
// is the lower case under i -> n - 1 - i, that is negated strides with the base
// at the last element.  A column-major A is passed by the caller as the
// transposed row-major operand with uplo flipped, so |cs| = 1 always and every
// staging load below runs along memory.
//
// The algorithm is block forward substitution on L X = I over NB = 64 wide
// diagonal blocks k = 0, 1, ..., overwriting L.  With A11 the diagonal block,
// A10 the 64 x 64 k block to its left, A21 the panel below it and A20 the block
// below-left (A10 and A20 hold partial sums from the earlier steps), a step is
// three launches of 256-thread workgroups:
//
//   1. k_trtri_row     A10 <- A11^-1 A10 by substitution with true divisions
//                      (no inverse of a block is multiplied in): the four waves
//                      stage A11 in LDS in one pass of loads, then one lane per
//                      column keeps its 64 unknowns in registers (broadcast reads
//                      of A11), one workgroup per 64 columns: the family's
//                      substitution (sl_tri_f64.hpp).
//   2. k_trtri_update  A20 -= A21 A10 with the new A10 and the still original
//                      A21: the family's 128 x 128 tile, K = 64 in two slices,
//                      two workgroups per CU.  Workgroup 0 of
//                      this launch takes no tile: it computes X11 = A11^-1 I
//                      with the same substitution (the identity is generated,
//                      not loaded; only the triangle of X11 is stored; with diag
//                      'U' nothing on the diagonal is read or stored).  Its
//                      unknowns are spread over the lanes (16 registers each,
//                      see ident_solve): the 64 per lane of launch 1 spilled 516
//                      bytes next to the tiles' accumulators.
//   3. k_trtri_panel   A21 <- -A21 X11: a workgroup stages its own 64 rows of
//                      A21 and X11 in LDS, lane = row, wave = 16 columns of the
//                      product, the row in registers, X11 by broadcast reads;
//                      the product goes back through LDS so that loads and
//                      stores run along memory.
//
// Hazards.  X11 overwrites A11, which every workgroup of launch 1 reads, so it
// cannot be stored by launch 1; launch 3 needs it.  Launch 2 touches A21, A10
// (reads) and A20 (writes) and never A11, so its extra workgroup is the one
// place where X11 can be made without a fourth launch.  Launch 3 overwrites
// A21, which the tiles of launch 2 read: it is a launch of its own.  Launch 1
// of the next step reads rows that launches 2 and 3 wrote: stream order.
// The first step has no A10 / A20 (launch 1 is skipped, launch 2 is workgroup
// 0 alone), the last has no A21 / A20 (launch 2 is workgroup 0 alone, launch 3
// is skipped): 3 ceil(n / 64) - 2 launches for n > 64, one for n <= 64.
//
// This is scalar forward substitution on every column of L X = I in another
// summation order, so Higham's Theorem 8.5 bounds the residual componentwise:
// |I - L X| <= (n + 1) u |L| |X| to first order.  No workgroup waits on another,
// there are no atomics and every element is written by exactly one lane per
// launch: bit-identical from run to run.
//
// Compile log (gfx950, -O3, kernel resource usage): no kernel spills, scratch
// is 0 bytes per lane in all 6 instantiations.  k_trtri_row 256 VGPRs + 6-8
// AGPRs (one workgroup per CU), k_trtri_update 249 (two per CU), k_trtri_panel
// 244-246.
//
// Measured (one MI355X, uplo U, diag N, R = the transposed Cholesky factor of
// B B^T + n I, median of 5, ms; profiles/r7/trtri_tri_ab.jsonl,
// benchmarks/bench_trtri.py): native / the 1024-column-block workaround of
// algorithms/regression.py::_tri_inv_upper / one solve_triangular(R, I):
//   n = 4096    4.46 /  5.92 / 3.06     (190 launches)
//   n = 5000    6.18 /  5.52 / failed   (235 launches; the library's trsm
//                                        workspace does not allocate)
//   n = 16384  92.6  / 278.9 / 164.3    (766 launches)
// Per launch at n = 4096 (kernel trace, mean): row 20.9 us, update 33.8 us
// (14.5 us when workgroup 0 runs alone), panel 13.9 us: up to n = 5000 the call
// is bound by the serial chain through the diagonal blocks and by the latency
// of an update tile (its staging loads, four in flight per thread), not by the
// matrix cores; at n = 16384 it reaches 15.8 TFLOP/s of n^3 / 3.  What moved
// the time on the way (per launch, n = 4096): staging loops that waited on
// every load, 41 / 45 / 59 us for row / update / panel; all loads of a pass in
// flight, 24.5 / 41 / 28; panel on four waves, 13; X11 with its reads of A11
// unguarded (a guarded read is a branch with its own wait), 36 -> 14.5 alone.
// A right-looking launch 1 was slower (41.6 us).
// Not measured: the K = 128 pairing of two diagonal blocks per pass over A20,
// folding launch 3 into a neighbour, uplo L, diag U and column-major timings,
// n between 5000 and 16384, more staging loads in flight in the update tile.
#include "sl_tri_f64.hpp"

namespace {

using namespace sl_tri;         // NB: diagonal block width, T: edge of an update tile
constexpr int CH = 16;          // global loads a lane keeps in flight while staging
constexpr int DP = NB + 2;      // LDS pitch of a diagonal block: rows i .. i + 3 fall in different banks, 16-B aligned rows
constexpr int AP = NB + 1;      // LDS pitch of a staged 64 x 64 piece of A21: lane = row reads are conflict-free
constexpr int PANEL_LDS = (NB * DP + 2 * NB * AP) * (int)sizeof(double);  // 98 KB: X11, the rows of A21, their product
static_assert(NB * NB == 256 * CH, "the 256-thread kernels stage a 64 x 64 block in one pass of CH loads per thread");
// Rows of pitch DP that workgroup 0 of the update may read in the tiles' LDS: the 64 of A11 and, into registers
// that nothing uses, on to row 3 + 4 (15 + 15) (see ident_step).
constexpr int IDENT_ROWS = 3 + 4 * 2 * (NB / 4 - 1) + 1;
static_assert(IDENT_ROWS * DP * (int)sizeof(double) <= TILE_LDS, "workgroup 0 of the update reads inside the tiles' LDS");

// the logical lower-triangular view L[i][c] = M[i * rs + c * cs], |cs| = 1
struct View {
  double* M;
  int64_t rs, cs, n;
};

// A11 (the w x w block at j0) into Ld[c][k], k <= c: its own triangle only, identity past row w.  The loads of a
// pass are all issued before the first is used: one round trip to memory per CH * NT elements, not one per element.
template <bool UNIT, int NT>
__device__ __forceinline__ void load_diag(const View& v, int64_t j0, int w, double* __restrict__ Ld, int tid) {
#pragma unroll 1
  for (int base = 0; base < NB * NB; base += NT * CH) {
    double t[CH];
#pragma unroll
    for (int u = 0; u < CH; ++u) {
      const int idx = base + tid + u * NT, k = idx & (NB - 1), c = idx / NB;     // k runs along memory
      t[u] = k == c ? 1.0 : 0.0;
      if (k <= c && c < w && (UNIT ? k < c : true)) t[u] = v.M[(j0 + c) * v.rs + (j0 + k) * v.cs];
    }
#pragma unroll
    for (int u = 0; u < CH; ++u) {
      const int idx = base + tid + u * NT, k = idx & (NB - 1), c = idx / NB;
      if (k <= c) Ld[c * DP + k] = t[u];
    }
  }
}

// Column r < j0 of rows [j0, j0 + w), a column of A10: x <- A11^-1 x in place, the 64 unknowns in registers.
// (The right-looking form, which takes L[i][c] x[c] off every x[i] below a finished x[c], was measured here too:
// 41.6 us per launch against 24.5 us, its column reads of Ld wait on each division.)
template <bool UNIT>
__device__ __forceinline__ void col_solve(const View& v, const double* Ld, int64_t j0, int w, int64_t r) {
  double* R = v.M + j0 * v.rs + r * v.cs;
  double x[NB];
  if (w == NB) {                      // block-uniform; the full block loads without a test per row
#pragma unroll
    for (int c = 0; c < NB; ++c) x[c] = R[c * v.rs];
  } else {
#pragma unroll
    for (int c = 0; c < NB; ++c) x[c] = c < w ? R[c * v.rs] : 0.0;
  }
  // sl_tri::fwd_subst<UNIT, DP> written out: the call was tried, same registers but another branch order, and
  // n = 16384 then missed its timing limit in one of two runs
#pragma unroll
  for (int c = 0; c < NB; ++c) {
    double acc = x[c];
    int off = c * DP;
    if (c) asm volatile("" : "+v"(off) : "v"(x[c - 1]));
    const double* row = Ld + off;
#pragma unroll
    for (int k = 0; k < c; ++k) acc = fma(-x[k], row[k], acc);
    x[c] = UNIT ? acc : acc / row[c];
  }
#pragma unroll
  for (int c = 0; c < NB; ++c)
    if (c < w) R[c * v.rs] = x[c];
}

// x of lane S of each quad (lanes 4 i .. 4 i + 3) in all four lanes of the quad: two DPP moves, no LDS.
template <int S>
__device__ __forceinline__ double quad_bcast(double x) {
  constexpr int ctrl = S | (S << 2) | (S << 4) | (S << 6);      // quad_perm: [S, S, S, S]
  const uint64_t u = (uint64_t)__double_as_longlong(x);
  const uint32_t lo = (uint32_t)__builtin_amdgcn_mov_dpp((int)(uint32_t)u, ctrl, 0xf, 0xf, true);
  const uint32_t hi = (uint32_t)__builtin_amdgcn_mov_dpp((int)(uint32_t)(u >> 32), ctrl, 0xf, 0xf, true);
  return __longlong_as_double((long long)((uint64_t)hi << 32 | lo));
}

// Step c = 4 g + S of ident_solve: b[u] is row rg + 4 (g + u) of column q.
template <bool UNIT, int S>
__device__ __forceinline__ void ident_step(const View& v, const double* Ld, double* R, int w, int q, int rg, int g,
                                           double (&b)[NB / 4]) {
  const int c = 4 * g + S;
  double x = b[0];                      // row c in the lanes with rg == S
  if (!UNIT) x /= Ld[c * DP + c];
  x = quad_bcast<S>(x);
  if (c < q) x = 0.0;                   // exact zeros above the diagonal of X11, whatever A11's diagonal holds
  if (rg == S && c < w && q < w && (c > q || (c == q && !UNIT))) R[c * v.rs] = x;
  // The reads of A11's column c are not guarded, so that they are all issued at once: a read under a test
  // becomes a branch with its own wait.  Rows past 63 (g + u >= 16) read on inside the workgroup's LDS (row 123 at
  // most, 65 KB of the 72 KB) into registers that no later step uses.
  const double* colc = Ld + (rg + 4 * g) * DP + c;
  const double own = fma(-x, colc[0], b[0]);
  b[0] = rg > S ? own : b[0];
#pragma unroll
  for (int u = 1; u < NB / 4; ++u) b[u] = fma(-x, colc[4 * u * DP], b[u]);
}

// X11 = A11^-1 I over A11 by the four waves of a workgroup: the same substitution on the columns of the identity,
// which is generated, not loaded, in its right-looking form and the same summation order.  Wave wv takes columns
// [16 wv, 16 wv + 16) and starts at row 16 wv (X11 is zero above the diagonal); lane 4 ql + rg holds column q = 16
// wv + ql of rows rg, rg + 4, ... in registers (at most 16 values: this runs inside the update kernel, whose tiles
// need the registers).  Step c: the lanes that own row c finish it (one true division) and hand it to the other
// three lanes of their quad, which hold the same column; every lane then takes L[i][c] x[c][q] off its rows i > c.
// No barrier, no LDS traffic but the reads of A11.  Only the triangle of X11 (without the diagonal if UNIT) is
// stored.
template <bool UNIT>
__device__ __forceinline__ void ident_solve(const View& v, const double* Ld, int64_t j0, int w, int tid) {
  const int lane = tid & 63, wv = tid >> 6, ql = lane >> 2, rg = lane & 3;
  const int q = 16 * wv + ql;
  double* R = v.M + j0 * v.rs + (j0 + q) * v.cs;
  double b[NB / 4];                     // b[u]: row rg + 4 (g + u) in group g, rotated down once per group
#pragma unroll
  for (int u = 0; u < NB / 4; ++u) b[u] = rg + 4 * (4 * wv + u) == q ? 1.0 : 0.0;
#pragma unroll 1
  for (int g = 4 * wv; g < NB / 4; ++g) {         // rows 4 g .. 4 g + 3, one per lane of a quad
    ident_step<UNIT, 0>(v, Ld, R, w, q, rg, g, b);
    ident_step<UNIT, 1>(v, Ld, R, w, q, rg, g, b);
    ident_step<UNIT, 2>(v, Ld, R, w, q, rg, g, b);
    ident_step<UNIT, 3>(v, Ld, R, w, q, rg, g, b);
#pragma unroll
    for (int u = 0; u + 1 < NB / 4; ++u) b[u] = b[u + 1];
  }
}

// ---------------------------------------------------------------- launch 1
// A10 <- A11^-1 A10: columns [0, j0) of rows [j0, j0 + w), one lane per column.
template <bool UNIT>
__global__ void __launch_bounds__(256)
k_trtri_row(const View v, const int64_t j0, const int w) {
  __shared__ double Ld[NB * DP];
  const int tid = threadIdx.x;
  load_diag<UNIT, 256>(v, j0, w, Ld, tid);          // four waves stage A11 in one pass, the first one solves
  __syncthreads();
  const int64_t r = (int64_t)blockIdx.x * 64 + tid;
  if (tid >= 64 || r >= j0) return;
  col_solve<UNIT>(v, Ld, j0, w, r);
}

// ---------------------------------------------------------------- launch 2
// Workgroup 0: X11 = A11^-1 I over A11 (w x w at j0).  Workgroup 1 + t: tile t of A20[i, r] -= A21[i, :] A10[:, r],
// rows i >= j0 + 64, columns r < j0, `ntc` tiles across; there are tiles only when w = 64.  The MFMA row index
// (lane >> 4, registers) is the row and the column index (lane & 15) the column, which runs along memory.
template <bool UNIT>
__global__ void __launch_bounds__(256, 2)
k_trtri_update(const View v, const int64_t j0, const int w, const unsigned ntc) {
  extern __shared__ __align__(16) unsigned char smem[];
  double* Ms = (double*)smem;
  double* Xs = Ms + T * LP;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  if (blockIdx.x == 0) {                  // block-uniform
    load_diag<UNIT, 256>(v, j0, w, Ms, tid);
    __syncthreads();
    ident_solve<UNIT>(v, Ms, j0, w, tid);
    return;
  }
  const unsigned tile = blockIdx.x - 1;
  const int64_t r0 = j0 + NB;
  const int64_t ri = r0 + (int64_t)(tile / ntc) * T, cb = (int64_t)(tile % ntc) * T;
  const Quadrant q(lane, wave);
  const int64_t gp0 = ri + q.wp * 64 + q.fq, gq0 = cb + q.wq * 64 + q.fr;
  // wave-uniform: a quadrant past the last row or the last column stores nothing
  const bool active = gp0 - q.fq < v.n && gq0 - q.fr < j0;
  const double* pa = q.operand(Ms, q.wp);
  const double* pb = q.operand(Xs, q.wq);
  f64x4 acc[4][4];
#pragma unroll
  for (int mi = 0; mi < 4; ++mi)
#pragma unroll
    for (int ni = 0; ni < 4; ++ni)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int64_t gp = gp0 + mi * 16 + 4 * r, gq = gq0 + ni * 16;
        double c = 0.0;
        if (active && gp < v.n && gq < j0) c = v.M[gp * v.rs + gq * v.cs];
        acc[mi][ni][r] = c;
      }
#pragma unroll 1
  for (int h = 0; h < NB / KH; ++h) {
    if (h) __syncthreads();               // the previous slice has been read
    // slice h of A21 (rows [ri, ri + T), columns [j0 + 32 h, + 32) of L) as P[row][k], and of A10 (rows [j0 + 32 h,
    // + 32) of L) for the columns [cb, cb + T) as P[column][k]; columns >= j0 are zero
    stage_slice<true, 4>(v.M, v.rs, v.cs, ri, j0 + h * KH, v.n, Ms, tid);
    stage_slice<false, 4>(v.M, v.cs, v.rs, cb, j0 + h * KH, j0, Xs, tid);
    __syncthreads();
    if (active) mma_slice<true>(pa, pb, acc);
  }
  if (!active) return;
#pragma unroll
  for (int mi = 0; mi < 4; ++mi)
#pragma unroll
    for (int ni = 0; ni < 4; ++ni)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int64_t gp = gp0 + mi * 16 + 4 * r, gq = gq0 + ni * 16;
        if (gp < v.n && gq < j0) v.M[gp * v.rs + gq * v.cs] = acc[mi][ni][r];
      }
}

// ---------------------------------------------------------------- launch 3
// Wave WV's share of a row's product: entries [16 WV, 16 WV + 16) of -a X11, which need a[c] for c >= 16 WV only.
// The row is read from As and the entries go to Os, so no wave overwrites what another still reads.
template <bool UNIT, int WV>
__device__ __forceinline__ void panel_part(const double* Xs, const double* As, double* Os, int lane) {
  constexpr int JB = 16 * WV;
  double a[NB - JB];
#pragma unroll
  for (int c = JB; c < NB; ++c) a[c - JB] = As[lane * AP + c];
#pragma unroll
  for (int j = JB; j < JB + 16; ++j) {
    // Column j's LDS offset is made to depend on the previous entry, as in fwd_subst.
    int off = j;
    if (j > JB) asm volatile("" : "+v"(off) : "v"(a[j - 1 - JB]));
    const double* col = Xs + off;
    double acc = UNIT ? a[j - JB] : a[j - JB] * col[j * DP];
#pragma unroll
    for (int c = j + 1; c < NB; ++c) acc = fma(a[c - JB], col[c * DP], acc);
    a[j - JB] = -acc;                   // entry j needs entries >= j only
  }
#pragma unroll
  for (int j = JB; j < JB + 16; ++j) Os[lane * AP + j] = a[j - JB];
}

// A21 <- -A21 X11 for the rows [rb, rb + 64) of workgroup b, rb = j0 + 64 (1 + b); the diagonal block is full here.
// The workgroup stages its own rows and X11 in LDS (one pass of loads along memory), lane = row, wave = 16 columns
// of the product.
template <bool UNIT>
__global__ void __launch_bounds__(256)
k_trtri_panel(const View v, const int64_t j0) {
  extern __shared__ __align__(16) unsigned char smem[];
  double* Xs = (double*)smem;             // Xs[c][j] = X11[c][j], j <= c
  double* As = Xs + NB * DP;              // As[i][c], the workgroup's own rows of A21
  double* Os = As + NB * AP;              // Os[i][j], their product
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int64_t rb = j0 + NB + (int64_t)blockIdx.x * NB;
  load_diag<UNIT, 256>(v, j0, NB, Xs, tid);         // X11 is stored as A11 was: its triangle, ones on a unit diagonal
  const int64_t col = (j0 + lane) * v.cs;
  {
    double t[CH];                         // rows wave, wave + 4, ...: one row of A21 per load, along memory
#pragma unroll
    for (int u = 0; u < CH; ++u) {
      t[u] = 0.0;                         // rows >= n are zero and are not stored
      if (rb + wave + 4 * u < v.n) t[u] = v.M[(rb + wave + 4 * u) * v.rs + col];
    }
#pragma unroll
    for (int u = 0; u < CH; ++u) As[(wave + 4 * u) * AP + lane] = t[u];
  }
  __syncthreads();
  switch (wave) {                         // wave-uniform
    case 0: panel_part<UNIT, 0>(Xs, As, Os, lane); break;
    case 1: panel_part<UNIT, 1>(Xs, As, Os, lane); break;
    case 2: panel_part<UNIT, 2>(Xs, As, Os, lane); break;
    default: panel_part<UNIT, 3>(Xs, As, Os, lane); break;
  }
  __syncthreads();
#pragma unroll
  for (int u = 0; u < CH; ++u)
    if (rb + wave + 4 * u < v.n) v.M[(rb + wave + 4 * u) * v.rs + col] = Os[(wave + 4 * u) * AP + lane];
}

template <bool UNIT>
int run(const View& v, hipStream_t st) {
  const int64_t n = v.n;
  SL_LDS_ATTR((k_trtri_update<UNIT>), TILE_LDS);
  SL_LDS_ATTR((k_trtri_panel<UNIT>), PANEL_LDS);
  for (int64_t j0 = 0; j0 < n; j0 += NB) {
    const int w = (int)(n - j0 < NB ? n - j0 : NB);
    if (j0 > 0) {
      k_trtri_row<UNIT><<<(unsigned)(j0 / NB), 256, 0, st>>>(v, j0, w);
      SL_LAUNCH_CHECK();
    }
    const int64_t rem = n - j0 - w;       // rem > 0 only below a full block
    const unsigned ntc = rem > 0 ? (unsigned)((j0 + T - 1) / T) : 0u, ntr = (unsigned)((rem + T - 1) / T);
    k_trtri_update<UNIT><<<1u + ntc * ntr, 256, TILE_LDS, st>>>(v, j0, w, ntc ? ntc : 1u);
    SL_LAUNCH_CHECK();
    if (rem <= 0) break;
    k_trtri_panel<UNIT><<<(unsigned)((rem + NB - 1) / NB), 256, PANEL_LDS, st>>>(v, j0);
    SL_LAUNCH_CHECK();
  }
  return SL_OK;
}

}  // namespace

// The sizes at which the code changes path: diagonal block width and edge of an update tile.
SL_API int sl_trtri_tri_block(int* nb, int* tile) {
  if (nb) *nb = NB;
  if (tile) *tile = T;
  return SL_OK;
}

// In-place inverse of the `uplo` ('L' / 'U') triangle of the row-major f64 n x n matrix A, row pitch `pitch` >= n
// (elements), 8-B aligned; diag 'N' / 'U'.  Ordinary launches on `stream`, no host synchronisation; n = 0 returns at
// once.
SL_API int sl_trtri_tri(void* A, int uplo, int diag, int64_t n, int64_t pitch, void* stream) {
  if (n < 0 || (uplo != 'L' && uplo != 'U') || (diag != 'N' && diag != 'U') || (n > 0 && (!A || pitch < n)) ||
      n > (int64_t)65535 * T || ((uintptr_t)A & 7)) {
    sl_set_last_error("trtri_tri: needs an 8-B aligned f64 A, 0 <= n <= 65535 * 128, pitch >= n, uplo 'L' / 'U', "
                      "diag 'N' / 'U'");
    return SL_ERR_INVALID;
  }
  if (n == 0) return SL_OK;
  int64_t rs = pitch, cs = 1;
  double* Ab = (double*)A;
  if (uplo == 'U') {      // the lower case under i -> n - 1 - i
    Ab += (n - 1) * (rs + cs);
    rs = -rs, cs = -cs;
  }
  const View v{Ab, rs, cs, n};
  hipStream_t st = (hipStream_t)stream;
  return diag == 'U' ? run<true>(v, st) : run<false>(v, st);
}
