// Blocked, in-place f64 triangular solve: op(A) X = B (side 'L', B n x t) or
// X op(A) = B (side 'R', B t x n) overwrites B with X.  A is a row-major n x n
// matrix of which only the `uplo` triangle is stored, op = identity ('N') or
// transpose ('T'), diag 'U' takes a unit diagonal.  The reference's El::Trsm,
// and the two halves of its cholesky::SolveAfter (ml/krr.hpp:398, :650).
//
// Storage rules: the strict other triangle of A is never read, with diag 'U'
// neither is its diagonal, the pitch padding of A and B is never read or
// written, A is never written.  They may all hold NaN.  A zero on a non-unit
// diagonal gives inf / NaN as in BLAS; there is no status word, no workspace,
// no host synchronisation and no allocation.
//
// All 16 variants run one code path on a logical lower-triangular view
// M[i][c] = A[abase + i ars + c acs] and Bv[i][r] = B[bbase + i brs + r bcs]
// (chol_tri.hip's trick, with signed strides).  Orient 'T' swaps A's strides;
// side 'R' swaps them again and swaps B's, since X op(A) = B is op(A)^T X^T =
// B^T; a view that is then upper triangular is the lower case under i -> n - 1
// - i, that is negated strides with the bases at the last element.  No
// transposed or masked copy is made.  The kernels are templated only on which
// stride of A (AROW: along c) and of B (BROW: along r) is the unit one, so
// that staging loads run along memory, and on the unit diagonal.
//
// Right-looking sweep over NB = 64 wide diagonal blocks: X_j = M_jj^-1 B_j by
// substitution with true divisions (no inverse of a block is formed), then
// B[r0:, :] -= M[r0:, j] X_j.  Two regimes by the number of right-hand sides:
//
//   thin (t <= 8)  k_trsm_thin, ceil(n / 64) launches per solve.  Launch j
//                  applies block column j - 1 to all rows below it, 64 rows per
//                  workgroup (the 64 x 64 piece of A through LDS, pitch 65; lane
//                  = row, wave w owns right-hand sides w and w + 4, partial
//                  results in registers), and its workgroup 0, which owns the
//                  rows of block j, then solves them: lane = row, the finished
//                  x_c goes round with v_readlane, one division per column.  The
//                  diagonal block is fetched into registers before the update.
//                  The next launch finds x_j in B by stream order.
//   wide (t > 8)   2 ceil(n / 64) - 1 launches.  k_trsm_wdiag: one lane per
//                  right-hand side keeps its 64 unknowns in registers, M_jj in
//                  LDS (broadcast reads), one 64-lane workgroup per 64
//                  right-hand sides (the family's substitution,
//                  sl_tri_f64.hpp).  k_trsm_wupdate: the family's 128 x 128
//                  tile of (rows x right-hand sides), K = 64 in two slices,
//                  two workgroups per CU, C loaded into the accumulators.  The
//                  MFMA column index (lane & 15) is put on B's unit-stride
//                  dimension: (-M) X for side L, (-X^T) M^T for side R.
//
// No workgroup waits on another, there are no atomics and every element of B
// is written by exactly one lane per launch: bit-identical from run to run.
//
// Compile log (gfx950, -O3, kernel resource usage): no kernel spills, scratch
// is 0 bytes per lane in all 16 instantiations.  k_trsm_thin 54-58 VGPRs,
// k_trsm_wdiag 255-256, k_trsm_wupdate 242-250 (two workgroups per CU).
// k_trsm_wdiag kept 15 KB of scratch per lane until each row's LDS offset was
// tied to the previous unknown (see fwd_subst); k_trsm_wupdate spilled 12-28 bytes
// with its staging loops unrolled by 8 and does not with 4.
//
// Measured (one MI355X, side L, uplo L, median of 5, ms; native / rocBLAS
// through torch.linalg.solve_triangular, orient N then T;
// profiles/r7/trsm_tri_ab.jsonl):
//   n = 4096   t = 1     1.15 / 1.04    1.16 / 0.97      (thin, 64 launches)
//              t = 8     1.21 / 0.43    1.21 / 0.51
//              t = 256   4.33 / 1.71    4.39 / 3.46      (wide, 127 launches)
//              t = 4096  7.06 / 2.54    7.07 / 3.04
//   n = 16384  t = 1     5.28 / 14.2    5.33 / 13.5      (thin, 256 launches)
//              t = 8     5.53 / 3.46    5.59 / 3.40
//              t = 256   21.2 / 3.80    21.6 / 124       (wide, 511 launches)
//              t = 4096  71.4 / 101     73.1 / 138
// HPDSolve (chol_tri + two thin solves, t = 8) against torch.linalg.cholesky +
// cholesky_solve: 8.98 / 14.34 ms at n = 4096, 91.3 / 111.2 ms at n = 16384.
// A thin launch costs 18-21 us and a wide diagonal-plus-update pair 35-80 us:
// both regimes are bound by the serial chain through the diagonal blocks (one
// division per column on the chain in the thin solve, 2016 dependent
// multiply-adds per lane in the wide one), not by memory or the matrix cores.
// Not measured: the K = 128 pairing of two diagonal blocks per pass over B,
// side R and uplo U timings, a kernel trace that splits a launch into gap,
// update and solve, and t between 9 and 255.
#include "sl_tri_f64.hpp"

namespace {

using namespace sl_tri;         // NB: diagonal block width, T: edge of a wide-update tile
constexpr int THIN = 8;         // t <= THIN takes the thin regime
constexpr int TP = NB + 1;      // LDS pitch of a thin 64 x 64 piece: lane = row reads are conflict-free

// the logical views
struct View {
  const double* M;              // M[i][c] = M[i * ars + c * acs]
  double* B;                    // Bv[i][r] = B[i * brs + r * bcs]
  int64_t ars, acs, brs, bcs, n, t;
};

// ---------------------------------------------------------------- thin
// Rows [r0 + 64 b, + 64) for workgroup b: B -= M[rows, r0 - 64 : r0] X (r0 > 0),
// and workgroup 0 then solves its rows against the diagonal block at r0.
template <bool AROW, bool BROW, bool UNIT>
__global__ void __launch_bounds__(256)
k_trsm_thin(const View v, const int64_t r0) {
  __shared__ double Ms[NB * TP];
  __shared__ double Xs[NB * THIN];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int64_t rb = r0 + (int64_t)blockIdx.x * NB;
  const bool solve = blockIdx.x == 0;     // block-uniform
  const int t = (int)v.t;
  // the diagonal block, fetched early: its own triangle only, identity elsewhere
  double dreg[NB * NB / 256];
  if (solve) {
#pragma unroll
    for (int u = 0; u < NB * NB / 256; ++u) {
      const int idx = tid + 256 * u, f = idx & (NB - 1), s = idx / NB;     // f runs along memory
      const int i = AROW ? s : f, k = AROW ? f : s;
      double d = i == k ? 1.0 : 0.0;
      if (rb + i < v.n && (UNIT ? k < i : k <= i)) d = v.M[(rb + i) * v.ars + (rb + k) * v.acs];
      dreg[u] = d;
    }
  }
  const int64_t gi = rb + lane;
  double b0 = 0.0, b1 = 0.0;
  if (gi < v.n && wave < t) b0 = v.B[gi * v.brs + wave * v.bcs];
  if (gi < v.n && wave + 4 < t) b1 = v.B[gi * v.brs + (wave + 4) * v.bcs];
  if (r0 > 0) {
    const int64_t j0 = r0 - NB;
#pragma unroll
    for (int u = 0; u < NB * NB / 256; ++u) {
      const int idx = tid + 256 * u, f = idx & (NB - 1), s = idx / NB;
      const int i = AROW ? s : f, k = AROW ? f : s;
      double m = 0.0;
      if (rb + i < v.n) m = v.M[(rb + i) * v.ars + (j0 + k) * v.acs];
      Ms[i * TP + k] = m;
    }
#pragma unroll
    for (int u = 0; u < NB * THIN / 256; ++u) {
      const int idx = tid + 256 * u;
      const int c = BROW ? idx / THIN : idx & (NB - 1), r = BROW ? idx & (THIN - 1) : idx / NB;
      double x = 0.0;
      if (r < t) x = v.B[(j0 + c) * v.brs + r * v.bcs];
      Xs[c * THIN + r] = x;
    }
    __syncthreads();
#pragma unroll 16
    for (int c = 0; c < NB; ++c) {
      const double m = Ms[lane * TP + c];
      b0 = fma(-m, Xs[c * THIN + wave], b0);
      b1 = fma(-m, Xs[c * THIN + wave + 4], b1);
    }
  }
  if (solve) {
    if (r0 > 0) __syncthreads();          // the update has read Ms
#pragma unroll
    for (int u = 0; u < NB * NB / 256; ++u) {
      const int idx = tid + 256 * u, f = idx & (NB - 1), s = idx / NB;
      const int i = AROW ? s : f, k = AROW ? f : s;
      Ms[i * TP + k] = dreg[u];
    }
    __syncthreads();
    if (wave >= t) return;                // wave-uniform, after the last barrier
#pragma unroll
    for (int c = 0; c < NB; ++c) {
      double x0 = bcast(b0, c), x1 = bcast(b1, c);
      if (!UNIT) {
        const double d = Ms[c * TP + c];
        x0 /= d;
        x1 /= d;
      }
      const double m = Ms[lane * TP + c];
      if (lane > c) {
        b0 = fma(-m, x0, b0);
        b1 = fma(-m, x1, b1);
      } else if (lane == c) {
        b0 = x0;
        b1 = x1;
      }
    }
  }
  if (gi < v.n && wave < t) v.B[gi * v.brs + wave * v.bcs] = b0;
  if (gi < v.n && wave + 4 < t) v.B[gi * v.brs + (wave + 4) * v.bcs] = b1;
}

// ---------------------------------------------------------------- wide
// X_j = M_jj^-1 B_j for the w rows from j0, one lane per right-hand side.
template <bool AROW, bool UNIT>
__global__ void __launch_bounds__(64)
k_trsm_wdiag(const View v, const int64_t j0, const int w) {
  __shared__ double Ld[NB * NB];
  const int tid = threadIdx.x;
  for (int idx = tid; idx < NB * NB; idx += 64) {
    const int f = idx & (NB - 1), s = idx / NB;     // f runs along memory
    const int c = AROW ? s : f, k = AROW ? f : s;
    if (k > c) continue;
    double d = k == c ? 1.0 : 0.0;
    if (c < w && (UNIT ? k < c : true)) d = v.M[(j0 + c) * v.ars + (j0 + k) * v.acs];
    Ld[c * NB + k] = d;
  }
  __syncthreads();
  const int64_t r = (int64_t)blockIdx.x * 64 + tid;
  if (r >= v.t) return;
  double* R = v.B + j0 * v.brs + r * v.bcs;
  double x[NB];
#pragma unroll
  for (int c = 0; c < NB; ++c) x[c] = c < w ? R[c * v.brs] : 0.0;
  fwd_subst<UNIT, NB>(Ld, x);
#pragma unroll
  for (int c = 0; c < NB; ++c)
    if (c < w) R[c * v.brs] = x[c];
}

// Bv[i, r] -= M[i, j0 : j0 + 64] X_j[:, r] over rows i >= r0, a T x T tile of (rows x rhs) per workgroup.
// The MFMA row index p (lane >> 4, registers) and column index q (lane & 15) are
// (row, rhs) when B runs along r in memory and (rhs, row) when it runs along i.
template <bool AROW, bool BROW>
__global__ void __launch_bounds__(256, 2)
k_trsm_wupdate(const View v, const int64_t j0, const int64_t r0) {
  extern __shared__ __align__(16) unsigned char smem[];
  double* Ms = (double*)smem;
  double* Xs = Ms + T * LP;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int64_t ri = r0 + (int64_t)blockIdx.y * T, cb = (int64_t)blockIdx.x * T;
  const Quadrant q(lane, wave);
  const int64_t plim = BROW ? v.n : v.t, qlim = BROW ? v.t : v.n;
  const int64_t ps = BROW ? v.brs : v.bcs, qs = BROW ? v.bcs : v.brs;
  const int64_t gp0 = (BROW ? ri : cb) + q.wp * 64 + q.fq, gq0 = (BROW ? cb : ri) + q.wq * 64 + q.fr;
  // wave-uniform: a quadrant past the last row or the last right-hand side stores nothing
  const bool active = gp0 - q.fq < plim && gq0 - q.fr < qlim;
  const double* pa = q.operand(BROW ? Ms : Xs, q.wp);
  const double* pb = q.operand(BROW ? Xs : Ms, q.wq);
  f64x4 acc[4][4];
#pragma unroll
  for (int mi = 0; mi < 4; ++mi)
#pragma unroll
    for (int ni = 0; ni < 4; ++ni)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int64_t gp = gp0 + mi * 16 + 4 * r, gq = gq0 + ni * 16;
        double c = 0.0;
        if (active && gp < plim && gq < qlim) c = v.B[gp * ps + gq * qs];
        acc[mi][ni][r] = c;
      }
#pragma unroll 1
  for (int h = 0; h < NB / KH; ++h) {
    if (h) __syncthreads();               // the previous slice has been read
    // slice h of M[ri : ri + T, j0 : j0 + 64] and of X_j for the right-hand sides [cb, cb + T), as P[row or rhs][k];
    // 4 loads in flight: 8 spill
    stage_slice<AROW, 4>(v.M, v.ars, v.acs, ri, j0 + h * KH, v.n, Ms, tid);
    stage_slice<!BROW, 4>(v.B, v.bcs, v.brs, cb, j0 + h * KH, v.t, Xs, tid);
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
        if (gp < plim && gq < qlim) v.B[gp * ps + gq * qs] = acc[mi][ni][r];
      }
}

template <bool AROW, bool BROW, bool UNIT>
int run(const View& v, hipStream_t st) {
  const int64_t n = v.n, t = v.t;
  if (t <= THIN) {
    // launch j: update from block column j - 1, then workgroup 0 solves block j
    for (int64_t r0 = 0; r0 < n; r0 += NB) {
      k_trsm_thin<AROW, BROW, UNIT><<<(unsigned)((n - r0 + NB - 1) / NB), 256, 0, st>>>(v, r0);
      SL_LAUNCH_CHECK();
    }
    return SL_OK;
  }
  SL_LDS_ATTR((k_trsm_wupdate<AROW, BROW>), TILE_LDS);
  const unsigned ntc = (unsigned)((t + T - 1) / T);
  for (int64_t j0 = 0; j0 < n; j0 += NB) {
    const int w = (int)(n - j0 < NB ? n - j0 : NB);
    k_trsm_wdiag<AROW, UNIT><<<(unsigned)((t + 63) / 64), 64, 0, st>>>(v, j0, w);
    SL_LAUNCH_CHECK();
    const int64_t r0 = j0 + w, rem = n - r0;
    if (rem <= 0) break;
    k_trsm_wupdate<AROW, BROW><<<dim3(ntc, (unsigned)((rem + T - 1) / T)), 256, TILE_LDS, st>>>(v, j0, r0);
    SL_LAUNCH_CHECK();
  }
  return SL_OK;
}

template <bool AROW, bool BROW>
int run_diag(const View& v, bool unit, hipStream_t st) {
  return unit ? run<AROW, BROW, true>(v, st) : run<AROW, BROW, false>(v, st);
}

}  // namespace

// The sizes at which the code changes path: diagonal block width, edge of a
// wide-update tile, and the largest t that takes the thin regime.
SL_API int sl_trsm_tri_block(int* nb, int* tile, int* thin) {
  if (nb) *nb = NB;
  if (tile) *tile = T;
  if (thin) *thin = THIN;
  return SL_OK;
}

// In-place solve of op(A) X = B (side 'L', B n x t) or X op(A) = B (side 'R',
// B t x n).  A: row-major f64 n x n, row pitch lda >= n (elements), the `uplo`
// ('L' / 'U') triangle stored; orient 'N' / 'T'; diag 'N' / 'U'.  B: row-major
// f64, row pitch ldb >= its row length.  Both 8-B aligned and not overlapping.
// Ordinary launches on `stream`, no host synchronisation; n = 0 or t = 0
// returns at once.
SL_API int sl_trsm_tri(const void* A, int side, int uplo, int orient, int diag, int64_t n, int64_t t, int64_t lda,
                       void* B, int64_t ldb, void* stream) {
  const bool left = side == 'L';
  if (n < 0 || t < 0 || (side != 'L' && side != 'R') || (uplo != 'L' && uplo != 'U') ||
      (orient != 'N' && orient != 'T') || (diag != 'N' && diag != 'U') ||
      (n > 0 && t > 0 && (!A || !B || lda < n || ldb < (left ? t : n))) || n > (int64_t)65535 * T ||
      t > (int64_t)0x7fffffff * 64 || ((uintptr_t)A & 7) || ((uintptr_t)B & 7)) {
    sl_set_last_error("trsm_tri: needs 8-B aligned f64 A and B, 0 <= n <= 65535 * 128, 0 <= t <= (2^31 - 1) * 64, "
                      "lda >= n, ldb >= the row length of B, side 'L' / 'R', uplo 'L' / 'U', orient 'N' / 'T', "
                      "diag 'N' / 'U'");
    return SL_ERR_INVALID;
  }
  if (n == 0 || t == 0) return SL_OK;
  // E = op(A) (side L) or op(A)^T (side R), E[i][c] = A[i er + c ec], solves E Bv = Bv
  const bool flip = (orient == 'T') != !left;
  int64_t er = flip ? 1 : lda, ec = flip ? lda : 1;
  int64_t br = left ? ldb : 1, bc = left ? 1 : ldb;
  const bool lower = (uplo == 'L') != flip;
  const double* Ab = (const double*)A;
  double* Bb = (double*)B;
  if (!lower) {       // the lower case under i -> n - 1 - i
    Ab += (n - 1) * (er + ec);
    Bb += (n - 1) * br;
    er = -er, ec = -ec, br = -br;
  }
  const View v{Ab, Bb, er, ec, br, bc, n, t};
  const bool arow = !flip, brow = left;
  const bool unit = diag == 'U';
  hipStream_t st = (hipStream_t)stream;
  if (arow) return brow ? run_diag<true, true>(v, unit, st) : run_diag<true, false>(v, unit, st);
  return brow ? run_diag<false, true>(v, unit, st) : run_diag<false, false>(v, unit, st);
}
