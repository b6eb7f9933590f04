// Blocked, in-place f64 Cholesky of a row-major n x n matrix of which only the
// `uplo` triangle is stored: 'L' leaves L (A = L L^T) in the lower triangle,
// 'U' leaves U (A = U^T U) in the upper one.  The reference's
// El::Cholesky(El::LOWER, C) between its Herk and its SolveAfter
// (ml/krr.hpp:371-398, :639-650).  The strict other triangle and the pitch
// padding are never read and never written: they may hold NaN.
//
// Both triangles run the same code on a logical lower-triangular view
// M[i][c] = A[i rs + c cs]: 'L' has (rs, cs) = (lda, 1), 'U' has (1, lda), so
// 'U' is the transposed-operand form of the same three steps and there is no
// transposed copy.  A call is a sequence of ordinary launches on the caller's
// stream, right-looking, three per panel of width NB = 64 (3 ceil(n / 64) - 2
// in all):
//
//   1. k_chol_diag    one wave factors the w x w diagonal block.  Lane i keeps
//                     row i in registers; column c takes the finished row c
//                     from lane c with v_readlane (no LDS, no barrier).  Every
//                     pivot is tested (d > 0 and finite); the first failure
//                     writes its 1-based global index to the status word
//                     unless the word is already non-zero.  A failure changes
//                     no loop bound: the block, and everything after it, then
//                     carries NaN.
//   2. k_chol_panel   M[i, j] <- M[i, j] L_jj^-T for the rows below by forward
//                     substitution with true divisions, one row per lane in
//                     registers, the factored diagonal block in LDS (broadcast
//                     reads).  No inverse of L_jj is formed.
//   3. k_chol_update  M[i, l] -= P_i P_l^T over the T x T (T = 128) tiles
//                     i >= l of the trailing triangle on v_mfma_f64_16x16x4_f64.
//                     Panels go in pairs: the first updates only the 64
//                     columns of the second, the update after the second
//                     applies both with K = 128, so the trailing matrix is
//                     read and written once per 128 columns.  The tile, its
//                     operand and accumulator layout and the LDS pitch are
//                     the family's (sl_tri_f64.hpp): C loaded into the
//                     accumulators, the negated P_i as the A operand, two
//                     workgroups per CU.  Diagonal tiles load and store only
//                     their own triangle (a select on row >= col).
//
// No workgroup waits on another, there are no atomics and every element is
// written by exactly one lane per launch: results are bit-identical from run
// to run.  The only workspace is the caller's int32 status word.
//
// Measured (one MI355X, uplo L): n = 4096 6.6 ms, n = 16384 79 ms (18.5 TFLOP/s
// of n^3 / 3).  One update per panel (K = 64) took 93 ms at n = 16384: the
// update is bound by the read-modify-write of the trailing matrix.  A
// right-looking diagonal block and panel solve (finished column through LDS,
// independent multiply-adds) were slower than the dot-product forms here
// (7.0 against 5.9 ms at n = 4096).  Open items: wider panel groups, the
// serial diagonal and panel kernels (33 and 26 us each in a kernel trace) that
// dominate small n, and the 'U' form's tile stores (32-B runs per row).
#include "sl_tri_f64.hpp"
#include <math.h>

namespace {

using namespace sl_tri;         // NB: panel width, T: edge of a trailing-update tile

template <bool LOWER>
__global__ void __launch_bounds__(64)
k_chol_diag(double* __restrict__ A, int64_t lda, int64_t j0, int w, int* __restrict__ info) {
  const int i = threadIdx.x;
  const int64_t rs = LOWER ? lda : 1, cs = LOWER ? 1 : lda;
  double* D = A + j0 * lda + j0;
  double x[NB];
#pragma unroll
  for (int c = 0; c < NB; ++c) {
    x[c] = 0.0;
    if (i < w && c <= i) x[c] = D[i * rs + c * cs];
  }
  int fail = 0;
#pragma unroll
  for (int c = 0; c < NB; ++c) {
    double acc = x[c];
#pragma unroll
    for (int k = 0; k < c; ++k) acc = fma(-x[k], bcast(x[k], c), acc);
    const double d = bcast(acc, c);
    if (c < w && fail == 0 && !(d > 0.0 && d < INFINITY)) fail = c + 1;
    const double s = sqrt(d);
    x[c] = i == c ? s : acc / s;
  }
#pragma unroll
  for (int c = 0; c < NB; ++c)
    if (i < w && c <= i) D[i * rs + c * cs] = x[c];
  // one workgroup per launch, launches in stream order: the first failure wins
  if (fail != 0 && i == 0 && *info == 0) *info = (int)(j0 + fail);
}

template <bool LOWER>
__global__ void __launch_bounds__(256)
k_chol_panel(double* __restrict__ A, int64_t lda, int64_t n, int64_t j0) {
  __shared__ double Ld[NB * NB];
  const int tid = threadIdx.x;
  const int64_t rs = LOWER ? lda : 1, cs = LOWER ? 1 : lda;
  const double* D = A + j0 * lda + j0;
  for (int idx = tid; idx < NB * NB; idx += 256) {
    const int f = idx & (NB - 1), s = idx / NB;     // f runs along memory
    const int c = LOWER ? s : f, k = LOWER ? f : s;
    if (k <= c) Ld[c * NB + k] = D[c * rs + k * cs];
  }
  __syncthreads();
  const int64_t i = j0 + NB + (int64_t)blockIdx.x * 256 + tid;
  if (i >= n) return;
  double* R = A + i * rs + j0 * cs;
  double x[NB];
#pragma unroll
  for (int c = 0; c < NB; ++c) x[c] = R[c * cs];
  // not sl_tri::fwd_subst: its pinned row offset was tried here and costs registers (150 -> 162 and 266 -> 268 VGPRs)
#pragma unroll
  for (int c = 0; c < NB; ++c) {
    double acc = x[c];
#pragma unroll
    for (int k = 0; k < c; ++k) acc = fma(-x[k], Ld[c * NB + k], acc);
    x[c] = acc / Ld[c * NB + c];
  }
#pragma unroll
  for (int c = 0; c < NB; ++c) R[c * cs] = x[c];
}

template <bool LOWER>
__global__ void __launch_bounds__(256, 2)
k_chol_update(double* __restrict__ A, int64_t lda, int64_t n, int64_t kc, int halves, int64_t r0, int64_t cend) {
  // M[i, l] -= P_i P_l^T with P = columns [kc, kc + 32 halves) of M, over rows i >= r0
  // and columns r0 <= l < cend, l <= i
  const int I = blockIdx.y, J = blockIdx.x;
  if (J > I) return;
  extern __shared__ __align__(16) unsigned char smem[];
  double* Pi = (double*)smem;
  double* Pl = I == J ? Pi : Pi + T * LP;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int64_t rs = LOWER ? lda : 1, cs = LOWER ? 1 : lda;
  const int64_t ri = r0 + (int64_t)I * T, rl = r0 + (int64_t)J * T;
  const bool two = I != J;                // block-uniform
  // not sl_tri::Quadrant: tried, same registers but another prologue, and n = 16384 then missed its timing limit
  const int wr = wave >> 1, wc = wave & 1;
  // wave-uniform: a quadrant above the diagonal or right of cend stores nothing
  const bool active = (two || wc <= wr) && rl + wc * 64 < cend;
  const int fr = lane & 15, fq = lane >> 4;
  const int64_t gi0 = ri + wr * 64 + fq, gc0 = rl + wc * 64 + fr;
  const double* pa = Pi + (wr * 64 + fr) * LP + fq;
  const double* pb = Pl + (wc * 64 + fr) * LP + fq;
  f64x4 acc[4][4];
#pragma unroll
  for (int mi = 0; mi < 4; ++mi)
#pragma unroll
    for (int ni = 0; ni < 4; ++ni)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int64_t gi = gi0 + mi * 16 + 4 * r, gc = gc0 + ni * 16;
        double v = 0.0;
        if (active && gi < n && gc <= gi && gc < cend) v = A[gi * rs + gc * cs];
        acc[mi][ni][r] = v;
      }
#pragma unroll 1
  for (int h = 0; h < halves; ++h) {
    if (h) __syncthreads();               // the previous half has been read
    // half h of the panel rows [ri, ri + T) and [rl, rl + T): 'L' runs along k in memory, 'U' along the rows
    stage_slice<LOWER, 8>(A, rs, cs, ri, kc + h * KH, n, Pi, tid);
    if (two) stage_slice<LOWER, 8>(A, rs, cs, rl, kc + h * KH, n, Pl, tid);
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
        const int64_t gi = gi0 + mi * 16 + 4 * r, gc = gc0 + ni * 16;
        if (gi < n && gc <= gi && gc < cend) A[gi * rs + gc * cs] = acc[mi][ni][r];
      }
}

template <bool LOWER>
int run(double* A, int64_t n, int64_t lda, int* info, hipStream_t st) {
  SL_LDS_ATTR((k_chol_update<LOWER>), TILE_LDS);
  // Panels go in pairs, so the trailing matrix is read and written once per
  // 128 columns: the first panel of a pair updates only the second panel's 64
  // columns, and the update after the second applies both (K = 128).
  for (int64_t j0 = 0; j0 < n; j0 += NB) {
    const int w = (int)(n - j0 < NB ? n - j0 : NB);
    k_chol_diag<LOWER><<<1, 64, 0, st>>>(A, lda, j0, w, info);
    SL_LAUNCH_CHECK();
    const int64_t r0 = j0 + w, rem = n - r0;
    if (rem <= 0) break;
    k_chol_panel<LOWER><<<(unsigned)((rem + 255) / 256), 256, 0, st>>>(A, lda, n, j0);
    SL_LAUNCH_CHECK();
    const bool first = (j0 / NB) % 2 == 0;
    const int64_t cend = first ? (r0 + NB < n ? r0 + NB : n) : n;
    const unsigned ntr = (unsigned)((rem + T - 1) / T), ntc = (unsigned)((cend - r0 + T - 1) / T);
    k_chol_update<LOWER><<<dim3(ntc, ntr), 256, TILE_LDS, st>>>(A, lda, n, first ? j0 : j0 - NB, first ? 2 : 4, r0, cend);
    SL_LAUNCH_CHECK();
  }
  return SL_OK;
}

}  // namespace

// The panel width and the trailing tile edge: sizes at which the code changes path.
SL_API int sl_chol_tri_block(int* nb, int* tile) {
  if (nb) *nb = NB;
  if (tile) *tile = T;
  return SL_OK;
}

// In-place Cholesky of the `uplo` ('L' / 'U') triangle of the row-major f64
// n x n matrix A with row pitch lda >= n (elements), 8-B aligned.  info: one
// device int32, zeroed here on the stream and left 0 on success, else the
// 1-based index of the first pivot that is not positive and finite.  No host
// synchronisation; n = 0 returns at once.
SL_API int sl_chol_tri(void* A, int uplo, int64_t n, int64_t lda, void* info, void* stream) {
  if (n < 0 || (uplo != 'L' && uplo != 'U') || !info || (n > 0 && (!A || lda < n)) || n > (int64_t)65535 * T ||
      ((uintptr_t)A & 7) || ((uintptr_t)info & 3)) {
    sl_set_last_error("chol_tri: needs an 8-B aligned f64 A, 0 <= n <= 65535 * 128, lda >= n, uplo 'L' / 'U', "
                      "a device int32 status word");
    return SL_ERR_INVALID;
  }
  hipStream_t st = (hipStream_t)stream;
  SL_HIP_CHECK(hipMemsetAsync(info, 0, sizeof(int), st));
  if (n == 0) return SL_OK;
  return uplo == 'L' ? run<true>((double*)A, n, lda, (int*)info, st) : run<false>((double*)A, n, lda, (int*)info, st);
}
