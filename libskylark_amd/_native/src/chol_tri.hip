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
//                     read and written once per 128 columns.  The two 128 x K
//                     panel blocks pass through LDS in slices of 32 columns
//                     (72 KB, two workgroups per CU: one loads while the
//                     other multiplies); a 64 x 64 quadrant per wave (16
//                     accumulator tiles), C loaded into the accumulators and
//                     the negated P_i as the A operand.  f64 C/D layout:
//                     col = lane & 15, row = (lane >> 4) + 4 reg.  Diagonal
//                     tiles load and store only their own triangle (a select
//                     on row >= col).
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
#include "sl_common.hpp"
#include <math.h>

namespace {

constexpr int NB = 64;          // panel width
constexpr int T = 128;          // edge of a trailing-update tile
constexpr int KH = NB / 2;      // panel columns staged in LDS at a time
constexpr int LP = KH + 4;      // LDS pitch of a staged block (doubles): conflict-free MFMA operand reads
constexpr int UPD_LDS = 2 * T * LP * (int)sizeof(double);   // 72 KB: two workgroups per CU

typedef __attribute__((ext_vector_type(4))) double f64x4;

// v of lane `lane` (wave-uniform) in every lane
__device__ __forceinline__ double bcast(double v, int lane) {
  const uint64_t u = (uint64_t)__double_as_longlong(v);
  const uint32_t lo = __builtin_amdgcn_readlane((uint32_t)u, lane);
  const uint32_t hi = __builtin_amdgcn_readlane((uint32_t)(u >> 32), lane);
  return __longlong_as_double((long long)((uint64_t)hi << 32 | lo));
}

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

// Half `h` (columns [j0 + 32 h, j0 + 32 h + 32) of M) of the panel rows
// [rb, rb + T) into P[r][k]; rows >= n are zero.  'L' runs along k in memory,
// 'U' along the rows.
template <bool LOWER>
__device__ __forceinline__ void stage_half(const double* __restrict__ A, int64_t lda, int64_t n, int64_t rb,
                                           int64_t j0, int h, double* __restrict__ P, int tid) {
  const int64_t rs = LOWER ? lda : 1, cs = LOWER ? 1 : lda;
#pragma unroll 8
  for (int idx = tid; idx < T * KH; idx += 256) {
    const int r = LOWER ? idx / KH : idx & (T - 1), k = LOWER ? idx & (KH - 1) : idx / T;
    double v = 0.0;
    if (rb + r < n) v = A[(rb + r) * rs + (j0 + h * KH + k) * cs];
    P[r * LP + k] = v;
  }
}

__device__ __forceinline__ void mma_half(const double* __restrict__ pa, const double* __restrict__ pb,
                                         f64x4 (&acc)[4][4]) {
#pragma unroll 4
  for (int kk = 0; kk < KH / 4; ++kk) {
    double a[4], b[4];
#pragma unroll
    for (int m = 0; m < 4; ++m) {
      a[m] = -pa[m * 16 * LP + 4 * kk];
      b[m] = pb[m * 16 * LP + 4 * kk];
    }
#pragma unroll
    for (int mi = 0; mi < 4; ++mi)
#pragma unroll
      for (int ni = 0; ni < 4; ++ni)
        acc[mi][ni] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[mi], b[ni], acc[mi][ni], 0, 0, 0);
  }
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
    stage_half<LOWER>(A, lda, n, ri, kc, h, Pi, tid);
    if (two) stage_half<LOWER>(A, lda, n, rl, kc, h, Pl, tid);
    __syncthreads();
    if (active) mma_half(pa, pb, acc);
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
  SL_LDS_ATTR((k_chol_update<LOWER>), UPD_LDS);
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
    k_chol_update<LOWER><<<dim3(ntc, ntr), 256, UPD_LDS, st>>>(A, lda, n, first ? j0 : j0 - NB, first ? 2 : 4, r0, cend);
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
