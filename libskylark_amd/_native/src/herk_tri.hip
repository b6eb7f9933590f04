// One-triangle f64 rank-k update (Elemental's Herk / BLAS dsyrk): the `uplo` triangle of the row-major s x s matrix
// C becomes alpha op(A) op(A)^T + beta C, op(A) of order s x K.  The first link of the reference's Gram-to-weights
// chain, El::Herk(El::LOWER, ...) of ml/krr.hpp:371 / :639, ml/kernels.hpp:241 and base/distance.hpp:92, whose
// result goes to El::Cholesky (chol_tri.hip).
//
// Storage rules (the family's): the strict other triangle of C and its pitch padding are never read or written and
// may hold NaN; beta == 0 reads nothing of C, so the stored triangle may hold NaN on entry; alpha == 0 or K == 0
// reads nothing of A.  A's pitch padding and the elements past K are never read.  No operand is copied.
//
// One code path for every layout.  The operand is the view P[x][k] = A[x xs + k ks], x < s, k < K, with one of the
// two strides equal to 1: orient N of a row-major A has (xs, ks) = (lda, 1), orient T has (1, lda), and a
// column-major A is the row-major transpose with the orientation flipped.  The kernel is instantiated on which
// stride is 1 (ALONG_K: k runs along memory) so that consecutive threads stage consecutive doubles in both.  C is
// always row-major here; a column-major C is its transpose with uplo flipped (C is symmetric, the stored values are
// the same).  uplo 'U' is the transposed tile: tile [I][J], J <= I, of the lower-triangular view lies at block row
// BM = J and block column BN = I of memory, and the MFMA's row operand is block BM, so that the accumulator's
// column index (lane & 15, see sl_tri_f64.hpp) runs along memory in both triangles and a lane's address is one
// expression.  Only the side of the diagonal that is kept differs.
//
// Schedule.  A work item is (tile, K range).  The tiles are the nt (nt + 1) / 2 tiles [I][J], J <= I, of 128 x 128
// with nt = ceil(s / 128); the K ranges are S runs of whole 32-slices, range z holding slices [z n / S, (z + 1) n / S)
// of the n = ceil(K / 32), as even as whole slices allow.  A 256-thread workgroup owns an item: the family's tile
// (sl_tri_f64.hpp), each of four waves a 64 x 64 quadrant, K through LDS in slices of 32 at pitch 36, mma_slice<false>,
// 72 KB of LDS and two workgroups per CU, so that one stages while the other multiplies.  A diagonal tile stages one
// operand slice and uses it for both sides, and its quadrant in the other triangle, like any quadrant outside the
// matrix, issues no MFMA and stores nothing.  Staging masks both directions: positions with x >= s or k >= K are
// explicit zeros and are not loaded; a slice that lies wholly inside the operand (all but the last of a range and
// the last tile row) is staged without tests.
//
// Split K.  Without it a tall A^T A leaves the chip empty: s = 512 has 10 tiles for 256 CUs.  S is a pure function
// of (s, K, CUs) (plan() below): 1 once the tiles alone fill the 2 CUs slots of two workgroups per CU, else the
// largest S with tiles x S within twice that number, never more than the number of slices.
//   S == 1: one launch (k_herk, direct) whose epilogue applies alpha and beta and stores the triangle.
//   S > 1:  two ordinary launches.  k_herk (partial) writes each item's raw 128 x 128 accumulators to its slab of
//           the caller's workspace, slab (tile S + z), element ((mi 4 + ni) 4 + g) 256 + thread: every store of a
//           wave is 512 contiguous bytes.  k_herk_reduce, one workgroup per (tile, 16 x 16-block position), adds
//           the S partials of each element in the order z = 0, 1, ..., S - 1, applies alpha and beta and stores
//           the triangle.  It reads only the elements it stores, all of which lie in quadrants that wrote them.
// Why two launches and not one: the alternatives are atomics (f64 adds in arrival order: not reproducible), or a
// ticket with the last arriver reducing (a workgroup that depends on the arrival order of others, and a fence on
// every item).  The launch boundary is the only synchronisation here: no atomics, no workgroup waits on another, no
// spin, no ticket.  Every element of C and of the workspace is written by exactly one lane per launch, so results
// are bit-identical from run to run for a fixed (s, K, S).  They differ in the last bits between different S.
//
// Hazards.  Inside a workgroup the two barriers of a slice separate the staging stores from the MFMA's LDS reads and
// those from the next slice's stores.  k_herk reads A and, in the direct epilogue with beta != 0, exactly the
// elements of C that the same lane then writes; no other workgroup touches them.  The partial launch writes the
// workspace only and the reduce launch, after it in stream order, reads it.  A and C must not overlap (not checked).
//
// Rounding: a dot product of length K in some order of fused multiply-adds (four terms per MFMA, slices in order,
// then the splits in order), one rounding for the product by alpha, one fused multiply-add for beta C.
//
// Compile log (gfx950, -O3, -Rpass-analysis=kernel-resource-usage), no spills, scratch 0 bytes per lane everywhere:
//   k_herk<true>    (k along memory)  224 VGPRs, 0 AGPRs, 80 SGPRs, 72 KB of dynamic LDS, 2 waves per SIMD
//   k_herk<false>   (x along memory)  226 VGPRs, 0 AGPRs, 86 SGPRs, 72 KB of dynamic LDS, 2 waves per SIMD
//   k_herk_reduce                      24 VGPRs, 0 AGPRs, 46 SGPRs, no LDS,               8 waves per SIMD
// The 128 accumulator registers are counted among the VGPRs (the register file is unified on gfx950).
//
// Measured (one MI355X, 256 CUs, uplo L, alpha 1, beta 0, A uniform in (-1, 1), median of 5 after a warm-up, same
// process, alternating; profiles/r8/herk_f64_ab.jsonl, benchmarks/bench_herk64.py).  ms of base.Herk on this kernel /
// of the path base.Herk took before it (full torch product, then the triangle through a mask) / of the bare
// torch.mm; TFLOP/s count the triangle's s^2 K flops:
//   A^T A, K = 200000, s = 1024    5.14 / 10.81 / 10.78   0.48 x   40.8 TFLOP/s   (36 tiles x 28 splits, two launches)
//   A^T A, K = 65536,  s = 4096   35.56 / 30.94 / 28.42   1.15 x   30.9           (528 tiles, one launch)
//   A A^T, K = 4096,   s = 4096    2.17 /  2.08 /  1.89   1.04 x   31.7           (528 tiles)
//   A A^T, K = 512,    s = 8192    0.88 /  1.65 /  1.01   0.53 x   39.1           (2080 tiles)
// Extra device memory at the peak of a call: the workspace alone (126 MiB at s = 1024, none where S = 1) against
// 2.25 s x s buffers for the old path (18.25 at s = 1024, where the product's own workspace counts) and 1 for the
// product.  Error e / ((K + 4) u) on the leading 512 x 512 block against an f64 CPU product: 0.0017, 0.0011, 0.0083,
// 0.012, as the library product's or below.  With half the flops the kernel is at par with the library's full
// product where the triangle alone fills the chip and K is long (0.39 to 0.52 of the 79 TFLOP/s f64 matrix-core
// peak counting the triangle, a few percent more counting the diagonal tiles' other halves) and twice as fast where
// the product is short of work (the tall Gram) or bound by the write of C (K = 512).
// Not measured: uplo U and column-major timings; beta != 0; sizes that are no multiple of 128; splits other than the
// plan's, and a lower limit on the slices per split (s = 130, K = 8197 runs 257 splits of one slice each); loads of
// the next slice in flight during the MFMAs (the staging here waits for its loads, the second workgroup of the CU
// is what overlaps them); another staging map for the x-along-memory case, whose LDS stores have a 4-way bank
// conflict (see trtrmm_tri.hip); a kernel trace of the two launches; anything on fewer or more than 256 CUs.
#include "sl_tri_f64.hpp"

namespace {

using namespace sl_tri;

constexpr int64_t MAX_S = (int64_t)1 << 22;      // nt <= 2^15: the tile count fits a grid dimension
constexpr int64_t MAX_SPLITS = 65535;            // the K ranges are the grid's second dimension

struct Args {
  const double* A;
  int64_t xs, ks, s, K;
  double* C;
  int64_t ldc;
  int upper;                 // the upper triangle of the row-major C is the stored one
  double alpha, beta;
  int S;                     // K ranges
  double* W;                 // S > 1: the slabs
};

// tile t of the lower-triangular enumeration: t = I (I + 1) / 2 + J, J <= I
__device__ __forceinline__ void tile_of(int64_t t, int64_t& I, int64_t& J) {
  I = (int64_t)((sqrt(8.0 * (double)t + 1.0) - 1.0) * 0.5);
  while (I * (I + 1) / 2 > t) --I;
  while ((I + 1) * (I + 2) / 2 <= t) ++I;
  J = t - I * (I + 1) / 2;
}

// sl_tri::stage_slice with the K tail masked as well: P[x][k] = S[(x0 + x) xs + (k0 + k) ks], zero and not loaded
// where x0 + x >= xlim or k0 + k >= klim.  GUARD false: the caller knows that the whole slice lies inside.
template <bool ALONG_K, bool GUARD, int UNROLL>
__device__ __forceinline__ void stage_slice_k(const double* S, int64_t xs, int64_t ks, int64_t x0, int64_t k0,
                                              int64_t xlim, int64_t klim, double* __restrict__ P, int tid) {
#pragma unroll UNROLL
  for (int idx = tid; idx < T * KH; idx += 256) {
    const int x = ALONG_K ? idx / KH : idx & (T - 1), k = ALONG_K ? idx & (KH - 1) : idx / T;
    double v = 0.0;
    if (!GUARD || (x0 + x < xlim && k0 + k < klim)) v = S[(x0 + x) * xs + (k0 + k) * ks];
    P[x * LP + k] = v;
  }
}

// alpha acc + beta C for the element at (row, col) of C, if it is stored
__device__ __forceinline__ void put(const Args& a, int64_t row, int64_t col, double acc) {
  if (row < a.s && col < a.s && (a.upper ? col >= row : col <= row)) {
    double* c = a.C + row * a.ldc + col;
    double v = a.alpha * acc;
    if (a.beta != 0.0) v = fma(a.beta, *c, v);
    *c = v;
  }
}

template <bool ALONG_K>
__global__ void __launch_bounds__(256, 2)
k_herk(const Args a) {
  extern __shared__ __align__(16) unsigned char smem[];
  int64_t I, J;
  tile_of((int64_t)blockIdx.x, I, J);
  const int64_t BM = a.upper ? J : I, BN = a.upper ? I : J;     // memory row / column block of the tile
  const bool two = I != J;                                      // block-uniform
  double* Pa = (double*)smem;
  double* Pb = two ? Pa + T * LP : Pa;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const Quadrant q(lane, wave);
  // wave-uniform: a quadrant outside the matrix or in the other triangle of a diagonal tile takes no part
  const bool active = BM * T + q.wp * 64 < a.s && BN * T + q.wq * 64 < a.s &&
                      (two || (a.upper ? q.wq >= q.wp : q.wq <= q.wp));
  const double* pa = q.operand(Pa, q.wp);
  const double* pb = q.operand(Pb, q.wq);
  f64x4 acc[4][4];
#pragma unroll
  for (int mi = 0; mi < 4; ++mi)
#pragma unroll
    for (int ni = 0; ni < 4; ++ni) acc[mi][ni] = f64x4{0.0, 0.0, 0.0, 0.0};
  const int64_t nsl = (a.K + KH - 1) / KH, z = blockIdx.y;
  const int64_t sl0 = z * nsl / a.S, sl1 = (z + 1) * nsl / a.S;
  const bool rows_in = (BM + 1) * T <= a.s && (BN + 1) * T <= a.s;   // block-uniform
#pragma unroll 1
  for (int64_t sl = sl0; sl < sl1; ++sl) {
    if (sl != sl0) __syncthreads();       // the previous slice has been read
    const int64_t k0 = sl * KH;
    if (rows_in && k0 + KH <= a.K) {
      stage_slice_k<ALONG_K, false, 8>(a.A, a.xs, a.ks, BM * T, k0, a.s, a.K, Pa, tid);
      if (two) stage_slice_k<ALONG_K, false, 8>(a.A, a.xs, a.ks, BN * T, k0, a.s, a.K, Pb, tid);
    } else {
      stage_slice_k<ALONG_K, true, 8>(a.A, a.xs, a.ks, BM * T, k0, a.s, a.K, Pa, tid);
      if (two) stage_slice_k<ALONG_K, true, 8>(a.A, a.xs, a.ks, BN * T, k0, a.s, a.K, Pb, tid);
    }
    __syncthreads();
    if (active) mma_slice<false>(pa, pb, acc);
  }
  if (!active) return;
  if (a.S > 1) {
    double* w = a.W + ((int64_t)blockIdx.x * a.S + z) * (T * T) + tid;
#pragma unroll
    for (int mi = 0; mi < 4; ++mi)
#pragma unroll
      for (int ni = 0; ni < 4; ++ni)
#pragma unroll
        for (int g = 0; g < 4; ++g) w[((mi * 4 + ni) * 4 + g) * 256] = acc[mi][ni][g];
    return;
  }
  const int64_t r0 = BM * T + q.wp * 64 + q.fq, c0 = BN * T + q.wq * 64 + q.fr;
#pragma unroll
  for (int mi = 0; mi < 4; ++mi)
#pragma unroll
    for (int ni = 0; ni < 4; ++ni)
#pragma unroll
      for (int g = 0; g < 4; ++g) put(a, r0 + mi * 16 + 4 * g, c0 + ni * 16, acc[mi][ni][g]);
}

// blockIdx.x: tile; blockIdx.y: the block position mi 4 + ni inside every quadrant.  A thread has the four elements
// (registers g) that it has in k_herk.
__global__ void __launch_bounds__(256)
k_herk_reduce(const Args a) {
  int64_t I, J;
  tile_of((int64_t)blockIdx.x, I, J);
  const int64_t BM = a.upper ? J : I, BN = a.upper ? I : J;
  const int tid = threadIdx.x, mi = blockIdx.y >> 2, ni = blockIdx.y & 3;
  const Quadrant q(tid & 63, tid >> 6);
  const int64_t row0 = BM * T + q.wp * 64 + mi * 16 + q.fq, col = BN * T + q.wq * 64 + ni * 16 + q.fr;
  const double* w = a.W + (int64_t)blockIdx.x * a.S * (T * T) + (int)blockIdx.y * 4 * 256 + tid;
  bool keep[4];
  double sum[4];
#pragma unroll
  for (int g = 0; g < 4; ++g) {
    const int64_t row = row0 + 4 * g;
    keep[g] = row < a.s && col < a.s && (a.upper ? col >= row : col <= row);
    sum[g] = keep[g] ? w[g * 256] : 0.0;
  }
#pragma unroll 4
  for (int z = 1; z < a.S; ++z) {
    const double* wz = w + (int64_t)z * (T * T);
#pragma unroll
    for (int g = 0; g < 4; ++g)
      if (keep[g]) sum[g] += wz[g * 256];
  }
#pragma unroll
  for (int g = 0; g < 4; ++g) put(a, row0 + 4 * g, col, sum[g]);
}

// the static partition: tiles, and the number S of K ranges
void plan(int64_t s, int64_t K, int64_t cus, int64_t& tiles, int64_t& S) {
  const int64_t nt = (s + T - 1) / T, nsl = (K + KH - 1) / KH, slots = 2 * cus;
  tiles = nt * (nt + 1) / 2;
  S = 1;
  if (tiles > 0 && tiles < slots) S = 2 * slots / tiles;
  if (S > nsl) S = nsl;
  if (S < 1) S = 1;
}

int device_cus(int64_t& cus) {
  int dev = 0, n = 0;
  SL_HIP_CHECK(hipGetDevice(&dev));
  SL_HIP_CHECK(hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev));
  cus = n;
  return SL_OK;
}

template <bool ALONG_K>
int run(const Args& a, int64_t tiles, hipStream_t st) {
  SL_LDS_ATTR((k_herk<ALONG_K>), TILE_LDS);
  k_herk<ALONG_K><<<dim3((unsigned)tiles, (unsigned)a.S), 256, TILE_LDS, st>>>(a);
  SL_LAUNCH_CHECK();
  if (a.S > 1) {
    k_herk_reduce<<<dim3((unsigned)tiles, 16u), 256, 0, st>>>(a);
    SL_LAUNCH_CHECK();
  }
  return SL_OK;
}

}  // namespace

// The sizes at which the code changes path: the edge of a tile and the K slice.
SL_API int sl_herk_tri_block(int* tile, int* kslice) {
  if (tile) *tile = T;
  if (kslice) *kslice = KH;
  return SL_OK;
}

// out[0] = tiles, out[1] = S of the static partition of (s, K) on `cus` compute units (cus <= 0: the current
// device's).
SL_API int sl_herk_tri_plan(int64_t s, int64_t K, int64_t cus, int64_t* out) {
  if (s < 0 || K < 0 || s > MAX_S || !out) {
    sl_set_last_error("herk_tri_plan: needs 0 <= s <= 2^22, K >= 0, out[2]");
    return SL_ERR_INVALID;
  }
  if (cus <= 0) {
    const int rc = device_cus(cus);
    if (rc != SL_OK) return rc;
  }
  plan(s, K, cus, out[0], out[1]);
  return SL_OK;
}

// The `uplo` ('L' / 'U') triangle of the row-major f64 s x s matrix C, row pitch ldc >= s (elements), becomes
// alpha P P^T + beta C with P[x][k] = A[x xs + k ks], x < s, k < K, one of xs, ks equal to 1 (or the extent along
// it at most 1).  splits: 0 takes the plan's S for the current device, a positive value forces S and is clamped to
// the number of 32-slices of K.  S > 1 needs `workspace`, ws_elems >= S x tiles x 128 x 128 doubles; with S == 1 it
// is not looked at.  Ordinary launches on `stream`, no host synchronisation; s = 0 returns at once.
SL_API int sl_herk_tri(const void* A, int64_t xs, int64_t ks, int64_t s, int64_t K, void* C, int64_t ldc, int uplo,
                       double alpha, double beta, int64_t splits, void* workspace, int64_t ws_elems, void* stream) {
  if (s < 0 || K < 0 || s > MAX_S || splits < 0 || (uplo != 'L' && uplo != 'U') || (s > 0 && (!C || ldc < s)) ||
      ((uintptr_t)C & 7) || ((uintptr_t)A & 7) || ((uintptr_t)workspace & 7)) {
    sl_set_last_error("herk_tri: needs 8-B aligned f64 A and C, 0 <= s <= ldc, s <= 2^22, K >= 0, splits >= 0, "
                      "uplo 'L' / 'U'");
    return SL_ERR_INVALID;
  }
  if (s == 0) return SL_OK;
  if (alpha == 0.0) K = 0;                     // A is not read
  if (K > 0 && (!A || !(ks == 1 || K == 1 || xs == 1 || s == 1))) {
    sl_set_last_error("herk_tri: A needs unit stride along x or along k");
    return SL_ERR_INVALID;
  }
  int64_t cus = 1, tiles = 0, S = 1;
  if (splits == 0) {
    const int rc = device_cus(cus);
    if (rc != SL_OK) return rc;
  }
  plan(s, K, cus, tiles, S);
  if (splits > 0) {
    const int64_t nsl = (K + KH - 1) / KH;
    S = splits < nsl ? splits : nsl;
    if (S < 1) S = 1;
  }
  if (S > MAX_SPLITS) S = MAX_SPLITS;
  if (S > 1 && (!workspace || ws_elems < S * tiles * (int64_t)(T * T))) {
    sl_set_last_error("herk_tri: the workspace is smaller than splits x tiles x 128 x 128 doubles");
    return SL_ERR_INVALID;
  }
  const Args a{(const double*)A, xs, ks, s, K, (double*)C, ldc, uplo == 'U', alpha, beta, (int)S, (double*)workspace};
  hipStream_t st = (hipStream_t)stream;
  // either instantiation is right for any strides; the choice only decides which loads are consecutive
  return ks == 1 ? run<true>(a, tiles, st) : run<false>(a, tiles, st);
}
