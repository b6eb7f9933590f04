// The shared parts of the f64 one-triangle kernel family (chol_tri.hip, trsm_tri.hip, trtri_tri.hip,
// trtrmm_tri.hip): the 128 x 128 tile on v_mfma_f64_16x16x4_f64 and the 64-unknown forward substitution.  Each file
// keeps its own schedule, hazards, compile log and measurements; what they have in common is described here, once.
//
// The tile.  A workgroup of 256 threads owns a T x T (128 x 128) tile of the output.  Each of its four waves owns a
// 64 x 64 quadrant (Quadrant below): 4 x 4 MFMA blocks of 16 x 16, 16 accumulators of four doubles, 128 registers.
// K passes through LDS in slices of KH = 32: two operand slices of 128 x 32 doubles, one per side of the product,
// TILE_LDS = 72 KB in all, so two workgroups fit a CU's 160 KB and one stages while the other multiplies.
//
// Operand layout.  A slice is stored as P[x][k] at pitch LP, x the operand's position along the tile edge and k the
// summation index: both operands have K as their fast index, the product is sum over k of Pa[p][k] Pb[q][k].  The
// MFMA takes from lane l the elements a[p = l & 15][k = l >> 4] and b[q = l & 15][k = l >> 4], so a lane reads
// P[(16 m + (l & 15)) * LP + (l >> 4) + 4 kk] for block m and K step kk: Quadrant::operand gives the address for
// m = kk = 0.
//
// Accumulator layout.  Register g of lane l of block (mi, ni) is the element at row 16 mi + (l >> 4) + 4 g of the a
// operand's direction and column 16 ni + (l & 15) of the b operand's: col = lane & 15, row = (lane >> 4) + 4 reg.
// Consecutive lanes hold consecutive columns, so a kernel puts the direction that runs along memory on the b
// operand.  The loops that load and store the accumulators stay in the kernels: behind a functor they cost 4 VGPRs
// in k_trsm_wupdate and 2.8 % more instructions.
//
// Why the pitch is 36.  With a pitch of 32 doubles the 16 rows that a wave reads at once start in the same bank.
// At 36 doubles (144 B) row x starts 4 x doubles = 8 x banks further on, and the four k of a read (lanes l >> 4)
// fill the 8 banks in between: the 64 lanes of an operand read fall on all 64 banks twice, which is the minimum for
// 64 doubles, and rows stay 16-B aligned.
//
// The substitution.  fwd_subst solves L x = b for 64 unknowns that one lane keeps in registers against a
// lower-triangular block in LDS, which all lanes read at the same address (broadcast reads, no conflicts).  It is
// the dot-product form, x[c] = (b[c] - sum over k < c of L[c][k] x[k]) / L[c][c] with a true division: no inverse of
// a block is formed anywhere in the family.  Fully unrolled it has 2080 LDS reads none of which depends on a
// computed value, and the compiler hoists them all to the top and spills them (15 KB of scratch per lane).  So the
// LDS offset of row c is passed through an empty asm statement that also names x[c - 1]: the reads of a row cannot
// be issued before the previous unknown exists, and registers stay within one row's worth.
#pragma once
#include "sl_common.hpp"

namespace sl_tri {

constexpr int NB = 64;          // width of a diagonal block / panel
constexpr int T = 128;          // edge of a tile
constexpr int KH = NB / 2;      // K positions staged in LDS at a time
constexpr int LP = KH + 4;      // LDS pitch of a staged slice (doubles): conflict-free MFMA operand reads
constexpr int TILE_LDS = 2 * T * LP * (int)sizeof(double);   // 72 KB: two operand slices

typedef __attribute__((ext_vector_type(4))) double f64x4;

// v of lane `lane` (wave-uniform) in every lane
__device__ __forceinline__ double bcast(double v, int lane) {
  const uint64_t u = (uint64_t)__double_as_longlong(v);
  const uint32_t lo = __builtin_amdgcn_readlane((uint32_t)u, lane);
  const uint32_t hi = __builtin_amdgcn_readlane((uint32_t)(u >> 32), lane);
  return __longlong_as_double((long long)((uint64_t)hi << 32 | lo));
}

// A thread's place in the tile: wave (wp, wq) owns the quadrant at rows 64 wp, columns 64 wq; inside a 16 x 16 block
// the lane holds column fr and rows fq, fq + 4, fq + 8, fq + 12.
struct Quadrant {
  int wp, wq, fr, fq;
  __device__ __forceinline__ Quadrant(int lane, int wave) : wp(wave >> 1), wq(wave & 1), fr(lane & 15), fq(lane >> 4) {}
  // this lane's first element of the staged slice P for the quadrant at position w (wp or wq) of the tile edge
  __device__ __forceinline__ const double* operand(const double* P, int w) const { return P + (w * 64 + fr) * LP + fq; }
};

// acc += (NEG ? -Pa : Pa) Pb^T over one staged slice: 4 x 4 blocks by KH / 4 MFMAs.
template <bool NEG>
__device__ __forceinline__ void mma_slice(const double* __restrict__ pa, const double* __restrict__ pb,
                                          f64x4 (&acc)[4][4]) {
#pragma unroll 4
  for (int kk = 0; kk < KH / 4; ++kk) {
    double a[4], b[4];
#pragma unroll
    for (int m = 0; m < 4; ++m) {
      a[m] = NEG ? -pa[m * 16 * LP + 4 * kk] : pa[m * 16 * LP + 4 * kk];
      b[m] = pb[m * 16 * LP + 4 * kk];
    }
#pragma unroll
    for (int mi = 0; mi < 4; ++mi)
#pragma unroll
      for (int ni = 0; ni < 4; ++ni)
        acc[mi][ni] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[mi], b[ni], acc[mi][ni], 0, 0, 0);
  }
}

// P[x][k] = S[(x0 + x) xs + (k0 + k) ks] for x < T, k < KH by the 256 threads of a workgroup; positions with x0 + x >=
// xlim are zero and are not loaded.  ALONG_K: k is the direction that runs along memory (ks = +-1), else x is;
// consecutive threads then load consecutive doubles.  UNROLL loads are in flight per thread.
template <bool ALONG_K, int UNROLL>
__device__ __forceinline__ void stage_slice(const double* S, int64_t xs, int64_t ks, int64_t x0,
                                            int64_t k0, int64_t xlim, double* __restrict__ P, int tid) {
#pragma unroll UNROLL
  for (int idx = tid; idx < T * KH; idx += 256) {
    const int x = ALONG_K ? idx / KH : idx & (T - 1), k = ALONG_K ? idx & (KH - 1) : idx / T;
    double v = 0.0;
    if (x0 + x < xlim) v = S[(x0 + x) * xs + (k0 + k) * ks];
    P[x * LP + k] = v;
  }
}

// x <- L^-1 x for the NB unknowns of one lane, L[c][k] = Ld[c * PITCH + k] (k <= c) in LDS; UNIT takes ones on the
// diagonal and does not read it.  See the top of the file for the asm statement.
template <bool UNIT, int PITCH>
__device__ __forceinline__ void fwd_subst(const double* Ld, double (&x)[NB]) {
#pragma unroll
  for (int c = 0; c < NB; ++c) {
    double acc = x[c];
    int off = c * PITCH;
    if (c) asm volatile("" : "+v"(off) : "v"(x[c - 1]));
    const double* row = Ld + off;
#pragma unroll
    for (int k = 0; k < c; ++k) acc = fma(-x[k], row[k], acc);
    x[c] = UNIT ? acc : acc / row[c];
  }
}

}  // namespace sl_tri
