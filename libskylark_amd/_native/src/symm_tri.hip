// Y <- alpha S X + beta Y for a symmetric S of which only the `uplo` triangle
// is stored, and a short block X (k <= 8 columns): the triangle-reading Symm
// (reference base/Symm.hpp, El::Symm: "only the uplo triangle is referenced")
// and the K x product of a CG iteration on a stored kernel Gram (reference
// ml/krr.hpp:452-541).  Every stored a_ij (i != j) is read once and used
// twice, y_i += a_ij x_j and y_j += a_ij x_i, so a product streams n^2 / 2
// elements instead of n^2.
//
// The operand is the row block [r0, r0 + m) of the n x n matrix (row-major,
// 16-B aligned rows): r0 = 0, m = n on one GPU, or one rank's [VC,*] block (a
// trapezoid); Y receives the block's complete contribution to S X.
//
// gfx950 design.  The stored region is cut into T x T tiles (T = 256): row
// tile I of the block (rows r0 + I T ...) meets the column tiles that hold a
// stored element of one of its rows.  The tiles, in row-major order, are cut
// evenly over one workgroup per CU.  In a tile every wave streams its rows
// with 16-B loads, RB rows per batch; as soon as a batch has been used the
// next one (of this tile or of the workgroup's next one) is issued into the
// same registers, so loads cross the tile's barriers.
// X at the tile's rows and columns sits in LDS.  A lane keeps
// 4 columns of the tile: its 4 k column sums stay in registers over the
// wave's rows and are combined across the waves in LDS at the end of the
// tile; the RB k row sums of a batch are reduced across the wave together by
// a transposing butterfly (about one cross-lane move per value instead of
// six).  Both are written as partials: row sums of tile (I, J) to slot J of
// the row table at the rows of I, column sums to slot I of the column table
// at the rows of J.  Each slot element is written exactly once by exactly one
// workgroup, so the workspace needs no clearing and there are no atomics; a
// finishing kernel adds an output row's slots in increasing slot order in
// f64 (row table, then column table), applies alpha and beta and stores.
// Results are bit-identical from run to run for a fixed number of workgroups.
//
// Elements of the other triangle, of columns >= n and of rows past the block
// are loaded (clamped inside the block) and replaced by a select before any
// arithmetic: NaN or Inf there never reaches a sum.
//
// Accumulation, f32 A: products and sums in f32 inside a tile.  Longest f32
// addition chain: a column sum is 32 fused multiply-adds in one wave plus 7
// additions across the 8 waves = 39 terms; a row sum is 4 in the lane plus 6
// butterfly steps = 10.  Across tiles f64.  f64 A: f64 throughout.
//
// Measured (n = 65536 f32, one MI355X): k = 1 streams the triangle at 4.7 TB/s.
// For k >= 2 the f32 kernels need more than the 256 registers of two waves
// per SIMD and spill (up to 290 per lane at k = 4); k = 4 and 8 run at 0.6
// and 0.9 TB/s.  Fewer waves or rows per batch for wide X is the open item.
#include "sl_common.hpp"

namespace {

constexpr int T = 256;        // tile edge
constexpr int MAX_WG = 4096;

template <typename F> struct Cfg;
template <> struct Cfg<float> {
  static constexpr int NW = 8, RB = 8;    // waves per workgroup, rows per batch
};
template <> struct Cfg<double> {
  static constexpr int NW = 4, RB = 4;
};

constexpr int pow2_ge(int k) { return k <= 1 ? 1 : k <= 2 ? 2 : k <= 4 ? 4 : 8; }
constexpr int log2_of(int v) { return v <= 1 ? 0 : 1 + log2_of(v / 2); }

struct Shape {
  int64_t r0, m, n, lda;
  int lower;
  int nI, nJ;       // row tiles of the block, column tiles of the matrix
  int64_t W;        // tiles in all
};

// column tiles [jlo, jhi] that row tile I of the block meets
__host__ __device__ inline void jrange(const Shape& s, int I, int* jlo, int* jhi) {
  const int64_t g0 = s.r0 + (int64_t)I * T;
  const int64_t g1 = (g0 + T < s.r0 + s.m ? g0 + T : s.r0 + s.m) - 1;
  if (s.lower) {
    *jlo = 0;
    *jhi = (int)(g1 / T);
  } else {
    *jlo = (int)(g0 / T);
    *jhi = s.nJ - 1;
  }
}

// 4 elements of one row for this lane, 16 B per load, as columns relative to
// the tile: f32 4 lane + e; f64 128 (e / 2) + 2 lane + e % 2.
template <typename F> __device__ __forceinline__ int col_of(int lane, int e);
template <> __device__ __forceinline__ int col_of<float>(int lane, int e) { return 4 * lane + e; }
template <> __device__ __forceinline__ int col_of<double>(int lane, int e) {
  return 128 * (e >> 1) + 2 * lane + (e & 1);
}

// row: the row at the tile's first column (wave-uniform); nc: columns of the
// tile inside the matrix.  SAFE: nc < T; the lane's elements are loaded one by
// one, those past the row's end re-read its last one (inside the block) and
// are masked by the caller
template <typename F, bool SAFE>
__device__ __forceinline__ void load_row(const F* __restrict__ row, int lane, int nc, F (&a)[4]) {
  if (SAFE) {
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int c = col_of<F>(lane, e);
      a[e] = row[c < nc ? c : nc - 1];
    }
  } else if (sizeof(F) == 4) {
    const float4 q = *(const float4*)(row + 4 * lane);
    a[0] = q.x, a[1] = q.y, a[2] = q.z, a[3] = q.w;
  } else {
    const double2 q0 = *(const double2*)(row + 2 * lane), q1 = *(const double2*)(row + 128 + 2 * lane);
    a[0] = q0.x, a[1] = q0.y, a[2] = q1.x, a[3] = q1.y;
  }
}

// Sums of V values per lane across the wave: V / 2 + V / 4 + ... exchanges
// that halve the values a lane holds, then a plain butterfly.  Afterwards
// v[0] of every lane is the wave's sum of value (lane >> (6 - log2 V)).
template <int V, typename F> __device__ __forceinline__ void wave_sums(F (&v)[V], int lane) {
  constexpr int LV = log2_of(V);
#pragma unroll
  for (int s = 0; s < LV; ++s) {
    const int h = V >> (s + 1), off = 32 >> s;
    const bool up = (lane & off) != 0;
#pragma unroll
    for (int i = 0; i < h; ++i) {
      const F send = up ? v[i] : v[i + h];
      const F keep = up ? v[i + h] : v[i];
      v[i] = keep + __shfl_xor(send, off, 64);
    }
  }
#pragma unroll
  for (int off = 32 >> LV; off > 0; off >>= 1) v[0] += __shfl_xor(v[0], off, 64);
}

template <typename F, int K> struct Tile {
  static constexpr int NW = Cfg<F>::NW, RB = Cfg<F>::RB, NT = 64 * NW;
  static constexpr int RPW = T / NW;        // rows of a tile per wave
  static constexpr int NB = RPW / RB;       // batches per tile and wave
  static constexpr int KP = pow2_ge(K), V = RB * KP;
  static constexpr int LDS = (T * KP + NW * K * T + K * T) * (int)sizeof(F);
};

// A wave-uniform pointer, handed to the loads through scalar registers.  It
// also keeps the compiler from turning the RB (or, at the matrix edge, 4 RB)
// addresses of a batch into per-lane 64-bit induction variables, which cost
// over a hundred vector registers.
template <typename F> __device__ __forceinline__ const F* uniform_ptr(const F* p) {
  const uint64_t v = (uint64_t)p;
  const uint32_t lo = __builtin_amdgcn_readfirstlane((uint32_t)v);
  const uint32_t hi = __builtin_amdgcn_readfirstlane((uint32_t)(v >> 32));
  return (const F*)((uint64_t)hi << 32 | lo);
}

// rows of one batch: local block rows I T + wave RPW + b RB + rb, clamped into the block
template <typename F, int K>
__device__ __forceinline__ void load_batch(const F* __restrict__ A, const Shape& sh, int I, int J, int b, int wave,
                                           int lane, F (&a)[Cfg<F>::RB][4]) {
  using TL = Tile<F, K>;
  const int64_t cb = (int64_t)J * T;
  const int64_t lr0 = (int64_t)I * T + wave * TL::RPW + b * TL::RB;
  if (cb + T <= sh.n) {
#pragma unroll
    for (int rb = 0; rb < TL::RB; ++rb) {
      const int64_t lr = lr0 + rb < sh.m ? lr0 + rb : sh.m - 1;
      load_row<F, false>(uniform_ptr(A + lr * sh.lda + cb), lane, T, a[rb]);
    }
  } else {
    const int nc = (int)(sh.n - cb);
#pragma unroll
    for (int rb = 0; rb < TL::RB; ++rb) {
      const int64_t lr = lr0 + rb < sh.m ? lr0 + rb : sh.m - 1;
      load_row<F, true>(uniform_ptr(A + lr * sh.lda + cb), lane, nc, a[rb]);
    }
  }
}

// One batch: column sums into cs, the batch's row sums to the row table.
// EDGE: the tile holds elements that are not stored (other triangle, columns
// >= n, rows past the block) or diagonal ones.
template <typename F, int K, bool EDGE>
__device__ __forceinline__ void use_batch(F (&a)[Cfg<F>::RB][4], const Shape& sh, int I, int J, int b, int wave,
                                          int lane, const F* __restrict__ xr, const F* __restrict__ xc, F (&cs)[K][4],
                                          F* __restrict__ wsR) {
  using TL = Tile<F, K>;
  const int64_t cb = (int64_t)J * T;
  const int lt0 = wave * TL::RPW + b * TL::RB;              // row in the tile
  const int64_t g0 = sh.r0 + (int64_t)I * T + lt0;          // global row
  const int64_t gend = sh.r0 + sh.m;
  const int nc = (int)(sh.n - cb < T ? sh.n - cb : T);      // columns of the tile inside the matrix
  F rs[TL::V];
#pragma unroll
  for (int i = 0; i < TL::V; ++i) rs[i] = F(0);
  uint32_t diag = 0;   // bit 4 rb + e: the element is a diagonal one (it adds to its row only)
  if (EDGE) {
#pragma unroll
    for (int rb = 0; rb < TL::RB; ++rb) {
      const int64_t gi = g0 + rb;
      // the diagonal's column in the tile, -1 / T when it lies left / right of it
      const int64_t dd = gi - cb;
      const int d = (int)(dd < -1 ? -1 : dd > T ? T : dd);
      const bool rowok = gi < gend;
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int j = col_of<F>(lane, e);
        const bool ok = rowok && j < nc && (sh.lower ? j <= d : j >= d);
        a[rb][e] = ok ? a[rb][e] : F(0);     // a select: the unused element may be NaN
        diag |= j == d ? 1u << (4 * rb + e) : 0u;
      }
    }
  }
#pragma unroll
  for (int kk = 0; kk < K; ++kk) {
    F x4[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) x4[e] = xc[kk * T + col_of<F>(lane, e)];
#pragma unroll
    for (int rb = 0; rb < TL::RB; ++rb) {
      const F xi = xr[(lt0 + rb) * TL::KP + kk];
      F r = F(0);
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        r = fma(a[rb][e], x4[e], r);
        const F ac = EDGE && (diag >> (4 * rb + e) & 1u) ? F(0) : a[rb][e];
        cs[kk][e] = fma(ac, xi, cs[kk][e]);
      }
      rs[rb * TL::KP + kk] = r;
    }
  }
  wave_sums<TL::V, F>(rs, lane);
  constexpr int GW = 64 / TL::V;             // lanes that end with the same value
  if ((lane & (GW - 1)) == 0) {
    const int idx = lane / GW, rb = idx / TL::KP, kk = idx % TL::KP;
    const int64_t gi = g0 + rb;
    if (kk < K && gi < gend) wsR[((int64_t)J * sh.n + gi) * K + kk] = rs[0];
  }
}

// The batches of one tile: as soon as a batch has been used the next one's
// loads are issued into the same registers, and after the tile's last batch
// the first one of the workgroup's next tile (In, Jn), which so crosses the
// barriers.  The workgroup's other waves keep the memory system busy
// meanwhile.
template <typename F, int K, bool EDGE>
__device__ __forceinline__ void tile_batches(const F* __restrict__ A, const Shape& sh, int I, int J, bool more, int In,
                                             int Jn, int wave, int lane, F (&a)[Cfg<F>::RB][4],
                                             const F* __restrict__ xr, const F* __restrict__ xc, F (&cs)[K][4],
                                             F* __restrict__ wsR) {
  using TL = Tile<F, K>;
#pragma unroll 1
  for (int b = 0; b < TL::NB; ++b) {
    use_batch<F, K, EDGE>(a, sh, I, J, b, wave, lane, xr, xc, cs, wsR);
    if (b + 1 < TL::NB) load_batch<F, K>(A, sh, I, J, b + 1, wave, lane, a);
    else if (more) load_batch<F, K>(A, sh, In, Jn, 0, wave, lane, a);
  }
}

template <typename F, int K>
__global__ void __launch_bounds__(64 * Cfg<F>::NW)
k_symm_tri(const F* __restrict__ A, Shape sh, const F* __restrict__ Xt, F* __restrict__ wsR, F* __restrict__ wsC) {
  using TL = Tile<F, K>;
  extern __shared__ __align__(16) unsigned char smem[];
  F* xr = (F*)smem;                 // [T][KP]: X at the tile's rows
  F* cl = xr + T * TL::KP;          // [NW][K][T]: the waves' column sums
  F* xc = cl + TL::NW * K * T;      // [K][T]: X at the tile's columns
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);   // uniform: row addresses stay scalar
  const int64_t t0 = sh.W * blockIdx.x / gridDim.x, t1 = sh.W * (blockIdx.x + 1) / gridDim.x;
  if (t0 >= t1) return;
  int I = 0, jlo, jhi;
  {
    int64_t rem = t0;
    for (;; ++I) {
      jrange(sh, I, &jlo, &jhi);
      const int64_t c = jhi - jlo + 1;
      if (rem < c) break;
      rem -= c;
    }
    jlo += (int)rem;
  }
  int J = jlo;
  F cur[TL::RB][4];
  load_batch<F, K>(A, sh, I, J, 0, wave, lane, cur);
  for (int64_t t = t0; t < t1; ++t) {
    int In = I, Jn = J + 1;
    if (Jn > jhi) {
      ++In;
      if (t + 1 < t1) {
        jrange(sh, In, &jlo, &jhi);
        Jn = jlo;
      }
    }
    const int64_t cb = (int64_t)J * T, gr = sh.r0 + (int64_t)I * T;
    for (int idx = tid; idx < T * K; idx += TL::NT) {
      const int kk = idx / T, lt = idx - kk * T;
      const int64_t g = gr + lt < sh.n ? gr + lt : sh.n - 1, j = cb + lt < sh.n ? cb + lt : sh.n - 1;
      xr[lt * TL::KP + kk] = Xt[(int64_t)kk * sh.n + g];
      xc[kk * T + lt] = Xt[(int64_t)kk * sh.n + j];
    }
    F cs[K][4];
#pragma unroll
    for (int kk = 0; kk < K; ++kk)
#pragma unroll
      for (int e = 0; e < 4; ++e) cs[kk][e] = F(0);
    __syncthreads();   // xr, xc are complete; the previous tile's cl has been read
    // stored, off-diagonal and whole: no element needs a mask
    const bool whole = gr + T <= sh.r0 + sh.m && cb + T <= sh.n &&
                       (sh.lower ? cb + T - 1 < gr : cb > gr + T - 1);
    if (whole) tile_batches<F, K, false>(A, sh, I, J, t + 1 < t1, In, Jn, wave, lane, cur, xr, xc, cs, wsR);
    else tile_batches<F, K, true>(A, sh, I, J, t + 1 < t1, In, Jn, wave, lane, cur, xr, xc, cs, wsR);
#pragma unroll
    for (int kk = 0; kk < K; ++kk)
#pragma unroll
      for (int e = 0; e < 4; ++e) cl[(wave * K + kk) * T + col_of<F>(lane, e)] = cs[kk][e];
    __syncthreads();   // cl is complete; xr, xc are free for the next tile
    for (int idx = tid; idx < T * K; idx += TL::NT) {
      const int c = idx / K, kk = idx - c * K;
      if (cb + c < sh.n) {
        F s = cl[kk * T + c];
#pragma unroll
        for (int w = 1; w < TL::NW; ++w) s += cl[(w * K + kk) * T + c];
        wsC[((int64_t)I * sh.n + cb + c) * K + kk] = s;
      }
    }
    I = In, J = Jn;
  }
}

// Y[r] <- alpha (row slots of r, then column slots of r, summed in f64) + beta Y[r]
template <typename F>
__global__ void __launch_bounds__(256)
k_symm_finish(Shape sh, int k, const F* __restrict__ wsR, const F* __restrict__ wsC, F* __restrict__ Y, int64_t ldy,
              double alpha, double beta) {
  const int64_t id = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (id >= sh.n * k) return;
  const int64_t r = id / k;
  const int kk = (int)(id - r * k);
  double s = 0.0;
  int jlo, jhi;
  if (r >= sh.r0 && r < sh.r0 + sh.m) {
    jrange(sh, (int)((r - sh.r0) / T), &jlo, &jhi);
    for (int J = jlo; J <= jhi; ++J) s += (double)wsR[((int64_t)J * sh.n + r) * k + kk];
  }
  const int Jr = (int)(r / T);
  for (int I = 0; I < sh.nI; ++I) {
    jrange(sh, I, &jlo, &jhi);
    if (jlo <= Jr && Jr <= jhi) s += (double)wsC[((int64_t)I * sh.n + r) * k + kk];
  }
  s *= alpha;
  if (beta != 0.0) s += beta * (double)Y[r * ldy + kk];
  Y[r * ldy + kk] = (F)s;
}

int cu_count() {
  static int cus = 0;
  if (cus == 0) {
    int dev = 0;
    hipDeviceProp_t prop;
    if (hipGetDevice(&dev) != hipSuccess || hipGetDeviceProperties(&prop, dev) != hipSuccess) return 256;
    cus = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
  }
  return cus;
}

bool make_shape(int64_t n, int64_t r0, int64_t m, int64_t lda, int uplo, Shape* sh) {
  if (n <= 0 || m <= 0 || r0 < 0 || r0 + m > n || lda < n || (uplo != 'L' && uplo != 'U') ||
      n > (int64_t)T * (1 << 20))
    return false;
  sh->r0 = r0, sh->m = m, sh->n = n, sh->lda = lda;
  sh->lower = uplo == 'L';
  sh->nI = (int)((m + T - 1) / T);
  sh->nJ = (int)((n + T - 1) / T);
  sh->W = 0;
  for (int I = 0; I < sh->nI; ++I) {
    int jlo, jhi;
    jrange(*sh, I, &jlo, &jhi);
    sh->W += jhi - jlo + 1;
  }
  return true;
}

template <typename F, int K>
int launch(const F* A, const Shape& sh, const F* Xt, F* ws, int G, hipStream_t st) {
  using TL = Tile<F, K>;
  SL_LDS_ATTR((k_symm_tri<F, K>), TL::LDS);
  F* wsR = ws;
  F* wsC = ws + (int64_t)sh.nJ * sh.n * K;
  k_symm_tri<F, K><<<(unsigned)G, TL::NT, TL::LDS, st>>>(A, sh, Xt, wsR, wsC);
  SL_LAUNCH_CHECK();
  return SL_OK;
}

template <typename F>
int run(const F* A, const Shape& sh, const F* Xt, int k, F* ws, int G, F* Y, int64_t ldy, double alpha, double beta,
        hipStream_t st) {
  int rc = SL_OK;
  switch (k) {
    case 1: rc = launch<F, 1>(A, sh, Xt, ws, G, st); break;
    case 2: rc = launch<F, 2>(A, sh, Xt, ws, G, st); break;
    case 3: rc = launch<F, 3>(A, sh, Xt, ws, G, st); break;
    case 4: rc = launch<F, 4>(A, sh, Xt, ws, G, st); break;
    case 5: rc = launch<F, 5>(A, sh, Xt, ws, G, st); break;
    case 6: rc = launch<F, 6>(A, sh, Xt, ws, G, st); break;
    case 7: rc = launch<F, 7>(A, sh, Xt, ws, G, st); break;
    default: rc = launch<F, 8>(A, sh, Xt, ws, G, st); break;
  }
  if (rc != SL_OK) return rc;
  const unsigned grid = (unsigned)((sh.n * k + 255) / 256);
  k_symm_finish<F><<<grid, 256, 0, st>>>(sh, k, ws, ws + (int64_t)sh.nJ * sh.n * k, Y, ldy, alpha, beta);
  SL_LAUNCH_CHECK();
  return SL_OK;
}

}  // namespace

// Bytes of workspace a call on rows [r0, r0 + m) of an n x n matrix with k
// right-hand sides needs: ceil(n / 256) + ceil(m / 256) slots of n k elements
// of A's type.  -1 when the arguments are out of range.
SL_API int64_t sl_symm_tri_workspace(int64_t n, int64_t m, int k, int dtype) {
  if (n <= 0 || m <= 0 || m > n || k < 1 || k > 8 || (dtype != SL_F32 && dtype != SL_F64)) return -1;
  const int64_t slots = (n + T - 1) / T + (m + T - 1) / T;
  return slots * n * k * (dtype == SL_F64 ? 8 : 4);
}

// Y (n x k, row pitch ldy) <- alpha (contribution of the block to S X) + beta Y.
//   A: rows [r0, r0 + m) of the n x n symmetric S, row-major with pitch lda
//      (elements), f32 / f64, base and pitch 16-B aligned; only its `uplo`
//      ('L' / 'U') triangle is used;
//   Xt: X transposed and contiguous (k x n), A's type, 1 <= k <= 8;
//   ws: sl_symm_tri_workspace bytes, 16-B aligned, contents irrelevant;
//   workgroups: <= 0 for one per CU (fewer when there are fewer tiles);
//   beta == 0 does not read Y.
SL_API int sl_symm_tri(const void* A, int dtype, int uplo, int64_t n, int64_t r0, int64_t m, int64_t lda,
                       const void* Xt, int k, void* ws, int64_t ws_bytes, int workgroups, void* Y, int64_t ldy,
                       double alpha, double beta, void* stream) {
  Shape sh;
  const int64_t need = sl_symm_tri_workspace(n, m, k, dtype);
  if (need < 0 || !make_shape(n, r0, m, lda, uplo, &sh) || !A || !Xt || !Y || !ws || ws_bytes < need || ldy < k ||
      workgroups > MAX_WG) {
    sl_set_last_error("symm_tri: needs f32 / f64 A, 0 <= r0, r0 + m <= n, lda >= n, 1 <= k <= 8, uplo 'L' / 'U', "
                      "ldy >= k, a workspace from symm_tri_workspace, workgroups <= 4096");
    return SL_ERR_INVALID;
  }
  const int64_t es = dtype == SL_F64 ? 8 : 4;
  if (((uintptr_t)A & 15) || (lda * es) % 16 || ((uintptr_t)ws & 15) || ((uintptr_t)Xt & (es - 1)) ||
      ((uintptr_t)Y & (es - 1))) {
    sl_set_last_error("symm_tri: A needs a 16-B aligned base and row pitch, ws 16-B alignment");
    return SL_ERR_INVALID;
  }
  const int cus = cu_count();
  const int G = workgroups > 0 ? workgroups : (int)(sh.W < cus ? sh.W : cus);
  hipStream_t st = (hipStream_t)stream;
  if (dtype == SL_F64)
    return run<double>((const double*)A, sh, (const double*)Xt, k, (double*)ws, G, (double*)Y, ldy, alpha, beta, st);
  return run<float>((const float*)A, sh, (const float*)Xt, k, (float*)ws, G, (float*)Y, ldy, alpha, beta, st);
}
