// Thresholded weighted Jaccard (Ruzicka) similarity of real-valued feature rows, produced straight as CSR: the
// featurize cutoff (src/core.jl:106-112) applied to `1 .- pairwise(Jaccard(), X, dims=1)`
// (docs/src/tutorial/fishers-flowers.jl:66,95-96), without the dense n x n similarity ever existing.
//
//   smin = smax = +0; for k = 0 .. d-1 in order, in T: smin += min(a_k, b_k), smax += max(a_k, b_k)
//   s = smax == 0 ? 1 : smin / smax                                          (one correctly rounded division in T)
//   keep (i, j) iff s >= alpha and v != 0 with v = weighted ? s : 1          (keep_entry of assemble.hip)
//
// This is jaccard_kernel (kernels.hip) pair for pair: the two sums run sequentially over k in T, nothing is
// reassociated or split, and the quotient is the plain division (the Makefile builds without fast-math), so the CSR is
// bitwise equal to the dense route followed by the cutoff.  v_min / v_max stand in for the compare-and-select of the
// dense kernel: for non-NaN inputs they differ only in the sign of a zero, and adding -0 instead of +0 to a sum that
// started at +0 changes nothing.  NaN features are refused before anything is written.
//
// Two passes over 128 x 128 tiles of (row, column) pairs; the tiles, the symmetric mode and the emit epilogue are
// pair_tile.hpp, the host side PairCsr (pair_csr.hip):
//   count  per (column tile, row): the number of kept entries -> counts[jt * rows + i]; per tile: any kept -> tile_nz
//   fill   the tiles that kept something, again, each slot written at ptr[i] + its offset in column order.
// Register blocks: fp32 8 x 8 pairs per thread (256 threads, 128 accumulator VGPRs), fp64 4 x 8 (512 threads, the
// same 128 VGPRs).  This file holds what is the producer's own: the staging, the two sums and the keep rule.
#include <hip/hip_runtime.h>

#include "graph.hpp"
#include "pair_tile.hpp"

namespace ss {

namespace {

constexpr int TILE = 128;  // rows and columns per workgroup tile
constexpr int BK = 16;     // feature columns staged per step
constexpr int RC = 8;      // columns per thread
constexpr int NTX = TILE / RC;  // 16 thread columns

template <class T>
struct Block;
template <>
struct Block<float> {
  static constexpr int RA = 8;  // rows per thread
};
template <>
struct Block<double> {
  static constexpr int RA = 4;
};

__device__ __forceinline__ float vmin(float a, float b) { return __builtin_fminf(a, b); }
__device__ __forceinline__ float vmax(float a, float b) { return __builtin_fmaxf(a, b); }
__device__ __forceinline__ double vmin(double a, double b) { return __builtin_fmin(a, b); }
__device__ __forceinline__ double vmax(double a, double b) { return __builtin_fmax(a, b); }

template <class T>
__device__ __forceinline__ bool jaccard_keep(T smin, T smax, T alpha, bool weighted, T& v) {
  const T s = smax == T(0) ? T(1) : smin / smax;
  v = weighted ? s : T(1);
  return s >= alpha && v != T(0);
}

// FILL == false: write the per-(tile, row) counts and the tile flag.  FILL == true: write the entries of the tiles that
// kept something (counts then hold in-row offsets).
template <class T, bool SYM, bool FILL>
__global__ void __launch_bounds__(NTX * (TILE / Block<T>::RA)) jaccard_tile_kernel(
    const T* __restrict__ Fa, int64_t na, int64_t lda, const T* __restrict__ Fb, int64_t nb, int64_t ldb, int64_t d,
    T alpha, int weighted, int64_t nti, int* __restrict__ counts, int* __restrict__ tile_nz,
    const int64_t* __restrict__ ptr, int* __restrict__ oidx, T* __restrict__ oval, int* __restrict__ not_binary) {
  constexpr int RA = Block<T>::RA;
  constexpr int NTY = TILE / RA;       // thread rows
  constexpr int NT = NTX * NTY;        // threads
  __shared__ __attribute__((aligned(16))) T As[BK][TILE];
  __shared__ __attribute__((aligned(16))) T Bs[BK][TILE];

  if (FILL && tile_nz[pair_tile_index<SYM>()] == 0) return;  // uniform over the block
  const PairTile t = pair_tile<SYM, TILE>(nti);
  const int64_t i0 = t.i0, j0 = t.j0;
  const int tid = threadIdx.x, tx = tid % NTX, ty = tid / NTX;

  // acc[a][b] = (smin, smax) of one pair: the two sums sit in adjacent registers, so that fp32 adds them with one
  // v_pk_add_f32 (lane-wise, each lane one correctly rounded add -- the same two adds)
  typedef T T2 __attribute__((ext_vector_type(2)));
  T2 acc[RA][RC];
#pragma unroll
  for (int a = 0; a < RA; ++a)
#pragma unroll
    for (int b = 0; b < RC; ++b) acc[a][b] = T2{T(0), T(0)};

  // staging: BK feature columns of the tile's 128 rows of each side; consecutive threads read consecutive rows of one
  // column (coalesced).  Past d or past the last row the value is 0: a padded k adds +0 to both sums, which changes
  // nothing, and padded rows / columns are masked below.
  constexpr int PER = BK * TILE / NT;
  T ra[PER], rb[PER];
  auto load = [&](int64_t k0) {
#pragma unroll
    for (int q = 0; q < PER; ++q) {
      const int e = tid + q * NT;
      const int kk = e / TILE, r = e % TILE;
      const int64_t k = k0 + kk;
      ra[q] = (k < d && i0 + r < na) ? Fa[i0 + r + k * lda] : T(0);
      rb[q] = (k < d && j0 + r < nb) ? Fb[j0 + r + k * ldb] : T(0);
    }
  };
  if (d > 0) load(0);
  for (int64_t k0 = 0; k0 < d; k0 += BK) {
#pragma unroll
    for (int q = 0; q < PER; ++q) {
      const int e = tid + q * NT;
      As[e / TILE][e % TILE] = ra[q];
      Bs[e / TILE][e % TILE] = rb[q];
    }
    __syncthreads();
    if (k0 + BK < d) load(k0 + BK);  // the next step's loads are in flight during this step's arithmetic
#pragma unroll
    for (int kk = 0; kk < BK; ++kk) {
      T av[RA], bv[RC];
#pragma unroll
      for (int a = 0; a < RA; ++a) av[a] = As[kk][RA * ty + a];
#pragma unroll
      for (int b = 0; b < RC; ++b) bv[b] = Bs[kk][RC * tx + b];
#pragma unroll
      for (int a = 0; a < RA; ++a)
#pragma unroll
        for (int b = 0; b < RC; ++b) acc[a][b] += T2{vmin(av[a], bv[b]), vmax(av[a], bv[b])};
    }
    __syncthreads();
  }

  const bool wgt = weighted != 0;
  pair_tile_emit<T, TILE, RA, RC, SYM, FILL, true>(
      t, na, nb, [&](int a, int b, T& v) { return jaccard_keep<T>(acc[a][b].x, acc[a][b].y, alpha, wgt, v); }, counts,
      tile_nz, ptr, oidx, oval, not_binary);
}

template <class T>
constexpr int threads() {
  return NTX * (TILE / Block<T>::RA);
}

}  // namespace

template <class T>
int JaccardCsr<T>::count(const T* Fa_, int64_t na_, int64_t lda_, const T* Fb_, int64_t nb_, int64_t ldb_, int64_t d_,
                         T alpha_, bool weighted_) {
  what = "jaccard";
  sym = (Fb_ == nullptr);
  Fa = Fa_;
  Fb = sym ? Fa_ : Fb_;
  lda = lda_;
  ldb = sym ? lda_ : ldb_;
  d = d_;
  alpha = alpha_;
  weighted = weighted_;
  if (alpha != alpha) return fail(SS_EINVAL, "jaccard: alpha is NaN");
  SS_TRY(this->refuse_nan_features(Fa, na_, lda, Fb, nb_, ldb, d));
  SS_TRY(this->begin_tiles(na_, sym ? na_ : nb_, TILE, true));
  if (na == 0 || nb == 0) return SS_OK;
  return this->count_pass();
}

template <class T>
int JaccardCsr<T>::launch(bool fill, int* idx, T* val, int* flag) {
  auto* kernel = sym ? (fill ? jaccard_tile_kernel<T, true, true> : jaccard_tile_kernel<T, true, false>)
                     : (fill ? jaccard_tile_kernel<T, false, true> : jaccard_tile_kernel<T, false, false>);
  hipLaunchKernelGGL(kernel, this->tile_grid(), dim3(threads<T>()), 0, ctx().stream, Fa, na, lda, Fb, nb, ldb, d, alpha,
                     weighted ? 1 : 0, nti, counts.p, tile_nz.p, ptr.p, idx, val, flag);
  SS_LAUNCH_CHECK();
  return SS_OK;
}

template struct JaccardCsr<float>;
template struct JaccardCsr<double>;

}  // namespace ss
