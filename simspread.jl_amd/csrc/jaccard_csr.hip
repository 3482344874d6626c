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
// This file holds what is the producer's own: the keep rule and the host side.  The staging, the two sums and the
// expression of s are jaccard_tile.hpp, shared with the selection pass of the neighbour floor (real_floor.hip): with
// k > 0, count() first asks it for tau[na], the k-th largest positive similarity of every row, and the tile kernel keeps
// (i, j) iff v != 0 and (s >= alpha or (s > 0 and s >= tau[i])).  That rule is not symmetric, so the floor case runs the
// full (ntj, nti) grid with Fb = Fa instead of the triangle.
#include <hip/hip_runtime.h>

#include "graph.hpp"
#include "jaccard_tile.hpp"
#include "pair_tile.hpp"

namespace ss {

namespace {

using jctile::BK;
using jctile::Block;
using jctile::NTX;
using jctile::RC;
using jctile::threads;
using jctile::TILE;

template <class T>
__device__ __forceinline__ bool jaccard_keep(T smin, T smax, T alpha, bool weighted, T& v) {
  const T s = jctile::jaccard_similarity<T>(smin, smax);
  v = weighted ? s : T(1);
  return s >= alpha && v != T(0);
}

// the neighbour floor (real_floor.hip): row i also keeps its positive similarities >= tau = tau[i], the k-th largest of
// them (+0 when it has fewer than k: all of them stay)
template <class T>
__device__ __forceinline__ bool jaccard_keep_floor(T smin, T smax, T alpha, T tau, bool weighted, T& v) {
  const T s = jctile::jaccard_similarity<T>(smin, smax);
  v = weighted ? s : T(1);
  return v != T(0) && (s >= alpha || (s > T(0) && s >= tau));
}

// FILL == false: write the per-(tile, row) counts and the tile flag.  FILL == true: write the entries of the tiles that
// kept something (counts then hold in-row offsets).
// FLOOR: the per-row cut tau[na] next to alpha; a pair is then decided by its row alone, so there is no mirror (!SYM).
template <class T, bool SYM, bool FILL, bool FLOOR>
__global__ void __launch_bounds__(threads<T>()) jaccard_tile_kernel(
    const T* __restrict__ Fa, int64_t na, int64_t lda, const T* __restrict__ Fb, int64_t nb, int64_t ldb, int64_t d,
    T alpha, const T* __restrict__ tau, int weighted, int64_t nti, int* __restrict__ counts,
    int* __restrict__ tile_nz, const int64_t* __restrict__ ptr, int* __restrict__ oidx, T* __restrict__ oval,
    int* __restrict__ not_binary) {
  static_assert(!(SYM && FLOOR), "a per-row cut decides (i, j) and (j, i) separately");
  constexpr int RA = Block<T>::RA;

  if (FILL && tile_nz[pair_tile_index<SYM>()] == 0) return;  // uniform over the block
  const PairTile t = pair_tile<SYM, TILE>(nti);

  jctile::Sums<T> acc[RA][RC];
  jctile::jaccard_tile_sums<T>(Fa, na, lda, Fb, nb, ldb, d, t.i0, t.j0, acc);

  const bool wgt = weighted != 0;
  if constexpr (FLOOR) {
    const int ty = threadIdx.x / NTX;
    T ta[RA];
#pragma unroll
    for (int a = 0; a < RA; ++a) {
      const int64_t i = t.i0 + RA * ty + a;
      ta[a] = i < na ? tau[i] : T(0);
    }
    pair_tile_emit<T, TILE, RA, RC, false, FILL, true>(
        t, na, nb,
        [&](int a, int b, T& v) { return jaccard_keep_floor<T>(acc[a][b].x, acc[a][b].y, alpha, ta[a], wgt, v); },
        counts, tile_nz, ptr, oidx, oval, not_binary);
  } else {
    pair_tile_emit<T, TILE, RA, RC, SYM, FILL, true>(
        t, na, nb, [&](int a, int b, T& v) { return jaccard_keep<T>(acc[a][b].x, acc[a][b].y, alpha, wgt, v); }, counts,
        tile_nz, ptr, oidx, oval, not_binary);
  }
}

}  // namespace

template <class T>
int JaccardCsr<T>::count(const T* Fa_, int64_t na_, int64_t lda_, const T* Fb_, int64_t nb_, int64_t ldb_, int64_t d_,
                         T alpha_, bool weighted_, int k) {
  what = "jaccard";
  self = (Fb_ == nullptr);
  sym = self;
  Fa = Fa_;
  Fb = self ? Fa_ : Fb_;
  lda = lda_;
  ldb = self ? lda_ : ldb_;
  d = d_;
  alpha = alpha_;
  weighted = weighted_;
  tau = nullptr;
  if (alpha != alpha) return fail(SS_EINVAL, "jaccard: alpha is NaN");
  SS_TRY(this->refuse_nan_features(Fa, na_, lda, Fb, nb_, ldb, d));
  sym = self && k == 0;  // a per-row cut has no mirror: the full grid
  SS_TRY(this->begin_tiles(na_, self ? na_ : nb_, TILE, true));
  if (na == 0 || nb == 0) return SS_OK;
  if (k > 0) {
    SS_TRY(tau_buf.alloc(na));
    SS_TRY(jaccard_kth<T>(Fa, na, lda, self ? nullptr : Fb, nb, ldb, d, k, tau_buf.p));
    tau = tau_buf.p;
  }
  return this->count_pass();
}

template <class T>
int JaccardCsr<T>::launch(bool fill, int* idx, T* val, int* flag) {
  auto* kernel =
      tau   ? (fill ? jaccard_tile_kernel<T, false, true, true> : jaccard_tile_kernel<T, false, false, true>)
      : sym ? (fill ? jaccard_tile_kernel<T, true, true, false> : jaccard_tile_kernel<T, true, false, false>)
            : (fill ? jaccard_tile_kernel<T, false, true, false> : jaccard_tile_kernel<T, false, false, false>);
  hipLaunchKernelGGL(kernel, this->tile_grid(), dim3(threads<T>()), 0, ctx().stream, Fa, na, lda, Fb, nb, ldb, d, alpha,
                     tau, weighted ? 1 : 0, nti, counts.p, tile_nz.p, ptr.p, idx, val, flag);
  SS_LAUNCH_CHECK();
  return SS_OK;
}

template struct JaccardCsr<float>;
template struct JaccardCsr<double>;

}  // namespace ss
