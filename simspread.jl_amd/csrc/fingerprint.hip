// Thresholded Tanimoto similarity of packed binary fingerprints, produced straight as CSR: the featurize cutoff
// (src/core.jl:106-112) applied to `1 .- pairwise(Jaccard(), F, dims=1)` (docs/src/tutorial/fishers-flowers.jl:66) on
// 0/1 rows, without the dense n x n similarity ever existing.
//
//   c = popcount(a & b), u = popcount(a) + popcount(b) - c, s = u == 0 ? 1 : T(c) / T(u)
//   keep (i, j) iff s >= alpha and v != 0 with v = weighted ? s : 1          (keep_entry of assemble.hip)
//
// The counts are exact integers and the quotient is one correctly rounded division, the same one jaccard_kernel
// (kernels.hip) performs on the float sums of min / max, so the CSR is bitwise equal to the dense route.
//
// Two passes over 128 x 128 tiles of (row, column) pairs, 256 threads, an 8 x 8 block of pairs per thread; the tiles,
// the symmetric mode and the emit epilogue are pair_tile.hpp, the host side PairCsr (pair_csr.hip):
//   count  per (column tile, row): the number of kept entries          -> counts[jt * rows + i]
//   (per row: in-row exclusive offsets of the slots and the row total; a 64-bit scan of the totals gives ptr, and the
//    nnz >= 2^31 refusal happens there, before any output exists)
//   fill   the same tiles again (every one: this producer keeps no per-tile flag), each slot written at ptr[i] + its
//          offset in column order.
// This file holds what is the producer's own: the keep rule and the host side.  The row popcounts, the staging and the
// AND-popcount sums are tanimoto_tile.hpp, shared with the selection pass of the neighbour floor (neighbour_floor.hip):
// with k > 0, count() first asks it for tau[na], the k-th largest positive similarity of every row, and the tile kernel
// keeps (i, j) iff v != 0 and (s >= alpha or (s > 0 and s >= tau[i])).  That rule is not symmetric, so the floor case
// runs the full (ntj, nti) grid with Fb = Fa instead of the triangle: twice the pair work of the symmetric mode.
#include <cstdlib>
#include <cstring>
#include <hip/hip_runtime.h>
#include <rocprim/rocprim.hpp>

#include "graph.hpp"
#include "pair_tile.hpp"
#include "tanimoto_tile.hpp"

namespace ss {

namespace {

using fptile::BK;
using fptile::RB;
using fptile::TILE;
using fptile::popcount_rows_kernel;

template <class T>
__device__ __forceinline__ bool tanimoto_keep(int c, int pa, int pb, T alpha, bool weighted, T& v) {
  const T s = fptile::tanimoto_similarity<T>(c, pa, pb);
  v = weighted ? s : T(1);
  return s >= alpha && v != T(0);
}

// the neighbour floor (neighbour_floor.hip): row i also keeps its positive similarities >= tau = tau[i], the k-th
// largest of them (+0 when it has fewer than k: all of them stay)
template <class T>
__device__ __forceinline__ bool tanimoto_keep_floor(int c, int pa, int pb, T alpha, T tau, bool weighted, T& v) {
  const T s = fptile::tanimoto_similarity<T>(c, pa, pb);
  v = weighted ? s : T(1);
  return v != T(0) && (s >= alpha || (s > T(0) && s >= tau));
}

// FILL == false: write the per-(tile, row) counts.  FILL == true: write the entries (counts then hold in-row offsets).
// FLOOR: the per-row cut tau[na] next to alpha; a pair is then decided by its row alone, so there is no mirror (!SYM).
template <class T, bool SYM, bool FILL, bool FLOOR>
__global__ void __launch_bounds__(256) tanimoto_tile_kernel(
    const uint64_t* __restrict__ Fa, int64_t na, const uint64_t* __restrict__ Fb, int64_t nb, int64_t nwords,
    const int* __restrict__ pop_a, const int* __restrict__ pop_b, T alpha, const T* __restrict__ tau, int weighted,
    int64_t nti, int* __restrict__ counts, const int64_t* __restrict__ ptr, int* __restrict__ oidx,
    T* __restrict__ oval, int* __restrict__ not_binary) {
  static_assert(!(SYM && FLOOR), "a per-row cut decides (i, j) and (j, i) separately");
  __shared__ __attribute__((aligned(16))) uint32_t As[BK][TILE];
  __shared__ __attribute__((aligned(16))) uint32_t Bs[BK][TILE];

  const PairTile t = pair_tile<SYM, TILE>(nti);
  const int64_t i0 = t.i0, j0 = t.j0;
  const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;

  uint32_t acc[RB][RB];
  fptile::tanimoto_tile_counts(As, Bs, Fa, na, Fb, nb, nwords, i0, j0, acc);

  // popcounts of the thread's rows and columns; those past the last row / column are never used
  int pa[RB], pb[RB];
#pragma unroll
  for (int a = 0; a < RB; ++a) {
    const int64_t i = i0 + RB * ty + a;
    pa[a] = i < na ? pop_a[i] : 0;
  }
#pragma unroll
  for (int b = 0; b < RB; ++b) {
    const int64_t j = j0 + RB * tx + b;
    pb[b] = j < nb ? pop_b[j] : 0;
  }
  const bool wgt = weighted != 0;
  if constexpr (FLOOR) {
    T ta[RB];
#pragma unroll
    for (int a = 0; a < RB; ++a) {
      const int64_t i = i0 + RB * ty + a;
      ta[a] = i < na ? tau[i] : T(0);
    }
    pair_tile_emit<T, TILE, RB, RB, false, FILL, false>(
        t, na, nb,
        [&](int a, int b, T& v) {
          return tanimoto_keep_floor<T>((int)acc[a][b], pa[a], pb[b], alpha, ta[a], wgt, v);
        },
        counts, nullptr, ptr, oidx, oval, not_binary);
  } else {
    pair_tile_emit<T, TILE, RB, RB, SYM, FILL, false>(
        t, na, nb, [&](int a, int b, T& v) { return tanimoto_keep<T>((int)acc[a][b], pa[a], pb[b], alpha, wgt, v); },
        counts, nullptr, ptr, oidx, oval, not_binary);
  }
}

}  // namespace

template <class T>
int TanimotoCsr<T>::count(const uint64_t* Fa_, int64_t na_, const uint64_t* Fb_, int64_t nb_, int64_t nwords_, T alpha_,
                          bool weighted_, int k) {
  hipStream_t st = ctx().stream;
  self = (Fb_ == nullptr);
  what = k > 0 ? "tanimoto floor" : "tanimoto";
  sym = self && k == 0;  // a per-row cut has no mirror: the full grid
  Fa = Fa_;
  Fb = self ? Fa_ : Fb_;
  nwords = nwords_;
  alpha = alpha_;
  weighted = weighted_;
  tau = nullptr;
  SS_TRY(this->begin_tiles(na_, self ? na_ : nb_, TILE, false));
  if (na == 0 || nb == 0) return SS_OK;
  SS_TRY(pop_a.alloc(na));
  hipLaunchKernelGGL(popcount_rows_kernel, dim3((unsigned)ceil_div(na, 256)), dim3(256), 0, st, Fa, na, nwords, pop_a.p);
  SS_LAUNCH_CHECK();
  if (!self) {
    SS_TRY(pop_b.alloc(nb));
    hipLaunchKernelGGL(popcount_rows_kernel, dim3((unsigned)ceil_div(nb, 256)), dim3(256), 0, st, Fb, nb, nwords,
                       pop_b.p);
    SS_LAUNCH_CHECK();
  }
  if (k > 0) {
    SS_TRY(tau_buf.alloc(na));
    SS_TRY(tanimoto_kth<T>(Fa, na, Fb, nb, nwords, pop_a.p, self ? pop_a.p : pop_b.p, k, tau_buf.p));
    tau = tau_buf.p;
  }
  return this->count_pass();
}

template <class T>
int TanimotoCsr<T>::launch(bool fill, int* idx, T* val, int* flag) {
  auto* kernel = tau   ? (fill ? tanimoto_tile_kernel<T, false, true, true> : tanimoto_tile_kernel<T, false, false, true>)
                 : sym ? (fill ? tanimoto_tile_kernel<T, true, true, false> : tanimoto_tile_kernel<T, true, false, false>)
                       : (fill ? tanimoto_tile_kernel<T, false, true, false>
                               : tanimoto_tile_kernel<T, false, false, false>);
  hipLaunchKernelGGL(kernel, this->tile_grid(), dim3(256), 0, ctx().stream, Fa, na, Fb, nb, nwords, pop_a.p,
                     self ? pop_a.p : pop_b.p, alpha, tau, weighted ? 1 : 0, nti, counts.p, ptr.p, idx, val, flag);
  SS_LAUNCH_CHECK();
  return SS_OK;
}

template struct TanimotoCsr<float>;
template struct TanimotoCsr<double>;

}  // namespace ss
