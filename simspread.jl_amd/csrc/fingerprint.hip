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
// This file holds what is the producer's own: the row popcounts, the staging, the AND-popcount sums and the keep rule.
#include <cstdlib>
#include <cstring>
#include <hip/hip_runtime.h>
#include <rocprim/rocprim.hpp>

#include "graph.hpp"
#include "pair_tile.hpp"

namespace ss {

namespace {

constexpr int TILE = 128;  // rows and columns per workgroup tile
constexpr int BK = 16;     // 32-bit fingerprint words staged per step (8 uint64 words)
constexpr int RB = 8;      // rows / columns per thread

__global__ void popcount_rows_kernel(const uint64_t* __restrict__ F, int64_t n, int64_t nwords, int* __restrict__ pop) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const uint64_t* row = F + i * nwords;
  int c = 0;
  for (int64_t w = 0; w < nwords; ++w) c += __popcll(row[w]);
  pop[i] = c;
}

template <class T>
__device__ __forceinline__ bool tanimoto_keep(int c, int pa, int pb, T alpha, bool weighted, T& v) {
  const int u = pa + pb - c;
  const T s = u == 0 ? T(1) : T(c) / T(u);
  v = weighted ? s : T(1);
  return s >= alpha && v != T(0);
}

// FILL == false: write the per-(tile, row) counts.  FILL == true: write the entries (counts then hold in-row offsets).
template <class T, bool SYM, bool FILL>
__global__ void __launch_bounds__(256) tanimoto_tile_kernel(
    const uint64_t* __restrict__ Fa, int64_t na, const uint64_t* __restrict__ Fb, int64_t nb, int64_t nwords,
    const int* __restrict__ pop_a, const int* __restrict__ pop_b, T alpha, int weighted, int64_t nti,
    int* __restrict__ counts, const int64_t* __restrict__ ptr, int* __restrict__ oidx, T* __restrict__ oval,
    int* __restrict__ not_binary) {
  __shared__ __attribute__((aligned(16))) uint32_t As[BK][TILE];
  __shared__ __attribute__((aligned(16))) uint32_t Bs[BK][TILE];

  const PairTile t = pair_tile<SYM, TILE>(nti);
  const int64_t i0 = t.i0, j0 = t.j0;
  const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;

  uint32_t acc[RB][RB];
#pragma unroll
  for (int a = 0; a < RB; ++a)
#pragma unroll
    for (int b = 0; b < RB; ++b) acc[a][b] = 0;

  for (int64_t w0 = 0; w0 < nwords; w0 += BK / 2) {
    // stage 8 uint64 words of 128 rows of each side: consecutive threads read consecutive words of a row
#pragma unroll
    for (int e = tid; e < TILE * (BK / 2); e += 256) {
      const int r = e >> 3, w = e & 7;
      const int64_t k = w0 + w;
      const int64_t ia = i0 + r, jb = j0 + r;
      const uint64_t x = (k < nwords && ia < na) ? Fa[ia * nwords + k] : 0ull;
      const uint64_t y = (k < nwords && jb < nb) ? Fb[jb * nwords + k] : 0ull;
      As[2 * w][r] = (uint32_t)x;
      As[2 * w + 1][r] = (uint32_t)(x >> 32);
      Bs[2 * w][r] = (uint32_t)y;
      Bs[2 * w + 1][r] = (uint32_t)(y >> 32);
    }
    __syncthreads();
#pragma unroll
    for (int kk = 0; kk < BK; ++kk) {
      const uint4 a0 = *reinterpret_cast<const uint4*>(&As[kk][RB * ty]);
      const uint4 a1 = *reinterpret_cast<const uint4*>(&As[kk][RB * ty + 4]);
      const uint4 b0 = *reinterpret_cast<const uint4*>(&Bs[kk][RB * tx]);
      const uint4 b1 = *reinterpret_cast<const uint4*>(&Bs[kk][RB * tx + 4]);
      const uint32_t av[RB] = {a0.x, a0.y, a0.z, a0.w, a1.x, a1.y, a1.z, a1.w};
      const uint32_t bv[RB] = {b0.x, b0.y, b0.z, b0.w, b1.x, b1.y, b1.z, b1.w};
#pragma unroll
      for (int a = 0; a < RB; ++a)
#pragma unroll
        for (int b = 0; b < RB; ++b) acc[a][b] += __popc(av[a] & bv[b]);
    }
    __syncthreads();
  }

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
  pair_tile_emit<T, TILE, RB, RB, SYM, FILL, false>(
      t, na, nb, [&](int a, int b, T& v) { return tanimoto_keep<T>((int)acc[a][b], pa[a], pb[b], alpha, wgt, v); },
      counts, nullptr, ptr, oidx, oval, not_binary);
}

}  // namespace

template <class T>
int TanimotoCsr<T>::count(const uint64_t* Fa_, int64_t na_, const uint64_t* Fb_, int64_t nb_, int64_t nwords_, T alpha_,
                          bool weighted_) {
  hipStream_t st = ctx().stream;
  what = "tanimoto";
  sym = (Fb_ == nullptr);
  Fa = Fa_;
  Fb = sym ? Fa_ : Fb_;
  nwords = nwords_;
  alpha = alpha_;
  weighted = weighted_;
  SS_TRY(this->begin_tiles(na_, sym ? na_ : nb_, TILE, false));
  if (na == 0 || nb == 0) return SS_OK;
  SS_TRY(pop_a.alloc(na));
  hipLaunchKernelGGL(popcount_rows_kernel, dim3((unsigned)ceil_div(na, 256)), dim3(256), 0, st, Fa, na, nwords, pop_a.p);
  SS_LAUNCH_CHECK();
  if (!sym) {
    SS_TRY(pop_b.alloc(nb));
    hipLaunchKernelGGL(popcount_rows_kernel, dim3((unsigned)ceil_div(nb, 256)), dim3(256), 0, st, Fb, nb, nwords,
                       pop_b.p);
    SS_LAUNCH_CHECK();
  }
  return this->count_pass();
}

template <class T>
int TanimotoCsr<T>::launch(bool fill, int* idx, T* val, int* flag) {
  auto* kernel = sym ? (fill ? tanimoto_tile_kernel<T, true, true> : tanimoto_tile_kernel<T, true, false>)
                     : (fill ? tanimoto_tile_kernel<T, false, true> : tanimoto_tile_kernel<T, false, false>);
  hipLaunchKernelGGL(kernel, this->tile_grid(), dim3(256), 0, ctx().stream, Fa, na, Fb, nb, nwords, pop_a.p,
                     sym ? pop_a.p : pop_b.p, alpha, weighted ? 1 : 0, nti, counts.p, ptr.p, idx, val, flag);
  SS_LAUNCH_CHECK();
  return SS_OK;
}

template struct TanimotoCsr<float>;
template struct TanimotoCsr<double>;

}  // namespace ss
