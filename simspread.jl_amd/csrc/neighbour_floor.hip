// The neighbour floor of the fingerprint producer: tau[i], the k-th largest positive Tanimoto similarity of row i of Fa
// against the rows of Fb, for every row, without the na x nb similarity ever existing.  fingerprint.hip keeps entry
// (i, j) iff v != 0 and (s >= alpha or (s > 0 and s >= tau[i])): "at least the k nearest sources, whatever alpha says".
//
//   P_i   = multiset { s(i, j) : 0 <= j < nb, s(i, j) > 0 },   s as in fingerprint.hip (tanimoto_tile.hpp)
//   tau_i = the k-th largest element of P_i, multiplicity counted, when |P_i| >= k, else +0
//
// Ties at tau_i are all kept by the emit pass, so only the VALUE of the k-th entry is needed, never which column holds
// it: the selection keeps multisets of values and no indices.
//
// Two kernels:
//   partial  the all-pairs tile pass of the producer (same 128 x 128 tiles, same staging, same AND-popcount loop, same
//            expression of s: tanimoto_tile.hpp) with the selection skeleton of row_select.hpp as its epilogue.  Block
//            (x, g) owns ROWS rows of row strip x / (TILE / ROWS) and walks the column tiles of column group g; it
//            leaves the k largest positive values of every row among those columns in part[g][row][0..k), +0 padded.
//            Column groups are the second level of parallelism: few rows against many columns (query batches) would
//            otherwise be a handful of blocks.
//   merge    kth_merge.hpp, shared with the selections of the real-valued producers (real_floor.hip), as is the sizing
//            of the column groups.
// Scratch: na * k * groups values.  Every device loop is bounded by k, the tile width, the tiles of a group or
// groups * k <= 4096 (host-checked); there are no spin-waits and no flags between workgroups.
//
// LDS: the lists of a block take ROWS * k values and are held to 32 KiB, so that with the 16 KiB of tile staging and
// the candidate buffers the block stays inside the 64 KiB of static LDS: ROWS = 128, the whole strip, except for
// T = double with k > 32, where a block selects for 64 rows and two blocks share a strip (each computes the strip's
// full tile and uses half of it).
#include <algorithm>
#include <hip/hip_runtime.h>

#include "graph.hpp"
#include "kth_merge.hpp"
#include "row_select.hpp"
#include "tanimoto_tile.hpp"

namespace ss {

namespace {

using fptile::BK;
using fptile::RB;
using fptile::TILE;

// the pair similarity of the selection: THE expression of the emit pass
template <class T>
struct TanimotoSim {
  __device__ __forceinline__ T operator()(int c, int pa, int pb) const { return fptile::tanimoto_similarity<T>(c, pa, pb); }
};

// Sim: the pair similarity from (popcount(a & b), popcount(a), popcount(b)), a functor so that another similarity of
// the same counts can select with this kernel
template <class T, int ROWS, class Sim>
__global__ void __launch_bounds__(256) tanimoto_kth_partial_kernel(
    const uint64_t* __restrict__ Fa, int64_t na, const uint64_t* __restrict__ Fb, int64_t nb, int64_t nwords,
    const int* __restrict__ pop_a, const int* __restrict__ pop_b, int k, int64_t ntj, int64_t tiles_per_group,
    T* __restrict__ part, Sim sim) {
  __shared__ __attribute__((aligned(16))) uint32_t As[BK][TILE];
  __shared__ __attribute__((aligned(16))) uint32_t Bs[BK][TILE];
  __shared__ RowSelect<T, TILE, ROWS> sel;

  constexpr int NH = TILE / ROWS;  // blocks per row strip
  const int64_t it = blockIdx.x / NH;
  const int sel0 = (int)(blockIdx.x % NH) * ROWS;
  const int64_t g = blockIdx.y;
  const int64_t i0 = it * TILE;
  const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
  const bool mine = RB * ty >= sel0 && RB * ty < sel0 + ROWS;

  int pa[RB];  // -1: the row does not exist
#pragma unroll
  for (int a = 0; a < RB; ++a) {
    const int64_t i = i0 + RB * ty + a;
    pa[a] = i < na ? pop_a[i] : -1;
  }

  int cnt;
  sel.init(cnt);

  const int64_t jt_end = min((g + 1) * tiles_per_group, ntj);
#pragma unroll 1
  for (int64_t jt = g * tiles_per_group; jt < jt_end; ++jt) {
    const int64_t j0 = jt * TILE;
    uint32_t acc[RB][RB];
    fptile::tanimoto_tile_counts(As, Bs, Fa, na, Fb, nb, nwords, i0, j0, acc);
    int pb[RB];
#pragma unroll
    for (int b = 0; b < RB; ++b) {
      const int64_t j = j0 + RB * tx + b;
      pb[b] = j < nb ? pop_b[j] : -1;
    }
    T s[RB][RB];
#pragma unroll
    for (int a = 0; a < RB; ++a)
#pragma unroll
      for (int b = 0; b < RB; ++b)
        s[a][b] = pa[a] >= 0 && pb[b] >= 0 ? sim((int)acc[a][b], pa[a], pb[b]) : T(0);
    sel.absorb(RB * ty - sel0, mine, k, cnt, s);
  }
  sel.store(i0 + sel0, na, k, cnt, part + g * na * k);
}

}  // namespace

template <class T>
int tanimoto_kth(const uint64_t* Fa, int64_t na, const uint64_t* Fb, int64_t nb, int64_t nwords, const int* pop_a,
                 const int* pop_b, int k, T* tau) {
  hipStream_t st = ctx().stream;
  if (k < 1 || k > NEIGHBOUR_K_MAX) return fail(SS_EINVAL, "tanimoto kth: k = %d outside 1..%d", k, NEIGHBOUR_K_MAX);
  if (na == 0) return SS_OK;
  if (!Fb) {
    Fb = Fa;
    nb = na;
    pop_b = pop_a;
  }
  if (nb == 0) {
    SS_HIP(hipMemsetAsync(tau, 0, (size_t)na * sizeof(T), st));
    SS_HIP(hipStreamSynchronize(st));
    return SS_OK;
  }
  DevBuf<int> own_a, own_b;
  if (!pop_a) {
    SS_TRY(own_a.alloc(na));
    hipLaunchKernelGGL(fptile::popcount_rows_kernel, dim3((unsigned)ceil_div(na, 256)), dim3(256), 0, st, Fa, na, nwords,
                       own_a.p);
    SS_LAUNCH_CHECK();
    pop_a = own_a.p;
    if (Fb == Fa && nb == na) pop_b = pop_a;
  }
  if (!pop_b) {
    SS_TRY(own_b.alloc(nb));
    hipLaunchKernelGGL(fptile::popcount_rows_kernel, dim3((unsigned)ceil_div(nb, 256)), dim3(256), 0, st, Fb, nb, nwords,
                       own_b.p);
    SS_LAUNCH_CHECK();
    pop_b = own_b.p;
  }

  const int rows = (int64_t)TILE * k * (int64_t)sizeof(T) <= ROW_SELECT_LIST_BYTES ? TILE : TILE / 2;
  if ((int64_t)rows * k * (int64_t)sizeof(T) > ROW_SELECT_LIST_BYTES)
    return fail(SS_EUNSUPPORTED, "tanimoto kth: the lists of %d rows x k = %d do not fit in LDS", rows, k);
  const int64_t ntj = ceil_div(nb, TILE);
  const int64_t row_blocks = ceil_div(na, TILE) * (TILE / rows);
  int64_t groups = 0, tiles_per_group = 0;
  SS_TRY(kth::plan_groups<T>("tanimoto kth", na, ntj, row_blocks, k, groups, tiles_per_group));

  DevBuf<T> part;
  SS_TRY(part.alloc((size_t)groups * (size_t)na * (size_t)k));
  auto* partial = rows == TILE ? tanimoto_kth_partial_kernel<T, TILE, TanimotoSim<T>>
                               : tanimoto_kth_partial_kernel<T, TILE / 2, TanimotoSim<T>>;
  hipLaunchKernelGGL(partial, dim3((unsigned)row_blocks, (unsigned)groups), dim3(256), 0, st, Fa, na, Fb, nb, nwords,
                     pop_a, pop_b, k, ntj, tiles_per_group, part.p, TanimotoSim<T>());
  SS_LAUNCH_CHECK();
  SS_TRY(kth::launch_merge<T>(part.p, na, k, groups, tau, st));
  SS_HIP(hipStreamSynchronize(st));  // part and the popcounts are freed on return
  return SS_OK;
}

template int tanimoto_kth<float>(const uint64_t*, int64_t, const uint64_t*, int64_t, int64_t, const int*, const int*, int,
                                 float*);
template int tanimoto_kth<double>(const uint64_t*, int64_t, const uint64_t*, int64_t, int64_t, const int*, const int*,
                                  int, double*);

}  // namespace ss
