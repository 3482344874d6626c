// What the neighbour-floor selections of the three tiled producers share past their own tile pass (neighbour_floor.hip:
// fingerprints; real_floor.hip: weighted Jaccard and the inner-product similarities): how the column tiles of a row strip
// are cut into column groups, and the merge of the groups' partial lists into tau.
//
//   partial  (the producer's own kernel) block (x, g) leaves the k largest positive values of every row it owns among
//            the columns of group g in part[g][row][0..k), +0 padded
//   merge    one wave per row: the k-th largest of the row's groups * k partial values by rank counting (value v is
//            the answer iff fewer than k values are greater and at least k are greater or equal), which does not
//            depend on the order of the values.
// Scratch: na * k * groups values.  The merge's loops are bounded by groups * k <= 4096 (host-checked); there are no
// spin-waits and no flags between workgroups.
#pragma once
#include <algorithm>
#include <hip/hip_runtime.h>

#include "graph.hpp"

namespace ss {
namespace kth {

constexpr int MAX_GROUPS = 64;                         // column groups: groups * k values per row fit the merge's LDS
constexpr int MERGE_VALUES = MAX_GROUPS * NEIGHBOUR_K_MAX;
constexpr int MIN_GROUP_TILES = 4;                     // a group's first tile fills the lists: not worth less
constexpr int64_t TARGET_BLOCKS = 4096;                // 256 CUs x 3 resident blocks, a few rounds of them
constexpr int64_t MAX_SCRATCH_BYTES = 512LL << 20;

// tau[i] = the k-th largest of part[g][i][0..k), g < groups, when at least k of them are positive, else +0
template <class T>
__global__ void __launch_bounds__(64) kth_merge_kernel(const T* __restrict__ part, int64_t na, int k, int groups,
                                                       T* __restrict__ tau) {
  __shared__ T buf[MERGE_VALUES];
  const int64_t i = blockIdx.x;
  const int lane = threadIdx.x;
  const int n = groups * k;  // <= MERGE_VALUES (host-checked)
  for (int e = lane; e < n; e += 64) {
    const int g = e / k, j = e - g * k;
    buf[e] = part[((int64_t)g * na + i) * k + j];
  }
  __syncthreads();
  T found = T(0);
  for (int e = lane; e < n; e += 64) {
    const T v = buf[e];
    if (!(v > T(0))) continue;
    int gt = 0, ge = 0;
    for (int x = 0; x < n; ++x) {
      const T w = buf[x];
      gt += w > v ? 1 : 0;
      ge += w >= v ? 1 : 0;
    }
    if (gt < k && ge >= k) found = v;  // every lane that finds one finds the same value
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    const T o = __shfl_xor(found, off);
    found = o > found ? o : found;
  }
  if (lane == 0) tau[i] = found;
}

// The column groups of a selection whose row strips take row_blocks blocks: enough groups to fill the device when the
// rows alone do not, none below MIN_GROUP_TILES tiles, none empty.  SS_EUNSUPPORTED when a launch or the merge buffer
// cannot hold the result.
template <class T>
inline int plan_groups(const char* what, int64_t na, int64_t ntj, int64_t row_blocks, int k, int64_t& groups,
                       int64_t& tiles_per_group) {
  if (row_blocks >= (1LL << 31))
    return fail(SS_EUNSUPPORTED, "%s: %lld rows need more blocks than one launch holds", what, (long long)na);
  groups = ceil_div(TARGET_BLOCKS, row_blocks);
  groups = std::min<int64_t>(groups, ceil_div(ntj, MIN_GROUP_TILES));
  groups = std::min<int64_t>(groups, MAX_GROUPS);
  groups = std::min<int64_t>(groups, MAX_SCRATCH_BYTES / (na * k * (int64_t)sizeof(T)));
  groups = std::max<int64_t>(groups, 1);
  tiles_per_group = ceil_div(ntj, groups);
  groups = ceil_div(ntj, tiles_per_group);  // no empty group
  if (groups * k > MERGE_VALUES)
    return fail(SS_EUNSUPPORTED, "%s: %lld column groups x k = %d exceed the merge buffer", what, (long long)groups, k);
  return SS_OK;
}

// enqueue the merge of part[groups][na][k] into tau[na]
template <class T>
inline int launch_merge(const T* part, int64_t na, int k, int64_t groups, T* tau, hipStream_t st) {
  hipLaunchKernelGGL(kth_merge_kernel<T>, dim3((unsigned)na), dim3(64), 0, st, part, na, k, (int)groups, tau);
  SS_LAUNCH_CHECK();
  return SS_OK;
}

}  // namespace kth
}  // namespace ss
