// What the kernels over packed binary fingerprints share (fingerprint.hip: the thresholded CSR producer;
// neighbour_floor.hip: the k-th largest similarity of every row): the tile shape, the row popcounts, the staging and
// AND-popcount loop of one 128 x 128 tile, and THE expression of the pair similarity.  A selection pass and an emit pass
// that must agree bit for bit on s(i, j) both call tanimoto_similarity().
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace ss {
namespace fptile {

constexpr int TILE = 128;  // rows and columns per workgroup tile
constexpr int BK = 16;     // 32-bit fingerprint words staged per step (8 uint64 words)
constexpr int RB = 8;      // rows / columns per thread

static __global__ void popcount_rows_kernel(const uint64_t* __restrict__ F, int64_t n, int64_t nwords,
                                            int* __restrict__ pop) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const uint64_t* row = F + i * nwords;
  int c = 0;
  for (int64_t w = 0; w < nwords; ++w) c += __popcll(row[w]);
  pop[i] = c;
}

// c = popcount(a & b), pa / pb the popcounts of the two rows: exact integer counts, one correctly rounded division
template <class T>
__device__ __forceinline__ T tanimoto_similarity(int c, int pa, int pb) {
  const int u = pa + pb - c;
  return u == 0 ? T(1) : T(c) / T(u);
}

// acc[a][b] = popcount(Fa[i0 + RB*ty + a] & Fb[j0 + RB*tx + b]) for the 256 threads (tx, ty) = (tid & 15, tid >> 4) of
// a block; rows past na / nb count as zero rows.  Every thread of the block must call it (it synchronises); As and Bs
// are free again when it returns.
__device__ __forceinline__ void tanimoto_tile_counts(uint32_t (&As)[BK][TILE], uint32_t (&Bs)[BK][TILE],
                                                     const uint64_t* __restrict__ Fa, int64_t na,
                                                     const uint64_t* __restrict__ Fb, int64_t nb, int64_t nwords,
                                                     int64_t i0, int64_t j0, uint32_t (&acc)[RB][RB]) {
  const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
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
}

}  // namespace fptile
}  // namespace ss
