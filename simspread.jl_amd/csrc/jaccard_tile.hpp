// What the kernels over real-valued feature rows under weighted Jaccard share (jaccard_csr.hip: the thresholded CSR
// producer; real_floor.hip: the k-th largest similarity of every row): the tile shape, the staging and the min / max
// sums of one 128 x 128 tile, and THE expression of the pair similarity.  A selection pass and an emit pass that must
// agree bit for bit on s(i, j) both call jaccard_tile_sums() and jaccard_similarity().
//
//   smin = smax = +0; for k = 0 .. d-1 in order, in T: smin += min(a_k, b_k), smax += max(a_k, b_k)
//   s = smax == 0 ? 1 : smin / smax                                          (one correctly rounded division in T)
//
// Register blocks: fp32 8 x 8 pairs per thread (256 threads, 128 accumulator VGPRs), fp64 4 x 8 (512 threads, the
// same 128 VGPRs).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace ss {
namespace jctile {

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

template <class T>
constexpr int threads() {
  return NTX * (TILE / Block<T>::RA);
}

__device__ __forceinline__ float vmin(float a, float b) { return __builtin_fminf(a, b); }
__device__ __forceinline__ float vmax(float a, float b) { return __builtin_fmaxf(a, b); }
__device__ __forceinline__ double vmin(double a, double b) { return __builtin_fmin(a, b); }
__device__ __forceinline__ double vmax(double a, double b) { return __builtin_fmax(a, b); }

template <class T>
__device__ __forceinline__ T jaccard_similarity(T smin, T smax) {
  return smax == T(0) ? T(1) : smin / smax;
}

// (smin, smax) of one pair: the two sums sit in adjacent registers, so that fp32 adds them with one v_pk_add_f32
// (lane-wise, each lane one correctly rounded add -- the same two adds)
template <class T>
using Sums = T __attribute__((ext_vector_type(2)));

// acc[a][b] = (smin, smax) of rows i0 + RA*ty + a of Fa and j0 + RC*tx + b of Fb for the threads (tx, ty) =
// (tid % NTX, tid / NTX) of a block of threads<T>(); rows past na / nb count as zero rows (the caller masks them).
// Every thread of the block must call it (it synchronises).  The staging buffers are the function's own LDS (32 bytes
// per row and staged column of either side: 16 KiB in fp32, 32 KiB in fp64), declared here and not handed in by the
// caller: through a reference parameter the compiler sees them as generic pointers until late, which costs the plain
// producer a fifth more registers and, in fp64, scratch.
template <class T>
__device__ __forceinline__ void jaccard_tile_sums(const T* __restrict__ Fa,
                                                  int64_t na, int64_t lda, const T* __restrict__ Fb, int64_t nb,
                                                  int64_t ldb, int64_t d, int64_t i0, int64_t j0,
                                                  Sums<T> (&acc)[Block<T>::RA][RC]) {
  constexpr int RA = Block<T>::RA;
  constexpr int NT = threads<T>();
  __shared__ __attribute__((aligned(16))) T As[BK][TILE];
  __shared__ __attribute__((aligned(16))) T Bs[BK][TILE];
  const int tid = threadIdx.x, tx = tid % NTX, ty = tid / NTX;
#pragma unroll
  for (int a = 0; a < RA; ++a)
#pragma unroll
    for (int b = 0; b < RC; ++b) acc[a][b] = Sums<T>{T(0), T(0)};

  // staging: BK feature columns of the tile's 128 rows of each side; consecutive threads read consecutive rows of one
  // column (coalesced).  Past d or past the last row the value is 0: a padded k adds +0 to both sums, which changes
  // nothing, and padded rows / columns are masked by the caller.
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
        for (int b = 0; b < RC; ++b) acc[a][b] += Sums<T>{vmin(av[a], bv[b]), vmax(av[a], bv[b])};
    }
    __syncthreads();
  }
}

}  // namespace jctile
}  // namespace ss
