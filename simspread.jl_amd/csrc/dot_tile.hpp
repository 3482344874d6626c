// What the kernels over real-valued rows under an inner-product similarity share (dot_csr.hip: the thresholded CSR
// producer; real_floor.hip: the k-th largest similarity of every row): the tile shape, the matrix instruction of each
// precision and where its results lie, the staging and the MFMA sequence of one 128 x 128 Gram tile, the squared row
// norms, and THE expression of the pair similarity.  A selection pass and an emit pass that must agree bit for bit on
// s(i, j) both call dot_tile_gram(), stage_norms() and dot_pair_sim(): the same staging steps, the same MFMAs in the
// same k order, the same epilogue.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "simspread_hip.h"

namespace ss {
namespace dottile {

constexpr int TILE = 128;  // rows and columns per workgroup tile
constexpr int BK = 16;     // feature columns staged per step
constexpr int NT = 256;    // 4 waves as 2 x 2, a wave owns 64 x 64 pairs
constexpr int WT = 64;     // rows and columns per wave

using f32x16 = __attribute__((ext_vector_type(16))) float;
using f64x4 = __attribute__((ext_vector_type(4))) double;

// The matrix instruction of T: MT x MT results per instruction from KS feature columns, NR results per lane.
// Operands: lane l holds A[l % MT][l / MT] and B[l / MT][l % MT].  Result register r of lane l is the pair
// (row(r, l), l % MT) of the MFMA tile.
template <class T>
struct Mma;
template <>
struct Mma<float> {
  static constexpr int MT = 32, KS = 2, NR = 16;
  static constexpr int PAD = 0;  // ds_read_b32 serves 32 lanes per cycle: 32 consecutive floats never conflict
  using acc_t = f32x16;
  static __device__ __forceinline__ acc_t mma(float a, float b, acc_t c) {
    return __builtin_amdgcn_mfma_f32_32x32x2f32(a, b, c, 0, 0, 0);
  }
  static __device__ __forceinline__ int row(int r, int lane) { return (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5); }
};
template <>
struct Mma<double> {
  static constexpr int MT = 16, KS = 4, NR = 4;
  static constexpr int PAD = 16;  // ds_read_b64 serves 32 lanes = two k rows per cycle: the rows go to opposite bank halves
  using acc_t = f64x4;
  static __device__ __forceinline__ acc_t mma(double a, double b, acc_t c) {
    return __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, c, 0, 0, 0);
  }
  static __device__ __forceinline__ int row(int r, int lane) { return (lane >> 4) + 4 * r; }
};

template <class T>
constexpr int NM = WT / Mma<T>::MT;  // MFMA tiles per wave edge
template <class T>
constexpr int LDT = TILE + Mma<T>::PAD;  // leading dimension of the staged operands

// the rule after the three sums; ra, rb: sqrt(A), sqrt(B) for the cosine, A, B otherwise
template <class T>
__device__ __forceinline__ T dot_sim(T g, T ra, T rb, int metric) {
#pragma clang fp contract(off)
  T num = g, den;
  if (metric == SS_SIM_COSINE) {
    den = ra * rb;
  } else if (metric == SS_SIM_TANIMOTO) {
    den = (ra + rb) - g;
  } else {
    den = ra + rb;
    num = g + g;
  }
  if (den == T(0)) return (ra == T(0) && rb == T(0)) ? T(1) : T(0);  // sqrt(A) == 0 iff A == 0
  T s = num / den;
  if (metric == SS_SIM_COSINE) s = s < T(-1) ? T(-1) : (s > T(1) ? T(1) : s);  // a NaN stays a NaN
  return s;
}

// s of one pair from its Gram value and the staged norms; diag: the pair is (i, i) of a block against itself, s = 1
template <class T>
__device__ __forceinline__ T dot_pair_sim(T g, T ra, T rb, int metric, bool diag) {
  const T s = dot_sim<T>(g, ra, rb, metric);
  return diag ? T(1) : s;
}

// N[i] = sum_k F[i, k]^2 in T, one thread per row (consecutive threads read consecutive rows of a column)
template <class T>
static __global__ void row_norm_kernel(const T* __restrict__ F, int64_t n, int64_t ld, int64_t d, T* __restrict__ N) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  T s = T(0);
  for (int64_t k = 0; k < d; ++k) {
    const T x = F[i + k * ld];
    s += x * x;
  }
  N[i] = s;
}

// out[r] = sqrt(N) (cosine) or N of row r0 + r, 0 past the last row: what dot_sim takes as ra / rb.  One thread per row.
template <class T>
__device__ __forceinline__ void stage_norm(T* out, int r, const T* __restrict__ norm, int64_t r0, int64_t n,
                                           int metric) {
  const T x = r0 + r < n ? norm[r0 + r] : T(0);
  out[r] = metric == SS_SIM_COSINE ? sqrt(x) : x;
}

// acc[i][j] = the Gram block of MFMA tile (i, j) of the calling wave: rows i0 + wm*WT + i*MT .. of Fa against rows
// j0 + wn*WT + j*MT .. of Fb, (wm, wn) = (wave >> 1, wave & 1), for the NT threads of a block; rows past na / nb count
// as zero rows (the caller masks them).  Every thread of the block must call it (it synchronises).  The staging buffers
// are the function's own LDS (2 x BK x LDT values: 16 KiB in fp32, 36 KiB in fp64), declared here and not handed in by
// the caller, so that the compiler knows them as LDS from the start (see jaccard_tile.hpp).
constexpr int gram_lds_bytes(int size_of_t, int ldt) { return 2 * BK * ldt * size_of_t; }
template <class T>
__device__ __forceinline__ void dot_tile_gram(const T* __restrict__ Fa,
                                              int64_t na, int64_t lda, const T* __restrict__ Fb, int64_t nb,
                                              int64_t ldb, int64_t d, int64_t i0, int64_t j0,
                                              typename Mma<T>::acc_t (&acc)[NM<T>][NM<T>]) {
  using M = Mma<T>;
  constexpr int MT = M::MT, KS = M::KS, NR = M::NR, NMM = NM<T>;
  __shared__ __attribute__((aligned(16))) T As[BK][LDT<T>];
  __shared__ __attribute__((aligned(16))) T Bs[BK][LDT<T>];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave >> 1, wn = wave & 1;
#pragma unroll
  for (int i = 0; i < NMM; ++i)
#pragma unroll
    for (int j = 0; j < NMM; ++j)
#pragma unroll
      for (int r = 0; r < NR; ++r) acc[i][j][r] = T(0);

  // staging: BK feature columns of the tile's 128 rows of each side; consecutive threads read consecutive rows of one
  // column (coalesced).  Past d or past the last row the value is 0: a padded k adds a zero product, and padded rows /
  // columns are masked by the caller.
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
    if (k0 + BK < d) load(k0 + BK);  // the next step's loads are in flight during this step's matrix work
#pragma unroll
    for (int kk = 0; kk < BK; kk += KS) {
      const int kr = kk + lane / MT, c = lane % MT;
      T av[NMM], bv[NMM];
#pragma unroll
      for (int i = 0; i < NMM; ++i) av[i] = As[kr][wm * WT + i * MT + c];
#pragma unroll
      for (int j = 0; j < NMM; ++j) bv[j] = Bs[kr][wn * WT + j * MT + c];
#pragma unroll
      for (int i = 0; i < NMM; ++i)
#pragma unroll
        for (int j = 0; j < NMM; ++j) acc[i][j] = M::mma(av[i], bv[j], acc[i][j]);
    }
    __syncthreads();
  }
}

}  // namespace dottile
}  // namespace ss
