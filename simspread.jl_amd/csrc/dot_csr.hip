// Thresholded inner-product similarities (cosine, real-valued Tanimoto, Dice) of real-valued rows, produced straight as
// CSR: featurize's cutoff (src/core.jl:106-112) applied to the similarity of every pair of rows, without the dense
// n x n similarity ever existing.  For row i of Fa and row j of Fb:
//
//   g = sum_k a_k b_k, A = sum_k a_k^2, B = sum_k b_k^2, accumulated in T.  The order of summation is the
//   implementation's own (the matrix cores choose it for g); nothing below depends on it.
//   Everything after the three sums is fixed, in T, with correctly rounded sqrt, *, / (no fast-math):
//     SS_SIM_COSINE    den = sqrt(A) * sqrt(B)   s = clamp(g / den, -1, 1)
//     SS_SIM_TANIMOTO  den = (A + B) - g         s = g / den
//     SS_SIM_DICE      den = A + B               s = (g + g) / den
//     den == 0:        s = (A == 0 && B == 0) ? 1 : 0     (two all-zero rows are identical, as in jaccard_csr.hip and
//                                                          fingerprint.hip; d == 0 therefore gives s = 1 everywhere)
//   symmetric mode (Fb == NULL): entry (i, i) has s = 1 exactly, entry (j, i) carries the bits of (i, j)
//   keep (i, j) iff s >= alpha and v != 0 with v = weighted ? s : 1     (keep_entry of assemble.hip; a NaN s, which
//                                                                        only infinite features give, is dropped)
//   s of a pair does not depend on alpha, weighted, the pass (count or fill) or the run.
//
// When every product and every partial sum is exactly representable in T (small-integer features, say), g, A and B are
// exact whatever the order, and the CSR is then bitwise defined by the rule above.  NaN features are refused before
// anything is written.
//
// Two passes over 128 x 128 tiles of (row, column) pairs; which tile a block owns and the symmetric mode are
// pair_tile.hpp, the host side PairCsr (pair_csr.hip):
//   count  per (column tile, row): the number of kept entries -> counts[jt * rows + i]; per tile: any kept -> tile_nz
//   fill   the tiles that kept something, again, each slot written at ptr[i] + its offset in column order.
// A tile's Gram block runs on the matrix cores in full T precision: v_mfma_f32_32x32x2_f32 (a wave owns 2 x 2 MFMA tiles
// of 32 x 32) or v_mfma_f64_16x16x4_f64 (4 x 4 tiles of 16 x 16); 4 waves as 2 x 2, operands staged through LDS in
// [BK][TILE] steps from the column-major features, padded k and padded rows loaded as 0.  The epilogue turns the
// accumulators into s in place; the kept pairs of a tile become bit rows in LDS (one wave ballot per accumulator
// register, no atomics), and counts and in-row offsets are popcounts of those.  In symmetric mode only the tiles on and
// above the diagonal run; an off-diagonal tile emits its pairs for its rows and, mirrored, for its columns.
#include <algorithm>
#include <hip/hip_runtime.h>

#include "graph.hpp"
#include "pair_tile.hpp"

namespace ss {

namespace {

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

// N[i] = sum_k F[i, k]^2 in T, one thread per row (consecutive threads read consecutive rows of a column)
template <class T>
__global__ void row_norm_kernel(const T* __restrict__ F, int64_t n, int64_t ld, int64_t d, T* __restrict__ N) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  T s = T(0);
  for (int64_t k = 0; k < d; ++k) {
    const T x = F[i + k * ld];
    s += x * x;
  }
  N[i] = s;
}

// MT bits of a 128-bit row of the tile's bit matrices: piece p = bits MT * p .. MT * p + MT - 1
template <int MT>
__device__ __forceinline__ void put_bits(uint32_t (*m)[4], int r, int p, uint32_t bits) {
  if (MT == 32) m[r][p] = bits;
  else reinterpret_cast<uint16_t*>(&m[r][0])[p] = (uint16_t)bits;
}
// set bits of m[r] below position c
__device__ __forceinline__ int bits_before(const uint32_t (*m)[4], int r, int c) {
  int n = __popc(m[r][c >> 5] & ((1u << (c & 31)) - 1u));
  for (int w = 0; w < (c >> 5); ++w) n += __popc(m[r][w]);
  return n;
}

// FILL == false: write the per-(tile, row) counts and the tile flag.  FILL == true: write the entries of the tiles that
// kept something (counts then hold in-row offsets).
template <class T, bool SYM, bool FILL>
__global__ void __launch_bounds__(NT) dot_tile_kernel(
    const T* __restrict__ Fa, int64_t na, int64_t lda, const T* __restrict__ Fb, int64_t nb, int64_t ldb, int64_t d,
    const T* __restrict__ norm_a, const T* __restrict__ norm_b, int metric, T alpha, int weighted, int64_t nti,
    int* __restrict__ counts, int* __restrict__ tile_nz, const int64_t* __restrict__ ptr, int* __restrict__ oidx,
    T* __restrict__ oval, int* __restrict__ not_binary) {
  using M = Mma<T>;
  constexpr int MT = M::MT, KS = M::KS, NR = M::NR;
  constexpr int NM = WT / MT;          // MFMA tiles per wave edge
  constexpr int LDT = TILE + M::PAD;
  static_assert(NM * NM * NR == 64, "one kept bit per accumulator register in a 64-bit mask");
  __shared__ __attribute__((aligned(16))) T As[BK][LDT];
  __shared__ __attribute__((aligned(16))) T Bs[BK][LDT];
  __shared__ T na_s[TILE], nb_s[TILE];  // sqrt(A), sqrt(B) (cosine) or A, B of the tile's rows and columns
  __shared__ uint32_t rowbits[TILE][4];  // [row]: bit c = pair (row, c) is kept
  __shared__ uint32_t colbits[TILE][4];  // [column]: bit r = pair (r, column) is kept (SYM, off-diagonal tiles)

  if (FILL && tile_nz[pair_tile_index<SYM>()] == 0) return;  // uniform over the block
  const PairTile t = pair_tile<SYM, TILE>(nti);
  const int64_t tlin = t.tlin, it = t.it, jt = t.jt, i0 = t.i0, j0 = t.j0;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave >> 1, wn = wave & 1;
  const bool mirror = t.mirror;

  typename M::acc_t acc[NM][NM];
#pragma unroll
  for (int i = 0; i < NM; ++i)
#pragma unroll
    for (int j = 0; j < NM; ++j)
#pragma unroll
      for (int r = 0; r < NR; ++r) acc[i][j][r] = T(0);

  // staging: BK feature columns of the tile's 128 rows of each side; consecutive threads read consecutive rows of one
  // column (coalesced).  Past d or past the last row the value is 0: a padded k adds a zero product, and padded rows /
  // columns are masked below.
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
      T av[NM], bv[NM];
#pragma unroll
      for (int i = 0; i < NM; ++i) av[i] = As[kr][wm * WT + i * MT + c];
#pragma unroll
      for (int j = 0; j < NM; ++j) bv[j] = Bs[kr][wn * WT + j * MT + c];
#pragma unroll
      for (int i = 0; i < NM; ++i)
#pragma unroll
        for (int j = 0; j < NM; ++j) acc[i][j] = M::mma(av[i], bv[j], acc[i][j]);
    }
    __syncthreads();
  }

  if (tid < TILE) {
    const T x = i0 + tid < na ? norm_a[i0 + tid] : T(0);
    na_s[tid] = metric == SS_SIM_COSINE ? sqrt(x) : x;
  } else {
    const int r = tid - TILE;
    const T x = j0 + r < nb ? norm_b[j0 + r] : T(0);
    nb_s[r] = metric == SS_SIM_COSINE ? sqrt(x) : x;
  }
  __syncthreads();

  // acc becomes v in place; bit (i * NM + j) * NR + r of kept = this lane's pair of register r of MFMA tile (i, j)
  uint64_t kept = 0;
  const bool wgt = weighted != 0;
  const int cl = lane % MT;
#pragma unroll
  for (int i = 0; i < NM; ++i)
#pragma unroll
    for (int j = 0; j < NM; ++j) {
      const int col = wn * WT + j * MT + cl;
      const T cb = nb_s[col];
      uint32_t cm = 0;
#pragma unroll
      for (int r = 0; r < NR; ++r) {
        const int row = wm * WT + i * MT + M::row(r, lane);
        T s = dot_sim<T>(acc[i][j][r], na_s[row], cb, metric);
        if (SYM && i0 + row == j0 + col) s = T(1);
        const T v = wgt ? s : T(1);
        const bool k = i0 + row < na && j0 + col < nb && s >= alpha && v != T(0);
        acc[i][j][r] = v;
        kept |= (uint64_t)(k ? 1 : 0) << ((i * NM + j) * NR + r);
        cm |= (k ? 1u : 0u) << M::row(r, lane);
        // the wave's lanes hold 64 / MT rows x MT columns of this register: one ballot is MT bits of each of those rows
        const uint64_t b = __ballot(k);
        if (cl == 0) put_bits<MT>(rowbits, row, (wn * WT + j * MT) / MT, (uint32_t)(b >> (lane & (64 - MT))));
      }
      if (mirror) {
        // the lanes l, l + MT, ... hold the rows of column l between them
#pragma unroll
        for (int o = MT; o < 64; o <<= 1) cm |= __shfl_xor(cm, o);
        if (lane < MT) put_bits<MT>(colbits, col, (wm * WT + i * MT) / MT, cm);
      }
    }
  const bool any = __syncthreads_or(kept != 0);
  if (!FILL) {
    if (tid == 0) tile_nz[tlin] = any ? 1 : 0;
    if (tid < TILE) {
      if (i0 + tid < na)
        counts[jt * na + i0 + tid] =
            __popc(rowbits[tid][0]) + __popc(rowbits[tid][1]) + __popc(rowbits[tid][2]) + __popc(rowbits[tid][3]);
    } else if (mirror) {
      const int r = tid - TILE;
      if (j0 + r < nb)  // SYM: na == nb
        counts[it * na + j0 + r] =
            __popc(colbits[r][0]) + __popc(colbits[r][1]) + __popc(colbits[r][2]) + __popc(colbits[r][3]);
    }
    return;
  }

  bool nb_flag = false;
#pragma unroll
  for (int i = 0; i < NM; ++i)
#pragma unroll
    for (int j = 0; j < NM; ++j) {
      const int col = wn * WT + j * MT + cl;
#pragma unroll
      for (int r = 0; r < NR; ++r) {
        if (!((kept >> ((i * NM + j) * NR + r)) & 1)) continue;
        const int row = wm * WT + i * MT + M::row(r, lane);
        const T v = acc[i][j][r];
        const int64_t gi = i0 + row, gj = j0 + col;
        const int64_t o = ptr[gi] + counts[jt * na + gi] + bits_before(rowbits, row, col);
        oidx[o] = (int)gj;
        if (oval) oval[o] = v;
        nb_flag |= (v != T(1));
        if (mirror) {
          const int64_t om = ptr[gj] + counts[it * na + gj] + bits_before(colbits, col, row);
          oidx[om] = (int)gi;
          if (oval) oval[om] = v;
        }
      }
    }
  if (nb_flag) *not_binary = 1;
}

}  // namespace

template <class T>
int DotCsr<T>::count(const T* Fa_, int64_t na_, int64_t lda_, const T* Fb_, int64_t nb_, int64_t ldb_, int64_t d_,
                     int metric_, T alpha_, bool weighted_) {
  hipStream_t st = ctx().stream;
  what = "dot_csr";
  sym = (Fb_ == nullptr);
  Fa = Fa_;
  Fb = sym ? Fa_ : Fb_;
  lda = lda_;
  ldb = sym ? lda_ : ldb_;
  d = d_;
  metric = metric_;
  alpha = alpha_;
  weighted = weighted_;
  if (metric != SS_SIM_COSINE && metric != SS_SIM_TANIMOTO && metric != SS_SIM_DICE)
    return fail(SS_EINVAL, "dot_csr: unknown metric %d", metric);
  if (alpha != alpha) return fail(SS_EINVAL, "dot_csr: alpha is NaN");
  SS_TRY(this->refuse_nan_features(Fa, na_, lda, Fb, nb_, ldb, d));
  SS_TRY(this->begin_tiles(na_, sym ? na_ : nb_, TILE, true));
  if (na == 0 || nb == 0) return SS_OK;
  SS_TRY(norm_a.alloc((size_t)na));
  hipLaunchKernelGGL(row_norm_kernel<T>, dim3((unsigned)ceil_div(na, 256)), dim3(256), 0, st, Fa, na, lda, d, norm_a.p);
  SS_LAUNCH_CHECK();
  if (!sym) {
    SS_TRY(norm_b.alloc((size_t)nb));
    hipLaunchKernelGGL(row_norm_kernel<T>, dim3((unsigned)ceil_div(nb, 256)), dim3(256), 0, st, Fb, nb, ldb, d,
                       norm_b.p);
    SS_LAUNCH_CHECK();
  }
  return this->count_pass();
}

template <class T>
int DotCsr<T>::launch(bool fill, int* idx, T* val, int* flag) {
  auto* kernel = sym ? (fill ? dot_tile_kernel<T, true, true> : dot_tile_kernel<T, true, false>)
                     : (fill ? dot_tile_kernel<T, false, true> : dot_tile_kernel<T, false, false>);
  hipLaunchKernelGGL(kernel, this->tile_grid(), dim3(NT), 0, ctx().stream, Fa, na, lda, Fb, nb, ldb, d, norm_a.p,
                     sym ? norm_a.p : norm_b.p, metric, alpha, weighted ? 1 : 0, nti, counts.p, tile_nz.p, ptr.p, idx,
                     val, flag);
  SS_LAUNCH_CHECK();
  return SS_OK;
}

template struct DotCsr<float>;
template struct DotCsr<double>;

}  // namespace ss
