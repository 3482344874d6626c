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
//
// This file holds what is the producer's own: the keep rule, the bit-row epilogue and the host side.  The staging, the
// MFMA sequence, the norms and the expression of s are dot_tile.hpp, shared with the selection pass of the neighbour
// floor (real_floor.hip): with k > 0, count() first asks it for tau[na], the k-th largest positive similarity of every
// row, and the tile kernel keeps (i, j) iff v != 0 and (s >= alpha or (s > 0 and s >= tau[i])).  That rule is not
// symmetric, so the floor case runs the full (ntj, nti) grid with Fb = Fa instead of the triangle; its diagonal is
// still exactly 1, and every other pair is what the cross producer computes for (i, j).
//
// 16-bit rows (DotCsrH16, include/simspread_hip_half.h): the same kernel with the operand type as a template parameter.
// The rows are raw bf16 / fp16 patterns, ROW-MAJOR; the Gram block is dot_tile_gram_h16 (dot_tile_h16.hpp) on
// v_mfma_f32_32x32x16_{bf16,f16}, whose products are exact in fp32 and whose results lie in the accumulator registers
// exactly as the fp32 instruction's do, so everything from the norms on is the text below with T = float.
//
// int8 rows (DotCsrI8, include/simspread_hip_int8.h): the operand tag dottile::I8.  The Gram block is dot_tile_gram_i8
// (dot_tile_i8.hpp) on v_mfma_i32_32x32x32_i8: g is an exact int32, converted to fp32 once, and the norms are (float) of
// exact integer sums, so s is a pure function of the two rows and the CSR is bitwise defined for every input.  The
// selection pass of the neighbour floor runs the same Gram tile (dot_kth_i8 of real_floor.hip), so this operand, unlike
// the 16-bit ones, has the per-row cut.
#include <algorithm>
#include <hip/hip_runtime.h>

#include "dot_tile.hpp"
#include "dot_tile_h16.hpp"
#include "dot_tile_i8.hpp"
#include "graph.hpp"
#include "pair_tile.hpp"

namespace ss {

namespace {

using dottile::Mma;
using dottile::NT;
using dottile::row_norm_kernel;
using dottile::TILE;
using dottile::WT;

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
// FLOOR: the per-row cut tau[na] next to alpha; a pair is then decided by its row alone, so there is no mirror (!SYM);
// flags & TILE_SELF: Fb is Fa, so the pairs (i, i) have s = 1 as in the symmetric mode.
// Op: the operands.  Op == T: column-major rows of T, dot_tile_gram.  dottile::Bf16 / dottile::F16 (T == float): row-major
// 16-bit patterns, dot_tile_gram_h16, with flags & TILE_FAST_A / TILE_FAST_B allowing a side its 16-byte loads.
// dottile::I8 (T == float): row-major int8, dot_tile_gram_i8, the same flags; the only tagged operand with FLOOR.  The
// accumulators come out in the same registers either way, so everything after the Gram block is one text.
enum { TILE_SELF = 1, TILE_FAST_A = 2, TILE_FAST_B = 4 };
template <class Op>
struct OperandElem { using type = typename Op::elem; };
template <>
struct OperandElem<float> { using type = float; };
template <>
struct OperandElem<double> { using type = double; };

template <class T, bool SYM, bool FILL, bool FLOOR, class Op = T>
__global__ void __launch_bounds__(NT) dot_tile_kernel(
    const typename OperandElem<Op>::type* __restrict__ Fa, int64_t na, int64_t lda,
    const typename OperandElem<Op>::type* __restrict__ Fb, int64_t nb, int64_t ldb, int64_t d,
    const T* __restrict__ norm_a, const T* __restrict__ norm_b, int metric, T alpha, const T* __restrict__ tau, int flags,
    int weighted, int64_t nti, int* __restrict__ counts, int* __restrict__ tile_nz, const int64_t* __restrict__ ptr,
    int* __restrict__ oidx, T* __restrict__ oval, int* __restrict__ not_binary) {
  static_assert(!(SYM && FLOOR), "a per-row cut decides (i, j) and (j, i) separately");
  static_assert(std::is_same<Op, T>::value ||
                    (std::is_same<T, float>::value && (!FLOOR || std::is_same<Op, dottile::I8>::value)),
                "16-bit and int8 operands: fp32 graphs; a per-row cut with int8 only");
  using M = Mma<T>;
  constexpr int MT = M::MT, NR = M::NR;
  constexpr int NM = dottile::NM<T>;   // MFMA tiles per wave edge
  static_assert(NM * NM * NR == 64, "one kept bit per accumulator register in a 64-bit mask");
  __shared__ T na_s[TILE], nb_s[TILE];  // sqrt(A), sqrt(B) (cosine) or A, B of the tile's rows and columns
  __shared__ T tau_s[FLOOR ? TILE : 1];  // FLOOR: the cut of the tile's rows
  __shared__ uint32_t rowbits[TILE][4];  // [row]: bit c = pair (row, c) is kept
  __shared__ uint32_t colbits[TILE][4];  // [column]: bit r = pair (r, column) is kept (SYM, off-diagonal tiles)

  if (FILL && tile_nz[pair_tile_index<SYM>()] == 0) return;  // uniform over the block
  const PairTile t = pair_tile<SYM, TILE>(nti);
  const int64_t tlin = t.tlin, it = t.it, jt = t.jt, i0 = t.i0, j0 = t.j0;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave >> 1, wn = wave & 1;
  const bool mirror = t.mirror;
  const bool diag1 = SYM || (FLOOR && (flags & TILE_SELF) != 0);  // the block is a set against itself: s(i, i) = 1

  typename M::acc_t acc[NM][NM];
  if constexpr (std::is_same<Op, T>::value)
    dottile::dot_tile_gram<T>(Fa, na, lda, Fb, nb, ldb, d, i0, j0, acc);
  else if constexpr (std::is_same<Op, dottile::I8>::value)
    dottile::dot_tile_gram_i8(Fa, na, lda, Fb, nb, ldb, d, i0, j0, (flags & TILE_FAST_A) != 0, (flags & TILE_FAST_B) != 0,
                              acc);
  else
    dottile::dot_tile_gram_h16<Op>(Fa, na, lda, Fb, nb, ldb, d, i0, j0, (flags & TILE_FAST_A) != 0,
                                   (flags & TILE_FAST_B) != 0, acc);

  if (tid < TILE) {
    dottile::stage_norm<T>(na_s, tid, norm_a, i0, na, metric);
    if constexpr (FLOOR) tau_s[tid] = i0 + tid < na ? tau[i0 + tid] : T(0);
  } else {
    dottile::stage_norm<T>(nb_s, tid - TILE, norm_b, j0, nb, metric);
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
        const T s = dottile::dot_pair_sim<T>(acc[i][j][r], na_s[row], cb, metric, diag1 && i0 + row == j0 + col);
        const T v = wgt ? s : T(1);
        bool k = i0 + row < na && j0 + col < nb && v != T(0);
        if constexpr (FLOOR) k = k && (s >= alpha || (s > T(0) && s >= tau_s[row]));
        else k = k && s >= alpha;
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
int dot_row_norms(const T* F, int64_t n, int64_t ld, int64_t d, T* norm) {
  hipLaunchKernelGGL(row_norm_kernel<T>, dim3((unsigned)ceil_div(n, 256)), dim3(256), 0, ctx().stream, F, n, ld, d, norm);
  SS_LAUNCH_CHECK();
  return SS_OK;
}

template <class T>
int DotCsr<T>::count(const T* Fa_, int64_t na_, int64_t lda_, const T* Fb_, int64_t nb_, int64_t ldb_, int64_t d_,
                     int metric_, T alpha_, bool weighted_, int k) {
  what = "dot_csr";
  self = (Fb_ == nullptr);
  sym = self;
  Fa = Fa_;
  Fb = self ? Fa_ : Fb_;
  lda = lda_;
  ldb = self ? lda_ : ldb_;
  d = d_;
  metric = metric_;
  alpha = alpha_;
  weighted = weighted_;
  tau = nullptr;
  if (metric != SS_SIM_COSINE && metric != SS_SIM_TANIMOTO && metric != SS_SIM_DICE)
    return fail(SS_EINVAL, "dot_csr: unknown metric %d", metric);
  if (alpha != alpha) return fail(SS_EINVAL, "dot_csr: alpha is NaN");
  SS_TRY(this->refuse_nan_features(Fa, na_, lda, Fb, nb_, ldb, d));
  sym = self && k == 0;  // a per-row cut has no mirror: the full grid
  SS_TRY(this->begin_tiles(na_, self ? na_ : nb_, TILE, true));
  if (na == 0 || nb == 0) return SS_OK;
  SS_TRY(norm_a.alloc((size_t)na));
  SS_TRY(dot_row_norms<T>(Fa, na, lda, d, norm_a.p));
  if (!self) {
    SS_TRY(norm_b.alloc((size_t)nb));
    SS_TRY(dot_row_norms<T>(Fb, nb, ldb, d, norm_b.p));
  }
  if (k > 0) {
    SS_TRY(tau_buf.alloc(na));
    SS_TRY(dot_kth<T>(Fa, na, lda, self ? nullptr : Fb, nb, ldb, d, metric, norm_a.p, self ? norm_a.p : norm_b.p, k,
                      tau_buf.p));
    tau = tau_buf.p;
  }
  return this->count_pass();
}

template <class T>
int DotCsr<T>::launch(bool fill, int* idx, T* val, int* flag) {
  auto* kernel = tau   ? (fill ? dot_tile_kernel<T, false, true, true> : dot_tile_kernel<T, false, false, true>)
                 : sym ? (fill ? dot_tile_kernel<T, true, true, false> : dot_tile_kernel<T, true, false, false>)
                       : (fill ? dot_tile_kernel<T, false, true, false> : dot_tile_kernel<T, false, false, false>);
  hipLaunchKernelGGL(kernel, this->tile_grid(), dim3(NT), 0, ctx().stream, Fa, na, lda, Fb, nb, ldb, d, norm_a.p,
                     self ? norm_a.p : norm_b.p, metric, alpha, tau, self ? (int)TILE_SELF : 0, weighted ? 1 : 0, nti,
                     counts.p, tile_nz.p, ptr.p, idx, val, flag);
  SS_LAUNCH_CHECK();
  return SS_OK;
}

// ---- 16-bit rows (include/simspread_hip_half.h)
// a side may use 16-byte loads: every chunk address base + 2 (i ld + k), k % 8 == 0, is then 16-byte aligned
bool h16_fast(const uint16_t* F, int64_t ld) { return (reinterpret_cast<uintptr_t>(F) & 15) == 0 && ld % 8 == 0; }

namespace {
template <class Op>
int h16_norms(const uint16_t* F, int64_t n, int64_t ld, int64_t d, float* norm) {
  hipLaunchKernelGGL(dottile::row_norm_h16_kernel<Op>, dim3((unsigned)ceil_div(n * 16, 256)), dim3(256), 0, ctx().stream,
                     F, n, ld, d, norm);
  SS_LAUNCH_CHECK();
  return SS_OK;
}
template <class Op>
int h16_nan_scan(const uint16_t* F, int64_t n, int64_t ld, int64_t d, int* flag) {
  if (n == 0 || d == 0) return SS_OK;
  const int64_t blocks = std::min<int64_t>(ceil_div(n * 16, 256), 4096);  // 16 lanes per row
  hipLaunchKernelGGL(dottile::nan_scan_h16_kernel<Op>, dim3((unsigned)blocks), dim3(256), 0, ctx().stream, F, n, ld, d,
                     flag);
  SS_LAUNCH_CHECK();
  return SS_OK;
}
// SS_EINVAL when an element k < d of Fa or (not NULL) Fb is a NaN pattern (synchronises)
template <class Op>
int h16_refuse_nan(const uint16_t* Fa, int64_t na, int64_t lda, const uint16_t* Fb, int64_t nb, int64_t ldb, int64_t d) {
  hipStream_t st = ctx().stream;
  DevBuf<int> flag;
  SS_TRY(flag.alloc(1));
  SS_HIP(hipMemsetAsync(flag.p, 0, sizeof(int), st));
  SS_TRY(h16_nan_scan<Op>(Fa, na, lda, d, flag.p));
  if (Fb) SS_TRY(h16_nan_scan<Op>(Fb, nb, ldb, d, flag.p));
  int bad = 0;
  SS_HIP(hipMemcpyAsync(&bad, flag.p, sizeof(int), hipMemcpyDeviceToHost, st));
  SS_HIP(hipStreamSynchronize(st));
  if (bad) return fail(SS_EINVAL, "dot_h16: the features hold a NaN");
  return SS_OK;
}
template <class Op>
void h16_launch(const DotCsrH16& p, dim3 grid, bool fill, int* idx, float* val, int* flag) {
  auto* kernel = p.sym ? (fill ? dot_tile_kernel<float, true, true, false, Op> : dot_tile_kernel<float, true, false, false, Op>)
                       : (fill ? dot_tile_kernel<float, false, true, false, Op>
                               : dot_tile_kernel<float, false, false, false, Op>);
  const int flags = (p.sym ? (int)TILE_SELF : 0) | (h16_fast(p.Fa, p.lda) ? (int)TILE_FAST_A : 0) |
                    (h16_fast(p.Fb, p.ldb) ? (int)TILE_FAST_B : 0);
  hipLaunchKernelGGL(kernel, grid, dim3(NT), 0, ctx().stream, p.Fa, p.na, p.lda, p.Fb, p.nb, p.ldb, p.d, p.norm_a.p,
                     p.sym ? p.norm_a.p : p.norm_b.p, p.metric, p.alpha, (const float*)nullptr, flags, p.weighted ? 1 : 0,
                     p.nti, p.counts.p, p.tile_nz.p, p.ptr.p, idx, val, flag);
}
}  // namespace

int h16_row_norms(int storage, const uint16_t* F, int64_t n, int64_t ld, int64_t d, float* norm) {
  return storage == SS_H16_BF16 ? h16_norms<dottile::Bf16>(F, n, ld, d, norm) : h16_norms<dottile::F16>(F, n, ld, d, norm);
}
int h16_refuse_nan_rows(int storage, const uint16_t* Fa, int64_t na, int64_t lda, const uint16_t* Fb, int64_t nb,
                        int64_t ldb, int64_t d) {
  return storage == SS_H16_BF16 ? h16_refuse_nan<dottile::Bf16>(Fa, na, lda, Fb, nb, ldb, d)
                                : h16_refuse_nan<dottile::F16>(Fa, na, lda, Fb, nb, ldb, d);
}

int DotCsrH16::count(const uint16_t* Fa_, int64_t na_, int64_t lda_, const uint16_t* Fb_, int64_t nb_, int64_t ldb_,
                     int64_t d_, int storage_, int metric_, float alpha_, bool weighted_) {
  what = "dot_h16";
  sym = (Fb_ == nullptr);
  Fa = Fa_;
  Fb = sym ? Fa_ : Fb_;
  lda = lda_;
  ldb = sym ? lda_ : ldb_;
  d = d_;
  storage = storage_;
  metric = metric_;
  alpha = alpha_;
  weighted = weighted_;
  // storage, metric and alpha are the caller's to check (check_h16_args of api.hip, before anything is staged)
  SS_TRY(h16_refuse_nan_rows(storage, Fa, na_, lda, sym ? nullptr : Fb, nb_, ldb, d));
  SS_TRY(this->begin_tiles(na_, sym ? na_ : nb_, TILE, true));
  if (na == 0 || nb == 0) return SS_OK;
  SS_TRY(norm_a.alloc((size_t)na));
  SS_TRY(h16_row_norms(storage, Fa, na, lda, d, norm_a.p));
  if (!sym) {
    SS_TRY(norm_b.alloc((size_t)nb));
    SS_TRY(h16_row_norms(storage, Fb, nb, ldb, d, norm_b.p));
  }
  return this->count_pass();
}

int DotCsrH16::launch(bool fill, int* idx, float* val, int* flag) {
  if (storage == SS_H16_BF16) h16_launch<dottile::Bf16>(*this, this->tile_grid(), fill, idx, val, flag);
  else h16_launch<dottile::F16>(*this, this->tile_grid(), fill, idx, val, flag);
  SS_LAUNCH_CHECK();
  return SS_OK;
}

// ---- int8 rows (include/simspread_hip_int8.h)
// a side may use 16-byte loads: every chunk address base + i ld + k, k % 16 == 0, is then 16-byte aligned
bool i8_fast(const int8_t* F, int64_t ld) { return (reinterpret_cast<uintptr_t>(F) & 15) == 0 && ld % 16 == 0; }

int i8_row_norms(const int8_t* F, int64_t n, int64_t ld, int64_t d, float* norm) {
  hipLaunchKernelGGL(dottile::row_norm_i8_kernel, dim3((unsigned)ceil_div(n * 16, 256)), dim3(256), 0, ctx().stream, F, n,
                     ld, d, norm);
  SS_LAUNCH_CHECK();
  return SS_OK;
}

int DotCsrI8::count(const int8_t* Fa_, int64_t na_, int64_t lda_, const int8_t* Fb_, int64_t nb_, int64_t ldb_,
                    int64_t d_, int metric_, float alpha_, bool weighted_, int k) {
  what = "dot_i8";
  self = (Fb_ == nullptr);
  Fa = Fa_;
  Fb = self ? Fa_ : Fb_;
  lda = lda_;
  ldb = self ? lda_ : ldb_;
  d = d_;
  metric = metric_;
  alpha = alpha_;
  weighted = weighted_;
  tau = nullptr;
  // d, metric, alpha and k are the caller's to check (check_i8_args of api.hip, before anything is staged); the sums
  // below are exact only up to I8_D_MAX, so that one is held here too
  if (d < 0 || d > dottile::I8_D_MAX) return fail(SS_EINVAL, "dot_i8: %lld features outside 0..131071", (long long)d);
  sym = self && k == 0;  // a per-row cut has no mirror: the full grid
  SS_TRY(this->begin_tiles(na_, self ? na_ : nb_, TILE, true));
  if (na == 0 || nb == 0) return SS_OK;
  SS_TRY(norm_a.alloc((size_t)na));
  SS_TRY(i8_row_norms(Fa, na, lda, d, norm_a.p));
  if (!self) {
    SS_TRY(norm_b.alloc((size_t)nb));
    SS_TRY(i8_row_norms(Fb, nb, ldb, d, norm_b.p));
  }
  if (k > 0) {
    SS_TRY(tau_buf.alloc(na));
    SS_TRY(dot_kth_i8(Fa, na, lda, self ? nullptr : Fb, nb, ldb, d, metric, norm_a.p, self ? norm_a.p : norm_b.p, k,
                      tau_buf.p));
    tau = tau_buf.p;
  }
  return this->count_pass();
}

int DotCsrI8::launch(bool fill, int* idx, float* val, int* flag) {
  using Op = dottile::I8;
  auto* kernel = tau   ? (fill ? dot_tile_kernel<float, false, true, true, Op> : dot_tile_kernel<float, false, false, true, Op>)
                 : sym ? (fill ? dot_tile_kernel<float, true, true, false, Op> : dot_tile_kernel<float, true, false, false, Op>)
                       : (fill ? dot_tile_kernel<float, false, true, false, Op>
                               : dot_tile_kernel<float, false, false, false, Op>);
  const int flags = (self ? (int)TILE_SELF : 0) | (i8_fast(Fa, lda) ? (int)TILE_FAST_A : 0) |
                    (i8_fast(Fb, ldb) ? (int)TILE_FAST_B : 0);
  hipLaunchKernelGGL(kernel, this->tile_grid(), dim3(NT), 0, ctx().stream, Fa, na, lda, Fb, nb, ldb, d, norm_a.p,
                     self ? norm_a.p : norm_b.p, metric, alpha, tau, flags, weighted ? 1 : 0, nti, counts.p, tile_nz.p,
                     ptr.p, idx, val, flag);
  SS_LAUNCH_CHECK();
  return SS_OK;
}

template int dot_row_norms<float>(const float*, int64_t, int64_t, int64_t, float*);
template int dot_row_norms<double>(const double*, int64_t, int64_t, int64_t, double*);
template struct DotCsr<float>;
template struct DotCsr<double>;

}  // namespace ss
