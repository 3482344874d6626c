// The neighbour floor of the two producers over real-valued rows (jaccard_csr.hip: weighted Jaccard; dot_csr.hip:
// cosine, real-valued Tanimoto, Dice on the matrix cores): tau[i], the k-th largest positive similarity of row i of Fa
// against the rows of Fb, for every row, without the na x nb similarity ever existing.  The producers then keep entry
// (i, j) iff v != 0 and (s >= alpha or (s > 0 and s >= tau[i])): "at least the k nearest sources, whatever alpha says".
//
//   P_i   = multiset { s(i, j) : 0 <= j < nb, s(i, j) > 0 },   s as the producer computes it (a NaN s is not > 0)
//   tau_i = the k-th largest element of P_i, multiplicity counted, when |P_i| >= k, else +0
//
// This is neighbour_floor.hip for another arithmetic: the partial pass is the producer's own tile pass -- the staging
// loop and the min / max sums of jaccard_tile.hpp, or the staging loop, the MFMA sequence in the same k order, the
// norms and dot_pair_sim of dot_tile.hpp, so that selection and emit see the same bits of s -- with the selection
// skeleton of row_select.hpp as its epilogue; the column groups and the merge are kth_merge.hpp.  Block (x, g) owns
// ROWS rows of row strip x / (TILE / ROWS) and walks the column tiles of column group g; it leaves the k largest
// positive values of every row among those columns in part[g][row][0..k), +0 padded.
//   jaccard  a thread holds an RA x RC block of pairs whose rows follow from its thread row: RowSelect::absorb
//   dot      a lane's 64 accumulator values lie in up to 32 rows (Mma<T>::row): RowSelect::absorb_flat with the
//            row-of-value functor; the diagonal of a block against itself is 1 before selection, as in the emit pass
// Ties at tau_i are all kept by the emit pass, so only the VALUE of the k-th entry is needed: the selection keeps
// multisets of values and no indices, no float atomics, and no position comes from an atomic.  Every device loop is
// bounded by k, the tile width, d, the tiles of a group or groups * k <= 4096 (host-checked); there are no spin-waits
// and no flags between workgroups.
//
// LDS (64 KiB static): the lists of a block take ROWS * k values next to the tile staging, so ROWS follows T and k:
//   fp32  staging 16 KiB (+ 1 KiB of norms for dot), lists of 128 rows x 64 values = 32 KiB: the whole strip
//   fp64  staging 32 KiB (jaccard) / 36 KiB + 2 KiB of norms (dot), lists of 2048 values = 16 KiB: 64 rows for k <= 32,
//         32 rows above; the 2 or 4 blocks of a strip each compute the strip's full tile and select from their rows
//   int8  (dot, operand dottile::I8, T = float) staging 36 KiB + 1 KiB of norms, lists of 4096 values = 16 KiB: 128 rows
//         for k <= 32, 64 rows above.  The Gram tile is dot_tile_gram_i8 (dot_tile_i8.hpp), the emit pass's own.
// floor_rows() is the host-side check of every configuration; one that does not fit is SS_EUNSUPPORTED, never launched.
#include <hip/hip_runtime.h>

#include "dot_tile.hpp"
#include "dot_tile_i8.hpp"
#include "graph.hpp"
#include "jaccard_tile.hpp"
#include "kth_merge.hpp"
#include "row_select.hpp"

namespace ss {

namespace {

constexpr int TILE = 128;
static_assert(jctile::TILE == TILE && dottile::TILE == TILE, "one strip height for both producers");

// the lists of a selecting block: LIST values for at most MAX_ROWS rows
template <class T>
struct Lists;
template <>
struct Lists<float> {
  static constexpr int LIST = 8192, MAX_ROWS = 128;
};
template <>
struct Lists<double> {
  static constexpr int LIST = 2048, MAX_ROWS = 64;
};

template <>
struct Lists<dottile::I8> {  // fp32 values next to the 36 KiB int8 staging
  static constexpr int LIST = 4096, MAX_ROWS = 128;
};

// Op: what the lists are sized for -- T, or the operand tag of a kernel whose staging is not T's
template <class T, int ROWS, class Op = T>
using Select = RowSelect<T, TILE, ROWS, Lists<Op>::LIST>;

template <class T, int ROWS>
__global__ void __launch_bounds__(jctile::threads<T>()) jaccard_kth_partial_kernel(
    const T* __restrict__ Fa, int64_t na, int64_t lda, const T* __restrict__ Fb, int64_t nb, int64_t ldb, int64_t d,
    int k, int64_t ntj, int64_t tiles_per_group, T* __restrict__ part) {
  using jctile::NTX;
  using jctile::RC;
  constexpr int RA = jctile::Block<T>::RA;
  __shared__ Select<T, ROWS> sel;
  static_assert(2 * jctile::BK * TILE * sizeof(T) + sizeof(sel) <= 64 * 1024, "static LDS with the tile staging");

  constexpr int NH = TILE / ROWS;  // blocks per row strip
  const int64_t it = blockIdx.x / NH;
  const int sel0 = (int)(blockIdx.x % NH) * ROWS;
  const int64_t g = blockIdx.y;
  const int64_t i0 = it * TILE;
  const int tid = threadIdx.x, tx = tid % NTX, ty = tid / NTX;
  const bool mine = RA * ty >= sel0 && RA * ty < sel0 + ROWS;

  int cnt;
  sel.init(cnt);

  const int64_t jt_end = min((g + 1) * tiles_per_group, ntj);
#pragma unroll 1
  for (int64_t jt = g * tiles_per_group; jt < jt_end; ++jt) {
    const int64_t j0 = jt * TILE;
    // the strip's first row and the leading dimensions, opaque per tile: otherwise the addresses of the staging loads
    // are hoisted out of this loop and held (in fp64: spilled) across the selection
    int64_t i0t = i0, ldat = lda, ldbt = ldb;
    asm volatile("" : "+s"(i0t), "+s"(ldat), "+s"(ldbt));
    jctile::Sums<T> acc[RA][RC];
    jctile::jaccard_tile_sums<T>(Fa, na, ldat, Fb, nb, ldbt, d, i0t, j0, acc);
    T s[RA][RC];
#pragma unroll
    for (int a = 0; a < RA; ++a)
#pragma unroll
      for (int b = 0; b < RC; ++b)
        s[a][b] = i0 + RA * ty + a < na && j0 + RC * tx + b < nb
                      ? jctile::jaccard_similarity<T>(acc[a][b].x, acc[a][b].y)
                      : T(0);
    sel.absorb(RA * ty - sel0, mine, k, cnt, s);
  }
  sel.store(i0 + sel0, na, k, cnt, part + g * na * k);
}

// Op: the operands, as in dot_tile_kernel.  Op == T: column-major rows of T.  dottile::I8 (T == float): row-major int8
// rows; `self` then also carries the sides that may use 16-byte loads (bit 0: Fb is Fa, bit 1: Fa, bit 2: Fb).
template <class T, int ROWS, class Op = T>
__global__ void __launch_bounds__(dottile::NT) dot_kth_partial_kernel(
    const typename dottile::operand_elem<Op>::type* __restrict__ Fa, int64_t na, int64_t lda,
    const typename dottile::operand_elem<Op>::type* __restrict__ Fb, int64_t nb, int64_t ldb, int64_t d,
    const T* __restrict__ norm_a, const T* __restrict__ norm_b, int metric, int self, int k, int64_t ntj,
    int64_t tiles_per_group, T* __restrict__ part) {
  using dottile::WT;
  using M = dottile::Mma<T>;
  constexpr int MT = M::MT, NR = M::NR;
  constexpr int NM = dottile::NM<T>;
  constexpr int NV = NM * NM * NR;  // 64 pairs per lane
  __shared__ T na_s[TILE], nb_s[TILE];  // sqrt(A), sqrt(B) (cosine) or A, B of the strip's rows and the tile's columns
  constexpr bool INT8 = std::is_same<Op, dottile::I8>::value;
  static_assert(std::is_same<Op, T>::value || (INT8 && std::is_same<T, float>::value), "int8 operands: fp32 values");
  __shared__ Select<T, ROWS, Op> sel;
  static_assert((INT8 ? dottile::gram_i8_lds_bytes() : dottile::gram_lds_bytes(sizeof(T), dottile::LDT<T>)) +
                        sizeof(na_s) + sizeof(nb_s) + sizeof(sel) <= 64 * 1024,
                "static LDS with the tile staging");

  constexpr int NH = TILE / ROWS;  // blocks per row strip
  const int64_t it = blockIdx.x / NH;
  const int sel0 = (int)(blockIdx.x % NH) * ROWS;
  const int64_t g = blockIdx.y;
  const int64_t i0 = it * TILE;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave >> 1, wn = wave & 1;
  const int cl = lane % MT;
  const bool diag1 = INT8 ? (self & 1) != 0 : self != 0;

  if (tid < TILE) dottile::stage_norm<T>(na_s, tid, norm_a, i0, na, metric);
  int cnt;
  sel.init(cnt);  // synchronises: na_s is staged

  const int64_t jt_end = min((g + 1) * tiles_per_group, ntj);
#pragma unroll 1
  for (int64_t jt = g * tiles_per_group; jt < jt_end; ++jt) {
    const int64_t j0 = jt * TILE;
    int64_t i0t = i0, ldat = lda, ldbt = ldb;  // opaque per tile, as in jaccard_kth_partial_kernel
    asm volatile("" : "+s"(i0t), "+s"(ldat), "+s"(ldbt));
    typename M::acc_t acc[NM][NM];
    if constexpr (INT8)
      dottile::dot_tile_gram_i8(Fa, na, ldat, Fb, nb, ldbt, d, i0t, j0, (self & 2) != 0, (self & 4) != 0, acc);
    else
      dottile::dot_tile_gram<T>(Fa, na, ldat, Fb, nb, ldbt, d, i0t, j0, acc);
    // the last read of the previous tile's nb_s lies before the barriers of its absorb_flat
    if (tid < TILE) dottile::stage_norm<T>(nb_s, tid, norm_b, j0, nb, metric);
    __syncthreads();

    // value (i * NM + j) * NR + r = this lane's pair of register r of MFMA tile (i, j), as the emit pass numbers them
    T s[NV];
#pragma unroll
    for (int i = 0; i < NM; ++i)
#pragma unroll
      for (int j = 0; j < NM; ++j) {
        const int col = wn * WT + j * MT + cl;
        const T cb = nb_s[col];
#pragma unroll
        for (int r = 0; r < NR; ++r) {
          const int row = wm * WT + i * MT + M::row(r, lane);
          s[(i * NM + j) * NR + r] =
              i0 + row < na && j0 + col < nb
                  ? dottile::dot_pair_sim<T>(acc[i][j][r], na_s[row], cb, metric, diag1 && i0 + row == j0 + col)
                  : T(0);
        }
      }
    sel.absorb_flat(k, cnt, s, [&](int e) {
      const int lr = wm * WT + (e / (NM * NR)) * MT + M::row(e % NR, lane) - sel0;
      return lr >= 0 && lr < ROWS ? lr : -1;
    });
  }
  sel.store(i0 + sel0, na, k, cnt, part + g * na * k);
}

// rows a block selects for: the most whose lists of k values fit; SS_EUNSUPPORTED when not even the fewest do
// (Op: the key of Lists)
template <class Op>
int floor_rows(const char* what, int k, int& rows) {
  rows = Lists<Op>::MAX_ROWS;
  if ((int64_t)rows * k > Lists<Op>::LIST) rows /= 2;
  if ((int64_t)rows * k > Lists<Op>::LIST)
    return fail(SS_EUNSUPPORTED, "%s: the lists of %d rows x k = %d do not fit in LDS", what, rows, k);
  return SS_OK;
}

// What the two selections share on the host: the checks, the empty cases, the column groups, the scratch and the merge.
// partial(rows, grid, ntj, tiles_per_group, part) enqueues the producer's partial kernel for `rows` rows per block.
template <class T, class Op = T, class Partial>
int kth_drive(const char* what, int64_t na, int64_t nb, int k, T* tau, Partial partial) {
  hipStream_t st = ctx().stream;
  if (k < 1 || k > NEIGHBOUR_K_MAX) return fail(SS_EINVAL, "%s: k = %d outside 1..%d", what, k, NEIGHBOUR_K_MAX);
  if (na == 0) return SS_OK;
  if (nb == 0) {
    SS_HIP(hipMemsetAsync(tau, 0, (size_t)na * sizeof(T), st));
    SS_HIP(hipStreamSynchronize(st));
    return SS_OK;
  }
  int rows = 0;
  SS_TRY(floor_rows<Op>(what, k, rows));
  const int64_t ntj = ceil_div(nb, TILE);
  const int64_t row_blocks = ceil_div(na, TILE) * (TILE / rows);
  int64_t groups = 0, tiles_per_group = 0;
  SS_TRY(kth::plan_groups<T>(what, na, ntj, row_blocks, k, groups, tiles_per_group));
  DevBuf<T> part;
  SS_TRY(part.alloc((size_t)groups * (size_t)na * (size_t)k));
  partial(rows, dim3((unsigned)row_blocks, (unsigned)groups), ntj, tiles_per_group, part.p);
  SS_LAUNCH_CHECK();
  SS_TRY(kth::launch_merge<T>(part.p, na, k, groups, tau, st));
  SS_HIP(hipStreamSynchronize(st));  // part is freed on return
  return SS_OK;
}

}  // namespace

template <class T>
int jaccard_kth(const T* Fa, int64_t na, int64_t lda, const T* Fb, int64_t nb, int64_t ldb, int64_t d, int k, T* tau) {
  if (!Fb) {
    Fb = Fa;
    nb = na;
    ldb = lda;
  }
  return kth_drive<T>("jaccard kth", na, nb, k, tau,
                      [&](int rows, dim3 grid, int64_t ntj, int64_t tiles_per_group, T* part) {
                        constexpr int R = Lists<T>::MAX_ROWS;
                        auto* kernel = jaccard_kth_partial_kernel<T, R>;
                        if constexpr (R * NEIGHBOUR_K_MAX > Lists<T>::LIST)
                          if (rows != R) kernel = jaccard_kth_partial_kernel<T, R / 2>;
                        hipLaunchKernelGGL(kernel, grid, dim3(jctile::threads<T>()), 0, ctx().stream, Fa, na, lda, Fb, nb,
                                           ldb, d, k, ntj, tiles_per_group, part);
                      });
}

template <class T>
int dot_kth(const T* Fa, int64_t na, int64_t lda, const T* Fb, int64_t nb, int64_t ldb, int64_t d, int metric,
            const T* norm_a, const T* norm_b, int k, T* tau) {
  if (metric != SS_SIM_COSINE && metric != SS_SIM_TANIMOTO && metric != SS_SIM_DICE)
    return fail(SS_EINVAL, "dot kth: unknown metric %d", metric);
  const bool self = !Fb;
  if (self) {
    Fb = Fa;
    nb = na;
    ldb = lda;
    norm_b = norm_a;
  }
  DevBuf<T> own_a, own_b;
  if (na > 0 && nb > 0 && k >= 1 && k <= NEIGHBOUR_K_MAX) {
    if (!norm_a) {
      SS_TRY(own_a.alloc((size_t)na));
      SS_TRY(dot_row_norms<T>(Fa, na, lda, d, own_a.p));
      norm_a = own_a.p;
      if (self) norm_b = norm_a;
    }
    if (!norm_b) {
      SS_TRY(own_b.alloc((size_t)nb));
      SS_TRY(dot_row_norms<T>(Fb, nb, ldb, d, own_b.p));
      norm_b = own_b.p;
    }
  }
  // (the norms are freed on return, after the synchronisation of kth_drive)
  return kth_drive<T>("dot kth", na, nb, k, tau, [&](int rows, dim3 grid, int64_t ntj, int64_t tiles_per_group, T* part) {
    constexpr int R = Lists<T>::MAX_ROWS;
    auto* kernel = dot_kth_partial_kernel<T, R>;
    if constexpr (R * NEIGHBOUR_K_MAX > Lists<T>::LIST)
      if (rows != R) kernel = dot_kth_partial_kernel<T, R / 2>;
    hipLaunchKernelGGL(kernel, grid, dim3(dottile::NT), 0, ctx().stream, Fa, na, lda, Fb, nb, ldb, d, norm_a, norm_b,
                       metric, self ? 1 : 0, k, ntj, tiles_per_group, part);
  });
}

int dot_kth_i8(const int8_t* Fa, int64_t na, int64_t lda, const int8_t* Fb, int64_t nb, int64_t ldb, int64_t d,
               int metric, const float* norm_a, const float* norm_b, int k, float* tau) {
  using Op = dottile::I8;
  if (metric != SS_SIM_COSINE && metric != SS_SIM_TANIMOTO && metric != SS_SIM_DICE)
    return fail(SS_EINVAL, "dot_i8 kth: unknown metric %d", metric);
  if (d < 0 || d > dottile::I8_D_MAX) return fail(SS_EINVAL, "dot_i8 kth: %lld features outside 0..131071", (long long)d);
  const bool self = !Fb;
  if (self) {
    Fb = Fa;
    nb = na;
    ldb = lda;
    norm_b = norm_a;
  }
  DevBuf<float> own_a, own_b;
  if (na > 0 && nb > 0 && k >= 1 && k <= NEIGHBOUR_K_MAX) {
    if (!norm_a) {
      SS_TRY(own_a.alloc((size_t)na));
      SS_TRY(i8_row_norms(Fa, na, lda, d, own_a.p));
      norm_a = own_a.p;
      if (self) norm_b = norm_a;
    }
    if (!norm_b) {
      SS_TRY(own_b.alloc((size_t)nb));
      SS_TRY(i8_row_norms(Fb, nb, ldb, d, own_b.p));
      norm_b = own_b.p;
    }
  }
  const int flags = (self ? 1 : 0) | (i8_fast(Fa, lda) ? 2 : 0) | (i8_fast(Fb, ldb) ? 4 : 0);
  // (the norms are freed on return, after the synchronisation of kth_drive)
  return kth_drive<float, Op>(
      "dot_i8 kth", na, nb, k, tau, [&](int rows, dim3 grid, int64_t ntj, int64_t tiles_per_group, float* part) {
        constexpr int R = Lists<Op>::MAX_ROWS;
        static_assert(R * NEIGHBOUR_K_MAX > Lists<Op>::LIST && (R / 2) * NEIGHBOUR_K_MAX <= Lists<Op>::LIST,
                      "two kernels: R rows while R k values fit, R / 2 above");
        auto* kernel = dot_kth_partial_kernel<float, R, Op>;
        if (rows != R) kernel = dot_kth_partial_kernel<float, R / 2, Op>;
        hipLaunchKernelGGL(kernel, grid, dim3(dottile::NT), 0, ctx().stream, Fa, na, lda, Fb, nb, ldb, d, norm_a, norm_b,
                           metric, flags, k, ntj, tiles_per_group, part);
      });
}

template int jaccard_kth<float>(const float*, int64_t, int64_t, const float*, int64_t, int64_t, int64_t, int, float*);
template int jaccard_kth<double>(const double*, int64_t, int64_t, const double*, int64_t, int64_t, int64_t, int, double*);
template int dot_kth<float>(const float*, int64_t, int64_t, const float*, int64_t, int64_t, int64_t, int, const float*,
                            const float*, int, float*);
template int dot_kth<double>(const double*, int64_t, int64_t, const double*, int64_t, int64_t, int64_t, int,
                             const double*, const double*, int, double*);

}  // namespace ss
