// Cutoff profiles of the four fused producers (fingerprint.hip, jaccard_csr.hip, dot_csr.hip and its 16-bit route): for
// up to 32 ascending cuts, the exact nnz and the exact row degrees of the CSR the plain producer (k == 0, no neighbour
// floor) would build at each of them, from ONE pass over the pairs -- s(i, j) does not depend on alpha.  No graph is
// built.  The rule is include/simspread_hip_profile.h:
//
//   v = weighted ? s : 1; pair (i, j) counts for cut b iff s >= cuts[b] and v != 0 (a NaN s counts for none)
//   rows[i * ncuts + b] = the number of j that count for cut b;  total[b] = sum_i rows[i, b]  (int64: no 2^31 refusal)
//
// This is real_floor.hip / neighbour_floor.hip for a third epilogue: a profile kernel runs the producer's own tile pass
// -- tanimoto_tile_counts + tanimoto_similarity, jaccard_tile_sums + jaccard_similarity, dot_tile_gram /
// dot_tile_gram_h16 + stage_norm + dot_pair_sim with the diagonal rule, called and not copied -- over the producer's own
// grid (pair_tile.hpp: the upper triangle when Fb == NULL, where an off-diagonal tile counts each pair for its row and,
// mirrored, for its column), so that the profile sees the bits of s the emit pass sees, (j, i) carrying the bits of
// (i, j) in symmetric mode, at half the pair work.  The epilogue is pair_tile_profile (pair_tile.hpp): binary search
// of each s in the cuts, a per-tile LDS histogram hist[row][m] of integer adds, the non-zero bins merged into the device
// table hist[na][ncuts + 1] (int32) with integer adds.  profile_finish_kernel then turns bins into
// rows[i][b] = sum_{m > b} hist[i][m] and total[b].  Only integers are ever added: no float atomics, no position comes
// from an atomic, the result does not depend on the order and is bitwise repeatable.  Every device loop is bounded by
// the tile, d or ncuts; there are no spin-waits and no flags between workgroups.
//
// LDS (64 KiB static): the tile's histogram takes 128 x 33 one-byte bins = 4.1 KB next to the tile staging (fingerprints
// 16 KB, jaccard 16 / 32 KB, dot 16 / 36 KB + norms, 16-bit 36 KB + norms).  As 128 x 33 ints (16.5 KB) it fitted too,
// but left the 16-bit kernel two workgroups per CU where its producer has three, and its profile cost 1.75 size
// queries instead of 1.29 (profiles/cut_profile_time.json); see pair_tile_profile.
#include <hip/hip_runtime.h>

#include "dot_tile.hpp"
#include "dot_tile_h16.hpp"
#include "graph.hpp"
#include "jaccard_tile.hpp"
#include "pair_tile.hpp"
#include "tanimoto_tile.hpp"

namespace ss {

namespace {

constexpr int TILE = 128;
static_assert(fptile::TILE == TILE && jctile::TILE == TILE && dottile::TILE == TILE, "one tile edge for every producer");

template <class T, bool SYM>
__global__ void __launch_bounds__(256) tanimoto_profile_kernel(
    const uint64_t* __restrict__ Fa, int64_t na, const uint64_t* __restrict__ Fb, int64_t nb, int64_t nwords,
    const int* __restrict__ pop_a, const int* __restrict__ pop_b, ProfileCuts<T> cuts, int weighted, int64_t nti,
    int* __restrict__ ghist) {
  using fptile::BK;
  using fptile::RB;
  __shared__ __attribute__((aligned(16))) uint32_t As[BK][TILE];
  __shared__ __attribute__((aligned(16))) uint32_t Bs[BK][TILE];

  const PairTile t = pair_tile<SYM, TILE>(nti);
  const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;

  uint32_t acc[RB][RB];
  fptile::tanimoto_tile_counts(As, Bs, Fa, na, Fb, nb, nwords, t.i0, t.j0, acc);

  // popcounts of the thread's rows and columns; those past the last row / column are never used
  int pa[RB], pb[RB];
#pragma unroll
  for (int a = 0; a < RB; ++a) {
    const int64_t i = t.i0 + RB * ty + a;
    pa[a] = i < na ? pop_a[i] : 0;
  }
#pragma unroll
  for (int b = 0; b < RB; ++b) {
    const int64_t j = t.j0 + RB * tx + b;
    pb[b] = j < nb ? pop_b[j] : 0;
  }
  pair_tile_profile<T, TILE, 256, RB * RB, SYM>(t, na, nb, cuts, weighted != 0, ghist, [&](int e, int& row, int& col) {
    const int a = e / RB, b = e % RB;
    row = RB * ty + a;
    col = RB * tx + b;
    return fptile::tanimoto_similarity<T>((int)acc[a][b], pa[a], pb[b]);
  });
}

template <class T, bool SYM>
__global__ void __launch_bounds__(jctile::threads<T>()) jaccard_profile_kernel(
    const T* __restrict__ Fa, int64_t na, int64_t lda, const T* __restrict__ Fb, int64_t nb, int64_t ldb, int64_t d,
    ProfileCuts<T> cuts, int weighted, int64_t nti, int* __restrict__ ghist) {
  using jctile::NTX;
  using jctile::RC;
  constexpr int RA = jctile::Block<T>::RA;

  const PairTile t = pair_tile<SYM, TILE>(nti);
  const int tid = threadIdx.x, tx = tid % NTX, ty = tid / NTX;

  jctile::Sums<T> acc[RA][RC];
  jctile::jaccard_tile_sums<T>(Fa, na, lda, Fb, nb, ldb, d, t.i0, t.j0, acc);

  pair_tile_profile<T, TILE, jctile::threads<T>(), RA * RC, SYM>(
      t, na, nb, cuts, weighted != 0, ghist, [&](int e, int& row, int& col) {
        const int a = e / RC, b = e % RC;
        row = RA * ty + a;
        col = RC * tx + b;
        return jctile::jaccard_similarity<T>(acc[a][b].x, acc[a][b].y);
      });
}

// Op as in dot_tile_kernel (dot_csr.hip): T (column-major rows of T) or dottile::Bf16 / dottile::F16 (T == float,
// row-major 16-bit patterns; fast_a / fast_b allow a side its 16-byte loads)
template <class Op>
struct OperandElem { using type = typename Op::elem; };
template <>
struct OperandElem<float> { using type = float; };
template <>
struct OperandElem<double> { using type = double; };

template <class T, bool SYM, class Op = T>
__global__ void __launch_bounds__(dottile::NT) dot_profile_kernel(
    const typename OperandElem<Op>::type* __restrict__ Fa, int64_t na, int64_t lda,
    const typename OperandElem<Op>::type* __restrict__ Fb, int64_t nb, int64_t ldb, int64_t d,
    const T* __restrict__ norm_a, const T* __restrict__ norm_b, int metric, int fast_a, int fast_b, ProfileCuts<T> cuts,
    int weighted, int64_t nti, int* __restrict__ ghist) {
  using dottile::NT;
  using dottile::WT;
  using M = dottile::Mma<T>;
  constexpr int MT = M::MT, NR = M::NR;
  constexpr int NM = dottile::NM<T>;    // MFMA tiles per wave edge
  constexpr int NV = NM * NM * NR;      // 64 pairs per lane
  __shared__ T na_s[TILE], nb_s[TILE];  // sqrt(A), sqrt(B) (cosine) or A, B of the tile's rows and columns

  const PairTile t = pair_tile<SYM, TILE>(nti);
  const int64_t i0 = t.i0, j0 = t.j0;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave >> 1, wn = wave & 1;
  const int cl = lane % MT;

  typename M::acc_t acc[NM][NM];
  if constexpr (std::is_same<Op, T>::value)
    dottile::dot_tile_gram<T>(Fa, na, lda, Fb, nb, ldb, d, i0, j0, acc);
  else
    dottile::dot_tile_gram_h16<Op>(Fa, na, lda, Fb, nb, ldb, d, i0, j0, fast_a != 0, fast_b != 0, acc);

  if (tid < TILE) dottile::stage_norm<T>(na_s, tid, norm_a, i0, na, metric);
  else dottile::stage_norm<T>(nb_s, tid - TILE, norm_b, j0, nb, metric);
  __syncthreads();

  // pair (i * NM + j) * NR + r = this lane's pair of register r of MFMA tile (i, j), as the emit pass numbers them;
  // SYM: the block is a set against itself, s(i, i) = 1
  pair_tile_profile<T, TILE, NT, NV, SYM>(t, na, nb, cuts, weighted != 0, ghist, [&](int e, int& row, int& col) {
    const int i = e / (NM * NR), j = (e / NR) % NM, r = e % NR;
    row = wm * WT + i * MT + M::row(r, lane);
    col = wn * WT + j * MT + cl;
    return dottile::dot_pair_sim<T>(acc[i][j][r], na_s[row], nb_s[col], metric, SYM && i0 + row == j0 + col);
  });
}

// rows[i][b] = sum_{m > b} hist[i][m] (rows may be null), total[b] += the block's sum of them
__global__ void __launch_bounds__(256) profile_finish_kernel(const int* __restrict__ hist, int64_t na, int ncuts,
                                                             int* __restrict__ rows,
                                                             unsigned long long* __restrict__ total) {
  __shared__ unsigned long long tot_s[PROFILE_CUTS_MAX];
  const int tid = threadIdx.x;
  if (tid < PROFILE_CUTS_MAX) tot_s[tid] = 0;
  __syncthreads();
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + tid;
  if (i < na) {
    const int* h = hist + i * (ncuts + 1);
    int run = 0;
    for (int b = ncuts - 1; b >= 0; --b) {
      run += h[b + 1];
      if (rows) rows[i * ncuts + b] = run;
      if (run) atomicAdd(&tot_s[b], (unsigned long long)run);
    }
  }
  __syncthreads();
  if (tid < ncuts && tot_s[tid]) atomicAdd(&total[tid], tot_s[tid]);
}

template <class T>
ProfileCuts<T> pack_cuts(const T* cuts, int ncuts) {
  ProfileCuts<T> c;
  for (int b = 0; b < PROFILE_CUTS_MAX; ++b) c.c[b] = b < ncuts ? cuts[b] : cuts[ncuts - 1];
  c.n = ncuts;
  return c;
}

// What the four profiles share on the host: the empty cases, the tile grid, the table and the finish.  prepare() is
// what the producer's count() does before its tile pass (refusals first, then popcounts or norms; it writes neither
// total nor rows); tiles(sym grid, nti, ghist) enqueues the profile kernel.
template <class Prepare, class Tiles>
int profile_drive(const char* what, int64_t na, int64_t nb, bool sym, int ncuts, int64_t* total, int* rows,
                  Prepare prepare, Tiles tiles) {
  hipStream_t st = ctx().stream;
  if (ncuts < 1 || ncuts > PROFILE_CUTS_MAX)
    return fail(SS_EINVAL, "%s: %d cuts outside 1..%d", what, ncuts, PROFILE_CUTS_MAX);
  int64_t nti = 0, ntj = 0, nblocks = 0;
  if (na > 0 && nb > 0) SS_TRY(pair_tile_blocks(what, na, nb, TILE, sym, nti, ntj, nblocks));
  SS_TRY(prepare());
  SS_HIP(hipMemsetAsync(total, 0, (size_t)ncuts * sizeof(int64_t), st));
  if (na == 0 || nb == 0) {
    if (rows && na > 0) SS_HIP(hipMemsetAsync(rows, 0, (size_t)na * (size_t)ncuts * sizeof(int), st));
    SS_HIP(hipStreamSynchronize(st));
    return SS_OK;
  }
  DevBuf<int> hist;
  SS_TRY(hist.alloc((size_t)na * (size_t)(ncuts + 1)));
  SS_HIP(hipMemsetAsync(hist.p, 0, (size_t)na * (size_t)(ncuts + 1) * sizeof(int), st));
  tiles(pair_tile_grid(sym, nti, ntj), nti, hist.p);
  SS_LAUNCH_CHECK();
  hipLaunchKernelGGL(profile_finish_kernel, dim3((unsigned)ceil_div(na, 256)), dim3(256), 0, st, hist.p, na, ncuts, rows,
                     reinterpret_cast<unsigned long long*>(total));
  SS_LAUNCH_CHECK();
  SS_HIP(hipStreamSynchronize(st));  // hist and the caller's popcounts / norms are freed on return
  return SS_OK;
}

}  // namespace

template <class T>
int tanimoto_profile(const uint64_t* Fa, int64_t na, const uint64_t* Fb, int64_t nb, int64_t nwords, const T* cuts,
                     int ncuts, bool weighted, int64_t* total, int* rows) {
  const bool sym = !Fb;
  if (sym) {
    Fb = Fa;
    nb = na;
  }
  DevBuf<int> pop_a, pop_b;
  return profile_drive(
      "tanimoto profile", na, nb, sym, ncuts, total, rows,
      [&] {
        if (na == 0 || nb == 0) return (int)SS_OK;
        hipStream_t st = ctx().stream;
        SS_TRY(pop_a.alloc(na));
        hipLaunchKernelGGL(fptile::popcount_rows_kernel, dim3((unsigned)ceil_div(na, 256)), dim3(256), 0, st, Fa, na,
                           nwords, pop_a.p);
        SS_LAUNCH_CHECK();
        if (!sym) {
          SS_TRY(pop_b.alloc(nb));
          hipLaunchKernelGGL(fptile::popcount_rows_kernel, dim3((unsigned)ceil_div(nb, 256)), dim3(256), 0, st, Fb, nb,
                             nwords, pop_b.p);
          SS_LAUNCH_CHECK();
        }
        return (int)SS_OK;
      },
      [&](dim3 grid, int64_t nti, int* ghist) {
        auto* kernel = sym ? tanimoto_profile_kernel<T, true> : tanimoto_profile_kernel<T, false>;
        hipLaunchKernelGGL(kernel, grid, dim3(256), 0, ctx().stream, Fa, na, Fb, nb, nwords, pop_a.p,
                           sym ? pop_a.p : pop_b.p, pack_cuts<T>(cuts, ncuts), weighted ? 1 : 0, nti, ghist);
      });
}

template <class T>
int jaccard_profile(const T* Fa, int64_t na, int64_t lda, const T* Fb, int64_t nb, int64_t ldb, int64_t d,
                    const T* cuts, int ncuts, bool weighted, int64_t* total, int* rows) {
  const bool sym = !Fb;
  if (sym) {
    Fb = Fa;
    nb = na;
    ldb = lda;
  }
  return profile_drive(
      "jaccard profile", na, nb, sym, ncuts, total, rows,
      [&] { return refuse_nan_rows<T>("jaccard profile", Fa, na, lda, sym ? nullptr : Fb, nb, ldb, d); },
      [&](dim3 grid, int64_t nti, int* ghist) {
        auto* kernel = sym ? jaccard_profile_kernel<T, true> : jaccard_profile_kernel<T, false>;
        hipLaunchKernelGGL(kernel, grid, dim3(jctile::threads<T>()), 0, ctx().stream, Fa, na, lda, Fb, nb, ldb, d,
                           pack_cuts<T>(cuts, ncuts), weighted ? 1 : 0, nti, ghist);
      });
}

template <class T>
int dot_profile(const T* Fa, int64_t na, int64_t lda, const T* Fb, int64_t nb, int64_t ldb, int64_t d, int metric,
                const T* cuts, int ncuts, bool weighted, int64_t* total, int* rows) {
  if (metric != SS_SIM_COSINE && metric != SS_SIM_TANIMOTO && metric != SS_SIM_DICE)
    return fail(SS_EINVAL, "dot profile: unknown metric %d", metric);
  const bool sym = !Fb;
  if (sym) {
    Fb = Fa;
    nb = na;
    ldb = lda;
  }
  DevBuf<T> norm_a, norm_b;
  return profile_drive(
      "dot profile", na, nb, sym, ncuts, total, rows,
      [&] {
        SS_TRY(refuse_nan_rows<T>("dot profile", Fa, na, lda, sym ? nullptr : Fb, nb, ldb, d));
        if (na == 0 || nb == 0) return (int)SS_OK;
        SS_TRY(norm_a.alloc((size_t)na));
        SS_TRY(dot_row_norms<T>(Fa, na, lda, d, norm_a.p));
        if (!sym) {
          SS_TRY(norm_b.alloc((size_t)nb));
          SS_TRY(dot_row_norms<T>(Fb, nb, ldb, d, norm_b.p));
        }
        return (int)SS_OK;
      },
      [&](dim3 grid, int64_t nti, int* ghist) {
        auto* kernel = sym ? dot_profile_kernel<T, true> : dot_profile_kernel<T, false>;
        hipLaunchKernelGGL(kernel, grid, dim3(dottile::NT), 0, ctx().stream, Fa, na, lda, Fb, nb, ldb, d, norm_a.p,
                           sym ? norm_a.p : norm_b.p, metric, 0, 0, pack_cuts<T>(cuts, ncuts), weighted ? 1 : 0, nti,
                           ghist);
      });
}

int dot_profile_h16(const uint16_t* Fa, int64_t na, int64_t lda, const uint16_t* Fb, int64_t nb, int64_t ldb, int64_t d,
                    int storage, int metric, const float* cuts, int ncuts, bool weighted, int64_t* total, int* rows) {
  if (storage != SS_H16_BF16 && storage != SS_H16_F16) return fail(SS_EINVAL, "dot_h16 profile: unknown storage %d", storage);
  if (metric != SS_SIM_COSINE && metric != SS_SIM_TANIMOTO && metric != SS_SIM_DICE)
    return fail(SS_EINVAL, "dot_h16 profile: unknown metric %d", metric);
  const bool sym = !Fb;
  if (sym) {
    Fb = Fa;
    nb = na;
    ldb = lda;
  }
  DevBuf<float> norm_a, norm_b;
  return profile_drive(
      "dot_h16 profile", na, nb, sym, ncuts, total, rows,
      [&] {
        SS_TRY(h16_refuse_nan_rows(storage, Fa, na, lda, sym ? nullptr : Fb, nb, ldb, d));
        if (na == 0 || nb == 0) return (int)SS_OK;
        SS_TRY(norm_a.alloc((size_t)na));
        SS_TRY(h16_row_norms(storage, Fa, na, lda, d, norm_a.p));
        if (!sym) {
          SS_TRY(norm_b.alloc((size_t)nb));
          SS_TRY(h16_row_norms(storage, Fb, nb, ldb, d, norm_b.p));
        }
        return (int)SS_OK;
      },
      [&](dim3 grid, int64_t nti, int* ghist) {
        using dottile::Bf16;
        using dottile::F16;
        auto* kernel = storage == SS_H16_BF16
                           ? (sym ? dot_profile_kernel<float, true, Bf16> : dot_profile_kernel<float, false, Bf16>)
                           : (sym ? dot_profile_kernel<float, true, F16> : dot_profile_kernel<float, false, F16>);
        hipLaunchKernelGGL(kernel, grid, dim3(dottile::NT), 0, ctx().stream, Fa, na, lda, Fb, nb, ldb, d, norm_a.p,
                           sym ? norm_a.p : norm_b.p, metric, h16_fast(Fa, lda) ? 1 : 0, h16_fast(Fb, ldb) ? 1 : 0,
                           pack_cuts<float>(cuts, ncuts), weighted ? 1 : 0, nti, ghist);
      });
}

template int tanimoto_profile<float>(const uint64_t*, int64_t, const uint64_t*, int64_t, int64_t, const float*, int, bool,
                                     int64_t*, int*);
template int tanimoto_profile<double>(const uint64_t*, int64_t, const uint64_t*, int64_t, int64_t, const double*, int,
                                      bool, int64_t*, int*);
template int jaccard_profile<float>(const float*, int64_t, int64_t, const float*, int64_t, int64_t, int64_t, const float*,
                                    int, bool, int64_t*, int*);
template int jaccard_profile<double>(const double*, int64_t, int64_t, const double*, int64_t, int64_t, int64_t,
                                     const double*, int, bool, int64_t*, int*);
template int dot_profile<float>(const float*, int64_t, int64_t, const float*, int64_t, int64_t, int64_t, int,
                                const float*, int, bool, int64_t*, int*);
template int dot_profile<double>(const double*, int64_t, int64_t, const double*, int64_t, int64_t, int64_t, int,
                                 const double*, int, bool, int64_t*, int*);

}  // namespace ss
