// Device skeleton of the fused thresholded-similarity producers (fingerprint.hip, jaccard_csr.hip, dot_csr.hip): which
// TILE x TILE tile of (row, column) pairs a block owns, and the epilogue that turns a register block of decided pairs
// into CSR slots.  The host side of the same protocol is PairCsr (graph.hpp, pair_csr.hip).
//
//   count  per (column tile, row): the number of kept entries -> counts[jt * rows + i]
//   fill   the same tile again, each slot written at ptr[i] + counts[jt * rows + i] (by then the in-row offset of the
//          tile) + its offset inside the tile, in column order
// In symmetric mode (Fb = Fa) only the tiles on and above the diagonal run, as a 1-D grid over the triangle; an
// off-diagonal tile emits its pairs for its rows and, mirrored, for its columns (na == nb there).  Positions come from
// scans, never from atomics, so the output is bitwise repeatable.
// A third epilogue next to count and fill, pair_tile_profile at the end of this file, counts the kept pairs of every row
// at up to 32 cuts at once (cut_profile.hip).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace ss {

// tile (it, jt) of the upper triangle (it <= jt) from its linear index t: rows of the triangle hold nt, nt-1, ... tiles
__device__ __forceinline__ void triangle_tile(int64_t t, int64_t nt, int64_t& it, int64_t& jt) {
  // first tile of row r: r * nt - r * (r - 1) / 2
  const double b = 2.0 * (double)nt + 1.0;
  int64_t r = (int64_t)((b - sqrt(b * b - 8.0 * (double)t)) * 0.5);
  if (r < 0) r = 0;
  if (r > nt - 1) r = nt - 1;
  while (r > 0 && r * nt - r * (r - 1) / 2 > t) --r;
  while (r + 1 < nt && (r + 1) * nt - (r + 1) * r / 2 <= t) ++r;
  it = r;
  jt = r + (t - (r * nt - r * (r - 1) / 2));
}

struct PairTile {
  int64_t tlin;    // index of the block in launch order (the slot of its tile_nz flag)
  int64_t it, jt;  // row tile, column tile
  int64_t i0, j0;  // first row, first column
  bool mirror;     // SYM and off the diagonal: the tile also stands for (jt, it)
};

// PairTile::tlin alone: what a fill pass needs to leave a tile without a flag before it resolves anything else
template <bool SYM>
__device__ __forceinline__ int64_t pair_tile_index() {
  return SYM ? (int64_t)blockIdx.x : (int64_t)blockIdx.y * gridDim.x + blockIdx.x;
}

// The tile of this block.  SYM: a 1-D grid over the upper triangle of nti x nti tiles; otherwise blockIdx = (jt, it).
template <bool SYM, int TILE>
__device__ __forceinline__ PairTile pair_tile(int64_t nti) {
  PairTile t;
  t.tlin = pair_tile_index<SYM>();
  if (SYM) {
    triangle_tile(t.tlin, nti, t.it, t.jt);
  } else {
    t.it = blockIdx.y;
    t.jt = blockIdx.x;
  }
  t.i0 = t.it * TILE;
  t.j0 = t.jt * TILE;
  t.mirror = SYM && t.it != t.jt;
  return t;
}

// The emit epilogue of a kernel whose (TILE / RC) x (TILE / RA) threads each hold an RA x RC block of pairs: thread
// (tx, ty) = (tid % (TILE / RC), tid / (TILE / RC)) owns rows RA * ty + a and columns RC * tx + b of the tile.
// keep(a, b, v) decides pair (a, b) of the calling thread and sets its stored value v; it is asked again for v when
// the pair is written.  Pairs past the last row or column are dropped here.
//   FILL == false: counts[jt * na + i] (and the mirror's counts[it * na + j]) = kept entries of the slot
//   FILL == true:  the entries, rows in column order and mirrored columns in row order; *not_binary = 1 when a value
//                  is not 1
//   NZ:            tile_nz[tlin] = 1 when the tile kept a pair (count pass; the caller's fill pass may skip the others)
template <class T, int TILE, int RA, int RC, bool SYM, bool FILL, bool NZ, class Keep>
__device__ __forceinline__ void pair_tile_emit(const PairTile& t, int64_t na, int64_t nb, Keep keep, int* counts,
                                               int* tile_nz, const int64_t* ptr, int* oidx, T* oval, int* not_binary) {
  constexpr int NTX = TILE / RC, NTY = TILE / RA;  // thread columns, thread rows
  static_assert(RA <= 32 && RC <= 32, "a row / column of the register block is one 32-bit mask");
  static_assert(NTX * NTY >= 2 * TILE, "one thread per row and per mirrored column in the scans");
  __shared__ int rc[TILE][NTX + 1];  // [row][tx]: kept entries of the row in the columns of thread column tx -> offsets
  __shared__ int cc[TILE][NTY + 1];  // [column][ty]: the same for the mirror; never touched, so no LDS, unless SYM
  const int tid = threadIdx.x, tx = tid % NTX, ty = tid / NTX;
  const int64_t i0 = t.i0, j0 = t.j0;

  // which pairs are kept: bit b of rmask[a] = bit a of cmask[b] = pair (row RA*ty + a, column RC*tx + b)
  uint32_t rmask[RA], cmask[RC];
#pragma unroll
  for (int b = 0; b < RC; ++b) cmask[b] = 0;
#pragma unroll
  for (int a = 0; a < RA; ++a) {
    rmask[a] = 0;
    const bool va = i0 + RA * ty + a < na;
#pragma unroll
    for (int b = 0; b < RC; ++b) {
      T v;
      const bool k = va && j0 + RC * tx + b < nb && keep(a, b, v);
      rmask[a] |= (k ? 1u : 0u) << b;
      cmask[b] |= (k ? 1u : 0u) << a;
    }
  }
  bool any = false;
#pragma unroll
  for (int a = 0; a < RA; ++a) {
    rc[RA * ty + a][tx] = __popc(rmask[a]);
    any |= rmask[a] != 0;
  }
  if constexpr (SYM) {
    if (t.mirror) {
#pragma unroll
      for (int b = 0; b < RC; ++b) cc[RC * tx + b][ty] = __popc(cmask[b]);
    }
  }
  if constexpr (NZ) {
    any = __syncthreads_or(any);
    if (!FILL && tid == 0) tile_nz[t.tlin] = any ? 1 : 0;
  } else {
    __syncthreads();
  }
  // exclusive scans: threads 0..TILE-1 over the NTX thread columns of row tid, threads TILE..2*TILE-1 over the NTY
  // thread rows of column tid - TILE
  if (tid < TILE) {
    int run = 0;
#pragma unroll
    for (int q = 0; q < NTX; ++q) {
      const int c = rc[tid][q];
      rc[tid][q] = run;
      run += c;
    }
    if (!FILL && i0 + tid < na) counts[t.jt * na + i0 + tid] = run;
  } else if constexpr (SYM) {
    if (tid < 2 * TILE && t.mirror) {
      const int r = tid - TILE;
      int run = 0;
#pragma unroll
      for (int q = 0; q < NTY; ++q) {
        const int c = cc[r][q];
        cc[r][q] = run;
        run += c;
      }
      if (!FILL && j0 + r < nb) counts[t.it * na + j0 + r] = run;  // SYM: na == nb
    }
  }
  if constexpr (FILL) {
    __syncthreads();
    bool nb_flag = false;
#pragma unroll
    for (int a = 0; a < RA; ++a) {
      if (!rmask[a]) continue;
      const int64_t i = i0 + RA * ty + a;
      int64_t o = ptr[i] + counts[t.jt * na + i] + rc[RA * ty + a][tx];
#pragma unroll
      for (int b = 0; b < RC; ++b) {
        if (!((rmask[a] >> b) & 1u)) continue;
        T v;
        (void)keep(a, b, v);
        oidx[o] = (int)(j0 + RC * tx + b);
        if (oval) oval[o] = v;
        nb_flag |= (v != T(1));
        ++o;
      }
    }
    if constexpr (SYM) {
      if (t.mirror) {
#pragma unroll
        for (int b = 0; b < RC; ++b) {
          if (!cmask[b]) continue;
          const int64_t j = j0 + RC * tx + b;
          int64_t o = ptr[j] + counts[t.it * na + j] + cc[RC * tx + b][ty];
#pragma unroll
          for (int a = 0; a < RA; ++a) {
            if (!((cmask[b] >> a) & 1u)) continue;
            T v;
            (void)keep(a, b, v);
            oidx[o] = (int)(i0 + RA * ty + a);
            if (oval) oval[o] = v;
            ++o;
          }
        }
      }
    }
    if (nb_flag) *not_binary = 1;
  }
}

// ---- The count epilogue (cut_profile.hip): a cutoff profile.  Next to "emit" (which pairs stay at one alpha, and
// where) it answers "how many pairs of every row stay at each of up to 32 ascending cuts", without positions.
constexpr int PROFILE_CUTS_MAX = 32;
template <class T>
struct ProfileCuts {  // a kernel argument: the cuts, nondecreasing, no NaN (host-checked)
  T c[PROFILE_CUTS_MAX];
  int n;  // 1 .. PROFILE_CUTS_MAX
};

// m = #{b : s >= cuts[b]}: binary search over the nondecreasing cuts with the producers' own >=; a NaN s gives 0
template <class T>
__device__ __forceinline__ int profile_bin(const T* cuts, int ncuts, T s) {
  if (!(s >= cuts[0])) return 0;  // most pairs of a sparse graph
  int lo = 1, hi = ncuts;         // s >= cuts[b] for b < lo, not for b >= hi
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (s >= cuts[mid]) lo = mid + 1;
    else hi = mid;
  }
  return lo;
}

// The count epilogue of a kernel whose NT threads each hold NP pairs of the tile.  pair(e, row, col) gives the tile-local
// row and column and returns the similarity s of the calling thread's pair e (e is a constant after unrolling, so the
// caller's register block is indexed statically).  Pairs past the last row or column are dropped here.
//   v = weighted ? s : 1; pair (i, j) counts for cut b iff s >= cuts[b] and v != 0; a NaN s counts for none
//   every held pair finds its bin m = #{b : s >= cuts[b]} (0 when v == 0) and adds 1 to the tile's LDS histogram
//   hist[row][m]; after the tile the non-zero bins are added to ghist[(i0 + row) * (ncuts + 1) + m].  A mirrored tile
//   (SYM, off the diagonal) then clears the histogram and runs the same bins through it by column, for rows j0 + col.
//   Bin 0 (the pair counts for no cut) is never read by the finish, so nothing is added to it.
// Only integers are added (LDS and global integer atomics), so ghist does not depend on the order: bitwise repeatable.
// A bin of the tile's histogram holds at most TILE = 128 pairs (one row or one column of the tile), so it is one byte,
// four to a 32-bit word, and an add is an integer LDS add of 1 << 8 * (byte of the word), which never carries into the
// next bin: TILE x 33 bytes = 4.1 KB instead of 16.5 KB of ints.  That keeps the 16-bit profile kernel (36 KB of
// staging) at three workgroups per CU, like its producer.  There is still one histogram, used twice by a mirrored tile:
// the bins of a thread's pairs wait in NP / 4 registers meanwhile.
template <class T, int TILE, int NT, int NP, bool SYM, class Pair>
__device__ __forceinline__ void pair_tile_profile(const PairTile& t, int64_t na, int64_t nb, const ProfileCuts<T>& cuts,
                                                  bool weighted, int* __restrict__ ghist, Pair pair) {
  static_assert(NP % 4 == 0, "four 8-bit bins per register");
  static_assert(TILE <= 255, "a bin of the tile's histogram is one byte");
  constexpr int HS = PROFILE_CUTS_MAX + 1;  // bins (bytes) per row of the histogram
  constexpr int HW = (TILE * HS + 3) / 4;   // its words
  __shared__ T cuts_s[PROFILE_CUTS_MAX];
  __shared__ uint32_t hist[HW];
  const int tid = threadIdx.x;
  const int ncuts = cuts.n, nbin = ncuts + 1;
  auto clear = [&] {
    for (int e = tid; e < HW; e += NT) hist[e] = 0;
  };
  auto add = [&](int r, int m) {
    const int at = r * HS + m;
    atomicAdd(&hist[at >> 2], 1u << (8 * (at & 3)));
  };
  // the non-zero bins of the histogram's rows into the table rows r0 + r (a non-zero bin: that row exists)
  auto merge = [&](int64_t r0) {
    for (int e = tid; e < TILE * ncuts; e += NT) {
      const int r = e / ncuts, m = 1 + e % ncuts;
      const int at = r * HS + m;
      const int c = (int)((hist[at >> 2] >> (8 * (at & 3))) & 0xffu);
      if (c) atomicAdd(&ghist[(r0 + r) * nbin + m], c);
    }
  };
  if (tid < ncuts) cuts_s[tid] = cuts.c[tid];
  clear();
  __syncthreads();

  uint32_t bins[NP / 4];
#pragma unroll
  for (int q = 0; q < NP / 4; ++q) bins[q] = 0;
#pragma unroll
  for (int e = 0; e < NP; ++e) {
    int row, col;
    const T s = pair(e, row, col);
    const bool live = t.i0 + row < na && t.j0 + col < nb && (!weighted || s != T(0));
    const int m = live ? profile_bin<T>(cuts_s, ncuts, s) : 0;
    bins[e / 4] |= (uint32_t)m << (8 * (e % 4));
    if (m) add(row, m);
  }
  __syncthreads();
  merge(t.i0);
  if constexpr (SYM) {
    if (!t.mirror) return;  // uniform over the block
    __syncthreads();
    clear();
    __syncthreads();
#pragma unroll
    for (int e = 0; e < NP; ++e) {
      const int m = (bins[e / 4] >> (8 * (e % 4))) & 0xff;
      if (m) {
        int row, col;
        (void)pair(e, row, col);
        add(col, m);
      }
    }
    __syncthreads();
    merge(t.j0);  // SYM: na == nb
  }
}

}  // namespace ss
