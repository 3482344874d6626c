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

}  // namespace ss
