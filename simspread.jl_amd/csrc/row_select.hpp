// Device skeleton of a per-row selection fused into the all-pairs tile pass (neighbour_floor.hip, real_floor.hip): a
// workgroup whose threads hold the pair similarities of one TILE x TILE tile in registers keeps, for ROWS rows of its
// strip, the k largest positive values seen so far while it walks column tiles.  It sees the registers only, not how a
// similarity is computed, so any tiled producer can select with it.  Two entries, one per register layout:
//   absorb       every thread holds an RA x RC block of pairs, all of whose rows it knows from its thread row (the
//                fingerprint and the weighted-Jaccard tiles)
//   absorb_flat  every thread holds a flat array of values and a functor says which row each belongs to (the
//                accumulators of a matrix-core tile: a lane's values lie in many rows)
//
// Only the multiset of the k largest values is kept, so which thread wins a slot does not matter: the k-th largest of a
// multiset does not depend on the order of arrival, and the result is bitwise repeatable although slots are claimed with
// LDS integer atomics.  No float atomics.
//
// Layout (LDS): list[slot][row] and cand[slot][row], the row running fastest, so that the one thread that owns a row
// (thread r < ROWS owns row r) scans its list with consecutive lanes on consecutive banks, whatever k is.  thr[row] is
// the row's acceptance bound: +0 while its list holds fewer than k values (every positive value is taken), then the
// smallest value of the list -- a candidate is interesting only if it is strictly greater.  The list holds LIST values:
// ROWS * k <= LIST is the caller's host-side check, and LIST is a template argument so that a kernel whose tile staging
// is large selects for fewer rows with a shorter list.
//
// A tile is taken in rounds.  In a round every thread offers its values that beat thr[row] and claims a slot of the
// row's candidate buffer (CAND slots) with atomicAdd; those that find the buffer full stay pending.  Then the row
// owners merge the buffers into the lists and raise thr.  A row with pending candidates absorbs min(CAND, pending) of
// them per round and a tile offers a row at most TILE candidates, so TILE / CAND rounds always suffice: that is the
// loop bound, and the loop leaves earlier when a block-wide vote finds nothing pending.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace ss {

constexpr int ROW_SELECT_LIST_BYTES = 32 * 1024;  // default lists of a block: ROWS * k * sizeof(T) must fit

template <class T, int TILE, int ROWS, int LIST = ROW_SELECT_LIST_BYTES / (int)sizeof(T)>
struct RowSelect {
  static constexpr int CAND = 8;  // candidate slots per row and round
  static_assert(TILE % ROWS == 0 && ROWS <= 256, "whole strips, one owner thread per row");
  static_assert(LIST >= ROWS, "at least k = 1");

  T list[LIST];  // [slot][row], slots 0 .. k-1
  T cand[CAND][ROWS];
  T thr[ROWS];
  int ccnt[ROWS];  // candidates offered to the row this round (may exceed CAND: the excess stays pending)
  int lcnt[ROWS];  // values in the row's list, written by store()

  // Every thread of the block; cnt is the owner thread's count of its row's list (a register carried across tiles).
  __device__ __forceinline__ void init(int& cnt) {
    const int tid = threadIdx.x;
    cnt = 0;
    if (tid < ROWS) {
      thr[tid] = T(0);
      ccnt[tid] = 0;
    }
    __syncthreads();
  }

  // One tile.  Thread row ty of the block holds rows RA * ty + a of the strip in s[a][b]; selected: those rows are the
  // block's local rows lr0 + a (0 <= lr0, lr0 + RA <= ROWS).  s holds the pair similarities of the thread, +0 where the
  // row or the column does not exist; it is consumed: an offered value is replaced by +0, which no bound lets through.
  // Every thread of the block must call it (it synchronises).
  template <int RA, int RC>
  __device__ __forceinline__ void absorb(int lr0, bool selected, int k, int& cnt, T (&s)[RA][RC]) {
    static_assert(ROWS % RA == 0, "whole thread rows");
    rounds(k, cnt, [&]() {
      bool pending = false;
      if (selected) {
#pragma unroll
        for (int a = 0; a < RA; ++a) {
          const T th = thr[lr0 + a];
#pragma unroll
          for (int b = 0; b < RC; ++b) pending |= offer(lr0 + a, th, s[a][b]);
        }
      }
      return pending;
    });
  }

  // One tile held as NV values per thread: value e belongs to the block's local row row_of(e), or to none of them when
  // row_of(e) < 0.  v as s of absorb().  Every thread of the block must call it (it synchronises).
  template <int NV, class RowOf>
  __device__ __forceinline__ void absorb_flat(int k, int& cnt, T (&v)[NV], RowOf row_of) {
    rounds(k, cnt, [&]() {
      bool pending = false;
#pragma unroll
      for (int e = 0; e < NV; ++e) {
        const int r = row_of(e);
        if (r >= 0) pending |= offer(r, thr[r], v[e]);
      }
      return pending;
    });
  }

  // out[(row0 + r) * k + j] = the j-th value of row r's list, +0 past its end, for the rows r < ROWS with
  // row0 + r < nrows.  Every thread of the block.
  __device__ __forceinline__ void store(int64_t row0, int64_t nrows, int k, int cnt, T* __restrict__ out) {
    const int tid = threadIdx.x;
    if (tid < ROWS) lcnt[tid] = cnt;
    __syncthreads();
    for (int e = tid; e < ROWS * k; e += blockDim.x) {
      const int r = e / k, j = e - r * k;
      if (row0 + r < nrows) out[(row0 + r) * k + j] = j < lcnt[r] ? list[j * ROWS + r] : T(0);
    }
  }

 private:
  // value x of local row r against the row's bound th: taken into the candidate buffer (and replaced by +0) when a slot
  // is free; true when it beats th and has to wait for the next round
  __device__ __forceinline__ bool offer(int r, T th, T& x) {
    if (!(x > th)) return false;
    const int slot = atomicAdd(&ccnt[r], 1);
    if (slot >= CAND) return true;
    cand[slot][r] = x;
    x = T(0);
    return false;
  }

  // the rounds of one tile: offer_all() offers the calling thread's values and says whether one of them stays pending
  template <class Offer>
  __device__ __forceinline__ void rounds(int k, int& cnt, Offer offer_all) {
    const int tid = threadIdx.x;
#pragma unroll 1
    for (int round = 0; round < TILE / CAND; ++round) {
      const bool pending = offer_all();
      __syncthreads();
      if (tid < ROWS) {
        const int n = min(ccnt[tid], CAND);
        ccnt[tid] = 0;
        T th = thr[tid];
        for (int c = 0; c < n; ++c) {
          const T v = cand[c][tid];
          bool rescan = false;
          if (cnt < k) {
            list[cnt * ROWS + tid] = v;
            ++cnt;
            rescan = cnt == k;
          } else if (v > th) {
            int at = 0;
            for (int j = 0; j < k; ++j)
              if (list[j * ROWS + tid] == th) at = j;
            list[at * ROWS + tid] = v;
            rescan = true;
          }
          if (rescan) {
            th = list[tid];
            for (int j = 1; j < k; ++j) {
              const T x = list[j * ROWS + tid];
              th = x < th ? x : th;
            }
          }
        }
        thr[tid] = th;
      }
      if (!__syncthreads_or(pending)) break;
    }
  }
};

}  // namespace ss
