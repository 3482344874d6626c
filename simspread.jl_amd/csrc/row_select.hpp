// Device skeleton of a per-row selection fused into the all-pairs tile pass (neighbour_floor.hip): a workgroup of
// (TILE / RB) x (TILE / RB) = 256 threads that each hold an RB x RB register block of pair similarities keeps, for ROWS
// rows of its strip, the k largest positive values seen so far while it walks column tiles.  It sees the register
// blocks only, not how a similarity is computed, so any tiled producer can select with it.
//
// Only the multiset of the k largest values is kept, so which thread wins a slot does not matter: the k-th largest of a
// multiset does not depend on the order of arrival, and the result is bitwise repeatable although slots are claimed with
// LDS integer atomics.  No float atomics.
//
// Layout (LDS): list[slot][row] and cand[slot][row], the row running fastest, so that the one thread that owns a row
// (thread r < ROWS owns row r) scans its list with consecutive lanes on consecutive banks, whatever k is.  thr[row] is
// the row's acceptance bound: +0 while its list holds fewer than k values (every positive value is taken), then the
// smallest value of the list -- a candidate is interesting only if it is strictly greater.
//
// absorb() takes one tile in rounds.  In a round every thread offers its values that beat thr[row] and claims a slot of
// the row's candidate buffer (CAND slots) with atomicAdd; those that find the buffer full stay pending.  Then the row
// owners merge the buffers into the lists and raise thr.  A row with pending candidates absorbs min(CAND, pending) of
// them per round and a tile offers a row at most TILE candidates, so TILE / CAND rounds always suffice: that is the
// loop bound, and the loop leaves earlier when a block-wide vote finds nothing pending.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace ss {

constexpr int ROW_SELECT_LIST_BYTES = 32 * 1024;  // lists of a block: ROWS * k * sizeof(T) must fit (host-side check)

template <class T, int TILE, int RB, int ROWS>
struct RowSelect {
  static constexpr int CAND = 8;  // candidate slots per row and round
  static constexpr int LIST = ROW_SELECT_LIST_BYTES / (int)sizeof(T);
  static_assert(ROWS % RB == 0 && TILE % ROWS == 0 && ROWS <= 256, "whole thread rows, one owner thread per row");

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

  // One tile.  Thread (tx, ty) holds rows RB * ty + a of the strip in s[a][b]; selected: those rows are the block's
  // local rows lr0 + a (0 <= lr0, lr0 + RB <= ROWS).  s holds the pair similarities of the thread, +0 where the row or
  // the column does not exist; it is consumed: an offered value is replaced by +0, which no bound lets through.  Every
  // thread of the block must call it (it synchronises).
  __device__ __forceinline__ void absorb(int lr0, bool selected, int k, int& cnt, T (&s)[RB][RB]) {
    const int tid = threadIdx.x;
#pragma unroll 1
    for (int round = 0; round < TILE / CAND; ++round) {
      bool pending = false;
      if (selected) {
#pragma unroll
        for (int a = 0; a < RB; ++a) {
          const T th = thr[lr0 + a];
#pragma unroll
          for (int b = 0; b < RB; ++b) {
            if (!(s[a][b] > th)) continue;
            const int slot = atomicAdd(&ccnt[lr0 + a], 1);
            if (slot < CAND) {
              cand[slot][lr0 + a] = s[a][b];
              s[a][b] = T(0);
            } else {
              pending = true;
            }
          }
        }
      }
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
};

}  // namespace ss
