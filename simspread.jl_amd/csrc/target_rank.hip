// Per-target ranking metrics of whole sweeps without the score matrix (include/simspread_hip_target_rank.h holds the
// contract, the two-pass argument and the count layout).  The histograms are rank_rows.hip's gap / tieG / tieK, taken
// per TARGET over the negatives only, against that target's positives sorted by (score descending, row ascending);
// rr_finish's collapse of the trapezoid sums onto the positive score groups then gives the six numbers.
//
//   collect  tr_nan_kernel streams the block once for NaN; tr_gather_kernel copies the score of every label entry, with
//            its target and row id, behind the handle's triples (one wave per row, entry e of the block at slot e, so
//            the collected order is the blocks' label order).
//   seal     three stable rocPRIM radix sorts of a permutation -- by row, by inverted score key, by target -- then a
//            gather, the offsets by binary search in the sorted targets, and the route of every tile of 64 targets.
//   check    (count phase, first) tr_check_kernel looks every label entry of the block up in the sealed table by
//            (target, score key, row) and compares the score bits.
//   count    tr_count_kernel, the hot kernel: a workgroup owns a tile of 64 consecutive targets and up to TR_RPW rows.
//            Thread (c, q) owns target column c: its four waves q take the rows q, q + 4, ..., so a wave instruction
//            reads 64 consecutive scores of one row (coalesced, straight from global memory: no thread needs another
//            thread's score, so no LDS transpose) and every per-target quantity -- P_t, the smallest positive key, the
//            counters -- lives in that thread's registers; the four waves add theirs up in LDS at the end, so a workgroup
//            makes one global add per target for each of them.  The labels of the workgroup's rows are 64-bit masks in LDS,
//            built beforehand by one binary search per row in its CSR positives.  A negative below its target's smallest
//            positive (in the sparse regime nearly all: zeros) leaves after one compare into a register counter; the
//            rest are searched by binary search over (key, row) in the tile's sealed keys -- in LDS, with the tile's
//            histograms in LDS too (ds_add_u32, then one global add per touched bin), or, for a tile that exceeds the
//            LDS budget, in global memory with global integer adds.  nz / min / max of every score ride along.
//   metrics  tr_metrics_kernel: a workgroup per target scans gap + tieK and gap + tieG (positives added in) through
//            global scratch and sums rr_finish's terms in a fixed order.
// Only integer atomics; the counts are sums of integers, so neither block order nor scheduling reaches them.
#include <hip/hip_runtime.h>

#include <cstring>
#include <vector>

#include <rocprim/rocprim.hpp>

#include "graph.hpp"

namespace ss {

namespace {

constexpr int TR_THREADS = 256;
constexpr int TR_WAVES = TR_THREADS / 64;
constexpr int TR_TILE = 64;        // targets per count workgroup
constexpr int TR_RPW = 512;        // rows per count workgroup
constexpr int TR_LDS_POS = 2048;   // sealed positives of a tile on the LDS route
constexpr int TR_UNROLL = 4;       // rows in flight per thread

template <class T>
using tr_key_t = pool_key_t<T>;

// order-preserving unsigned key of a score as rank_rows.hip compares scores inside a row: by value, -0.0 == +0.0
__device__ inline uint32_t tr_key(float v) {
  const uint32_t u = __float_as_uint(v == 0.f ? 0.f : v);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ inline uint64_t tr_key(double v) {
  const uint64_t u = (uint64_t)__double_as_longlong(v == 0.0 ? 0.0 : v);
  return (u >> 63) ? ~u : (u | (1ULL << 63));
}
__device__ inline uint32_t tr_bits(float v) { return __float_as_uint(v); }
__device__ inline uint64_t tr_bits(double v) { return (uint64_t)__double_as_longlong(v); }
__device__ inline double tr_nan() { return __longlong_as_double(0x7ff8000000000000LL); }

inline int tr_blocks(int64_t n, int64_t cap = 4096) {
  int64_t g = (n + TR_THREADS - 1) / TR_THREADS;
  return (int)(g < 1 ? 1 : g > cap ? cap : g);
}

// ------------------------------------------------------------------ collect
template <class T>
__global__ void __launch_bounds__(TR_THREADS) tr_nan_kernel(const T* __restrict__ yhat, int64_t ld, int64_t nb,
                                                            int64_t nt, unsigned long long* __restrict__ flag) {
  bool nan = false;
  for (int64_t r = blockIdx.y; r < nb; r += gridDim.y) {
    const T* row = yhat + r * ld;
    for (int64_t t = (int64_t)blockIdx.x * TR_THREADS + threadIdx.x; t < nt; t += (int64_t)gridDim.x * TR_THREADS) {
      const T v = row[t];
      nan |= v != v;
    }
  }
  if (nan) flag[0] = 1ULL;
}

template <class T, class PtrT>
__global__ void __launch_bounds__(TR_THREADS) tr_gather_kernel(const PtrT* __restrict__ yptr, int64_t shift,
                                                               const int* __restrict__ yidx, int base,
                                                               const T* __restrict__ yhat, int64_t ld, int64_t nb,
                                                               int64_t row_begin, const int* __restrict__ rowmap,
                                                               int* __restrict__ ct, int64_t* __restrict__ cr,
                                                               T* __restrict__ cv) {
  const int lane = threadIdx.x & 63;
  const int64_t e00 = (int64_t)yptr[0] - shift;
  for (int64_t r = (int64_t)blockIdx.x * TR_WAVES + (threadIdx.x >> 6); r < nb; r += (int64_t)gridDim.x * TR_WAVES) {
    const int64_t e0 = (int64_t)yptr[r] - shift, e1 = (int64_t)yptr[r + 1] - shift;
    const int64_t rid = rowmap ? (int64_t)rowmap[r] : row_begin + r;
    for (int64_t e = e0 + lane; e < e1; e += 64) {
      const int t = yidx[e] - base;
      ct[e - e00] = t;
      cr[e - e00] = rid;
      cv[e - e00] = yhat[r * ld + t];
    }
  }
}

// flag bits (flag[0]): 1 NaN, 2 target out of range, 4 row out of range
template <class T>
__global__ void __launch_bounds__(TR_THREADS) tr_import_check_kernel(const int* __restrict__ t, const int64_t* __restrict__ r,
                                                                     const T* __restrict__ v, int64_t n, int64_t nt,
                                                                     unsigned long long* __restrict__ flag) {
  unsigned long long f = 0;
  for (int64_t i = (int64_t)blockIdx.x * TR_THREADS + threadIdx.x; i < n; i += (int64_t)gridDim.x * TR_THREADS) {
    if (v[i] != v[i]) f |= 1;
    if (t[i] < 0 || (int64_t)t[i] >= nt) f |= 2;
    if (r[i] < 0 || r[i] >= (1LL << 31)) f |= 4;
  }
  if (f) atomicOr(flag, f);
}

// ------------------------------------------------------------------ seal
// sort key of pass p for the entry perm[i]: 0 the row, 1 the inverted score key (ascending = score descending), 2 the
// target
template <class T>
__global__ void __launch_bounds__(TR_THREADS) tr_field_kernel(int pass, const unsigned* __restrict__ perm,
                                                              const int* __restrict__ ct, const int64_t* __restrict__ cr,
                                                              const T* __restrict__ cv, int64_t n,
                                                              uint64_t* __restrict__ key) {
  for (int64_t i = (int64_t)blockIdx.x * TR_THREADS + threadIdx.x; i < n; i += (int64_t)gridDim.x * TR_THREADS) {
    const unsigned p = perm[i];
    key[i] = pass == 0 ? (uint64_t)cr[p] : pass == 1 ? (uint64_t)(tr_key_t<T>)~tr_key(cv[p]) : (uint64_t)ct[p];
  }
}

__global__ void __launch_bounds__(TR_THREADS) tr_iota_kernel(unsigned* __restrict__ perm, int64_t n) {
  for (int64_t i = (int64_t)blockIdx.x * TR_THREADS + threadIdx.x; i < n; i += (int64_t)gridDim.x * TR_THREADS)
    perm[i] = (unsigned)i;
}

template <class T>
__global__ void __launch_bounds__(TR_THREADS) tr_permute_kernel(const unsigned* __restrict__ perm,
                                                                const int* __restrict__ ct, const int64_t* __restrict__ cr,
                                                                const T* __restrict__ cv, int64_t n, int* __restrict__ st,
                                                                int64_t* __restrict__ sr, T* __restrict__ sv) {
  for (int64_t i = (int64_t)blockIdx.x * TR_THREADS + threadIdx.x; i < n; i += (int64_t)gridDim.x * TR_THREADS) {
    const unsigned p = perm[i];
    st[i] = ct[p];
    sr[i] = cr[p];
    sv[i] = cv[p];
  }
}

// off[t] = entries with a target < t, t = 0..nt
__global__ void __launch_bounds__(TR_THREADS) tr_offsets_kernel(const int* __restrict__ st, int64_t n, int64_t nt,
                                                                int* __restrict__ off) {
  for (int64_t t = (int64_t)blockIdx.x * TR_THREADS + threadIdx.x; t <= nt; t += (int64_t)gridDim.x * TR_THREADS) {
    int64_t lo = 0, hi = n;
    while (lo < hi) {
      const int64_t mid = (lo + hi) >> 1;
      if ((int64_t)st[mid] < t) lo = mid + 1;
      else hi = mid;
    }
    off[t] = (int)lo;
  }
}

// route[i] = 1: tile i's positives fit the LDS route (cap each, TR_LDS_POS together); n[0] / n[1] count the two kinds
__global__ void __launch_bounds__(TR_THREADS) tr_route_kernel(const int* __restrict__ off, int64_t nt, int64_t ntiles,
                                                              int cap, unsigned char* __restrict__ route,
                                                              int* __restrict__ n) {
  for (int64_t i = (int64_t)blockIdx.x * TR_THREADS + threadIdx.x; i < ntiles; i += (int64_t)gridDim.x * TR_THREADS) {
    const int64_t t0 = i * TR_TILE, t1 = t0 + TR_TILE < nt ? t0 + TR_TILE : nt;
    bool lds = off[t1] - off[t0] <= TR_LDS_POS;
    for (int64_t t = t0; t < t1; ++t) lds &= off[t + 1] - off[t] <= cap;
    route[i] = lds ? 1 : 0;
    atomicAdd(&n[lds ? 0 : 1], 1);
  }
}

__global__ void __launch_bounds__(TR_THREADS) tr_counts_init_kernel(int64_t* __restrict__ counts, int64_t hist_nz,
                                                                    int64_t nt) {
  for (int64_t i = (int64_t)blockIdx.x * TR_THREADS + threadIdx.x; i < hist_nz + 2 * nt;
       i += (int64_t)gridDim.x * TR_THREADS)
    counts[i] = i < hist_nz ? 0 : i < hist_nz + nt ? (int64_t)-1 : 0;
}

__global__ void __launch_bounds__(TR_THREADS) tr_delta_init_kernel(unsigned long long* __restrict__ dmm, int64_t nt) {
  for (int64_t i = (int64_t)blockIdx.x * TR_THREADS + threadIdx.x; i < 2 * nt; i += (int64_t)gridDim.x * TR_THREADS)
    dmm[i] = i < nt ? ~0ULL : 0ULL;
}

// ------------------------------------------------------------------ count phase
// every label entry of the block must be a sealed positive with the same score bits
template <class T, class PtrT>
__global__ void __launch_bounds__(TR_THREADS) tr_check_kernel(const PtrT* __restrict__ yptr, int64_t shift,
                                                              const int* __restrict__ yidx, int base,
                                                              const T* __restrict__ yhat, int64_t ld, int64_t nb,
                                                              int64_t row_begin, const int* __restrict__ rowmap,
                                                              const int* __restrict__ off, const int64_t* __restrict__ sr,
                                                              const T* __restrict__ sv,
                                                              unsigned long long* __restrict__ flag) {
  using K = tr_key_t<T>;
  const int lane = threadIdx.x & 63;
  for (int64_t r = (int64_t)blockIdx.x * TR_WAVES + (threadIdx.x >> 6); r < nb; r += (int64_t)gridDim.x * TR_WAVES) {
    const int64_t e0 = (int64_t)yptr[r] - shift, e1 = (int64_t)yptr[r + 1] - shift;
    const int64_t rid = rowmap ? (int64_t)rowmap[r] : row_begin + r;
    for (int64_t e = e0 + lane; e < e1; e += 64) {
      const int t = yidx[e] - base;
      const T v = yhat[r * ld + t];
      const K k = tr_key(v);
      const int o = off[t], P = off[t + 1] - o;
      int lo = 0, hi = P;  // the first entry not before (k, rid)
      while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        const K km = tr_key(sv[o + mid]);
        if (km > k || (km == k && sr[o + mid] < rid)) lo = mid + 1;
        else hi = mid;
      }
      const bool found = lo < P && sr[o + lo] == rid && tr_bits(sv[o + lo]) == tr_bits(v);
      if (!found) atomicMin(&flag[1], ((unsigned long long)rid << 32) | (unsigned long long)(unsigned)t);
    }
  }
}

template <class T, class PtrT>
__global__ void __launch_bounds__(TR_THREADS) tr_count_kernel(
    const T* __restrict__ yhat, int64_t ld, int64_t nt, int64_t nb, int64_t row_begin, const int* __restrict__ rowmap,
    const PtrT* __restrict__ yptr, int64_t shift, const int* __restrict__ yidx, int base, const int* __restrict__ off,
    const int64_t* __restrict__ sr, const T* __restrict__ sv, const unsigned char* __restrict__ route,
    unsigned* __restrict__ dhist, unsigned* __restrict__ dnz, unsigned long long* __restrict__ dmin,
    unsigned long long* __restrict__ dmax, unsigned long long* __restrict__ flag) {
  using K = tr_key_t<T>;
  __shared__ unsigned long long pmask[TR_RPW];
  __shared__ K lkey[TR_LDS_POS];
  __shared__ int lrow[TR_LDS_POS];
  __shared__ unsigned lhist[3 * (TR_LDS_POS + TR_TILE)];
  const int tid = threadIdx.x, c = tid & 63, q = tid >> 6;
  const int64_t t0 = (int64_t)blockIdx.x * TR_TILE;
  const int ntile = nt - t0 < TR_TILE ? (int)(nt - t0) : TR_TILE;
  const int64_t rA = (int64_t)blockIdx.y * TR_RPW;
  const int nr = nb - rA < TR_RPW ? (int)(nb - rA) : TR_RPW;
  const bool lds = route[blockIdx.x] != 0;
  const int pb = off[t0], ptot = off[t0 + ntile] - pb;  // the tile's sealed entries: pb .. pb + ptot
  const int hlen = lds ? 3 * (ptot + ntile) : 0;         // LDS route only (ptot <= TR_LDS_POS)
  unsigned* ghist = dhist + 3 * ((int64_t)pb + t0);      // the tile's histograms: 3 (ptot + ntile) entries
  __shared__ unsigned s_below[TR_TILE], s_nz[TR_TILE];
  __shared__ unsigned long long s_min[TR_TILE], s_max[TR_TILE];
  if (tid < TR_TILE) {
    s_below[tid] = 0;
    s_nz[tid] = 0;
    s_min[tid] = ~0ULL;
    s_max[tid] = 0ULL;
  }

  // label masks of the workgroup's rows: bit i of pmask[r] = target t0 + i is a positive of row rA + r
  for (int r = tid; r < nr; r += TR_THREADS) {
    int64_t lo = (int64_t)yptr[rA + r] - shift;
    const int64_t end = (int64_t)yptr[rA + r + 1] - shift;
    int64_t hi = end;
    const int64_t want = t0 + base;
    while (lo < hi) {
      const int64_t mid = (lo + hi) >> 1;
      if ((int64_t)yidx[mid] < want) lo = mid + 1;
      else hi = mid;
    }
    unsigned long long m = 0;
    for (; lo < end; ++lo) {
      const int64_t d = (int64_t)yidx[lo] - want;
      if (d >= TR_TILE) break;
      m |= 1ULL << d;
    }
    pmask[r] = m;
  }
  if (lds) {
    for (int i = tid; i < ptot; i += TR_THREADS) {
      lkey[i] = tr_key(sv[pb + i]);
      lrow[i] = (int)sr[pb + i];
    }
    for (int i = tid; i < hlen; i += TR_THREADS) lhist[i] = 0;
  }
  __syncthreads();

  if (c < ntile) {
    const int64_t t = t0 + c;
    const int o = off[t] - pb, P = off[t + 1] - pb - o;  // this target's entries inside the tile
    const int64_t hb = 3 * ((int64_t)o + c);             // its gap; tieG at hb + P + 1, tieK at hb + 2 (P + 1)
    const T* gv = sv + pb + o;
    const int64_t* gr = sr + pb + o;
    const K* lk = lkey + o;
    const int* lr = lrow + o;
    unsigned* H = (lds ? lhist : ghist) + hb;
    auto key_at = [&](int i) -> K { return lds ? lk[i] : tr_key(gv[i]); };
    auto row_at = [&](int i) -> int64_t { return lds ? (int64_t)lr[i] : gr[i]; };
    const K kfloor = P > 0 ? key_at(P - 1) : K(0);  // the smallest positive key
    unsigned below = 0, nz = 0;
    K kmin = ~K(0), kmax = K(0);
    bool nan = false;
    for (int r0 = q; r0 < nr; r0 += TR_WAVES * TR_UNROLL) {
      T v[TR_UNROLL];
#pragma unroll
      for (int u = 0; u < TR_UNROLL; ++u) {
        const int r = r0 + u * TR_WAVES;
        v[u] = r < nr ? yhat[(rA + r) * ld + t] : T(0);
      }
#pragma unroll
      for (int u = 0; u < TR_UNROLL; ++u) {
        const int r = r0 + u * TR_WAVES;
        if (r >= nr) break;
        const T x = v[u];
        nan |= x != x;
        nz += x != T(0) ? 1u : 0u;
        const K k = tr_key(x);
        kmin = k < kmin ? k : kmin;
        kmax = k > kmax ? k : kmax;
        if ((pmask[r] >> c) & 1ULL) continue;  // a positive: the metrics add it from the sealed table
        if (P == 0 || k < kfloor) {
          ++below;
          continue;
        }
        int lo = 0, hi = P;  // j = positives scoring higher
        while (lo < hi) {
          const int mid = (lo + hi) >> 1;
          if (key_at(mid) > k) lo = mid + 1;
          else hi = mid;
        }
        const int j = lo;
        if (j < P && key_at(j) == k) {
          hi = P;  // the end of the tie group
          while (lo < hi) {
            const int mid = (lo + hi) >> 1;
            if (key_at(mid) >= k) lo = mid + 1;
            else hi = mid;
          }
          const int64_t rid = rowmap ? (int64_t)rowmap[rA + r] : row_begin + rA + r;
          int a = j, b = lo;  // positives of the group with a smaller row id
          while (a < b) {
            const int mid = (a + b) >> 1;
            if (row_at(mid) < rid) a = mid + 1;
            else b = mid;
          }
          atomicAdd(&H[P + 1 + j], 1u);
          atomicAdd(&H[2 * (P + 1) + a], 1u);
        } else {
          atomicAdd(&H[j], 1u);
        }
      }
    }
    // the four waves of the workgroup meet in LDS: one global add per target and workgroup below
    if (below) atomicAdd(&s_below[c], below);
    if (nz) atomicAdd(&s_nz[c], nz);
    if (q < nr) {  // this thread saw at least one row
      atomicMin(&s_min[c], (unsigned long long)kmin);
      atomicMax(&s_max[c], (unsigned long long)kmax);
    }
    if (nan) flag[0] = 1ULL;
  }
  __syncthreads();
  if (tid < ntile && nr > 0) {
    const int64_t t = t0 + tid;
    const int o = off[t] - pb, P = off[t + 1] - pb - o;
    if (s_below[tid]) atomicAdd(&ghist[3 * ((int64_t)o + tid) + P], s_below[tid]);
    if (s_nz[tid]) atomicAdd(&dnz[t], s_nz[tid]);
    atomicMin(&dmin[t], s_min[tid]);
    atomicMax(&dmax[t], s_max[tid]);
  }
  for (int i = tid; i < hlen; i += TR_THREADS) {
    const unsigned x = lhist[i];
    if (x) atomicAdd(&ghist[i], x);
  }
}

// counts += delta: hist | nz, then min / max of the keys
__global__ void __launch_bounds__(TR_THREADS) tr_apply_kernel(const unsigned* __restrict__ delta,
                                                              const unsigned long long* __restrict__ dmm, int64_t hist_nz,
                                                              int64_t nt, int64_t* __restrict__ counts) {
  for (int64_t i = (int64_t)blockIdx.x * TR_THREADS + threadIdx.x; i < hist_nz + 2 * nt;
       i += (int64_t)gridDim.x * TR_THREADS) {
    if (i < hist_nz) {
      counts[i] += (int64_t)delta[i];
    } else {
      const unsigned long long a = (unsigned long long)counts[i], b = dmm[i - hist_nz];
      counts[i] = (int64_t)(i < hist_nz + nt ? (a < b ? a : b) : (a > b ? a : b));
    }
  }
}

__global__ void __launch_bounds__(TR_THREADS) tr_counts_check_kernel(const int64_t* __restrict__ src, int64_t hist_nz,
                                                                     unsigned long long* __restrict__ flag) {
  bool bad = false;
  for (int64_t i = (int64_t)blockIdx.x * TR_THREADS + threadIdx.x; i < hist_nz; i += (int64_t)gridDim.x * TR_THREADS)
    bad |= src[i] < 0;
  if (bad) flag[0] = 1ULL;
}

__global__ void __launch_bounds__(TR_THREADS) tr_counts_add_kernel(const int64_t* __restrict__ src, int64_t hist_nz,
                                                                   int64_t nt, int64_t* __restrict__ counts) {
  for (int64_t i = (int64_t)blockIdx.x * TR_THREADS + threadIdx.x; i < hist_nz + 2 * nt;
       i += (int64_t)gridDim.x * TR_THREADS) {
    if (i < hist_nz) {
      counts[i] += src[i];
    } else {
      const unsigned long long a = (unsigned long long)counts[i], b = (unsigned long long)src[i];
      counts[i] = (int64_t)(i < hist_nz + nt ? (a < b ? a : b) : (a > b ? a : b));
    }
  }
}

template <class T>
__global__ void __launch_bounds__(TR_THREADS) tr_same_kernel(const int* __restrict__ at, const int64_t* __restrict__ ar,
                                                             const T* __restrict__ av, const int* __restrict__ bt,
                                                             const int64_t* __restrict__ br, const T* __restrict__ bv,
                                                             int64_t n, unsigned long long* __restrict__ flag) {
  bool bad = false;
  for (int64_t i = (int64_t)blockIdx.x * TR_THREADS + threadIdx.x; i < n; i += (int64_t)gridDim.x * TR_THREADS)
    bad |= at[i] != bt[i] || ar[i] != br[i] || tr_bits(av[i]) != tr_bits(bv[i]);
  if (bad) flag[0] = 1ULL;
}

// ------------------------------------------------------------------ metrics
// fixed-order block sums, valid in thread 0 (scratch: TR_WAVES slots)
template <class V>
__device__ inline V tr_block_sum(V v, V* scratch) {
  for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o);
  if ((threadIdx.x & 63) == 0) scratch[threadIdx.x >> 6] = v;
  __syncthreads();
  V s = V(0);
  if (threadIdx.x == 0)
    for (int w = 0; w < TR_WAVES; ++w) s += scratch[w];
  __syncthreads();
  return s;
}

// One workgroup per target.  R[k] = rank of positive k = inclusive scan of gap + tieK + 1; Q[k] = inclusive scan of
// gap + tieG + 1, so at the last positive k of the score group that starts at a, Q[k] = #{score >= v} and
// Q[a - 1] + gap[a] = #{score > v} (gap and tieG are zero inside a group).  The sums are rank_rows.hip's rr_finish.
template <class T>
__global__ void __launch_bounds__(TR_THREADS) tr_metrics_kernel(int64_t nt, const int* __restrict__ off,
                                                                const T* __restrict__ sv,
                                                                const int64_t* __restrict__ counts, int64_t hist_len,
                                                                int64_t n, double alpha, int L, int64_t* __restrict__ R,
                                                                int64_t* __restrict__ Q, double* __restrict__ out) {
  __shared__ long long wsum[2 * TR_WAVES];
  __shared__ long long redl[TR_WAVES];
  __shared__ double redd[TR_WAVES];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t* nzp = counts + hist_len;
  const int64_t* kminp = nzp + nt;
  const int64_t* kmaxp = kminp + nt;
  for (int64_t t = blockIdx.x; t < nt; t += gridDim.x) {
    const int o = off[t], P = off[t + 1] - o;
    const int64_t* gap = counts + 3 * ((int64_t)o + t);
    const int64_t* tieG = gap + P + 1;
    const int64_t* tieK = tieG + P + 1;
    int64_t* Rt = R + o + t;
    int64_t* Qt = Q + o + t;
    const T* ps = sv + o;
    long long carry1 = 0, carry2 = 0;
    for (int b = 0; b <= P; b += TR_THREADS) {
      const int i = b + (int)threadIdx.x;
      long long x1 = 0, x2 = 0;
      if (i <= P) {
        const long long g = gap[i] + (i < P ? 1 : 0);
        x1 = g + tieK[i];
        x2 = g + tieG[i];
      }
      for (int s = 1; s < 64; s <<= 1) {
        const long long y1 = __shfl_up(x1, s), y2 = __shfl_up(x2, s);
        if (lane >= s) {
          x1 += y1;
          x2 += y2;
        }
      }
      if (lane == 63) {
        wsum[wave] = x1;
        wsum[TR_WAVES + wave] = x2;
      }
      __syncthreads();
      long long add1 = carry1, add2 = carry2, tot1 = carry1, tot2 = carry2;
      for (int w = 0; w < TR_WAVES; ++w) {
        if (w < wave) {
          add1 += wsum[w];
          add2 += wsum[TR_WAVES + w];
        }
        tot1 += wsum[w];
        tot2 += wsum[TR_WAVES + w];
      }
      if (i <= P) {
        Rt[i] = x1 + add1;
        Qt[i] = x2 + add2;
      }
      carry1 = tot1;
      carry2 = tot2;
      __syncthreads();
    }
    long long num2 = 0, hit = 0;
    double prc = 0.0, bed = 0.0;
    const double Pd = (double)P, nd = (double)n;
    for (int k = (int)threadIdx.x; k < P; k += TR_THREADS) {
      const long long rank = Rt[k];
      bed += exp(-alpha * (double)rank / nd);
      hit += rank <= (long long)L ? 1 : 0;
      const T v = ps[k];
      if (k == P - 1 || ps[k + 1] != v) {  // the last positive of its score group
        int lo = 0, hi = k;                // a = positives scoring higher = the group's first
        while (lo < hi) {
          const int mid = (lo + hi) >> 1;
          if (ps[mid] > v) lo = mid + 1;
          else hi = mid;
        }
        const int a = lo;
        const long long ge = Qt[k];
        const long long gt = (a > 0 ? Qt[a - 1] : 0LL) + gap[a];
        const long long tp_gt = a, tp_ge = (long long)k + 1;
        if (gt > 0) {
          num2 += tieG[a] * (tp_ge + tp_gt);
          const double tp1 = (double)tp_ge, tp0 = (double)tp_gt;
          prc += (tp1 / Pd - tp0 / Pd) * (tp1 / (double)ge + tp0 / (double)gt) * 0.5;
        }
        num2 += 2LL * gap[a] * tp_gt;
      }
    }
    if (threadIdx.x == 0) num2 += 2LL * gap[P] * (long long)P;
    num2 = tr_block_sum<long long>(num2, redl);
    prc = tr_block_sum<double>(prc, redd);
    bed = tr_block_sum<double>(bed, redd);
    hit = tr_block_sum<long long>(hit, redl);
    if (threadIdx.x == 0) {
      const bool distinct = kminp[t] != kmaxp[t];
      const double Nn = nd - Pd;
      double auroc;
      if (P == 0 || (int64_t)P == n) auroc = distinct ? tr_nan() : 0.0;  // a class is missing: 0/0 rates
      else auroc = (double)num2 / (2.0 * Nn * Pd);
      const double auprc = P == 0 ? (distinct ? tr_nan() : 0.0) : prc;
      const double Ra = Pd / nd;
      const double rand_sum = Ra * (1.0 - exp(-alpha)) / (exp(alpha / nd) - 1.0);
      const double fac = Ra * sinh(alpha / 2.0) / (cosh(alpha / 2.0) - cosh(alpha / 2.0 - alpha * Ra));
      const double cte = 1.0 / (1.0 - exp(alpha * (1.0 - Ra)));
      double* o6 = out + t * 6;
      o6[0] = auroc;
      o6[1] = auprc;
      o6[2] = bed * fac / rand_sum + cte;
      o6[3] = (double)nzp[t] / nd;
      o6[4] = P > 0 ? (double)hit / Pd : tr_nan();
      o6[5] = (double)hit / (double)L;
    }
    __syncthreads();
  }
}

// keep the first `keep` elements of b while growing it to hold n
template <class X>
int tr_grow(DevBuf<X>& b, size_t keep, size_t n) {
  if (b.p && b.n >= n) return SS_OK;
  size_t cap = b.n * 2 > n ? b.n * 2 : n;
  if (cap < 1024) cap = 1024;
  DevBuf<X> nb;
  SS_TRY(nb.alloc(cap));
  if (keep) SS_HIP(hipMemcpyAsync(nb.p, b.p, keep * sizeof(X), hipMemcpyDeviceToDevice, ctx().stream));
  SS_HIP(hipStreamSynchronize(ctx().stream));
  b = std::move(nb);
  return SS_OK;
}

}  // namespace

// ------------------------------------------------------------------ host side
template <class T>
int tr_begin(TrState<T>& s) {
  hipStream_t st = ctx().stream;
  if (!s.flag.p) SS_TRY(s.flag.alloc(2));
  unsigned long long f[2] = {0ULL, ~0ULL};
  SS_HIP(hipMemcpyAsync(s.flag.p, f, sizeof(f), hipMemcpyHostToDevice, st));
  SS_HIP(hipStreamSynchronize(st));  // f is on this stack
  if (s.phase == 1) {
    SS_HIP(hipMemsetAsync(s.delta.p, 0, (size_t)(s.hist_len() + s.nt) * sizeof(unsigned), st));
    hipLaunchKernelGGL(tr_delta_init_kernel, dim3(tr_blocks(2 * s.nt)), dim3(TR_THREADS), 0, st, s.dmm.p, s.nt);
    SS_LAUNCH_CHECK();
  }
  return SS_OK;
}

template <class T, class PtrT>
int tr_collect_block(TrState<T>& s, int64_t at, const PtrT* yptr, int64_t shift, const int* yidx, int base, int64_t nnz,
                     const T* yhat, int64_t nb, int64_t ld, int64_t row_begin, const int* rowmap) {
  hipStream_t st = ctx().stream;
  if (nb <= 0) return SS_OK;
  path_add("target_rank_collect");
  int64_t gy = nb < 1024 ? nb : 1024;
  hipLaunchKernelGGL(tr_nan_kernel<T>, dim3(tr_blocks(s.nt, 64), (unsigned)gy), dim3(TR_THREADS), 0, st, yhat, ld, nb,
                     s.nt, s.flag.p);
  SS_LAUNCH_CHECK();
  if (nnz <= 0) return SS_OK;
  SS_TRY(tr_grow(s.ct, (size_t)at, (size_t)(at + nnz)));
  SS_TRY(tr_grow(s.cr, (size_t)at, (size_t)(at + nnz)));
  SS_TRY(tr_grow(s.cv, (size_t)at, (size_t)(at + nnz)));
  hipLaunchKernelGGL((tr_gather_kernel<T, PtrT>), dim3(tr_blocks(nb * 64)), dim3(TR_THREADS), 0, st, yptr, shift, yidx,
                     base, yhat, ld, nb, row_begin, rowmap, s.ct.p + at, s.cr.p + at, s.cv.p + at);
  SS_LAUNCH_CHECK();
  return SS_OK;
}

template <class T, class PtrT>
int tr_count_block(TrState<T>& s, const PtrT* yptr, int64_t shift, const int* yidx, int base, int64_t nnz, const T* yhat,
                   int64_t nb, int64_t ld, int64_t row_begin, const int* rowmap) {
  hipStream_t st = ctx().stream;
  if (nb <= 0) return SS_OK;
  if (nnz > 0) {
    hipLaunchKernelGGL((tr_check_kernel<T, PtrT>), dim3(tr_blocks(nb * 64)), dim3(TR_THREADS), 0, st, yptr, shift, yidx,
                       base, yhat, ld, nb, row_begin, rowmap, s.off.p, s.sr.p, s.sv.p, s.flag.p);
    SS_LAUNCH_CHECK();
  }
  if (s.tiles_lds) path_add("target_rank_count_lds");
  if (s.tiles_large) path_add("target_rank_count_large");
  const int64_t ntiles = ceil_div(s.nt, TR_TILE);
  for (int64_t r0 = 0; r0 < nb; r0 += (int64_t)65535 * TR_RPW) {  // gridDim.y < 65536
    const int64_t n = nb - r0 < (int64_t)65535 * TR_RPW ? nb - r0 : (int64_t)65535 * TR_RPW;
    hipLaunchKernelGGL((tr_count_kernel<T, PtrT>), dim3((unsigned)ntiles, (unsigned)ceil_div(n, TR_RPW)),
                       dim3(TR_THREADS), 0, st, yhat + r0 * ld, ld, s.nt, n, row_begin + r0, rowmap ? rowmap + r0 : nullptr,
                       yptr + r0, shift, yidx, base, s.off.p, s.sr.p, s.sv.p, s.route.p, s.delta.p,
                       s.delta.p + s.hist_len(), s.dmm.p, s.dmm.p + s.nt, s.flag.p);
    SS_LAUNCH_CHECK();
  }
  return SS_OK;
}

template <class T>
int tr_finish(TrState<T>& s) {
  hipStream_t st = ctx().stream;
  unsigned long long f[2] = {0, 0};
  SS_HIP(hipMemcpyAsync(f, s.flag.p, sizeof(f), hipMemcpyDeviceToHost, st));
  SS_HIP(hipStreamSynchronize(st));
  if (f[0]) return fail(SS_EINVAL, "target rank: a score is NaN");
  if (f[1] != ~0ULL)
    return fail(SS_EINVAL,
                "target rank count: the positive at row %lld, target %lld is not the one collected (missing, or another "
                "score): the second pass must repeat the first",
                (long long)(f[1] >> 32), (long long)(f[1] & 0xffffffffULL));
  return SS_OK;
}

template <class T>
int tr_count_commit(TrState<T>& s) {
  const int64_t hn = s.hist_len() + s.nt;
  hipLaunchKernelGGL(tr_apply_kernel, dim3(tr_blocks(hn + 2 * s.nt)), dim3(TR_THREADS), 0, ctx().stream, s.delta.p,
                     s.dmm.p, hn, s.nt, s.counts.p);
  SS_LAUNCH_CHECK();
  SS_HIP(hipStreamSynchronize(ctx().stream));
  return SS_OK;
}

template <class T>
int tr_seal(TrState<T>& s) {
  hipStream_t st = ctx().stream;
  const int64_t n = s.npos, nt = s.nt;
  DevBuf<int> nst, noff;
  DevBuf<int64_t> nsr, ncounts;
  DevBuf<T> nsv;
  DevBuf<unsigned char> nroute;
  DevBuf<unsigned> ndelta;
  DevBuf<unsigned long long> ndmm;
  SS_TRY(nst.alloc((size_t)n));
  SS_TRY(nsr.alloc((size_t)n));
  SS_TRY(nsv.alloc((size_t)n));
  SS_TRY(noff.alloc((size_t)nt + 1));
  if (n > 0) {
    DevBuf<unsigned> pa, pb;
    DevBuf<uint64_t> ka, kb;
    DevBuf<unsigned char> tmp;
    SS_TRY(pa.alloc((size_t)n));
    SS_TRY(pb.alloc((size_t)n));
    SS_TRY(ka.alloc((size_t)n));
    SS_TRY(kb.alloc((size_t)n));
    const unsigned bits[3] = {32u, 8u * (unsigned)sizeof(T), 32u};
    size_t bytes = 0;
    for (int pass = 0; pass < 3; ++pass) {  // the largest scratch any pass asks for
      size_t b = 0;
      SS_HIP(rocprim::radix_sort_pairs(nullptr, b, ka.p, kb.p, pa.p, pb.p, (size_t)n, 0, bits[pass], st));
      bytes = b > bytes ? b : bytes;
    }
    SS_TRY(tmp.alloc(bytes));
    hipLaunchKernelGGL(tr_iota_kernel, dim3(tr_blocks(n)), dim3(TR_THREADS), 0, st, pa.p, n);
    SS_LAUNCH_CHECK();
    for (int pass = 0; pass < 3; ++pass) {
      hipLaunchKernelGGL(tr_field_kernel<T>, dim3(tr_blocks(n)), dim3(TR_THREADS), 0, st, pass, pa.p, s.ct.p, s.cr.p,
                         s.cv.p, n, ka.p);
      SS_LAUNCH_CHECK();
      size_t b2 = bytes;
      SS_HIP(rocprim::radix_sort_pairs(tmp.p, b2, ka.p, kb.p, pa.p, pb.p, (size_t)n, 0, bits[pass], st));
      std::swap(pa, pb);
    }
    hipLaunchKernelGGL(tr_permute_kernel<T>, dim3(tr_blocks(n)), dim3(TR_THREADS), 0, st, pa.p, s.ct.p, s.cr.p, s.cv.p, n,
                       nst.p, nsr.p, nsv.p);
    SS_LAUNCH_CHECK();
    SS_HIP(hipStreamSynchronize(st));  // the scratch goes out of scope
  }
  hipLaunchKernelGGL(tr_offsets_kernel, dim3(tr_blocks(nt + 1)), dim3(TR_THREADS), 0, st, nst.p, n, nt, noff.p);
  SS_LAUNCH_CHECK();
  const int64_t ntiles = ceil_div(nt, TR_TILE);
  SS_TRY(nroute.alloc((size_t)ntiles));
  DevBuf<int> kinds;
  SS_TRY(kinds.alloc(2));
  SS_HIP(hipMemsetAsync(kinds.p, 0, 2 * sizeof(int), st));
  int cap = TR_LDS_POS;
  if (ctx().target_rank_lds >= 0 && ctx().target_rank_lds < cap) cap = ctx().target_rank_lds;
  hipLaunchKernelGGL(tr_route_kernel, dim3(tr_blocks(ntiles)), dim3(TR_THREADS), 0, st, noff.p, nt, ntiles, cap,
                     nroute.p, kinds.p);
  SS_LAUNCH_CHECK();
  const int64_t hn = 3 * (n + nt) + nt;
  SS_TRY(ncounts.alloc((size_t)(hn + 2 * nt)));
  SS_TRY(ndelta.alloc((size_t)hn));
  SS_TRY(ndmm.alloc((size_t)(2 * nt)));
  hipLaunchKernelGGL(tr_counts_init_kernel, dim3(tr_blocks(hn + 2 * nt)), dim3(TR_THREADS), 0, st, ncounts.p, hn, nt);
  SS_LAUNCH_CHECK();
  int hk[2] = {0, 0};
  SS_HIP(hipMemcpyAsync(hk, kinds.p, sizeof(hk), hipMemcpyDeviceToHost, st));
  SS_HIP(hipStreamSynchronize(st));
  s.st = std::move(nst);
  s.sr = std::move(nsr);
  s.sv = std::move(nsv);
  s.off = std::move(noff);
  s.route = std::move(nroute);
  s.counts = std::move(ncounts);
  s.delta = std::move(ndelta);
  s.dmm = std::move(ndmm);
  s.tiles_lds = hk[0];
  s.tiles_large = hk[1];
  s.ct.release();
  s.cr.release();
  s.cv.release();
  s.phase = 1;
  s.rows_counted = 0;
  return SS_OK;
}

template <class T>
int tr_append(TrState<T>& s, const int* targets, const int64_t* rows, const T* scores, int64_t n, bool check) {
  hipStream_t st = ctx().stream;
  if (n <= 0) return SS_OK;
  if (check) {
    if (!s.flag.p) SS_TRY(s.flag.alloc(2));
    SS_HIP(hipMemsetAsync(s.flag.p, 0, sizeof(unsigned long long), st));
    hipLaunchKernelGGL(tr_import_check_kernel<T>, dim3(tr_blocks(n)), dim3(TR_THREADS), 0, st, targets, rows, scores, n,
                       s.nt, s.flag.p);
    SS_LAUNCH_CHECK();
    unsigned long long f = 0;
    SS_HIP(hipMemcpyAsync(&f, s.flag.p, sizeof(f), hipMemcpyDeviceToHost, st));
    SS_HIP(hipStreamSynchronize(st));
    if (f & 1) return fail(SS_EINVAL, "target rank import: a score is NaN");
    if (f & 2) return fail(SS_EINVAL, "target rank import: a target is outside [0, nt)");
    if (f & 4) return fail(SS_EINVAL, "target rank import: a row is outside [0, 2^31)");
  }
  SS_TRY(tr_grow(s.ct, (size_t)s.npos, (size_t)(s.npos + n)));
  SS_TRY(tr_grow(s.cr, (size_t)s.npos, (size_t)(s.npos + n)));
  SS_TRY(tr_grow(s.cv, (size_t)s.npos, (size_t)(s.npos + n)));
  SS_HIP(hipMemcpyAsync(s.ct.p + s.npos, targets, (size_t)n * sizeof(int), hipMemcpyDeviceToDevice, st));
  SS_HIP(hipMemcpyAsync(s.cr.p + s.npos, rows, (size_t)n * sizeof(int64_t), hipMemcpyDeviceToDevice, st));
  SS_HIP(hipMemcpyAsync(s.cv.p + s.npos, scores, (size_t)n * sizeof(T), hipMemcpyDeviceToDevice, st));
  SS_HIP(hipStreamSynchronize(st));
  return SS_OK;
}

template <class T>
int tr_same_table(const TrState<T>& a, const TrState<T>& b, bool* same) {
  hipStream_t st = ctx().stream;
  *same = a.npos == b.npos && a.nt == b.nt;
  if (!*same || a.npos == 0) return SS_OK;
  DevBuf<unsigned long long> flag;
  SS_TRY(flag.alloc(1));
  SS_HIP(hipMemsetAsync(flag.p, 0, sizeof(unsigned long long), st));
  hipLaunchKernelGGL(tr_same_kernel<T>, dim3(tr_blocks(a.npos)), dim3(TR_THREADS), 0, st, a.st.p, a.sr.p, a.sv.p, b.st.p,
                     b.sr.p, b.sv.p, a.npos, flag.p);
  SS_LAUNCH_CHECK();
  unsigned long long f = 0;
  SS_HIP(hipMemcpyAsync(&f, flag.p, sizeof(f), hipMemcpyDeviceToHost, st));
  SS_HIP(hipStreamSynchronize(st));
  *same = f == 0;
  return SS_OK;
}

template <class T>
int tr_add_counts(TrState<T>& s, const int64_t* counts, bool check) {
  hipStream_t st = ctx().stream;
  const int64_t hn = s.hist_len() + s.nt;
  if (check) {
    if (!s.flag.p) SS_TRY(s.flag.alloc(2));
    SS_HIP(hipMemsetAsync(s.flag.p, 0, sizeof(unsigned long long), st));
    hipLaunchKernelGGL(tr_counts_check_kernel, dim3(tr_blocks(hn)), dim3(TR_THREADS), 0, st, counts, hn, s.flag.p);
    SS_LAUNCH_CHECK();
    unsigned long long f = 0;
    SS_HIP(hipMemcpyAsync(&f, s.flag.p, sizeof(f), hipMemcpyDeviceToHost, st));
    SS_HIP(hipStreamSynchronize(st));
    if (f) return fail(SS_EINVAL, "target rank import: a count is negative");
  }
  hipLaunchKernelGGL(tr_counts_add_kernel, dim3(tr_blocks(hn + 2 * s.nt)), dim3(TR_THREADS), 0, st, counts, hn, s.nt,
                     s.counts.p);
  SS_LAUNCH_CHECK();
  SS_HIP(hipStreamSynchronize(st));
  return SS_OK;
}

template <class T>
int tr_metrics(const TrState<T>& s, double alpha, int L, double* out) {
  hipStream_t st = ctx().stream;
  DevBuf<int64_t> R, Q;
  SS_TRY(R.alloc((size_t)(s.npos + s.nt)));
  SS_TRY(Q.alloc((size_t)(s.npos + s.nt)));
  path_add("target_rank_metrics");
  const int grid = (int)(s.nt < 8192 ? s.nt : 8192);
  hipLaunchKernelGGL(tr_metrics_kernel<T>, dim3(grid), dim3(TR_THREADS), 0, st, s.nt, s.off.p, s.sv.p, s.counts.p,
                     s.hist_len(), s.rows, alpha, L, R.p, Q.p, out);
  SS_LAUNCH_CHECK();
  SS_HIP(hipStreamSynchronize(st));  // R and Q go out of scope
  return SS_OK;
}

#define SS_TR_INST(T)                                                                                                  \
  template int tr_begin<T>(TrState<T>&);                                                                               \
  template int tr_collect_block<T, int64_t>(TrState<T>&, int64_t, const int64_t*, int64_t, const int*, int, int64_t,    \
                                            const T*, int64_t, int64_t, int64_t, const int*);                          \
  template int tr_collect_block<T, int>(TrState<T>&, int64_t, const int*, int64_t, const int*, int, int64_t, const T*,  \
                                        int64_t, int64_t, int64_t, const int*);                                        \
  template int tr_count_block<T, int64_t>(TrState<T>&, const int64_t*, int64_t, const int*, int, int64_t, const T*,     \
                                          int64_t, int64_t, int64_t, const int*);                                      \
  template int tr_count_block<T, int>(TrState<T>&, const int*, int64_t, const int*, int, int64_t, const T*, int64_t,    \
                                      int64_t, int64_t, const int*);                                                   \
  template int tr_finish<T>(TrState<T>&);                                                                              \
  template int tr_count_commit<T>(TrState<T>&);                                                                        \
  template int tr_seal<T>(TrState<T>&);                                                                                \
  template int tr_append<T>(TrState<T>&, const int*, const int64_t*, const T*, int64_t, bool);                         \
  template int tr_same_table<T>(const TrState<T>&, const TrState<T>&, bool*);                                          \
  template int tr_add_counts<T>(TrState<T>&, const int64_t*, bool);                                                    \
  template int tr_metrics<T>(const TrState<T>&, double, int, double*);
SS_TR_INST(float)
SS_TR_INST(double)
#undef SS_TR_INST

}  // namespace ss
