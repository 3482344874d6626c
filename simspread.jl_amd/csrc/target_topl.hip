// Per-target top-L lists: recallatL / precisionatL(y, yhat, grouping, L) of the reference (src/performance.jl:308-409)
// with grouping = the target of every entry of vec(yhat).  Inside a target group Julia's stable
// sortperm(yhat_g, rev=true) orders the rows by (score descending, row ascending), because vec is column-major; under
// that total order the top L of a union of blocks is the top L of the blocks' own top-L lists, so an nt x L table
// absorbs row blocks, folds, ranks and shards in any order and ends as one table, bitwise.
//
// Scores are order-preserving unsigned keys (u32 / u64) of Julia's isless order: +0.0 ranks before -0.0 (no -0.0 ->
// +0.0 here, unlike the pool), clean!'s -99 is an ordinary score, NaN is refused.  An entry is (key, row, label); the
// composite order is key descending, row ascending (label ascending only separates copies of one row, which distinct
// rows never produce).
//
//   seed         while a target holds fewer than L entries, its top L of the old entries and the block's first
//                max(L - fill, 2L, TL_SEED) rows: tl_merge_large_kernel in its seed mode (every target; at most L
//                entries are sorted in LDS, more go through its radix select).  The filter's threshold stays fixed for
//                a block, so a target expects (rows - seed) * L / seed candidates in the first block: a seed of L rows
//                (whose L-th entry is their minimum, often a clean!ed -99) would make nearly every row one.
//   filter       tl_filter_kernel: one coalesced pass over the block, lanes across consecutive targets with 16-byte
//                loads; a score that beats its target's L-th entry is a candidate: its slot comes from an int atomic
//                on the target's counter, its label from a binary search in its row's sorted CSR positives.  NaN is
//                flagged in the same pass.  Targets with candidates are listed (act), targets with more than `cap`
//                (ovf).
//   merge (LDS)  tl_merge_lds_kernel: per listed target, the candidates are bitonic-sorted in LDS and merged with the
//                L old entries by rank (binary search on the other side); ranks < L are written in place.
//   merge (long) tl_merge_large_kernel: per overflowed target, the old entries and the target's whole column of the
//                block (cached in LDS up to TL_COLCACHE rows) go through a radix select on the 96 / 128-bit composite
//                (key, ~row), 8 bits a pass, which stops as soon as the digit's bucket is exactly what is still
//                needed; the L chosen entries are sorted in LDS.
// Both merges produce the unique top L under the total order, so the slot order of the atomics cannot reach the
// output.  Label counts per target are added with int64 atomics (tl_npos_kernel).  No float atomics anywhere.
#include <hip/hip_runtime.h>

#include <cstring>
#include <vector>

#include "graph.hpp"

namespace ss {

namespace {

constexpr int TL_THREADS = 256;
constexpr int TL_MAXL = 1024;       // the largest L
constexpr int TL_CAP_MAX = 2048;    // candidates per target on the LDS path
constexpr int TL_COLCACHE = 2048;   // column rows the long-list route keeps in LDS
constexpr int TL_ROWS = 32;         // rows per filter workgroup (at least)
constexpr int TL_SEED = 512;        // rows a seed takes at least (and 2L): the filter's threshold is the L-th of them

__device__ inline uint32_t tl_key(float v) {
  const uint32_t u = __float_as_uint(v);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ inline uint64_t tl_key(double v) {
  const uint64_t u = (uint64_t)__double_as_longlong(v);
  return (u >> 63) ? ~u : (u | (1ULL << 63));
}
__device__ inline float tl_value(uint32_t k) { return __uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k); }
__device__ inline double tl_value(uint64_t k) {
  return __longlong_as_double((long long)((k >> 63) ? (k & ~(1ULL << 63)) : ~k));
}

// a strictly before b in the table's order
template <class K>
__device__ inline bool tl_before(K ka, int64_t ra, uint8_t la, K kb, int64_t rb, uint8_t lb) {
  return ka > kb || (ka == kb && (ra < rb || (ra == rb && la < lb)));
}

// label of (block row r, target t): a binary search in the row's sorted positives
template <class PtrT>
__device__ inline uint8_t tl_label(const PtrT* __restrict__ yptr, int64_t shift, const int* __restrict__ yidx, int base,
                                   int64_t r, int64_t t) {
  int64_t lo = (int64_t)yptr[r] - shift;
  const int64_t end = (int64_t)yptr[r + 1] - shift;
  int64_t hi = end;
  const int want = (int)t + base;
  while (lo < hi) {
    const int64_t mid = (lo + hi) >> 1;
    if (yidx[mid] < want) lo = mid + 1;
    else hi = mid;
  }
  return (lo < end && yidx[lo] == want) ? 1 : 0;
}

template <class T>
struct TlVec;
template <>
struct TlVec<float> {
  using type = float4;
  static constexpr int V = 4;
};
template <>
struct TlVec<double> {
  using type = double2;
  static constexpr int V = 2;
};

inline int tl_grid(int64_t n, int64_t cap) { return (int)(n < 1 ? 1 : n > cap ? cap : n); }

template <class X>
int grow(DevBuf<X>& b, size_t n) {
  if (b.n >= n && b.p) return SS_OK;
  SS_HIP(hipStreamSynchronize(ctx().stream));
  return b.alloc(n);
}

// ------------------------------------------------------------------ small kernels
template <class PtrT>
__global__ void __launch_bounds__(TL_THREADS) tl_npos_kernel(const PtrT* __restrict__ yptr, int64_t shift,
                                                             const int* __restrict__ yidx, int base, int64_t nnz,
                                                             int64_t* __restrict__ npos) {
  const int64_t e0 = (int64_t)yptr[0] - shift;
  for (int64_t e = (int64_t)blockIdx.x * TL_THREADS + threadIdx.x; e < nnz; e += (int64_t)gridDim.x * TL_THREADS)
    atomicAdd(reinterpret_cast<unsigned long long*>(npos + (yidx[e0 + e] - base)), 1ULL);
}

template <class K>
__global__ void __launch_bounds__(TL_THREADS) tl_thresh_kernel(const K* __restrict__ key, const int64_t* __restrict__ row,
                                                               int64_t nt, int L, K* __restrict__ thk,
                                                               int64_t* __restrict__ thr) {
  for (int64_t t = (int64_t)blockIdx.x * TL_THREADS + threadIdx.x; t < nt; t += (int64_t)gridDim.x * TL_THREADS) {
    thk[t] = key[t * L + L - 1];
    thr[t] = row[t * L + L - 1];
  }
}

// ------------------------------------------------------------------ filter
template <class T, class K, class PtrT>
__global__ void __launch_bounds__(TL_THREADS) tl_filter_kernel(
    const T* __restrict__ yhat, int64_t ld, int64_t nt, int64_t r_lo, int64_t r_hi, int64_t rows_per_chunk, int vec,
    int64_t row_begin, const int* __restrict__ rowmap, const PtrT* __restrict__ yptr, int64_t shift,
    const int* __restrict__ yidx, int base, const K* __restrict__ thk, const int64_t* __restrict__ thr, int64_t cap,
    int* __restrict__ cnt, K* __restrict__ ck, int64_t* __restrict__ cr, uint8_t* __restrict__ cl,
    int* __restrict__ act, int* __restrict__ ovf, int* __restrict__ ctr, int* __restrict__ flag) {
  constexpr int V = TlVec<T>::V;
  const int64_t t0 = ((int64_t)blockIdx.x * TL_THREADS + threadIdx.x) * V;
  if (t0 >= nt) return;
  const int nv = nt - t0 < V ? (int)(nt - t0) : V;
  K tk[V];
  int64_t tr[V];
#pragma unroll
  for (int v = 0; v < V; ++v) {
    tk[v] = v < nv ? thk[t0 + v] : K(0);
    tr[v] = v < nv ? thr[t0 + v] : 0;
  }
  const int64_t ra = r_lo + (int64_t)blockIdx.y * rows_per_chunk;
  const int64_t rb = ra + rows_per_chunk < r_hi ? ra + rows_per_chunk : r_hi;
  bool nan = false;
  for (int64_t r = ra; r < rb; ++r) {
    const T* src = yhat + r * ld + t0;
    T x[V];
    if (vec && nv == V) {
      const typename TlVec<T>::type q = *reinterpret_cast<const typename TlVec<T>::type*>(src);
      __builtin_memcpy(x, &q, sizeof(q));
    } else {
#pragma unroll
      for (int v = 0; v < V; ++v) x[v] = v < nv ? src[v] : T(0);
    }
    const int64_t rid = rowmap ? (int64_t)rowmap[r] : row_begin + r;
#pragma unroll
    for (int v = 0; v < V; ++v) {
      if (v >= nv) break;
      nan |= x[v] != x[v];
      const K k = tl_key(x[v]);
      if (k > tk[v] || (k == tk[v] && rid < tr[v])) {
        const int64_t t = t0 + v;
        const int slot = atomicAdd(&cnt[t], 1);
        if (slot == 0) act[atomicAdd(&ctr[0], 1)] = (int)t;
        if (slot < cap) {
          const int64_t o = t * cap + slot;
          ck[o] = k;
          cr[o] = rid;
          cl[o] = tl_label(yptr, shift, yidx, base, r, t);
        } else if (slot == cap) {
          ovf[atomicAdd(&ctr[1], 1)] = (int)t;
        }
      }
    }
  }
  if (nan) flag[0] = 1;
}

// ------------------------------------------------------------------ LDS sort
template <class K>
__device__ void tl_bitonic(K* k, int64_t* r, uint8_t* l, int n2) {
  for (int size = 2; size <= n2; size <<= 1) {
    for (int stride = size >> 1; stride > 0; stride >>= 1) {
      for (int i = threadIdx.x; i < n2; i += TL_THREADS) {
        const int j = i ^ stride;
        if (j > i) {
          const bool swap = (i & size) == 0 ? tl_before(k[j], r[j], l[j], k[i], r[i], l[i])
                                            : tl_before(k[i], r[i], l[i], k[j], r[j], l[j]);
          if (swap) {
            const K tk = k[i];
            k[i] = k[j];
            k[j] = tk;
            const int64_t tr = r[i];
            r[i] = r[j];
            r[j] = tr;
            const uint8_t tl = l[i];
            l[i] = l[j];
            l[j] = tl;
          }
        }
      }
      __syncthreads();
    }
  }
}

// ------------------------------------------------------------------ merge, LDS path
// dynamic LDS: int64 rows of capp2 candidates and L old entries, then their keys, then their labels
template <class K>
__global__ void __launch_bounds__(TL_THREADS) tl_merge_lds_kernel(int L, int64_t cap, int capp2,
                                                                  const int* __restrict__ act,
                                                                  const int* __restrict__ ctr,
                                                                  const int* __restrict__ cnt, const K* __restrict__ ck,
                                                                  const int64_t* __restrict__ cr,
                                                                  const uint8_t* __restrict__ cl, K* __restrict__ tkey,
                                                                  int64_t* __restrict__ trow, uint8_t* __restrict__ tlab) {
  extern __shared__ __attribute__((aligned(16))) unsigned char tl_smem[];
  int64_t* sr = reinterpret_cast<int64_t*>(tl_smem);
  int64_t* orow = sr + capp2;
  K* sk = reinterpret_cast<K*>(orow + L);
  K* okey = sk + capp2;
  uint8_t* sl = reinterpret_cast<uint8_t*>(okey + L);
  uint8_t* olab = sl + capp2;
  const int tid = threadIdx.x;
  const int nact = ctr[0];
  for (int i = blockIdx.x; i < nact; i += gridDim.x) {
    const int64_t t = act[i];
    const int c = cnt[t];
    if (c > cap) continue;  // the long-list route's
    int n2 = 1;
    while (n2 < c) n2 <<= 1;
    const int64_t cb = t * cap, tb = t * L;
    for (int j = tid; j < n2; j += TL_THREADS) {
      if (j < c) {
        sk[j] = ck[cb + j];
        sr[j] = cr[cb + j];
        sl[j] = cl[cb + j];
      } else {  // after every real entry
        sk[j] = K(0);
        sr[j] = INT64_MAX;
        sl[j] = 0xff;
      }
    }
    for (int j = tid; j < L; j += TL_THREADS) {
      okey[j] = tkey[tb + j];
      orow[j] = trow[tb + j];
      olab[j] = tlab[tb + j];
    }
    __syncthreads();
    tl_bitonic(sk, sr, sl, n2);
    // an old entry's place: its index + the candidates before it; a candidate's: its index + the old entries not
    // after it (equal entries: the old one first)
    for (int j = tid; j < L; j += TL_THREADS) {
      int lo = 0, hi = c;
      while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (tl_before(sk[mid], sr[mid], sl[mid], okey[j], orow[j], olab[j])) lo = mid + 1;
        else hi = mid;
      }
      const int rank = j + lo;
      if (rank < L) {
        tkey[tb + rank] = okey[j];
        trow[tb + rank] = orow[j];
        tlab[tb + rank] = olab[j];
      }
    }
    for (int j = tid; j < c; j += TL_THREADS) {
      int lo = 0, hi = L;
      while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (!tl_before(sk[j], sr[j], sl[j], okey[mid], orow[mid], olab[mid])) lo = mid + 1;
        else hi = mid;
      }
      const int rank = j + lo;
      if (rank < L) {
        tkey[tb + rank] = sk[j];
        trow[tb + rank] = sr[j];
        tlab[tb + rank] = sl[j];
      }
    }
    __syncthreads();
  }
}

// ------------------------------------------------------------------ merge, long-list route (and the seed)
// seed != 0: every target, top L of its fill entries and block rows [r_lo, r_hi) (at most L: all kept);
// seed == 0: the overflowed targets listed in ovf[0..ctr[1]), top L of the union
template <class T, class K, class PtrT>
__global__ void __launch_bounds__(TL_THREADS) tl_merge_large_kernel(
    int seed, int64_t nt, int L, int64_t fill, const int* __restrict__ ovf, const int* __restrict__ ctr,
    const T* __restrict__ yhat, int64_t ld, int64_t r_lo, int64_t r_hi, int64_t row_begin, const int* __restrict__ rowmap,
    const PtrT* __restrict__ yptr, int64_t shift, const int* __restrict__ yidx, int base, K* __restrict__ tkey,
    int64_t* __restrict__ trow, uint8_t* __restrict__ tlab, int* __restrict__ flag) {
  constexpr int KB = 8 * (int)sizeof(K);
  __shared__ int64_t orow[TL_MAXL];
  __shared__ int64_t sr[TL_MAXL];
  __shared__ K okey[TL_MAXL];
  __shared__ K sk[TL_MAXL];
  __shared__ K colk[TL_COLCACHE];
  __shared__ uint8_t olab[TL_MAXL];
  __shared__ uint8_t sl[TL_MAXL];
  __shared__ unsigned hist[TL_THREADS];
  __shared__ uint64_t s_phi, s_plo, s_mhi, s_mlo;
  __shared__ int64_t s_need;
  __shared__ int s_stop, s_n, s_eq;
  const int tid = threadIdx.x;
  const int64_t ncol = r_hi - r_lo, total = fill + ncol;
  const bool cached = ncol <= TL_COLCACHE;
  const int64_t ntodo = seed ? nt : (int64_t)ctr[1];
  if (!seed && ntodo > 0 && blockIdx.x == 0 && tid == 0) flag[1] = 1;
  for (int64_t i = blockIdx.x; i < ntodo; i += gridDim.x) {
    const int64_t t = seed ? i : (int64_t)ovf[i];
    const int64_t tb = t * L;
    for (int64_t j = tid; j < fill; j += TL_THREADS) {
      okey[j] = tkey[tb + j];
      orow[j] = trow[tb + j];
      olab[j] = tlab[tb + j];
    }
    bool nan = false;
    if (cached) {
      for (int64_t r = tid; r < ncol; r += TL_THREADS) {
        const T v = yhat[(r_lo + r) * ld + t];
        nan |= v != v;
        colk[r] = tl_key(v);
      }
    } else {
      for (int64_t r = tid; r < ncol; r += TL_THREADS) {
        const T v = yhat[(r_lo + r) * ld + t];
        nan |= v != v;
      }
    }
    if (nan) flag[0] = 1;
    if (tid == 0) {
      s_phi = s_plo = s_mhi = s_mlo = 0;
      s_need = L;
      s_n = s_eq = 0;
    }
    __syncthreads();
    // element e: an old entry (e < fill) or block row r_lo + e - fill
    auto elem = [&](int64_t e, K& k, int64_t& row) {
      if (e < fill) {
        k = okey[e];
        row = orow[e];
      } else {
        const int64_t r = e - fill;
        k = cached ? colk[r] : tl_key(yhat[(r_lo + r) * ld + t]);
        row = rowmap ? (int64_t)rowmap[r_lo + r] : row_begin + r_lo + r;
      }
    };
    auto put = [&](int slot, int64_t e, K k, int64_t row) {
      sk[slot] = k;
      sr[slot] = row;
      sl[slot] = e < fill ? olab[e] : tl_label(yptr, shift, yidx, base, r_lo + (e - fill), t);
    };
    int nsel;
    if (total <= L) {
      for (int64_t e = tid; e < total; e += TL_THREADS) {
        K k;
        int64_t row;
        elem(e, k, row);
        put((int)e, e, k, row);
      }
      nsel = (int)total;
    } else {
      // radix select of the L-th entry on (key, ~row), most significant digit first
      for (int pos = KB + 64 - 8; pos >= 0; pos -= 8) {
        hist[tid] = 0;
        __syncthreads();
        const uint64_t phi = s_phi, plo = s_plo, mhi = s_mhi, mlo = s_mlo;
        for (int64_t e = tid; e < total; e += TL_THREADS) {
          K k;
          int64_t row;
          elem(e, k, row);
          const uint64_t hi = (uint64_t)k, lo = ~(uint64_t)row;
          if ((hi & mhi) == phi && (lo & mlo) == plo) {
            const unsigned d = pos >= 64 ? (unsigned)(hi >> (pos - 64)) & 0xffu : (unsigned)(lo >> pos) & 0xffu;
            atomicAdd(&hist[d], 1u);
          }
        }
        __syncthreads();
        if (tid == 0) {
          int64_t need = s_need, acc = 0;
          int d = 255;
          for (; d > 0; --d) {
            if (acc + (int64_t)hist[d] >= need) break;
            acc += hist[d];
          }
          need -= acc;
          if (pos >= 64) {
            s_phi |= (uint64_t)d << (pos - 64);
            s_mhi |= 0xffULL << (pos - 64);
          } else {
            s_plo |= (uint64_t)d << pos;
            s_mlo |= 0xffULL << pos;
          }
          s_need = need;
          s_stop = (int64_t)hist[d] == need;
        }
        __syncthreads();
        if (s_stop) break;
      }
      const uint64_t phi = s_phi, plo = s_plo, mhi = s_mhi, mlo = s_mlo;
      const int64_t need = s_need;
      for (int64_t e = tid; e < total; e += TL_THREADS) {
        K k;
        int64_t row;
        elem(e, k, row);
        const uint64_t hi = (uint64_t)k & mhi, lo = ~(uint64_t)row & mlo;
        const bool gt = hi > phi || (hi == phi && lo > plo);
        bool take = gt;
        if (!gt && hi == phi && lo == plo) take = atomicAdd(&s_eq, 1) < need;
        if (take) put(atomicAdd(&s_n, 1), e, k, row);
      }
      nsel = L;
    }
    __syncthreads();
    int n2 = 1;
    while (n2 < nsel) n2 <<= 1;
    for (int j = nsel + tid; j < n2; j += TL_THREADS) {
      sk[j] = K(0);
      sr[j] = INT64_MAX;
      sl[j] = 0xff;
    }
    __syncthreads();
    tl_bitonic(sk, sr, sl, n2);
    for (int j = tid; j < nsel; j += TL_THREADS) {
      tkey[tb + j] = sk[j];
      trow[tb + j] = sr[j];
      tlab[tb + j] = sl[j];
    }
    __syncthreads();
  }
}

// ------------------------------------------------------------------ whole tables
// out = top L of a (fa entries) and b (fb entries), per target; npos added
template <class K>
__global__ void __launch_bounds__(TL_THREADS) tl_merge_tables_kernel(
    const K* __restrict__ ak, const int64_t* __restrict__ ar, const uint8_t* __restrict__ al,
    const int64_t* __restrict__ an, int64_t fa, const K* __restrict__ bk, const int64_t* __restrict__ br,
    const uint8_t* __restrict__ bl, const int64_t* __restrict__ bn, int64_t fb, int64_t nt, int L, K* __restrict__ ok,
    int64_t* __restrict__ orow, uint8_t* __restrict__ ol, int64_t* __restrict__ on) {
  for (int64_t t = blockIdx.x; t < nt; t += gridDim.x) {
    const int64_t tb = t * L;
    for (int64_t j = threadIdx.x; j < fa; j += TL_THREADS) {
      const K k = ak[tb + j];
      const int64_t r = ar[tb + j];
      const uint8_t l = al[tb + j];
      int64_t lo = 0, hi = fb;
      while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        if (tl_before(bk[tb + mid], br[tb + mid], bl[tb + mid], k, r, l)) lo = mid + 1;
        else hi = mid;
      }
      const int64_t rank = j + lo;
      if (rank < L) {
        ok[tb + rank] = k;
        orow[tb + rank] = r;
        ol[tb + rank] = l;
      }
    }
    for (int64_t j = threadIdx.x; j < fb; j += TL_THREADS) {
      const K k = bk[tb + j];
      const int64_t r = br[tb + j];
      const uint8_t l = bl[tb + j];
      int64_t lo = 0, hi = fa;
      while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        if (!tl_before(k, r, l, ak[tb + mid], ar[tb + mid], al[tb + mid])) lo = mid + 1;
        else hi = mid;
      }
      const int64_t rank = j + lo;
      if (rank < L) {
        ok[tb + rank] = k;
        orow[tb + rank] = r;
        ol[tb + rank] = l;
      }
    }
    if (threadIdx.x == 0) on[t] = an[t] + bn[t];
  }
}

// flag bits: 1 NaN score, 2 a negative row, 4 a label other than 0 / 1, 8 entries not strictly in the table's order,
// 16 npos < 0 or fewer positives than labelled entries
template <class T, class K>
__global__ void __launch_bounds__(TL_THREADS) tl_import_kernel(const T* __restrict__ vals, const int64_t* __restrict__ rows,
                                                               const uint8_t* __restrict__ labels,
                                                               const int64_t* __restrict__ npos, int64_t nt, int L,
                                                               int64_t fill, K* __restrict__ ok, int64_t* __restrict__ orow,
                                                               uint8_t* __restrict__ ol, int64_t* __restrict__ on,
                                                               int* __restrict__ flag,
                                                               unsigned long long* __restrict__ psum) {
  int f = 0;
  unsigned long long ps = 0;
  for (int64_t t = (int64_t)blockIdx.x * TL_THREADS + threadIdx.x; t < nt; t += (int64_t)gridDim.x * TL_THREADS) {
    int64_t hits = 0;
    K pk = K(0);
    int64_t pr = 0;
    uint8_t pl = 0;
    for (int64_t j = 0; j < fill; ++j) {
      const int64_t s = t * fill + j;
      const T v = vals[s];
      const int64_t r = rows[s];
      const uint8_t l = labels[s];
      if (v != v) f |= 1;
      if (r < 0) f |= 2;
      if (l > 1) f |= 4;
      const K k = tl_key(v);
      if (j > 0 && !tl_before(pk, pr, pl, k, r, l)) f |= 8;
      pk = k;
      pr = r;
      pl = l;
      hits += l;
      ok[t * L + j] = k;
      orow[t * L + j] = r;
      ol[t * L + j] = l;
    }
    const int64_t p = npos[t];
    if (p < 0 || p < hits) f |= 16;
    on[t] = p;
    ps += (unsigned long long)(p > 0 ? p : 0);
  }
  if (f) atomicOr(flag, f);
  if (ps) atomicAdd(psum, ps);
}

template <class T, class K>
__global__ void __launch_bounds__(TL_THREADS) tl_export_kernel(const K* __restrict__ key, const int64_t* __restrict__ row,
                                                               const uint8_t* __restrict__ lab, int64_t nt, int L,
                                                               int64_t fill, T* __restrict__ vals,
                                                               int64_t* __restrict__ rows, uint8_t* __restrict__ labels) {
  const int64_t n = nt * fill;
  for (int64_t e = (int64_t)blockIdx.x * TL_THREADS + threadIdx.x; e < n; e += (int64_t)gridDim.x * TL_THREADS) {
    const int64_t s = (e / fill) * L + e % fill;
    if (vals) vals[e] = tl_value(key[s]);
    if (rows) rows[e] = row[s];
    if (labels) labels[e] = lab[s];
  }
}

__global__ void __launch_bounds__(TL_THREADS) tl_hits_kernel(const uint8_t* __restrict__ lab, int64_t nt, int L,
                                                             int64_t fill, int64_t* __restrict__ hits) {
  for (int64_t t = (int64_t)blockIdx.x * TL_THREADS + threadIdx.x; t < nt; t += (int64_t)gridDim.x * TL_THREADS) {
    int64_t h = 0;
    for (int64_t j = 0; j < fill; ++j) h += lab[t * L + j];
    hits[t] = h;
  }
}

inline int tl_blocks(int64_t n, int64_t cap = 4096) { return tl_grid((n + TL_THREADS - 1) / TL_THREADS, cap); }

}  // namespace

// ------------------------------------------------------------------ host side
template <class K>
int tl_alloc(TlTable<K>& t, int64_t nt, int L) {
  const size_t n = (size_t)nt * (size_t)L;
  SS_TRY(t.key.alloc(n));
  SS_TRY(t.row.alloc(n));
  SS_TRY(t.lab.alloc(n));
  SS_TRY(t.npos.alloc((size_t)nt));
  SS_HIP(hipMemsetAsync(t.npos.p, 0, (size_t)nt * sizeof(int64_t), ctx().stream));
  return SS_OK;
}

template <class K>
int tl_copy(const TlTable<K>& a, TlTable<K>& b, int64_t nt, int L, int64_t fill) {
  hipStream_t st = ctx().stream;
  if (!b.key.p || b.key.n < (size_t)nt * L) SS_TRY(tl_alloc(b, nt, L));
  const size_t n = (size_t)nt * (size_t)L;
  if (fill > 0) {
    SS_HIP(hipMemcpyAsync(b.key.p, a.key.p, n * sizeof(K), hipMemcpyDeviceToDevice, st));
    SS_HIP(hipMemcpyAsync(b.row.p, a.row.p, n * sizeof(int64_t), hipMemcpyDeviceToDevice, st));
    SS_HIP(hipMemcpyAsync(b.lab.p, a.lab.p, n * sizeof(uint8_t), hipMemcpyDeviceToDevice, st));
  }
  SS_HIP(hipMemcpyAsync(b.npos.p, a.npos.p, (size_t)nt * sizeof(int64_t), hipMemcpyDeviceToDevice, st));
  return SS_OK;
}

template <class K>
int tl_begin(TlWork<K>& w, int64_t nt, int L) {
  int64_t cap = 2 * (int64_t)L > 512 ? 2 * (int64_t)L : 512;
  if (cap > TL_CAP_MAX) cap = TL_CAP_MAX;
  // candidate scratch within 2 GiB: fewer slots per target for very wide tables (more targets take the long route)
  while (cap > 64 && nt * cap * (int64_t)(sizeof(K) + sizeof(int64_t) + 1) > (1LL << 31)) cap >>= 1;
  w.cap = cap;
  const size_t nc = (size_t)nt * (size_t)cap;
  SS_TRY(grow(w.ck, nc));
  SS_TRY(grow(w.cr, nc));
  SS_TRY(grow(w.cl, nc));
  SS_TRY(grow(w.thk, (size_t)nt));
  SS_TRY(grow(w.thr, (size_t)nt));
  SS_TRY(grow(w.cnt, (size_t)nt));
  SS_TRY(grow(w.act, (size_t)nt));
  SS_TRY(grow(w.ovf, (size_t)nt));
  SS_TRY(grow(w.ctr, 2));
  SS_TRY(grow(w.flag, 2));
  SS_HIP(hipMemsetAsync(w.flag.p, 0, 2 * sizeof(int), ctx().stream));
  return SS_OK;
}

template <class T, class PtrT>
int tl_add_block(TlTable<pool_key_t<T>>& tb, int64_t nt, int L, int64_t fill, const PtrT* yptr, int64_t shift,
                 const int* yidx, int base, int64_t nnz, const T* yhat, int64_t nb, int64_t ld, int64_t row_begin,
                 const int* rowmap, TlWork<pool_key_t<T>>& w) {
  using K = pool_key_t<T>;
  hipStream_t st = ctx().stream;
  if (nb <= 0) return SS_OK;
  if (nnz > 0) {
    hipLaunchKernelGGL((tl_npos_kernel<PtrT>), dim3(tl_blocks(nnz)), dim3(TL_THREADS), 0, st, yptr, shift, yidx, base,
                       nnz, tb.npos.p);
    SS_LAUNCH_CHECK();
  }
  int64_t s = 0;
  if (fill < L) {  // seed: the top L of the old entries and the block's first rows, at least TL_SEED of them
    s = (int64_t)L - fill;
    if (s < TL_SEED) s = TL_SEED;
    if (s < 2 * (int64_t)L) s = 2 * (int64_t)L;
    if (s > nb) s = nb;
    path_add("target_topl_seed");
    hipLaunchKernelGGL((tl_merge_large_kernel<T, K, PtrT>), dim3(tl_grid(nt, 8192)), dim3(TL_THREADS), 0, st, 1, nt, L,
                       fill, w.ovf.p, w.ctr.p, yhat, ld, (int64_t)0, s, row_begin, rowmap, yptr, shift, yidx, base,
                       tb.key.p, tb.row.p, tb.lab.p, w.flag.p);
    SS_LAUNCH_CHECK();
  }
  if (s == nb) return SS_OK;
  // every target holds L entries now
  hipLaunchKernelGGL(tl_thresh_kernel<K>, dim3(tl_blocks(nt)), dim3(TL_THREADS), 0, st, tb.key.p, tb.row.p, nt, L, w.thk.p,
                     w.thr.p);
  SS_LAUNCH_CHECK();
  SS_HIP(hipMemsetAsync(w.cnt.p, 0, (size_t)nt * sizeof(int), st));
  SS_HIP(hipMemsetAsync(w.ctr.p, 0, 2 * sizeof(int), st));
  constexpr int V = TlVec<T>::V;
  const int vec = (ld % V == 0) && (reinterpret_cast<uintptr_t>(yhat) % 16 == 0);
  const int64_t nf = nb - s;
  int64_t rpc = TL_ROWS;
  if (ceil_div(nf, rpc) > 65535) rpc = ceil_div(nf, 65535);
  const int64_t gx = ceil_div(nt, (int64_t)TL_THREADS * V), gy = ceil_div(nf, rpc);
  path_add("target_topl_filter");
  hipLaunchKernelGGL((tl_filter_kernel<T, K, PtrT>), dim3((unsigned)gx, (unsigned)gy), dim3(TL_THREADS), 0, st, yhat, ld,
                     nt, s, nb, rpc, vec, row_begin, rowmap, yptr, shift, yidx, base, w.thk.p, w.thr.p, w.cap, w.cnt.p,
                     w.ck.p, w.cr.p, w.cl.p, w.act.p, w.ovf.p, w.ctr.p, w.flag.p);
  SS_LAUNCH_CHECK();
  int capp2 = 1;
  while (capp2 < w.cap) capp2 <<= 1;
  const size_t lds = (size_t)(capp2 + L) * (sizeof(int64_t) + sizeof(K) + 1);
  path_add("target_topl_merge_lds");
  hipLaunchKernelGGL(tl_merge_lds_kernel<K>, dim3(tl_grid(nt, 4096)), dim3(TL_THREADS), lds, st, L, w.cap, capp2, w.act.p,
                     w.ctr.p, w.cnt.p, w.ck.p, w.cr.p, w.cl.p, tb.key.p, tb.row.p, tb.lab.p);
  SS_LAUNCH_CHECK();
  hipLaunchKernelGGL((tl_merge_large_kernel<T, K, PtrT>), dim3(tl_grid(nt, 1024)), dim3(TL_THREADS), 0, st, 0, nt, L,
                     (int64_t)L, w.ovf.p, w.ctr.p, yhat, ld, s, nb, row_begin, rowmap, yptr, shift, yidx, base, tb.key.p,
                     tb.row.p, tb.lab.p, w.flag.p);
  SS_LAUNCH_CHECK();
  return SS_OK;
}

template <class K>
int tl_finish(TlWork<K>& w) {
  hipStream_t st = ctx().stream;
  int f[2] = {0, 0};
  SS_HIP(hipMemcpyAsync(f, w.flag.p, sizeof(f), hipMemcpyDeviceToHost, st));
  SS_HIP(hipStreamSynchronize(st));
  if (f[0]) return fail(SS_EINVAL, "target top-L: a score is NaN");
  if (f[1]) path_add("target_topl_merge_large");
  return SS_OK;
}

template <class K>
int tl_merge_tables(const TlTable<K>& a, int64_t fa, const TlTable<K>& b, int64_t fb, int64_t nt, int L,
                    TlTable<K>& out) {
  if (!out.key.p || out.key.n < (size_t)nt * L) SS_TRY(tl_alloc(out, nt, L));
  hipLaunchKernelGGL(tl_merge_tables_kernel<K>, dim3(tl_grid(nt, 8192)), dim3(TL_THREADS), 0, ctx().stream, a.key.p,
                     a.row.p, a.lab.p, a.npos.p, fa, b.key.p, b.row.p, b.lab.p, b.npos.p, fb, nt, L, out.key.p, out.row.p,
                     out.lab.p, out.npos.p);
  SS_LAUNCH_CHECK();
  return SS_OK;
}

template <class T>
int tl_import_table(const T* vals, const int64_t* rows, const uint8_t* labels, const int64_t* npos, int64_t nt, int L,
                    int64_t fill, TlTable<pool_key_t<T>>& out, int64_t* P) {
  using K = pool_key_t<T>;
  hipStream_t st = ctx().stream;
  SS_TRY(tl_alloc(out, nt, L));
  DevBuf<int> flag;
  DevBuf<unsigned long long> psum;
  SS_TRY(flag.alloc(1));
  SS_TRY(psum.alloc(1));
  SS_HIP(hipMemsetAsync(flag.p, 0, sizeof(int), st));
  SS_HIP(hipMemsetAsync(psum.p, 0, sizeof(unsigned long long), st));
  hipLaunchKernelGGL((tl_import_kernel<T, K>), dim3(tl_blocks(nt)), dim3(TL_THREADS), 0, st, vals, rows, labels, npos, nt,
                     L, fill, out.key.p, out.row.p, out.lab.p, out.npos.p, flag.p, psum.p);
  SS_LAUNCH_CHECK();
  int f = 0;
  unsigned long long ps = 0;
  SS_HIP(hipMemcpyAsync(&f, flag.p, sizeof(int), hipMemcpyDeviceToHost, st));
  SS_HIP(hipMemcpyAsync(&ps, psum.p, sizeof(ps), hipMemcpyDeviceToHost, st));
  SS_HIP(hipStreamSynchronize(st));
  if (f & 1) return fail(SS_EINVAL, "target top-L import: a score is NaN");
  if (f & 2) return fail(SS_EINVAL, "target top-L import: a row is negative");
  if (f & 4) return fail(SS_EINVAL, "target top-L import: a label is not 0 or 1");
  if (f & 8)
    return fail(SS_EINVAL, "target top-L import: a target's entries are not strictly ordered by (score desc, row asc)");
  if (f & 16) return fail(SS_EINVAL, "target top-L import: npos is negative or below the labelled entries");
  *P = (int64_t)ps;
  return SS_OK;
}

template <class T>
int tl_export_table(const TlTable<pool_key_t<T>>& t, int64_t nt, int L, int64_t fill, T* vals, int64_t* rows,
                    uint8_t* labels) {
  if (nt * fill == 0) return SS_OK;
  hipLaunchKernelGGL((tl_export_kernel<T, pool_key_t<T>>), dim3(tl_blocks(nt * fill)), dim3(TL_THREADS), 0, ctx().stream,
                     t.key.p, t.row.p, t.lab.p, nt, L, fill, vals, rows, labels);
  SS_LAUNCH_CHECK();
  return SS_OK;
}

template <class K>
int tl_hits(const TlTable<K>& t, int64_t nt, int L, int64_t fill, int64_t* hits) {
  hipLaunchKernelGGL(tl_hits_kernel, dim3(tl_blocks(nt)), dim3(TL_THREADS), 0, ctx().stream, t.lab.p, nt, L, fill, hits);
  SS_LAUNCH_CHECK();
  return SS_OK;
}

#define SS_TL_INST(T, K)                                                                                             \
  template int tl_alloc<K>(TlTable<K>&, int64_t, int);                                                               \
  template int tl_copy<K>(const TlTable<K>&, TlTable<K>&, int64_t, int, int64_t);                                    \
  template int tl_begin<K>(TlWork<K>&, int64_t, int);                                                                \
  template int tl_add_block<T, int64_t>(TlTable<K>&, int64_t, int, int64_t, const int64_t*, int64_t, const int*, int, \
                                        int64_t, const T*, int64_t, int64_t, int64_t, const int*, TlWork<K>&);        \
  template int tl_add_block<T, int>(TlTable<K>&, int64_t, int, int64_t, const int*, int64_t, const int*, int, int64_t, \
                                    const T*, int64_t, int64_t, int64_t, const int*, TlWork<K>&);                     \
  template int tl_finish<K>(TlWork<K>&);                                                                             \
  template int tl_merge_tables<K>(const TlTable<K>&, int64_t, const TlTable<K>&, int64_t, int64_t, int, TlTable<K>&); \
  template int tl_import_table<T>(const T*, const int64_t*, const uint8_t*, const int64_t*, int64_t, int, int64_t,    \
                                  TlTable<K>&, int64_t*);                                                            \
  template int tl_export_table<T>(const TlTable<K>&, int64_t, int, int64_t, T*, int64_t*, uint8_t*);                 \
  template int tl_hits<K>(const TlTable<K>&, int64_t, int, int64_t, int64_t*);
SS_TL_INST(float, uint32_t)
SS_TL_INST(double, uint64_t)
#undef SS_TL_INST

}  // namespace ss
