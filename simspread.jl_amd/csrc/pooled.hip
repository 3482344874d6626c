// Pooled evaluation: the reference judges a model on the whole score matrix at once -- AuROC(vec(y), vec(yhat)),
// AuPRC(...), maxperformance(vec(y), vec(yhat), f1score) (docs/src/tutorial/*.jl, src/performance.jl:49-89,420-520) --
// and those numbers depend only on the multiset of (score, label) pairs.  A table of the distinct scores in descending
// order, each with an int64 count of positives and of negatives, is therefore exact and sufficient; tables merge by
// the union of their keys with the counts added, in any order, so a block, a rank or a whole sweep each becomes one.
//
// Scores are stored as order-preserving unsigned keys (u32 for fp32, u64 for fp64; -0.0 is +0.0's key): descending
// keys are descending scores.
//
//   block -> table   pl_keys_kernel writes the key of every score of a row-major block (and flags a NaN),
//                    pl_pos_keys_kernel the keys of the positives (CSR labels); both are sorted keys-only (rocPRIM radix
//                    sort, descending); run heads are counted and written in chunks of PL_ITEMS (pl_heads_*), giving
//                    (key, count) for all scores and for the positives; pl_join_kernel moves each positive run's count
//                    from "all" to npos of its key, so nneg = all - npos.  Sorting every score instead of the negatives
//                    alone costs the ~1 % positives and saves a compaction pass.
//   merge            merge path (pl_merge_*): each thread takes PL_ITEMS outputs of the merged order, found by a binary
//                    search on its diagonal; equal keys (at most one from each side) are coalesced; a count pass, an
//                    inclusive scan of the per-thread counts and a write pass give a dense table.
//   table -> numbers inclusive scans of npos / nneg give (tp, fp) at every threshold (the table's keys are the
//                    thresholds of sort(unique(yhat))); pl_terms_kernel forms the trapezoid terms as rank_terms_kernel
//                    does, the non-zero count and br_metrics (binary_metrics.hpp) for max / sum; pl_sqdev_kernel the
//                    squared deviations from the mean.  Partials per workgroup are summed on the host in block order,
//                    so the 21 numbers are bitwise a function of the table alone.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstring>
#include <vector>

#include <rocprim/rocprim.hpp>

#include "binary_metrics.hpp"
#include "graph.hpp"

namespace ss {

namespace {

#pragma clang fp contract(off)

constexpr int PL_THREADS = 256;
constexpr int PL_ITEMS = 16;       // consecutive outputs per thread in the run and merge passes
constexpr int PL_MAX_BLOCKS = 1024;
constexpr int PL_NQ = 3 + 6;       // auroc, auprc, non-zero count, six metric sums

__device__ inline uint32_t pl_key(float v) {
  const uint32_t u = __float_as_uint(v == 0.0f ? 0.0f : v);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ inline uint64_t pl_key(double v) {
  const uint64_t u = (uint64_t)__double_as_longlong(v == 0.0 ? 0.0 : v);
  return (u >> 63) ? ~u : (u | (1ULL << 63));
}
__device__ inline float pl_value(uint32_t k) { return __uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k); }
__device__ inline double pl_value(uint64_t k) {
  return __longlong_as_double((long long)((k >> 63) ? (k & ~(1ULL << 63)) : ~k));
}

inline int pl_grid(int64_t n, int64_t cap = 4096) {
  const int64_t g = (n + PL_THREADS - 1) / PL_THREADS;
  return (int)(g < 1 ? 1 : g > cap ? cap : g);
}

// scratch and tables are freed (hipFree) while the library's non-blocking stream may still read them: every place
// that drops a buffer another launch used waits for the stream first
template <class X>
int grow(DevBuf<X>& b, size_t n) {
  if (b.n >= n && b.p) return SS_OK;
  SS_HIP(hipStreamSynchronize(ctx().stream));
  return b.alloc(n);
}

// ------------------------------------------------------------------ block -> keys
template <class T, class K>
__global__ void __launch_bounds__(PL_THREADS) pl_keys_kernel(const T* __restrict__ yhat, int64_t nrows, int64_t ncols,
                                                             int64_t ld, K* __restrict__ out, int* __restrict__ nan_flag) {
  bool nan = false;
  for (int64_t r = blockIdx.y; r < nrows; r += gridDim.y) {
    const T* row = yhat + r * ld;
    K* o = out + r * ncols;
    for (int64_t c = (int64_t)blockIdx.x * PL_THREADS + threadIdx.x; c < ncols; c += (int64_t)gridDim.x * PL_THREADS) {
      const T v = row[c];
      nan |= v != v;
      o[c] = pl_key(v);
    }
  }
  if (nan) *nan_flag = 1;
}

// keys of the positives: entry e of the CSR slice (row found by a binary search over the row pointers)
template <class T, class K, class PtrT>
__global__ void __launch_bounds__(PL_THREADS) pl_pos_keys_kernel(const PtrT* __restrict__ yptr, int64_t shift,
                                                                 const int* __restrict__ yidx, int base,
                                                                 const T* __restrict__ yhat, int64_t nrows, int64_t ld,
                                                                 K* __restrict__ out) {
  const int64_t e0 = (int64_t)yptr[0] - shift, nnz = (int64_t)yptr[nrows] - shift - e0;
  for (int64_t e = (int64_t)blockIdx.x * PL_THREADS + threadIdx.x; e < nnz; e += (int64_t)gridDim.x * PL_THREADS) {
    int64_t lo = 0, hi = nrows;  // the last row whose first entry is <= e
    while (hi - lo > 1) {
      const int64_t mid = (lo + hi) >> 1;
      if ((int64_t)yptr[mid] - shift - e0 <= e) lo = mid;
      else hi = mid;
    }
    out[e] = pl_key(yhat[lo * ld + (yidx[e0 + e] - base)]);
  }
}

// ------------------------------------------------------------------ sorted keys -> runs
template <class K>
__global__ void __launch_bounds__(PL_THREADS) pl_heads_count_kernel(const K* __restrict__ s, int64_t n, int64_t nchunks,
                                                                    int64_t* __restrict__ cnt) {
  for (int64_t t = (int64_t)blockIdx.x * PL_THREADS + threadIdx.x; t < nchunks; t += (int64_t)gridDim.x * PL_THREADS) {
    const int64_t i0 = t * PL_ITEMS, i1 = i0 + PL_ITEMS < n ? i0 + PL_ITEMS : n;
    K prev = i0 > 0 ? s[i0 - 1] : K(0);
    int64_t c = 0;
    for (int64_t i = i0; i < i1; ++i) {
      const K k = s[i];
      c += (i == 0 || k != prev) ? 1 : 0;
      prev = k;
    }
    cnt[t] = c;
  }
}

// inc: inclusive scan of the chunk counts
template <class K>
__global__ void __launch_bounds__(PL_THREADS) pl_heads_write_kernel(const K* __restrict__ s, int64_t n, int64_t nchunks,
                                                                    const int64_t* __restrict__ cnt,
                                                                    const int64_t* __restrict__ inc,
                                                                    K* __restrict__ rkey, int64_t* __restrict__ rstart) {
  for (int64_t t = (int64_t)blockIdx.x * PL_THREADS + threadIdx.x; t < nchunks; t += (int64_t)gridDim.x * PL_THREADS) {
    const int64_t i0 = t * PL_ITEMS, i1 = i0 + PL_ITEMS < n ? i0 + PL_ITEMS : n;
    int64_t o = inc[t] - cnt[t];
    K prev = i0 > 0 ? s[i0 - 1] : K(0);
    for (int64_t i = i0; i < i1; ++i) {
      const K k = s[i];
      if (i == 0 || k != prev) {
        rkey[o] = k;
        rstart[o] = i;
        ++o;
      }
      prev = k;
    }
  }
}

// run lengths from the run starts; zero: a second array cleared alongside (npos of the block's table), may be NULL
__global__ void __launch_bounds__(PL_THREADS) pl_run_len_kernel(const int64_t* __restrict__ rstart, int64_t R, int64_t n,
                                                                int64_t* __restrict__ len, int64_t* __restrict__ zero) {
  for (int64_t o = (int64_t)blockIdx.x * PL_THREADS + threadIdx.x; o < R; o += (int64_t)gridDim.x * PL_THREADS) {
    len[o] = (o + 1 < R ? rstart[o + 1] : n) - rstart[o];
    if (zero) zero[o] = 0;
  }
}

// every positive run's key is among the keys of all scores: move its count there (one positive run per key)
template <class K>
__global__ void __launch_bounds__(PL_THREADS) pl_join_kernel(const K* __restrict__ qkey, const int64_t* __restrict__ qcnt,
                                                             int64_t Q, const K* __restrict__ key, int64_t R,
                                                             int64_t* __restrict__ npos, int64_t* __restrict__ nneg) {
  for (int64_t j = (int64_t)blockIdx.x * PL_THREADS + threadIdx.x; j < Q; j += (int64_t)gridDim.x * PL_THREADS) {
    const K k = qkey[j];
    int64_t lo = 0, hi = R - 1;  // key is descending
    while (lo < hi) {
      const int64_t mid = (lo + hi) >> 1;
      if (key[mid] > k) lo = mid + 1;
      else hi = mid;
    }
    npos[lo] = qcnt[j];
    nneg[lo] -= qcnt[j];
  }
}

// ------------------------------------------------------------------ merge path
// (i, j) with i + j = d: the first d elements of the merged order are a[0..i) and b[0..j) (descending, a first on ties)
template <class K>
__device__ inline void pl_diag(const K* a, int64_t na, const K* b, int64_t nb, int64_t d, int64_t& i, int64_t& j) {
  int64_t lo = d > nb ? d - nb : 0, hi = d < na ? d : na;
  while (lo < hi) {
    const int64_t mid = (lo + hi) >> 1;
    if (a[mid] >= b[d - 1 - mid]) lo = mid + 1;
    else hi = mid;
  }
  i = lo;
  j = d - lo;
}

// Each side has unique keys, so a key occurs at most twice, a's copy first: b[j] is a duplicate iff a[i - 1] == b[j]
// when it is taken.  Outputs are the a elements and the b elements that are not duplicates.
template <class K>
__global__ void __launch_bounds__(PL_THREADS) pl_merge_count_kernel(const K* __restrict__ a, int64_t na,
                                                                    const K* __restrict__ b, int64_t nb, int64_t nchunks,
                                                                    int64_t* __restrict__ cnt) {
  const int64_t n = na + nb;
  for (int64_t t = (int64_t)blockIdx.x * PL_THREADS + threadIdx.x; t < nchunks; t += (int64_t)gridDim.x * PL_THREADS) {
    const int64_t d0 = t * PL_ITEMS, d1 = d0 + PL_ITEMS < n ? d0 + PL_ITEMS : n;
    int64_t i, j, c = 0;
    pl_diag(a, na, b, nb, d0, i, j);
    for (int64_t d = d0; d < d1; ++d) {
      if (i < na && (j >= nb || a[i] >= b[j])) {
        ++c;
        ++i;
      } else {
        c += (i > 0 && a[i - 1] == b[j]) ? 0 : 1;
        ++j;
      }
    }
    cnt[t] = c;
  }
}

template <class K>
__global__ void __launch_bounds__(PL_THREADS) pl_merge_write_kernel(
    const K* __restrict__ a, const int64_t* __restrict__ ap, const int64_t* __restrict__ an, int64_t na,
    const K* __restrict__ b, const int64_t* __restrict__ bp, const int64_t* __restrict__ bn, int64_t nb, int64_t nchunks,
    const int64_t* __restrict__ cnt, const int64_t* __restrict__ inc, K* __restrict__ ok, int64_t* __restrict__ op,
    int64_t* __restrict__ on) {
  const int64_t n = na + nb;
  for (int64_t t = (int64_t)blockIdx.x * PL_THREADS + threadIdx.x; t < nchunks; t += (int64_t)gridDim.x * PL_THREADS) {
    const int64_t d0 = t * PL_ITEMS, d1 = d0 + PL_ITEMS < n ? d0 + PL_ITEMS : n;
    int64_t i, j, o = inc[t] - cnt[t];
    pl_diag(a, na, b, nb, d0, i, j);
    for (int64_t d = d0; d < d1; ++d) {
      if (i < na && (j >= nb || a[i] >= b[j])) {
        int64_t p = ap[i], q = an[i];
        if (j < nb && b[j] == a[i]) {
          p += bp[j];
          q += bn[j];
        }
        ok[o] = a[i];
        op[o] = p;
        on[o] = q;
        ++o;
        ++i;
      } else {
        if (!(i > 0 && a[i - 1] == b[j])) {
          ok[o] = b[j];
          op[o] = bp[j];
          on[o] = bn[j];
          ++o;
        }
        ++j;
      }
    }
  }
}

// ------------------------------------------------------------------ import / export
// flag bits: 1 NaN score, 2 a negative count or an entry without pairs, 4 scores not strictly descending
template <class T, class K>
__global__ void __launch_bounds__(PL_THREADS) pl_import_kernel(const T* __restrict__ v, const int64_t* __restrict__ np,
                                                               const int64_t* __restrict__ nn, int64_t n,
                                                               K* __restrict__ key, int* __restrict__ flag,
                                                               unsigned long long* __restrict__ sums) {
  int f = 0;
  unsigned long long sp = 0, sn = 0;
  for (int64_t k = (int64_t)blockIdx.x * PL_THREADS + threadIdx.x; k < n; k += (int64_t)gridDim.x * PL_THREADS) {
    const T x = v[k];
    const int64_t p = np[k], q = nn[k];
    if (x != x) f |= 1;
    if (p < 0 || q < 0 || p + q == 0) f |= 2;
    const K kk = pl_key(x);
    if (k > 0 && !(kk < pl_key(v[k - 1]))) f |= 4;
    key[k] = kk;
    sp += (unsigned long long)(p > 0 ? p : 0);
    sn += (unsigned long long)(q > 0 ? q : 0);
  }
  if (f) atomicOr(flag, f);
  if (sp) atomicAdd(&sums[0], sp);
  if (sn) atomicAdd(&sums[1], sn);
}

template <class T, class K>
__global__ void __launch_bounds__(PL_THREADS) pl_export_kernel(const K* __restrict__ key, int64_t n, T* __restrict__ v) {
  for (int64_t k = (int64_t)blockIdx.x * PL_THREADS + threadIdx.x; k < n; k += (int64_t)gridDim.x * PL_THREADS)
    v[k] = pl_value(key[k]);
}

// ------------------------------------------------------------------ table -> numbers
// ctp / cfp: inclusive scans of npos / nneg (tp and fp at the threshold of entry k).  part[b*PL_NQ + q] sums,
// pmax[b*6 + m] maxima, pnan[b] NaN bits of workgroup b.
template <class K>
__global__ void __launch_bounds__(PL_THREADS) pl_terms_kernel(const K* __restrict__ key, const int64_t* __restrict__ ctp,
                                                              const int64_t* __restrict__ cfp, int64_t E, K zero_key,
                                                              long long Pl, long long Nl, double* __restrict__ part,
                                                              double* __restrict__ pmax, int* __restrict__ pnan) {
  const double P = (double)Pl, Nn = (double)Nl;
  double s[PL_NQ], mx[6];
  int nanb = 0;
  for (int q = 0; q < PL_NQ; ++q) s[q] = 0.0;
  for (int k = 0; k < 6; ++k) mx[k] = -__builtin_inf();
  for (int64_t k = (int64_t)blockIdx.x * PL_THREADS + threadIdx.x; k < E; k += (int64_t)gridDim.x * PL_THREADS) {
    const long long tp = ctp[k], fp = cfp[k];
    const double tp1 = (double)tp, fp1 = (double)fp;
    long long prev_all = 0;
    if (k > 0) {  // rank_terms_kernel's terms between this threshold and the previous one
      const double tp0 = (double)ctp[k - 1], fp0 = (double)cfp[k - 1];
      s[0] += (fp1 / Nn - fp0 / Nn) * (tp1 / P + tp0 / P) * 0.5;
      s[1] += (tp1 / P - tp0 / P) * (tp1 / (tp1 + fp1) + tp0 / (tp0 + fp0)) * 0.5;
      prev_all = ctp[k - 1] + cfp[k - 1];
    }
    if (key[k] != zero_key) s[2] += (double)(tp + fp - prev_all);
    double m[6];
    br_metrics(tp, fp, Pl, Nl, m);
    for (int q = 0; q < 6; ++q) {
      if (m[q] != m[q]) nanb |= 1 << q;
      else if (m[q] > mx[q]) mx[q] = m[q];
      s[3 + q] += m[q];
    }
  }
  __shared__ double sh[PL_NQ + 6][PL_THREADS];
  __shared__ int shn[PL_THREADS];
  for (int q = 0; q < PL_NQ; ++q) sh[q][threadIdx.x] = s[q];
  for (int q = 0; q < 6; ++q) sh[PL_NQ + q][threadIdx.x] = mx[q];
  shn[threadIdx.x] = nanb;
  __syncthreads();
  for (int w = PL_THREADS / 2; w > 0; w >>= 1) {
    if ((int)threadIdx.x < w) {
      for (int q = 0; q < PL_NQ; ++q) sh[q][threadIdx.x] += sh[q][threadIdx.x + w];
      for (int q = PL_NQ; q < PL_NQ + 6; ++q) {
        const double y = sh[q][threadIdx.x + w];
        if (y > sh[q][threadIdx.x]) sh[q][threadIdx.x] = y;
      }
      shn[threadIdx.x] |= shn[threadIdx.x + w];
    }
    __syncthreads();
  }
  if (threadIdx.x < PL_NQ) part[(size_t)blockIdx.x * PL_NQ + threadIdx.x] = sh[threadIdx.x][0];
  if (threadIdx.x < 6) pmax[(size_t)blockIdx.x * 6 + threadIdx.x] = sh[PL_NQ + threadIdx.x][0];
  if (threadIdx.x == 0) pnan[blockIdx.x] = shn[0];
}

struct PlMean {
  double m[6];
};

__global__ void __launch_bounds__(PL_THREADS) pl_sqdev_kernel(const int64_t* __restrict__ ctp,
                                                              const int64_t* __restrict__ cfp, int64_t E, long long Pl,
                                                              long long Nl, PlMean mean, double* __restrict__ part) {
  double s[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  for (int64_t k = (int64_t)blockIdx.x * PL_THREADS + threadIdx.x; k < E; k += (int64_t)gridDim.x * PL_THREADS) {
    double m[6];
    br_metrics(ctp[k], cfp[k], Pl, Nl, m);
    for (int q = 0; q < 6; ++q) {
      const double dv = m[q] - mean.m[q];
      s[q] += dv * dv;
    }
  }
  __shared__ double sh[6][PL_THREADS];
  for (int q = 0; q < 6; ++q) sh[q][threadIdx.x] = s[q];
  __syncthreads();
  for (int w = PL_THREADS / 2; w > 0; w >>= 1) {
    if ((int)threadIdx.x < w)
      for (int q = 0; q < 6; ++q) sh[q][threadIdx.x] += sh[q][threadIdx.x + w];
    __syncthreads();
  }
  if (threadIdx.x < 6) part[(size_t)blockIdx.x * 6 + threadIdx.x] = sh[threadIdx.x][0];
}

// sorted keys s[0..n) -> run keys (rkey) and run lengths (rlen, R entries); zero: cleared alongside when not NULL
template <class K>
int pl_runs(const K* s, int64_t n, PoolWork<K>& w, DevBuf<K>& rkey, DevBuf<int64_t>& rlen, DevBuf<int64_t>* zero,
            int64_t* R) {
  hipStream_t st = ctx().stream;
  const int64_t nchunks = (n + PL_ITEMS - 1) / PL_ITEMS;
  SS_TRY(grow(w.cnt, (size_t)nchunks));
  SS_TRY(grow(w.inc, (size_t)nchunks));
  hipLaunchKernelGGL(pl_heads_count_kernel<K>, dim3(pl_grid(nchunks)), dim3(PL_THREADS), 0, st, s, n, nchunks, w.cnt.p);
  SS_LAUNCH_CHECK();
  size_t bytes = 0;
  SS_HIP(rocprim::inclusive_scan(nullptr, bytes, w.cnt.p, w.inc.p, (size_t)nchunks, rocprim::plus<int64_t>(), st));
  SS_TRY(grow(w.tmp, bytes));
  SS_HIP(rocprim::inclusive_scan(w.tmp.p, bytes, w.cnt.p, w.inc.p, (size_t)nchunks, rocprim::plus<int64_t>(), st));
  SS_HIP(hipMemcpyAsync(R, w.inc.p + nchunks - 1, sizeof(int64_t), hipMemcpyDeviceToHost, st));
  SS_HIP(hipStreamSynchronize(st));
  SS_TRY(rkey.alloc((size_t)*R));
  SS_TRY(rlen.alloc((size_t)*R));
  if (zero) SS_TRY(zero->alloc((size_t)*R));
  SS_TRY(grow(w.rstart, (size_t)*R));
  hipLaunchKernelGGL(pl_heads_write_kernel<K>, dim3(pl_grid(nchunks)), dim3(PL_THREADS), 0, st, s, n, nchunks, w.cnt.p,
                     w.inc.p, rkey.p, w.rstart.p);
  SS_LAUNCH_CHECK();
  hipLaunchKernelGGL(pl_run_len_kernel, dim3(pl_grid(*R)), dim3(PL_THREADS), 0, st, w.rstart.p, *R, n, rlen.p,
                     zero ? zero->p : nullptr);
  SS_LAUNCH_CHECK();
  return SS_OK;
}

template <class K>
int pl_sort_desc(const K* in, K* out, int64_t n, PoolWork<K>& w) {
  hipStream_t st = ctx().stream;
  size_t bytes = 0;
  SS_HIP(rocprim::radix_sort_keys_desc(nullptr, bytes, in, out, (size_t)n, 0, (unsigned)(8 * sizeof(K)), st));
  SS_TRY(grow(w.tmp, bytes));
  SS_HIP(rocprim::radix_sort_keys_desc(w.tmp.p, bytes, in, out, (size_t)n, 0, (unsigned)(8 * sizeof(K)), st));
  return SS_OK;
}

template <class K>
int pl_copy(const PoolTable<K>& a, PoolTable<K>& out) {
  hipStream_t st = ctx().stream;
  SS_TRY(out.key.alloc((size_t)a.n));
  SS_TRY(out.npos.alloc((size_t)a.n));
  SS_TRY(out.nneg.alloc((size_t)a.n));
  if (a.n) {
    SS_HIP(hipMemcpyAsync(out.key.p, a.key.p, (size_t)a.n * sizeof(K), hipMemcpyDeviceToDevice, st));
    SS_HIP(hipMemcpyAsync(out.npos.p, a.npos.p, (size_t)a.n * sizeof(int64_t), hipMemcpyDeviceToDevice, st));
    SS_HIP(hipMemcpyAsync(out.nneg.p, a.nneg.p, (size_t)a.n * sizeof(int64_t), hipMemcpyDeviceToDevice, st));
  }
  out.n = a.n;
  SS_HIP(hipStreamSynchronize(st));  // the caller may drop `a` next
  return SS_OK;
}

}  // namespace

// ------------------------------------------------------------------ host side
template <class T, class PtrT>
int pool_block_table(const PtrT* yptr, int64_t shift, const int* yidx, int base, int64_t nnz, const T* yhat,
                     int64_t nrows, int64_t ncols, int64_t ld, PoolWork<pool_key_t<T>>& w, PoolTable<pool_key_t<T>>& out) {
  using K = pool_key_t<T>;
  hipStream_t st = ctx().stream;
  const int64_t n = nrows * ncols;
  out = PoolTable<K>();
  if (n == 0) return SS_OK;
  SS_TRY(grow(w.s, (size_t)n));
  SS_TRY(grow(w.s2, (size_t)n));
  SS_TRY(grow(w.flag, 4));
  SS_HIP(hipMemsetAsync(w.flag.p, 0, sizeof(int), st));
  {
    const int64_t gx = (ncols + PL_THREADS - 1) / PL_THREADS < 2048 ? (ncols + PL_THREADS - 1) / PL_THREADS : 2048;
    int64_t gy = 16384 / gx;
    if (gy < 1) gy = 1;
    if (gy > nrows) gy = nrows;
    if (gy > 65535) gy = 65535;
    hipLaunchKernelGGL((pl_keys_kernel<T, K>), dim3((unsigned)gx, (unsigned)gy), dim3(PL_THREADS), 0, st, yhat, nrows,
                       ncols, ld, w.s.p, w.flag.p);
    SS_LAUNCH_CHECK();
  }
  int nan_flag = 0;
  SS_HIP(hipMemcpyAsync(&nan_flag, w.flag.p, sizeof(int), hipMemcpyDeviceToHost, st));
  SS_HIP(hipStreamSynchronize(st));
  if (nan_flag) return fail(SS_EINVAL, "pool: a score is NaN");
  path_add(sizeof(K) == 4 ? "pool_radix_u32" : "pool_radix_u64");
  SS_TRY(pl_sort_desc<K>(w.s.p, w.s2.p, n, w));
  int64_t R = 0;
  SS_TRY(pl_runs<K>(w.s2.p, n, w, out.key, out.nneg, &out.npos, &R));
  out.n = R;
  if (nnz > 0) {
    SS_TRY(grow(w.q, (size_t)nnz));
    SS_TRY(grow(w.q2, (size_t)nnz));
    hipLaunchKernelGGL((pl_pos_keys_kernel<T, K, PtrT>), dim3(pl_grid(nnz)), dim3(PL_THREADS), 0, st, yptr, shift, yidx,
                       base, yhat, nrows, ld, w.q.p);
    SS_LAUNCH_CHECK();
    SS_TRY(pl_sort_desc<K>(w.q.p, w.q2.p, nnz, w));
    int64_t Q = 0;
    SS_TRY(pl_runs<K>(w.q2.p, nnz, w, w.qkey, w.qcnt, nullptr, &Q));
    hipLaunchKernelGGL(pl_join_kernel<K>, dim3(pl_grid(Q)), dim3(PL_THREADS), 0, st, w.qkey.p, w.qcnt.p, Q, out.key.p,
                       R, out.npos.p, out.nneg.p);
    SS_LAUNCH_CHECK();
  }
  return SS_OK;
}

template <class K>
int pool_merge(const PoolTable<K>& a, const PoolTable<K>& b, PoolWork<K>& w, PoolTable<K>& out) {
  if (a.n == 0) return pl_copy(b, out);
  if (b.n == 0) return pl_copy(a, out);
  hipStream_t st = ctx().stream;
  const int64_t n = a.n + b.n, nchunks = (n + PL_ITEMS - 1) / PL_ITEMS;
  SS_TRY(grow(w.cnt, (size_t)nchunks));
  SS_TRY(grow(w.inc, (size_t)nchunks));
  hipLaunchKernelGGL(pl_merge_count_kernel<K>, dim3(pl_grid(nchunks)), dim3(PL_THREADS), 0, st, a.key.p, a.n, b.key.p,
                     b.n, nchunks, w.cnt.p);
  SS_LAUNCH_CHECK();
  size_t bytes = 0;
  SS_HIP(rocprim::inclusive_scan(nullptr, bytes, w.cnt.p, w.inc.p, (size_t)nchunks, rocprim::plus<int64_t>(), st));
  SS_TRY(grow(w.tmp, bytes));
  SS_HIP(rocprim::inclusive_scan(w.tmp.p, bytes, w.cnt.p, w.inc.p, (size_t)nchunks, rocprim::plus<int64_t>(), st));
  int64_t total = 0;
  SS_HIP(hipMemcpyAsync(&total, w.inc.p + nchunks - 1, sizeof(int64_t), hipMemcpyDeviceToHost, st));
  SS_HIP(hipStreamSynchronize(st));
  PoolTable<K> t;
  SS_TRY(t.key.alloc((size_t)total));
  SS_TRY(t.npos.alloc((size_t)total));
  SS_TRY(t.nneg.alloc((size_t)total));
  t.n = total;
  hipLaunchKernelGGL(pl_merge_write_kernel<K>, dim3(pl_grid(nchunks)), dim3(PL_THREADS), 0, st, a.key.p, a.npos.p,
                     a.nneg.p, a.n, b.key.p, b.npos.p, b.nneg.p, b.n, nchunks, w.cnt.p, w.inc.p, t.key.p, t.npos.p,
                     t.nneg.p);
  SS_LAUNCH_CHECK();
  SS_HIP(hipStreamSynchronize(st));  // the caller may drop a or b next
  out = std::move(t);
  return SS_OK;
}

template <class K>
int64_t pool_stored(const std::vector<PoolTable<K>>& lv) {
  int64_t s = 0;
  for (const auto& t : lv) s += t.n;
  return s;
}

// Levels like a binary counter, by size: the new table absorbs the top level while that level holds at most twice
// its entries, so an entry is merged O(log(adds)) times over a sweep, not once per block.  The levels are changed
// only once every merge has succeeded and the bound holds.
template <class K>
int pool_push(std::vector<PoolTable<K>>& lv, PoolTable<K>&& t, int64_t other, int64_t max_entries, PoolWork<K>& w) {
  if (t.n == 0) return SS_OK;
  PoolTable<K> cur = std::move(t);
  size_t k = lv.size();
  while (k > 0 && lv[k - 1].n <= 2 * cur.n) {
    PoolTable<K> m;
    SS_TRY(pool_merge(lv[k - 1], cur, w, m));
    cur = std::move(m);
    --k;
  }
  int64_t stored = other + cur.n;
  for (size_t i = 0; i < k; ++i) stored += lv[i].n;
  if (stored > max_entries)
    return fail(SS_ENOMEM, "pool: %lld table entries would exceed max_entries = %lld", (long long)stored,
                (long long)max_entries);
  lv.resize(k);
  lv.push_back(std::move(cur));
  return SS_OK;
}

// the union of all levels as one new table (the levels are left as they are)
template <class K>
int pool_union(const std::vector<PoolTable<K>>& lv, PoolWork<K>& w, PoolTable<K>& out) {
  out = PoolTable<K>();
  if (lv.empty()) return SS_OK;
  PoolTable<K> cur;
  SS_TRY(pl_copy(lv.back(), cur));
  for (size_t k = lv.size() - 1; k-- > 0;) {
    PoolTable<K> m;
    SS_TRY(pool_merge(lv[k], cur, w, m));
    cur = std::move(m);
  }
  out = std::move(cur);
  return SS_OK;
}

template <class K>
int pool_consolidate(std::vector<PoolTable<K>>& lv, PoolWork<K>& w) {
  if (lv.size() <= 1) return SS_OK;
  PoolTable<K> u;
  SS_TRY(pool_union(lv, w, u));
  lv.clear();
  lv.push_back(std::move(u));
  return SS_OK;
}

template <class T>
int pool_import_table(const T* v, const int64_t* np, const int64_t* nn, int64_t n, PoolWork<pool_key_t<T>>& w,
                      PoolTable<pool_key_t<T>>& out, int64_t* P, int64_t* N) {
  using K = pool_key_t<T>;
  hipStream_t st = ctx().stream;
  PoolTable<K> t;
  SS_TRY(t.key.alloc((size_t)n));
  SS_TRY(t.npos.alloc((size_t)n));
  SS_TRY(t.nneg.alloc((size_t)n));
  t.n = n;
  SS_HIP(hipMemcpyAsync(t.npos.p, np, (size_t)n * sizeof(int64_t), hipMemcpyDeviceToDevice, st));
  SS_HIP(hipMemcpyAsync(t.nneg.p, nn, (size_t)n * sizeof(int64_t), hipMemcpyDeviceToDevice, st));
  DevBuf<unsigned long long> sums;
  SS_TRY(sums.alloc(2));
  SS_TRY(grow(w.flag, 4));
  SS_HIP(hipMemsetAsync(w.flag.p, 0, sizeof(int), st));
  SS_HIP(hipMemsetAsync(sums.p, 0, 2 * sizeof(unsigned long long), st));
  hipLaunchKernelGGL((pl_import_kernel<T, K>), dim3(pl_grid(n)), dim3(PL_THREADS), 0, st, v, np, nn, n, t.key.p,
                     w.flag.p, sums.p);
  SS_LAUNCH_CHECK();
  int flag = 0;
  unsigned long long hs[2];
  SS_HIP(hipMemcpyAsync(&flag, w.flag.p, sizeof(int), hipMemcpyDeviceToHost, st));
  SS_HIP(hipMemcpyAsync(hs, sums.p, sizeof(hs), hipMemcpyDeviceToHost, st));
  SS_HIP(hipStreamSynchronize(st));
  if (flag & 1) return fail(SS_EINVAL, "pool import: a score is NaN");
  if (flag & 2) return fail(SS_EINVAL, "pool import: a count is negative or an entry has no pairs");
  if (flag & 4) return fail(SS_EINVAL, "pool import: scores are not strictly descending (-0.0 equals +0.0)");
  *P = (int64_t)hs[0];
  *N = (int64_t)hs[1];
  out = std::move(t);
  return SS_OK;
}

template <class T>
int pool_export_table(const PoolTable<pool_key_t<T>>& t, T* v) {
  if (t.n == 0) return SS_OK;
  hipLaunchKernelGGL((pl_export_kernel<T, pool_key_t<T>>), dim3(pl_grid(t.n)), dim3(PL_THREADS), 0, ctx().stream,
                     t.key.p, t.n, v);
  SS_LAUNCH_CHECK();
  return SS_OK;
}

// out[0..21): AuROC, AuPRC, validity ratio, then (max, mean, std) of f1score, mcc, accuracy, balancedaccuracy, recall,
// precision over the table's thresholds.  P positives, N negatives in all (P + N > 0).
template <class K>
int pool_table_metrics(const PoolTable<K>& t, int64_t P, int64_t N, PoolWork<K>& w, double* out) {
  hipStream_t st = ctx().stream;
  const int64_t E = t.n;
  DevBuf<int64_t> ctp, cfp;
  SS_TRY(ctp.alloc((size_t)E));
  SS_TRY(cfp.alloc((size_t)E));
  size_t bytes = 0;
  SS_HIP(rocprim::inclusive_scan(nullptr, bytes, t.npos.p, ctp.p, (size_t)E, rocprim::plus<int64_t>(), st));
  SS_TRY(grow(w.tmp, bytes));
  SS_HIP(rocprim::inclusive_scan(w.tmp.p, bytes, t.npos.p, ctp.p, (size_t)E, rocprim::plus<int64_t>(), st));
  SS_HIP(rocprim::inclusive_scan(w.tmp.p, bytes, t.nneg.p, cfp.p, (size_t)E, rocprim::plus<int64_t>(), st));
  const int G = pl_grid(E, PL_MAX_BLOCKS);
  DevBuf<double> part, pmax;
  DevBuf<int> pnan;
  SS_TRY(part.alloc((size_t)G * PL_NQ));
  SS_TRY(pmax.alloc((size_t)G * 6));
  SS_TRY(pnan.alloc((size_t)G));
  const K zero_key = (K)1 << (8 * sizeof(K) - 1);  // the key of +0.0
  hipLaunchKernelGGL(pl_terms_kernel<K>, dim3(G), dim3(PL_THREADS), 0, st, t.key.p, ctp.p, cfp.p, E, zero_key,
                     (long long)P, (long long)N, part.p, pmax.p, pnan.p);
  SS_LAUNCH_CHECK();
  std::vector<double> hp((size_t)G * PL_NQ), hm((size_t)G * 6);
  std::vector<int> hn((size_t)G);
  SS_HIP(hipMemcpyAsync(hp.data(), part.p, hp.size() * sizeof(double), hipMemcpyDeviceToHost, st));
  SS_HIP(hipMemcpyAsync(hm.data(), pmax.p, hm.size() * sizeof(double), hipMemcpyDeviceToHost, st));
  SS_HIP(hipMemcpyAsync(hn.data(), pnan.p, hn.size() * sizeof(int), hipMemcpyDeviceToHost, st));
  SS_HIP(hipStreamSynchronize(st));
  double s[PL_NQ], mx[6];
  int nanb = 0;
  for (int q = 0; q < PL_NQ; ++q) s[q] = 0.0;
  for (int q = 0; q < 6; ++q) mx[q] = -HUGE_VAL;
  for (int b = 0; b < G; ++b) {
    for (int q = 0; q < PL_NQ; ++q) s[q] += hp[(size_t)b * PL_NQ + q];
    for (int q = 0; q < 6; ++q) mx[q] = hm[(size_t)b * 6 + q] > mx[q] ? hm[(size_t)b * 6 + q] : mx[q];
    nanb |= hn[b];
  }
  PlMean mean;
  const double U = (double)E;
  for (int q = 0; q < 6; ++q) mean.m[q] = s[3 + q] / U;
  hipLaunchKernelGGL(pl_sqdev_kernel, dim3(G), dim3(PL_THREADS), 0, st, ctp.p, cfp.p, E, (long long)P, (long long)N,
                     mean, part.p);
  SS_LAUNCH_CHECK();
  SS_HIP(hipMemcpyAsync(hp.data(), part.p, (size_t)G * 6 * sizeof(double), hipMemcpyDeviceToHost, st));
  SS_HIP(hipStreamSynchronize(st));
  double sq[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  for (int b = 0; b < G; ++b)
    for (int q = 0; q < 6; ++q) sq[q] += hp[(size_t)b * 6 + q];
  out[0] = fabs(s[0]);  // 0/0 -> NaN when one class is missing, as for one vector (launch_rank_metrics)
  out[1] = fabs(s[1]);
  out[2] = s[2] / (double)(P + N);
  const double qnan = std::nan("");
  for (int q = 0; q < 6; ++q) {
    const bool isnan_q = (nanb >> q) & 1;
    out[3 + 3 * q] = isnan_q ? qnan : mx[q];
    out[4 + 3 * q] = isnan_q ? qnan : mean.m[q];
    out[5 + 3 * q] = isnan_q || E == 1 ? qnan : std::sqrt(sq[q] / (double)(E - 1));
  }
  return SS_OK;
}

#define SS_POOL_INST(T, K)                                                                                          \
  template int pool_block_table<T, int64_t>(const int64_t*, int64_t, const int*, int, int64_t, const T*, int64_t,   \
                                            int64_t, int64_t, PoolWork<K>&, PoolTable<K>&);                         \
  template int pool_block_table<T, int>(const int*, int64_t, const int*, int, int64_t, const T*, int64_t, int64_t,  \
                                        int64_t, PoolWork<K>&, PoolTable<K>&);                                      \
  template int pool_import_table<T>(const T*, const int64_t*, const int64_t*, int64_t, PoolWork<K>&, PoolTable<K>&, \
                                    int64_t*, int64_t*);                                                            \
  template int pool_export_table<T>(const PoolTable<K>&, T*);                                                       \
  template int pool_push<K>(std::vector<PoolTable<K>>&, PoolTable<K>&&, int64_t, int64_t, PoolWork<K>&);            \
  template int pool_union<K>(const std::vector<PoolTable<K>>&, PoolWork<K>&, PoolTable<K>&);                        \
  template int pool_consolidate<K>(std::vector<PoolTable<K>>&, PoolWork<K>&);                                       \
  template int64_t pool_stored<K>(const std::vector<PoolTable<K>>&);                                                \
  template int pool_table_metrics<K>(const PoolTable<K>&, int64_t, int64_t, PoolWork<K>&, double*);
SS_POOL_INST(float, uint32_t)
SS_POOL_INST(double, uint64_t)
#undef SS_POOL_INST

}  // namespace ss
