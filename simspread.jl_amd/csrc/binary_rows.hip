// Per-row binary prediction metrics of a score block on the device: for every row the six confusion-matrix metrics of
// the reference (f1score, mcc, accuracy, balancedaccuracy, recall, precision; src/performance.jl:102-296) at every
// threshold, summarised as maxperformance / meanperformance / meanstdperformance do (src/performance.jl:420-520):
// out[r*18 + 3*m + s], s = max, mean, std.  The thresholds of a row are its distinct scores; at threshold v a column is
// predicted positive iff score >= v.
//
// Every distinct score is a threshold, including those held only by negatives, so a row is ordered for real: its
// (score, label) pairs are sorted by score descending (the order inside a tie group does not matter) and scanned once
// per pass; the last element of every tie group is a threshold with tp = #positives so far and fp = position + 1 - tp.
// Pass 1 takes max, sum and the number U of thresholds; pass 2 the sum of squared deviations from sum / U.
//
// Two paths, one epilogue (br_row), so a row's 18 numbers do not depend on the path that served it: rows of at most
// BR_LDS_MAXN columns are loaded, bitonic-sorted, scanned and reduced in LDS by one workgroup per row; longer rows are
// staged in global scratch -- a rocPRIM segmented radix sort of (score, label) pairs, then one workgroup per row for the
// two passes.  The scratch of the long path is bounded by BR_BATCH_ELEMS elements, not by the row count.  The
// position -> thread map and every double sum have one fixed order: results are bitwise repeatable.
//
// The per-threshold arithmetic is the host mirror's (simspread.jl_amd/metrics.py) operation for operation, in double
// with integer counts, without FP contraction: a fused a*e - b*e would no longer be the mirror's value.
#include <hip/hip_runtime.h>

#include <cstring>
#include <vector>

#include <rocprim/rocprim.hpp>

#include "binary_metrics.hpp"
#include "graph.hpp"

namespace ss {

namespace {

#pragma clang fp contract(off)

constexpr int BR_THREADS = 1024;
constexpr int BR_WAVES = BR_THREADS / 64;
constexpr int BR_NM = 6;                     // metrics per row
constexpr int BR_LDS_MAXN = 16384;           // columns per row on the LDS path: 16384 x (8 + 1) B + scratch
constexpr int64_t BR_BATCH_ELEMS = 1 << 25;  // elements per long-path batch (bounds its scratch)

struct BrScratch {
  double d[BR_WAVES * BR_NM];
  double x[BR_WAVES * BR_NM];
  double mean[BR_NM];
  int cnt[BR_WAVES];
  int u[BR_WAVES];
  int nanb[BR_WAVES];
  int U, nan_all;
};

// The 18 numbers of one row from its elements sorted by score descending: key[0..n) (-0 already +0), lab[i] = 1 for a
// positive.  Position i is handled by thread i % BR_THREADS in increasing i; the block sums run in one fixed order.
// key / lab may live in LDS or in global memory.  Called by all BR_THREADS threads; thread 0 writes o[0..18).
template <class T>
__device__ void br_row(const T* key, const unsigned char* lab, int n, int P, double* o, BrScratch* sc) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const unsigned long long le = lane == 63 ? ~0ULL : ((1ULL << (lane + 1)) - 1ULL);
  const long long Pl = P, Nl = (long long)n - P;
  double mx[BR_NM], acc[BR_NM];
  int u = 0, nanb = 0;
  for (int k = 0; k < BR_NM; ++k) {
    mx[k] = -__builtin_inf();
    acc[k] = 0.0;
  }
  for (int pass = 0; pass < 2; ++pass) {
    double mean[BR_NM];
    if (pass == 1)
      for (int k = 0; k < BR_NM; ++k) {
        mean[k] = sc->mean[k];
        acc[k] = 0.0;
      }
    int carry = 0;
    for (int base = 0; base < n; base += BR_THREADS) {
      const int i = base + tid;
      const bool in = i < n;
      const unsigned long long b = __ballot(in && lab[i] != 0);
      if (lane == 0) sc->cnt[wave] = (int)__popcll(b);
      __syncthreads();
      int pre = carry, tot = carry;
      for (int w = 0; w < BR_WAVES; ++w) {
        const int c = sc->cnt[w];
        if (w < wave) pre += c;
        tot += c;
      }
      __syncthreads();
      carry = tot;
      if (in && (i == n - 1 || key[i] != key[i + 1])) {  // last element of its tie group: a threshold
        const long long tp = pre + (int)__popcll(b & le);
        double m[BR_NM];
        br_metrics(tp, (long long)i + 1 - tp, Pl, Nl, m);
        if (pass == 0) {
          ++u;
          for (int k = 0; k < BR_NM; ++k) {
            if (m[k] != m[k]) nanb |= 1 << k;
            else if (m[k] > mx[k]) mx[k] = m[k];
            acc[k] += m[k];
          }
        } else {
          for (int k = 0; k < BR_NM; ++k) {
            const double dv = m[k] - mean[k];
            acc[k] += dv * dv;
          }
        }
      }
    }
    // fixed-order block reduction: a shuffle tree per wave, then the waves in order
    for (int k = 0; k < BR_NM; ++k)
      for (int off = 32; off > 0; off >>= 1) {
        acc[k] += __shfl_down(acc[k], off);
        if (pass == 0) {
          const double y = __shfl_down(mx[k], off);
          mx[k] = y > mx[k] ? y : mx[k];
        }
      }
    if (pass == 0)
      for (int off = 32; off > 0; off >>= 1) {
        u += __shfl_down(u, off);
        nanb |= __shfl_down(nanb, off);
      }
    if (lane == 0) {
      for (int k = 0; k < BR_NM; ++k) {
        sc->d[wave * BR_NM + k] = acc[k];
        sc->x[wave * BR_NM + k] = mx[k];
      }
      sc->u[wave] = u;
      sc->nanb[wave] = nanb;
    }
    __syncthreads();
    if (tid == 0) {
      int U = 0, nb = 0;
      double s[BR_NM], x[BR_NM];
      for (int k = 0; k < BR_NM; ++k) {
        s[k] = 0.0;
        x[k] = -__builtin_inf();
      }
      for (int w = 0; w < BR_WAVES; ++w) {
        U += sc->u[w];
        nb |= sc->nanb[w];
        for (int k = 0; k < BR_NM; ++k) {
          s[k] += sc->d[w * BR_NM + k];
          const double y = sc->x[w * BR_NM + k];
          x[k] = y > x[k] ? y : x[k];
        }
      }
      if (pass == 0) {
        sc->U = U;
        sc->nan_all = nb;
        for (int k = 0; k < BR_NM; ++k) {
          sc->mean[k] = s[k] / (double)U;
          o[3 * k] = (nb >> k) & 1 ? br_nan() : x[k];
          o[3 * k + 1] = (nb >> k) & 1 ? br_nan() : sc->mean[k];
        }
      } else {
        for (int k = 0; k < BR_NM; ++k)
          o[3 * k + 2] = ((sc->nan_all >> k) & 1) || sc->U == 1 ? br_nan() : sqrt(s[k] / (double)(sc->U - 1));
      }
    }
    __syncthreads();
  }
}

template <class T>
__device__ inline T br_key(T v) { return v == T(0) ? T(0) : v; }  // -0 -> +0: one key for one tie group

// ------------------------------------------------------------------ LDS path
// LDS: key[NP] (T), lab[NP] (0 negative, 1 positive, 2 padding), BrScratch
template <class T, class PtrT>
__global__ void __launch_bounds__(BR_THREADS) br_lds_kernel(const PtrT* __restrict__ yptr, int64_t shift,
                                                            const int* __restrict__ yidx, int base,
                                                            const T* __restrict__ yhat, int n, int64_t ld, int NP,
                                                            double* __restrict__ out) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  T* key = reinterpret_cast<T*>(smem);
  unsigned char* lab = reinterpret_cast<unsigned char*>(key + NP);
  BrScratch* sc = reinterpret_cast<BrScratch*>(lab + NP);  // NP is a multiple of 64
  const int64_t r = blockIdx.x;
  const int tid = threadIdx.x;
  const int64_t e0 = (int64_t)yptr[r] - shift;
  const int P = (int)((int64_t)yptr[r + 1] - shift - e0);
  const T* row = yhat + r * ld;
  for (int i = tid; i < NP; i += BR_THREADS) {
    if (i < n) {
      key[i] = br_key(row[i]);
      lab[i] = 0;
    } else {
      key[i] = T(0);
      lab[i] = 2;
    }
  }
  __syncthreads();
  for (int e = tid; e < P; e += BR_THREADS) lab[yidx[e0 + e] - base] = 1;
  __syncthreads();
  // bitonic sort, score descending, padding last; equal scores may land in either order
  for (int kk = 2; kk <= NP; kk <<= 1) {
    for (int jj = kk >> 1; jj > 0; jj >>= 1) {
      for (int i = tid; i < NP; i += BR_THREADS) {
        const int x = i ^ jj;
        if (x > i) {
          const T si = key[i], sx = key[x];
          const unsigned char li = lab[i], lx = lab[x];
          const bool x_first = lx != 2 && (li == 2 || sx > si);  // does x belong before i?
          const bool i_first = li != 2 && (lx == 2 || si > sx);
          const bool swap = ((i & kk) == 0) ? x_first : i_first;
          if (swap) {
            key[i] = sx; key[x] = si;
            lab[i] = lx; lab[x] = li;
          }
        }
      }
      __syncthreads();
    }
  }
  br_row<T>(key, lab, n, P, out + r * 18, sc);
}

// ------------------------------------------------------------------ long path
// one workgroup per row of the batch: scores (-0 -> +0) and labels (zeroed by the caller) into the sort's input
template <class T, class PtrT>
__global__ void __launch_bounds__(BR_THREADS) br_stage_kernel(const PtrT* __restrict__ yptr, int64_t shift,
                                                              const int* __restrict__ yidx, int base,
                                                              const T* __restrict__ yhat, int64_t r0, int64_t n,
                                                              int64_t ld, T* __restrict__ key,
                                                              unsigned char* __restrict__ lab) {
  const int64_t r = r0 + blockIdx.x;
  const int64_t q = (int64_t)blockIdx.x * n;
  const T* row = yhat + r * ld;
  for (int64_t c = threadIdx.x; c < n; c += BR_THREADS) key[q + c] = br_key(row[c]);
  const int64_t e0 = (int64_t)yptr[r] - shift, e1 = (int64_t)yptr[r + 1] - shift;
  for (int64_t e = e0 + threadIdx.x; e < e1; e += BR_THREADS) lab[q + yidx[e] - base] = 1;
}

template <class T, class PtrT>
__global__ void __launch_bounds__(BR_THREADS) br_large_finish_kernel(const PtrT* __restrict__ yptr, int64_t r0,
                                                                     int64_t n, const T* __restrict__ key,
                                                                     const unsigned char* __restrict__ lab,
                                                                     double* __restrict__ out) {
  __shared__ BrScratch sc;
  const int64_t r = r0 + blockIdx.x;
  const int64_t q = (int64_t)blockIdx.x * n;
  const int P = (int)((int64_t)yptr[r + 1] - (int64_t)yptr[r]);
  br_row<T>(key + q, lab + q, (int)n, P, out + r * 18, &sc);
}

}  // namespace

template <class T, class PtrT>
int launch_binary_rows(const PtrT* yptr, int64_t shift, const int* yidx, int base, const T* yhat, int64_t nrows,
                       int64_t ncols, int64_t ld, double* out) {
  hipStream_t st = ctx().stream;
  if (nrows == 0) return SS_OK;
  int64_t cap = BR_LDS_MAXN;
  if (ctx().binary_lds_cols >= 0 && ctx().binary_lds_cols < cap) cap = ctx().binary_lds_cols;
  if (ncols <= cap) {
    int NP = 64;
    while (NP < ncols) NP <<= 1;
    const size_t lds = (size_t)NP * (sizeof(T) + 1) + sizeof(BrScratch);
    SS_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(&br_lds_kernel<T, PtrT>),
                               hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    hipLaunchKernelGGL((br_lds_kernel<T, PtrT>), dim3((unsigned)nrows), dim3(BR_THREADS), lds, st, yptr, shift, yidx,
                       base, yhat, (int)ncols, ld, NP, out);
    SS_LAUNCH_CHECK();
    path_add("binary_rows_lds");
    return SS_OK;
  }
  path_add("binary_rows_large");
  int64_t rb = BR_BATCH_ELEMS / ncols;
  if (rb < 1) rb = 1;
  if (rb > nrows) rb = nrows;
  const int64_t cap_elems = rb * ncols;
  DevBuf<T> key_in, key_out;
  DevBuf<unsigned char> lab_in, lab_out, tmp;
  DevBuf<int> dseg;
  SS_TRY(key_in.alloc((size_t)cap_elems));
  SS_TRY(key_out.alloc((size_t)cap_elems));
  SS_TRY(lab_in.alloc((size_t)cap_elems));
  SS_TRY(lab_out.alloc((size_t)cap_elems));
  SS_TRY(dseg.alloc((size_t)rb + 1));
  {
    std::vector<int> seg((size_t)rb + 1);
    for (int64_t i = 0; i <= rb; ++i) seg[(size_t)i] = (int)(i * ncols);
    SS_HIP(hipMemcpyAsync(dseg.p, seg.data(), seg.size() * sizeof(int), hipMemcpyHostToDevice, st));
    SS_HIP(hipStreamSynchronize(st));  // seg is a stack buffer
  }
  size_t bytes = 0;
  SS_HIP(rocprim::segmented_radix_sort_pairs_desc(nullptr, bytes, key_in.p, key_out.p, lab_in.p, lab_out.p,
                                                  (unsigned)cap_elems, (unsigned)rb, dseg.p, dseg.p + 1, 0,
                                                  (unsigned)(8 * sizeof(T)), st));
  SS_TRY(tmp.alloc(bytes));
  for (int64_t r0 = 0; r0 < nrows; r0 += rb) {
    const int64_t nb = nrows - r0 < rb ? nrows - r0 : rb;
    const size_t elems = (size_t)(nb * ncols);
    SS_HIP(hipMemsetAsync(lab_in.p, 0, elems, st));
    hipLaunchKernelGGL((br_stage_kernel<T, PtrT>), dim3((unsigned)nb), dim3(BR_THREADS), 0, st, yptr, shift, yidx, base,
                       yhat, r0, ncols, ld, key_in.p, lab_in.p);
    SS_LAUNCH_CHECK();
    SS_HIP(rocprim::segmented_radix_sort_pairs_desc(tmp.p, bytes, key_in.p, key_out.p, lab_in.p, lab_out.p,
                                                    (unsigned)elems, (unsigned)nb, dseg.p, dseg.p + 1, 0,
                                                    (unsigned)(8 * sizeof(T)), st));
    hipLaunchKernelGGL((br_large_finish_kernel<T, PtrT>), dim3((unsigned)nb), dim3(BR_THREADS), 0, st, yptr, r0, ncols,
                       key_out.p, lab_out.p, out);
    SS_LAUNCH_CHECK();
  }
  // the scratch is released on return: let the kernels finish first
  SS_HIP(hipStreamSynchronize(st));
  return SS_OK;
}

template int launch_binary_rows<float, int64_t>(const int64_t*, int64_t, const int*, int, const float*, int64_t,
                                                int64_t, int64_t, double*);
template int launch_binary_rows<double, int64_t>(const int64_t*, int64_t, const int*, int, const double*, int64_t,
                                                 int64_t, int64_t, double*);
template int launch_binary_rows<float, int>(const int*, int64_t, const int*, int, const float*, int64_t, int64_t,
                                            int64_t, double*);
template int launch_binary_rows<double, int>(const int*, int64_t, const int*, int, const double*, int64_t, int64_t,
                                             int64_t, double*);

}  // namespace ss
