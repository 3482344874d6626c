// Per-row ranking metrics of a score block on the device: for every row the six numbers the reference computes on
// one vector -- AuROC, AuPRC, BEDROC(alpha), validity ratio (src/performance.jl:22-89,558-560) and recall@L /
// precision@L (src/performance.jl:308-385) -- with the positives of row r given as CSR column indices.
//
// No row is sorted.  Every metric is a function of integer counts taken against the row's positives sorted as
// sortperm order (score descending, ties by ascending column).  For an element e of score s and column c:
//   j(e) = #{positives with score > s}
//   tied(e) = s equals some positive's score (then j(e) is the first positive of that tie group)
//   k(e) = #{positives before e in sortperm order} (only needed when tied: j(e) + #{group positives with column < c})
// and three histograms over 0..P:
//   gap[j]   elements that tie with no positive (they lie strictly between two positive score groups)
//   tieG[j]  elements tied with the group that starts at positive j (the group's positives included)
//   tieK[k]  tied elements by k
// With R = inclusive scan of gap + tieK and Q = inclusive scan of gap + tieG:
//   rank of positive k (1-based, sortperm order)  = R[k]
//   #{score >= v} of the group starting at a     = Q[a],   #{score > v} = Q[a] - tieG[a]
// Between two positive-bearing thresholds the ROC and PR curves only step horizontally, so the reference's
// trapezoid sums over all unique scores collapse onto the positive groups:
//   2 N P AuROC = sum_groups ([#{>v} > 0] negtied (tp_ge + tp_gt) + 2 gap[a] a) + 2 gap[P] P     (exact, int64)
//   AuPRC       = sum_groups [#{>v} > 0] (tp_ge/P - tp_gt/P) (tp_ge/#{>=v} + tp_gt/#{>v}) / 2
// ([#{>v} > 0]: the reference's trapezoid has no (0,0) point, so the topmost threshold opens no segment.)
//
// Two paths, the same counts and the same epilogue (so a row's six numbers do not depend on the path that served
// it): rows with at most RR_LDS_MAXP positives keep positives and histograms in LDS, one 256-thread workgroup per
// row that loads, bitonic-sorts, streams the row once and finishes it; longer rows (C5's hot sources reach nt
// positives) keep them in global memory -- gather, rocPRIM segmented radix sort, a count pass split over several
// workgroups per row, a finish pass.  Histogram updates are integer atomics aggregated per wave for the hot bucket;
// every double sum runs in a fixed order.  Results are bitwise repeatable.
#include <hip/hip_runtime.h>

#include <climits>
#include <cstring>
#include <vector>

#include <rocprim/rocprim.hpp>

#include "graph.hpp"

namespace ss {

namespace {

constexpr int RR_THREADS = 256;
constexpr int RR_WAVES = RR_THREADS / 64;
constexpr int RR_LDS_MAXP = 2048;        // positives per row on the LDS path
constexpr int RR_UNROLL = 4;             // row elements in flight per thread
constexpr int64_t RR_BATCH_POS = 1 << 24;  // positives per large-path batch (bounds its scratch)
constexpr int RR_SPLIT_COLS = 8192;      // columns per count workgroup on the large path

__device__ inline double rr_nan() { return __longlong_as_double(0x7ff8000000000000LL); }

// #{k in [lo,hi): ps[k] > v} + lo, ps descending
template <class T>
__device__ inline int rr_cnt_gt(const T* ps, int lo, int hi, T v) {
  while (lo < hi) {
    const int m = (lo + hi) >> 1;
    if (ps[m] > v) lo = m + 1; else hi = m;
  }
  return lo;
}
template <class T>
__device__ inline int rr_cnt_ge(const T* ps, int lo, int hi, T v) {
  while (lo < hi) {
    const int m = (lo + hi) >> 1;
    if (ps[m] >= v) lo = m + 1; else hi = m;
  }
  return lo;
}
__device__ inline int rr_col_lb(const int* pc, int lo, int hi, int c) {
  while (lo < hi) {
    const int m = (lo + hi) >> 1;
    if (pc[m] < c) lo = m + 1; else hi = m;
  }
  return lo;
}

// h[idx] += 1 for every lane with on; the lanes that share the first such lane's bucket add once, together.
// Called by all 64 lanes of the wave.
__device__ inline void rr_wave_add(int* h, int idx, bool on) {
  const unsigned long long m = __ballot(on);
  if (m == 0) return;
  const int leader = __ffsll((long long)m) - 1;
  const int lidx = __shfl(idx, leader);
  const bool same = on && idx == lidx;
  const unsigned long long sm = __ballot(same);
  if (same) {
    if ((int)(threadIdx.x & 63) == leader) atomicAdd(&h[idx], (int)__popcll(sm));
  } else if (on) {
    atomicAdd(&h[idx], 1);
  }
}

// count one element of score v at column c against the sorted positives (ps, pc; P of them)
template <class T>
__device__ inline void rr_count(const T* ps, const int* pc, int P, T v, int c, bool on, int* gap, int* tieG,
                                int* tieK) {
  int j = 0, k = 0;
  bool tied = false;
  if (on) {
    j = rr_cnt_gt(ps, 0, P, v);
    tied = j < P && ps[j] == v;
    if (tied) k = rr_col_lb(pc, j, rr_cnt_ge(ps, j, P, v), c);
  }
  rr_wave_add(gap, j, on && !tied);
  rr_wave_add(tieG, j, on && tied);
  rr_wave_add(tieK, k, on && tied);
}

// fixed-order block sums; the result is valid in thread 0 (scratch: RR_WAVES slots of 8 bytes)
template <class V>
__device__ inline V rr_block_sum(V v, V* scratch) {
  for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off);
  if ((threadIdx.x & 63) == 0) scratch[threadIdx.x >> 6] = v;
  __syncthreads();
  V s = V(0);
  if (threadIdx.x == 0)
    for (int w = 0; w < RR_WAVES; ++w) s += scratch[w];
  __syncthreads();
  return s;
}

// in place over [0, n): a1 = inclusive scan of (g + a1), a2 = inclusive scan of (g + a2); each element is read and
// written by one thread only, so the arrays may live in LDS or in global memory (one workgroup owns them)
__device__ inline void rr_scan2(const int* g, int* a1, int* a2, int n, int* wsum) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  int carry1 = 0, carry2 = 0;
  for (int base = 0; base < n; base += RR_THREADS) {
    const int i = base + (int)threadIdx.x;
    int x1 = 0, x2 = 0;
    if (i < n) {
      const int gi = g[i];
      x1 = gi + a1[i];
      x2 = gi + a2[i];
    }
    for (int off = 1; off < 64; off <<= 1) {
      const int y1 = __shfl_up(x1, off), y2 = __shfl_up(x2, off);
      if (lane >= off) { x1 += y1; x2 += y2; }
    }
    if (lane == 63) { wsum[wave] = x1; wsum[RR_WAVES + wave] = x2; }
    __syncthreads();
    int add1 = carry1, add2 = carry2, tot1 = carry1, tot2 = carry2;
    for (int w = 0; w < RR_WAVES; ++w) {
      if (w < wave) { add1 += wsum[w]; add2 += wsum[RR_WAVES + w]; }
      tot1 += wsum[w];
      tot2 += wsum[RR_WAVES + w];
    }
    if (i < n) { a1[i] = x1 + add1; a2[i] = x2 + add2; }
    carry1 = tot1;
    carry2 = tot2;
    __syncthreads();
  }
}

struct RedScratch {
  double d[RR_WAVES];
  long long l[RR_WAVES];
  int w[2 * RR_WAVES];
};

// The six numbers of one row from the scanned counts.  R = scan(gap + tieK), Q = scan(gap + tieG), both P + 1 long.
// Positive k is handled by thread k % RR_THREADS, in increasing k, so every double sum has one fixed order.
template <class T>
__device__ void rr_finish(const T* ps, const int* R, const int* Q, const int* gap, int P, int64_t n, double alpha,
                          int L, int nz, int distinct, double* o, RedScratch* red) {
  long long num2 = 0;
  double prc = 0.0, bed = 0.0;
  int hit = 0;
  const double Pd = (double)P, nd = (double)n;
  for (int k = (int)threadIdx.x; k < P; k += RR_THREADS) {
    const int rank = R[k];
    bed += exp(-alpha * (double)rank / nd);
    hit += rank <= L ? 1 : 0;
    const T v = ps[k];
    if (k == P - 1 || ps[k + 1] != v) {  // last positive of its score group
      const int a = rr_cnt_gt(ps, 0, k, v);
      const long long ge = Q[a];
      const long long tg = ge - (a > 0 ? (long long)Q[a - 1] : 0LL) - gap[a];
      const long long gt = ge - tg;
      const long long tp_gt = a, tp_ge = (long long)k + 1;
      if (gt > 0) {
        num2 += (tg - (tp_ge - tp_gt)) * (tp_ge + tp_gt);
        const double tp1 = (double)tp_ge, tp0 = (double)tp_gt;
        prc += (tp1 / Pd - tp0 / Pd) * (tp1 / (double)ge + tp0 / (double)gt) * 0.5;
      }
      num2 += 2LL * (long long)gap[a] * tp_gt;
    }
  }
  if (threadIdx.x == 0) num2 += 2LL * (long long)gap[P] * (long long)P;
  num2 = rr_block_sum<long long>(num2, red->l);
  prc = rr_block_sum<double>(prc, red->d);
  bed = rr_block_sum<double>(bed, red->d);
  const long long hits = rr_block_sum<long long>((long long)hit, red->l);
  if (threadIdx.x == 0) {
    const double Nn = nd - Pd;
    double auroc, auprc;
    if (P == 0 || (int64_t)P == n) auroc = distinct ? rr_nan() : 0.0;  // a class is missing: 0/0 rates
    else auroc = (double)num2 / (2.0 * Nn * Pd);
    auprc = P == 0 ? (distinct ? rr_nan() : 0.0) : prc;
    // BEDROC (src/performance.jl:22-38), as ss_rank_metrics_f32 evaluates it
    const double Ra = Pd / nd;
    const double rand_sum = Ra * (1.0 - exp(-alpha)) / (exp(alpha / nd) - 1.0);
    const double fac = Ra * sinh(alpha / 2.0) / (cosh(alpha / 2.0) - cosh(alpha / 2.0 - alpha * Ra));
    const double cte = 1.0 / (1.0 - exp(alpha * (1.0 - Ra)));
    o[0] = auroc;
    o[1] = auprc;
    o[2] = bed * fac / rand_sum + cte;
    o[3] = (double)nz / nd;
    o[4] = P > 0 ? (double)hits / Pd : rr_nan();
    o[5] = (double)hits / (double)L;
  }
}

// ------------------------------------------------------------------ label check
// status bits: 1 index out of range, 2 not strictly increasing within its row
template <class PtrT>
__global__ void __launch_bounds__(RR_THREADS) rr_validate_kernel(const PtrT* __restrict__ yptr, int64_t shift,
                                                                 const int* __restrict__ yidx, int base, int64_t nrows,
                                                                 int64_t ncols, int* __restrict__ status) {
  int bad = 0;
  for (int64_t r = blockIdx.x; r < nrows; r += gridDim.x) {
    const int64_t e0 = (int64_t)yptr[r] - shift, e1 = (int64_t)yptr[r + 1] - shift;
    for (int64_t e = e0 + threadIdx.x; e < e1; e += RR_THREADS) {
      const int64_t c = (int64_t)yidx[e] - base;
      if (c < 0 || c >= ncols) bad |= 1;
      if (e > e0 && yidx[e] <= yidx[e - 1]) bad |= 2;
    }
  }
  if (bad) atomicOr(status, bad);
}

// ------------------------------------------------------------------ LDS path
// LDS: ps[NP] (T), pc[NP], gap / tieG / tieK [P1 each], RedScratch
template <class T, class PtrT>
__global__ void __launch_bounds__(RR_THREADS) rr_lds_kernel(const PtrT* __restrict__ yptr, int64_t shift,
                                                            const int* __restrict__ yidx, int base,
                                                            const T* __restrict__ yhat, int64_t ncols, int64_t ld,
                                                            int cap, int NP, int P1, double alpha, int L,
                                                            double* __restrict__ out) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int64_t r = blockIdx.x;
  const int64_t e0 = (int64_t)yptr[r] - shift;
  const int P = (int)((int64_t)yptr[r + 1] - shift - e0);
  if (P > cap) return;  // the large path serves this row
  T* ps = reinterpret_cast<T*>(smem);
  int* pc = reinterpret_cast<int*>(ps + NP);
  int* gap = pc + NP;
  int* tieG = gap + P1;
  int* tieK = tieG + P1;
  RedScratch* red = reinterpret_cast<RedScratch*>(tieK + P1);
  const T* row = yhat + r * ld;
  const int tid = threadIdx.x;

  for (int i = tid; i < NP; i += RR_THREADS) {
    if (i < P) {
      const int c = yidx[e0 + i] - base;
      ps[i] = row[c];
      pc[i] = c;
    } else {
      ps[i] = T(0);
      pc[i] = INT_MAX;  // padding sorts last
    }
  }
  for (int i = tid; i < 3 * P1; i += RR_THREADS) gap[i] = 0;
  __syncthreads();
  // bitonic sort of (score desc, column asc); the keys are distinct (columns are)
  if (P > 1) {
    for (int kk = 2; kk <= NP; kk <<= 1) {
      for (int jj = kk >> 1; jj > 0; jj >>= 1) {
        for (int i = tid; i < NP; i += RR_THREADS) {
          const int x = i ^ jj;
          if (x > i) {
            const T si = ps[i], sx = ps[x];
            const int ci = pc[i], cx = pc[x];
            // does (sx, cx) come before (si, ci)?
            const bool x_first = cx != INT_MAX && (ci == INT_MAX || sx > si || (sx == si && cx < ci));
            const bool swap = ((i & kk) == 0) ? x_first : !x_first;
            if (swap) {
              ps[i] = sx; ps[x] = si;
              pc[i] = cx; pc[x] = ci;
            }
          }
        }
        __syncthreads();
      }
    }
  }

  const T s0 = row[0];
  int nz = 0, dif = 0;
  for (int64_t c0 = 0; c0 < ncols; c0 += (int64_t)RR_THREADS * RR_UNROLL) {
    T v[RR_UNROLL];
#pragma unroll
    for (int u = 0; u < RR_UNROLL; ++u) {
      const int64_t c = c0 + (int64_t)u * RR_THREADS + tid;
      v[u] = c < ncols ? row[c] : T(0);
    }
#pragma unroll
    for (int u = 0; u < RR_UNROLL; ++u) {
      const int64_t c = c0 + (int64_t)u * RR_THREADS + tid;
      const bool on = c < ncols;
      if (on) {
        nz += v[u] != T(0) ? 1 : 0;
        dif |= v[u] != s0 ? 1 : 0;
      }
      rr_count<T>(ps, pc, P, v[u], (int)c, on, gap, tieG, tieK);
    }
  }
  nz = (int)rr_block_sum<long long>((long long)nz, red->l);
  dif = (int)rr_block_sum<long long>((long long)dif, red->l);
  // every thread needs neither; thread 0 holds them for rr_finish
  rr_scan2(gap, tieK, tieG, P + 1, red->w);
  rr_finish<T>(ps, tieK, tieG, gap, P, ncols, alpha, L, nz, dif, out + r * 6, red);
}

// ------------------------------------------------------------------ large-P path
// per large row q: its row r, the offset of its positives in the batch scratch (histograms at off + q, P + 1 long)
struct RrLarge {
  int64_t row;
  int64_t off;
  int P;
  int pad;
};

template <class T, class PtrT>
__global__ void __launch_bounds__(RR_THREADS) rr_gather_kernel(const PtrT* __restrict__ yptr, int64_t shift,
                                                               const int* __restrict__ yidx, int base,
                                                               const T* __restrict__ yhat, int64_t ld,
                                                               const RrLarge* __restrict__ rows, T* __restrict__ keys,
                                                               int* __restrict__ cols, int* __restrict__ hist,
                                                               int64_t hist_stride, int* __restrict__ stat) {
  const RrLarge q = rows[blockIdx.x];
  const int64_t e0 = (int64_t)yptr[q.row] - shift;
  const T* row = yhat + q.row * ld;
  for (int i = threadIdx.x; i < q.P; i += RR_THREADS) {
    const int c = yidx[e0 + i] - base;
    const T v = row[c];
    keys[q.off + i] = v == T(0) ? T(0) : v;  // -0 -> +0: the radix sort must see one key for one tie group
    cols[q.off + i] = c;
  }
  const int64_t h0 = q.off + blockIdx.x;
  for (int i = threadIdx.x; i <= q.P; i += RR_THREADS) {
    hist[h0 + i] = 0;
    hist[hist_stride + h0 + i] = 0;
    hist[2 * hist_stride + h0 + i] = 0;
  }
  if (threadIdx.x < 2) stat[2 * blockIdx.x + threadIdx.x] = 0;
}

// grid (column splits, large rows)
template <class T>
__global__ void __launch_bounds__(RR_THREADS) rr_large_count_kernel(const T* __restrict__ yhat, int64_t ncols,
                                                                    int64_t ld, const RrLarge* __restrict__ rows,
                                                                    const T* __restrict__ keys,
                                                                    const int* __restrict__ cols,
                                                                    int* __restrict__ hist, int64_t hist_stride,
                                                                    int* __restrict__ stat, int64_t split) {
  const RrLarge q = rows[blockIdx.y];
  const T* ps = keys + q.off;
  const int* pc = cols + q.off;
  const int64_t h0 = q.off + blockIdx.y;
  int* gap = hist + h0;
  int* tieG = hist + hist_stride + h0;
  int* tieK = hist + 2 * hist_stride + h0;
  const T* row = yhat + q.row * ld;
  const T s0 = row[0];
  const int64_t cb = (int64_t)blockIdx.x * split;
  const int64_t ce = cb + split < ncols ? cb + split : ncols;
  const int tid = threadIdx.x;
  int nz = 0, dif = 0;
  for (int64_t c0 = cb; c0 < ce; c0 += (int64_t)RR_THREADS * RR_UNROLL) {
    T v[RR_UNROLL];
#pragma unroll
    for (int u = 0; u < RR_UNROLL; ++u) {
      const int64_t c = c0 + (int64_t)u * RR_THREADS + tid;
      v[u] = c < ce ? row[c] : T(0);
    }
#pragma unroll
    for (int u = 0; u < RR_UNROLL; ++u) {
      const int64_t c = c0 + (int64_t)u * RR_THREADS + tid;
      const bool on = c < ce;
      if (on) {
        nz += v[u] != T(0) ? 1 : 0;
        dif |= v[u] != s0 ? 1 : 0;
      }
      rr_count<T>(ps, pc, q.P, v[u], (int)c, on, gap, tieG, tieK);
    }
  }
  __shared__ long long sl[RR_WAVES];
  nz = (int)rr_block_sum<long long>((long long)nz, sl);
  dif = (int)rr_block_sum<long long>((long long)dif, sl);
  if (threadIdx.x == 0) {
    if (nz) atomicAdd(&stat[2 * blockIdx.y], nz);
    if (dif) atomicOr(&stat[2 * blockIdx.y + 1], 1);
  }
}

template <class T>
__global__ void __launch_bounds__(RR_THREADS) rr_large_finish_kernel(int64_t ncols, const RrLarge* __restrict__ rows,
                                                                     const T* __restrict__ keys,
                                                                     int* __restrict__ hist, int64_t hist_stride,
                                                                     const int* __restrict__ stat, double alpha, int L,
                                                                     double* __restrict__ out) {
  __shared__ RedScratch red;
  const RrLarge q = rows[blockIdx.x];
  const int64_t h0 = q.off + blockIdx.x;
  int* gap = hist + h0;
  int* tieG = hist + hist_stride + h0;
  int* tieK = hist + 2 * hist_stride + h0;
  rr_scan2(gap, tieK, tieG, q.P + 1, red.w);
  rr_finish<T>(keys + q.off, tieK, tieG, gap, q.P, ncols, alpha, L, stat[2 * blockIdx.x], stat[2 * blockIdx.x + 1],
               out + q.row * 6, &red);
}

}  // namespace

template <class PtrT>
int launch_rank_rows_validate(const PtrT* yptr, int64_t shift, const int* yidx, int base, int64_t nrows,
                              int64_t ncols) {
  hipStream_t st = ctx().stream;
  DevBuf<int> status;
  SS_TRY(status.alloc(1));
  SS_HIP(hipMemsetAsync(status.p, 0, sizeof(int), st));
  const int grid = (int)(nrows < 65536 ? nrows : 65536);
  hipLaunchKernelGGL((rr_validate_kernel<PtrT>), dim3(grid), dim3(RR_THREADS), 0, st, yptr, shift, yidx, base, nrows,
                     ncols, status.p);
  SS_LAUNCH_CHECK();
  int h = 0;
  SS_HIP(hipMemcpyAsync(&h, status.p, sizeof(int), hipMemcpyDeviceToHost, st));
  SS_HIP(hipStreamSynchronize(st));
  if (h & 1) return fail(SS_EINVAL, "rank metrics rows: label index out of range");
  if (h & 2) return fail(SS_EINVAL, "rank metrics rows: label indices not sorted / unique within a row");
  return SS_OK;
}

template <class T, class PtrT>
int launch_rank_rows(const PtrT* yptr, int64_t shift, const int* yidx, int base, const PtrT* host_ptr, const T* yhat,
                     int64_t nrows, int64_t ncols, int64_t ld, double alpha, int L, double* out) {
  hipStream_t st = ctx().stream;
  if (nrows == 0) return SS_OK;
  int max_small = 0;
  std::vector<RrLarge> large;
  for (int64_t r = 0; r < nrows; ++r) {
    const int64_t P = (int64_t)host_ptr[r + 1] - (int64_t)host_ptr[r];
    if (P <= RR_LDS_MAXP) {
      if (P > max_small) max_small = (int)P;
    } else {
      large.push_back(RrLarge{r, 0, (int)P, 0});
    }
  }
  if (large.size() < (size_t)nrows) {
    int NP = 64;
    while (NP < max_small) NP <<= 1;
    const int P1 = ((max_small + 1) + 3) & ~3;
    const size_t lds = (size_t)NP * (sizeof(T) + sizeof(int)) + (size_t)3 * P1 * sizeof(int) + sizeof(RedScratch);
    hipLaunchKernelGGL((rr_lds_kernel<T, PtrT>), dim3((unsigned)nrows), dim3(RR_THREADS), lds, st, yptr, shift, yidx,
                       base, yhat, ncols, ld, max_small, NP, P1, alpha, L, out);
    SS_LAUNCH_CHECK();
    path_add("rank_rows_lds");
  }
  if (large.empty()) return SS_OK;
  path_add("rank_rows_large");
  const int64_t split = RR_SPLIT_COLS;
  const int64_t nsplit = ceil_div(ncols, split);
  for (size_t b0 = 0; b0 < large.size();) {
    // one batch: consecutive large rows up to RR_BATCH_POS positives (at least one row)
    size_t b1 = b0;
    int64_t tot = 0;
    std::vector<int> seg;
    while (b1 < large.size() && (b1 == b0 || tot + large[b1].P <= RR_BATCH_POS)) {
      large[b1].off = tot;
      seg.push_back((int)tot);
      tot += large[b1].P;
      ++b1;
    }
    seg.push_back((int)tot);
    const int nb = (int)(b1 - b0);
    DevBuf<RrLarge> drows;
    DevBuf<int> dseg, cols_in, cols, hist, stat;
    DevBuf<T> keys_in, keys;
    SS_TRY(drows.alloc(nb));
    SS_TRY(dseg.alloc(nb + 1));
    SS_TRY(keys_in.alloc(tot));
    SS_TRY(keys.alloc(tot));
    SS_TRY(cols_in.alloc(tot));
    SS_TRY(cols.alloc(tot));
    const int64_t hs = tot + nb;
    SS_TRY(hist.alloc(3 * hs));
    SS_TRY(stat.alloc(2 * nb));
    SS_HIP(hipMemcpyAsync(drows.p, large.data() + b0, nb * sizeof(RrLarge), hipMemcpyHostToDevice, st));
    SS_HIP(hipMemcpyAsync(dseg.p, seg.data(), (nb + 1) * sizeof(int), hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL((rr_gather_kernel<T, PtrT>), dim3(nb), dim3(RR_THREADS), 0, st, yptr, shift, yidx, base, yhat,
                       ld, drows.p, keys_in.p, cols_in.p, hist.p, hs, stat.p);
    SS_LAUNCH_CHECK();
    {
      size_t bytes = 0;
      SS_HIP(rocprim::segmented_radix_sort_pairs_desc(nullptr, bytes, keys_in.p, keys.p, cols_in.p, cols.p,
                                                      (unsigned)tot, (unsigned)nb, dseg.p, dseg.p + 1, 0,
                                                      (unsigned)(8 * sizeof(T)), st));
      DevBuf<unsigned char> tmp;
      SS_TRY(tmp.alloc(bytes));
      SS_HIP(rocprim::segmented_radix_sort_pairs_desc(tmp.p, bytes, keys_in.p, keys.p, cols_in.p, cols.p,
                                                      (unsigned)tot, (unsigned)nb, dseg.p, dseg.p + 1, 0,
                                                      (unsigned)(8 * sizeof(T)), st));
      hipLaunchKernelGGL((rr_large_count_kernel<T>), dim3((unsigned)nsplit, (unsigned)nb), dim3(RR_THREADS), 0, st,
                         yhat, ncols, ld, drows.p, keys.p, cols.p, hist.p, hs, stat.p, split);
      SS_LAUNCH_CHECK();
      hipLaunchKernelGGL((rr_large_finish_kernel<T>), dim3(nb), dim3(RR_THREADS), 0, st, ncols, drows.p, keys.p, hist.p,
                         hs, stat.p, alpha, L, out);
      SS_LAUNCH_CHECK();
      // the batch buffers are released on return: let the kernels finish first
      SS_HIP(hipStreamSynchronize(st));
    }
    b0 = b1;
  }
  return SS_OK;
}

template int launch_rank_rows_validate<int64_t>(const int64_t*, int64_t, const int*, int, int64_t, int64_t);
template int launch_rank_rows_validate<int>(const int*, int64_t, const int*, int, int64_t, int64_t);
template int launch_rank_rows<float, int64_t>(const int64_t*, int64_t, const int*, int, const int64_t*, const float*,
                                              int64_t, int64_t, int64_t, double, int, double*);
template int launch_rank_rows<double, int64_t>(const int64_t*, int64_t, const int*, int, const int64_t*, const double*,
                                               int64_t, int64_t, int64_t, double, int, double*);
template int launch_rank_rows<float, int>(const int*, int64_t, const int*, int, const int*, const float*, int64_t,
                                          int64_t, int64_t, double, int, double*);
template int launch_rank_rows<double, int>(const int*, int64_t, const int*, int, const int*, const double*, int64_t,
                                           int64_t, int64_t, double, int, double*);

}  // namespace ss
