// featurize (src/core.jl:106-112) on a matrix that is already CSR on the device: entry (i, j) with stored value v stays
// iff v >= alpha, as w = weighted ? v : 1 (alpha > 0, so a kept w is never zero).  This is what lets a cutoff sweep
// re-threshold a resident graph instead of re-running the all-pairs producer: the edges at alpha' >= alpha are a subset
// of those at alpha, and a weighted graph stores the similarity itself.
//
// Two streaming passes over the value stream, both HBM-bound:
//   count  reads val, per-row kept counts by ballot + popcount
//   fill   re-reads val and idx; a kept lane's position is ptr[row] + (kept so far in the row) + its rank in the ballot
//          mask, so the order inside a row is preserved, no atomic touches an output position and the result is
//          bit-reproducible.  It also reports whether every kept value is 1 (DevCsr::binary).
// A row is served by a group of G lanes, G a power of two between 4 and 64 chosen from nnz / rows, 64 / G rows per wave:
// rows far shorter than a wave share one, and neighbouring groups read neighbouring rows, so a wave's load still covers
// one contiguous stretch of val.  A block whose longest row is more than 32 G falls back to G = 64 (its hot rows would
// otherwise be streamed G entries per step); a single row is still walked by one wave, 64 entries per step.
// Row pointers come from PairCsr::scan (64-bit scan of the row totals).
#include <hip/hip_runtime.h>

#include "graph.hpp"

namespace ss {

namespace {

// FILL = false: counts[r] = kept entries of row r.  FILL = true: the kept entries of row r go to optr[r] ... in order.
// Every loop condition is uniform across the wave (the ballots see all 64 lanes); a group whose row is finished, or
// that has no row, only contributes zero bits.
template <class T, bool FILL>
__global__ void __launch_bounds__(256) cut_rows_kernel(const int* __restrict__ ptr, const int* __restrict__ idx,
                                                       const T* __restrict__ val, int64_t rows, T alpha, int weighted,
                                                       int gshift, int* __restrict__ counts,
                                                       const int64_t* __restrict__ optr, int* __restrict__ oidx,
                                                       T* __restrict__ oval, int* __restrict__ not_binary) {
  const int lane = threadIdx.x & 63;
  const int G = 1 << gshift;
  const int gl = lane & (G - 1);   // lane within the group
  const int gbase = lane - gl;     // first lane of the group
  const unsigned long long gmask = G == 64 ? ~0ull : ((1ull << G) - 1ull);
  const unsigned long long below = (1ull << gl) - 1ull;
  const int64_t gpw = 64 >> gshift;  // rows per wave
  const int64_t wave = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
  const int64_t nwaves = ((int64_t)gridDim.x * blockDim.x) >> 6;
  bool nb_flag = false;
  for (int64_t r0 = wave * gpw; r0 < rows; r0 += nwaves * gpw) {
    const int64_t r = r0 + (gbase >> gshift);
    const bool valid = r < rows;
    const int64_t b = valid ? ptr[r] : 0, e = valid ? ptr[r + 1] : 0;
    int64_t o = 0;
    if (FILL && valid) o = optr[r];
    int n = 0;
    for (int64_t x0 = b; __any(x0 < e); x0 += G) {
      const int64_t x = x0 + gl;
      const bool in = x < e;
      const T v = in ? val[x] : T(0);
      const bool keep = in && v >= alpha;
      const unsigned long long gm = (__ballot(keep) >> gbase) & gmask;
      if (FILL) {
        if (keep) {
          const int64_t p = o + __popcll(gm & below);
          const T w = weighted ? v : T(1);
          oidx[p] = idx[x];
          if (oval) oval[p] = w;
          nb_flag |= (w != T(1));
        }
        o += __popcll(gm);
      } else {
        n += __popcll(gm);
      }
    }
    if (!FILL && valid && gl == 0) counts[r] = n;
  }
  if (FILL && nb_flag) *not_binary = 1;
}

__global__ void max_row_len_kernel(const int* __restrict__ ptr, int64_t rows, int* __restrict__ out) {
  int m = 0;
  for (int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; r < rows; r += (int64_t)gridDim.x * blockDim.x) {
    const int len = ptr[r + 1] - ptr[r];
    m = len > m ? len : m;
  }
  for (int o = 32; o > 0; o >>= 1) {
    const int other = __shfl_xor(m, o);
    m = other > m ? other : m;
  }
  if ((threadIdx.x & 63) == 0 && m > 0) atomicMax(out, m);
}

// G from the mean row length; a skewed block (a few hot rows among many short ones) would stream its hot rows G
// entries per step, so a longest row far above the group width takes the whole wave per row instead
inline int group_shift(int64_t nnz, int64_t rows, int64_t longest) {
  const int64_t mean = rows > 0 ? nnz / rows : 0;
  int s = 2;
  while (s < 6 && (1LL << s) < mean) ++s;
  if (longest > (32LL << s)) s = 6;
  return s;
}

inline unsigned cut_grid(int64_t rows, int gshift) {
  const int64_t waves = ceil_div(rows, 64 >> gshift);
  int64_t g = ceil_div(waves, 4);
  if (g < 1) g = 1;
  if (g > 256 * 16) g = 256 * 16;
  return (unsigned)g;
}

}  // namespace

template <class T>
int CutCsr<T>::count(const DevCsr<T>& in_, T alpha_, bool weighted_) {
  hipStream_t st = ctx().stream;
  what = "cutoff_csr";
  in = &in_;
  alpha = alpha_;
  weighted = weighted_;
  sym = false;
  SS_TRY(this->begin(in_.rows, in_.cols, in_.cols > 0 ? in_.cols : 1));  // one slot per row
  if (na == 0 || nb == 0) return SS_OK;
  SS_TRY(counts.alloc((size_t)na));
  int longest = 0;
  if (in_.nnz > 32 * 4 && in_.nnz / na <= 32) {  // only a sub-wave choice can be wrong, and only with a row past 32 * G
    SS_HIP(hipMemsetAsync(counts.p, 0, sizeof(int), st));
    int64_t g = ceil_div(na, 256);
    hipLaunchKernelGGL(max_row_len_kernel, dim3((unsigned)(g > 1024 ? 1024 : g)), dim3(256), 0, st, in_.ptr.p, na,
                       counts.p);
    SS_LAUNCH_CHECK();
    SS_HIP(hipMemcpyAsync(&longest, counts.p, sizeof(int), hipMemcpyDeviceToHost, st));
    SS_HIP(hipStreamSynchronize(st));
  }
  gshift = group_shift(in_.nnz, na, longest);
  return this->count_pass();
}

template <class T>
int CutCsr<T>::launch(bool fill, int* idx, T* val, int* flag) {
  auto* kernel = fill ? cut_rows_kernel<T, true> : cut_rows_kernel<T, false>;
  hipLaunchKernelGGL(kernel, dim3(cut_grid(na, gshift)), dim3(256), 0, ctx().stream, in->ptr.p, in->idx.p, in->val.p, na,
                     alpha, weighted ? 1 : 0, gshift, counts.p, ptr.p, idx, val, flag);
  SS_LAUNCH_CHECK();
  return SS_OK;
}

template <class T>
static int csr_cut(const DevCsr<T>& in, T alpha, bool weighted, DevCsr<T>& out) {
  CutCsr<T> cc;
  SS_TRY(cc.count(in, alpha, weighted));
  return cc.to_dev_csr(out);
}

template <class T>
static int csr_copy(const DevCsr<T>& in, DevCsr<T>& out) {
  hipStream_t st = ctx().stream;
  out.rows = in.rows;
  out.cols = in.cols;
  out.nnz = in.nnz;
  out.binary = in.binary;
  SS_TRY(out.ptr.alloc(in.rows + 1));
  SS_TRY(out.idx.alloc(in.nnz));
  SS_TRY(out.val.alloc(in.nnz));
  SS_HIP(hipMemcpyAsync(out.ptr.p, in.ptr.p, (size_t)(in.rows + 1) * sizeof(int), hipMemcpyDeviceToDevice, st));
  if (in.nnz > 0) {
    SS_HIP(hipMemcpyAsync(out.idx.p, in.idx.p, (size_t)in.nnz * sizeof(int), hipMemcpyDeviceToDevice, st));
    SS_HIP(hipMemcpyAsync(out.val.p, in.val.p, (size_t)in.nnz * sizeof(T), hipMemcpyDeviceToDevice, st));
  }
  return SS_OK;
}

// XsT is cut from the parent's XsT rather than transposed from the cut Xs: both hold the same (i, j, v) triples, the
// predicate looks at v alone, and csr_transpose is stable (row j of XsT lists its sources in ascending order before
// and after the cut), so the two routes give the same arrays.  The labels do not depend on the cutoff and are copied;
// the degrees are recounted from the new row pointers by the kernel every sparse graph uses.
template <class T>
int graph_recut(const Graph<T>& p, T alpha, bool weighted, Graph<T>& g) {
  g.nq = p.nq; g.ns = p.ns; g.nf = p.nf; g.nt = p.nt;
  SS_TRY(csr_cut(p.Xq, alpha, weighted, g.Xq));
  SS_TRY(csr_cut(p.Xs, alpha, weighted, g.Xs));
  SS_TRY(csr_cut(p.XsT, alpha, weighted, g.XsT));
  SS_TRY(csr_copy(p.Ys, g.Ys));
  SS_TRY(csr_copy(p.YsT, g.YsT));
  return graph_degrees(g);  // synchronises
}

template struct CutCsr<float>;
template struct CutCsr<double>;
template int graph_recut<float>(const Graph<float>&, float, bool, Graph<float>&);
template int graph_recut<double>(const Graph<double>&, double, bool, Graph<double>&);

}  // namespace ss
