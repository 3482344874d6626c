// Host skeleton of the fused thresholded-similarity producers (fingerprint.hip, jaccard_csr.hip, dot_csr.hip; their
// tiles and emit epilogue are pair_tile.hpp) and of the streaming cutoff (recut.hip).  A producer's count pass leaves
// the kept entries of every (column tile, row) slot in counts[jt * rows + i]; scan() turns them into exclusive in-row
// offsets and takes a 64-bit scan of the row totals into ptr, so that nnz >= 2^31 is seen (and refused by the caller)
// before any output exists; fill() runs the producer's fill pass.  Positions come from scans, never from atomics.
// What every tiled producer does around its kernel lives here too: the refusal of NaN features and of more tiles than
// one launch holds, the counts / tile_nz buffers and the launch grid.
#include <algorithm>
#include <cstring>
#include <hip/hip_runtime.h>
#include <rocprim/rocprim.hpp>

#include "graph.hpp"

namespace ss {

namespace {

// per row: the per-tile counts become exclusive in-row offsets; the row total goes to rowcnt
__global__ void pair_row_offsets_kernel(int* __restrict__ counts, int64_t rows, int64_t ntj, int* __restrict__ rowcnt) {
  const int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= rows) return;
  int run = 0;
#pragma unroll 8
  for (int64_t t = 0; t < ntj; ++t) {
    const int c = counts[t * rows + r];
    counts[t * rows + r] = run;
    run += c;
  }
  rowcnt[r] = run;
}

__global__ void ptr_tail_kernel(const int* in, int64_t* out, int64_t n) { out[n] = n ? out[n - 1] + in[n - 1] : 0; }

template <class T>
__global__ void nan_scan_kernel(const T* __restrict__ F, int64_t n, int64_t ld, int64_t d, int* __restrict__ flag) {
  const int64_t total = n * d;
  bool bad = false;
  for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (int64_t)gridDim.x * blockDim.x) {
    const int64_t k = e / n, i = e - k * n;
    const T x = F[i + k * ld];
    bad |= (x != x);
  }
  if (bad) *flag = 1;
}

// flag[0] = 1 when F (n x d, column-major, ld >= n; padding rows are not read) holds a NaN; enqueued only
template <class T>
int launch_feature_nan_scan(const T* F, int64_t n, int64_t ld, int64_t d, int* flag) {
  if (n == 0 || d == 0) return SS_OK;
  const int64_t blocks = std::min<int64_t>(ceil_div(n * d, 256), 4096);
  hipLaunchKernelGGL(nan_scan_kernel<T>, dim3((unsigned)blocks), dim3(256), 0, ctx().stream, F, n, ld, d, flag);
  SS_LAUNCH_CHECK();
  return SS_OK;
}

__global__ void ptr_narrow_kernel(const int64_t* __restrict__ in, int64_t n, int* __restrict__ out) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i <= n) out[i] = (int)in[i];
}

}  // namespace

template <class T>
int PairCsr<T>::begin(int64_t na_, int64_t nb_, int64_t tile) {
  na = na_;
  nb = nb_;
  nnz = 0;
  ntj = ceil_div(nb, tile);
  SS_TRY(ptr.alloc(na + 1));
  if (na == 0 || nb == 0) {
    hipStream_t st = ctx().stream;
    SS_HIP(hipMemsetAsync(ptr.p, 0, (na + 1) * sizeof(int64_t), st));
    SS_HIP(hipStreamSynchronize(st));
  }
  return SS_OK;
}

int pair_tile_blocks(const char* what, int64_t na, int64_t nb, int64_t tile, bool sym, int64_t& nti, int64_t& ntj,
                     int64_t& nblocks) {
  nti = ceil_div(na, tile);
  ntj = ceil_div(nb, tile);
  nblocks = sym ? nti * (nti + 1) / 2 : nti * ntj;
  if (sym ? nblocks >= (1LL << 31) : (ntj >= (1LL << 31) || nti > 65535))
    return fail(SS_EUNSUPPORTED, "%s: %lld x %lld pairs need more tiles than one launch holds", what, (long long)na,
                (long long)nb);
  return SS_OK;
}

dim3 pair_tile_grid(bool sym, int64_t nti, int64_t ntj) {
  return sym ? dim3((unsigned)(nti * (nti + 1) / 2)) : dim3((unsigned)ntj, (unsigned)nti);
}

template <class T>
int PairCsr<T>::begin_tiles(int64_t na_, int64_t nb_, int64_t tile, bool with_tile_nz) {
  SS_TRY(begin(na_, nb_, tile));
  if (na == 0 || nb == 0) return SS_OK;
  int64_t nblocks = 0;
  SS_TRY(pair_tile_blocks(what, na, nb, tile, sym, nti, ntj, nblocks));
  SS_TRY(counts.alloc((size_t)ntj * (size_t)na));
  if (with_tile_nz) SS_TRY(tile_nz.alloc((size_t)nblocks));
  return SS_OK;
}

template <class T>
dim3 PairCsr<T>::tile_grid() const {
  return pair_tile_grid(sym, nti, ntj);
}

template <class T>
int refuse_nan_rows(const char* what, const T* Fa, int64_t na, int64_t lda, const T* Fb, int64_t nb, int64_t ldb,
                    int64_t d) {
  hipStream_t st = ctx().stream;
  DevBuf<int> flag;
  SS_TRY(flag.alloc(1));
  SS_HIP(hipMemsetAsync(flag.p, 0, sizeof(int), st));
  SS_TRY(launch_feature_nan_scan<T>(Fa, na, lda, d, flag.p));
  if (Fb) SS_TRY(launch_feature_nan_scan<T>(Fb, nb, ldb, d, flag.p));
  int bad = 0;
  SS_HIP(hipMemcpyAsync(&bad, flag.p, sizeof(int), hipMemcpyDeviceToHost, st));
  SS_HIP(hipStreamSynchronize(st));
  if (bad) return fail(SS_EINVAL, "%s: the features hold a NaN", what);
  return SS_OK;
}

template <class T>
int PairCsr<T>::refuse_nan_features(const T* Fa, int64_t na_, int64_t lda, const T* Fb, int64_t nb_, int64_t ldb,
                                    int64_t d) {
  return refuse_nan_rows<T>(what, Fa, na_, lda, sym ? nullptr : Fb, nb_, ldb, d);
}

template <class T>
int PairCsr<T>::scan() {
  hipStream_t st = ctx().stream;
  DevBuf<int> rowcnt;
  SS_TRY(rowcnt.alloc(na));
  hipLaunchKernelGGL(pair_row_offsets_kernel, dim3((unsigned)ceil_div(na, 256)), dim3(256), 0, st, counts.p, na, ntj,
                     rowcnt.p);
  SS_LAUNCH_CHECK();
  // row totals are < 2^31 each; their sum is taken in 64 bits so that nnz >= 2^31 is seen rather than wrapped
  size_t bytes = 0;
  SS_HIP(rocprim::exclusive_scan(nullptr, bytes, rowcnt.p, ptr.p, (int64_t)0, (size_t)na, rocprim::plus<int64_t>(), st));
  DevBuf<unsigned char> tmp;
  SS_TRY(tmp.alloc(bytes));
  SS_HIP(rocprim::exclusive_scan(tmp.p, bytes, rowcnt.p, ptr.p, (int64_t)0, (size_t)na, rocprim::plus<int64_t>(), st));
  hipLaunchKernelGGL(ptr_tail_kernel, dim3(1), dim3(1), 0, st, rowcnt.p, ptr.p, na);
  SS_LAUNCH_CHECK();
  SS_HIP(hipMemcpyAsync(&nnz, ptr.p + na, sizeof(int64_t), hipMemcpyDeviceToHost, st));
  SS_HIP(hipStreamSynchronize(st));  // tmp, rowcnt are freed on return
  return SS_OK;
}

template <class T>
int PairCsr<T>::fill(int* idx, T* val, bool* binary) {
  hipStream_t st = ctx().stream;
  if (binary) *binary = true;
  if (nnz == 0) return SS_OK;
  DevBuf<int> flag;
  SS_TRY(flag.alloc(1));
  SS_HIP(hipMemsetAsync(flag.p, 0, sizeof(int), st));
  SS_TRY(launch(true, idx, val, flag.p));
  int notbin = 0;
  SS_HIP(hipMemcpyAsync(&notbin, flag.p, sizeof(int), hipMemcpyDeviceToHost, st));
  SS_HIP(hipStreamSynchronize(st));
  if (binary) *binary = (notbin == 0);
  return SS_OK;
}

template <class T>
int PairCsr<T>::to_dev_csr(DevCsr<T>& out) {
  hipStream_t st = ctx().stream;
  if (nnz >= (1LL << 31)) return fail(SS_EUNSUPPORTED, "%s: nnz = %lld >= 2^31", what, (long long)nnz);
  out.rows = na;
  out.cols = nb;
  out.nnz = nnz;
  SS_TRY(out.ptr.alloc(na + 1));
  SS_TRY(out.idx.alloc(nnz));
  SS_TRY(out.val.alloc(nnz));
  hipLaunchKernelGGL(ptr_narrow_kernel, dim3((unsigned)ceil_div(na + 1, 256)), dim3(256), 0, st, ptr.p, na, out.ptr.p);
  SS_LAUNCH_CHECK();
  bool bin = true;
  SS_TRY(fill(out.idx.p, out.val.p, &bin));
  out.binary = bin;
  return SS_OK;
}

template int refuse_nan_rows<float>(const char*, const float*, int64_t, int64_t, const float*, int64_t, int64_t, int64_t);
template int refuse_nan_rows<double>(const char*, const double*, int64_t, int64_t, const double*, int64_t, int64_t,
                                     int64_t);
template struct PairCsr<float>;
template struct PairCsr<double>;

}  // namespace ss
