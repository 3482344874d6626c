// Data movement of the k-fold row blocks (api.hip kfold_rows_device, ss_predict_kfold_rows_* / ss_evaluate_kfold_*).
// A k-fold block is produced fold by fold, so its rows come out in fold order; these kernels put them where the caller
// wants them and gather what the metric kernels read in that order:
//
//   scatter_rows_kernel   row q of a packed block -> row dst_rows[q] of the destination (member-ordered scores of the
//                         sorted stage-2 path -> source order; 6 / 18-double metric rows -> source order).  One
//                         workgroup per row, 16-byte loads and stores when both sides allow them.  Pure bandwidth.
//   gather_labels_kernel  the Ys rows of a block's members, in fold order, into one contiguous index array whose int64
//                         row pointers the host built (the CSR launch_rank_rows / launch_binary_rows read unchanged).
//
// Nothing here computes: every value is copied, so a row's bits are those its producer wrote.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "graph.hpp"

namespace ss {

namespace {

// blockIdx.y: row of the launch; nvec 16-byte vectors per row when vec, else ncols elements
template <class T>
__global__ void scatter_rows_kernel(const T* __restrict__ src, int64_t lds, int64_t ncols, const int* __restrict__ dst_rows,
                                    T* __restrict__ dst, int64_t ldd, int vec) {
  const int64_t r = blockIdx.y;
  const T* s = src + r * lds;
  T* d = dst + (int64_t)dst_rows[r] * ldd;
  const int64_t step = (int64_t)gridDim.x * blockDim.x;
  const int64_t t0 = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  int64_t done = 0;
  if (vec) {
    constexpr int E = 16 / (int)sizeof(T);
    const int64_t nvec = ncols / E;
    const uint4* sv = reinterpret_cast<const uint4*>(s);
    uint4* dv = reinterpret_cast<uint4*>(d);
    for (int64_t v = t0; v < nvec; v += step) dv[v] = sv[v];
    done = nvec * E;
  }
  for (int64_t c = done + t0; c < ncols; c += step) d[c] = s[c];
}

__global__ void gather_labels_kernel(const int* __restrict__ ys_ptr, const int* __restrict__ ys_idx,
                                     const int* __restrict__ members, const int64_t* __restrict__ pptr, int64_t shift,
                                     int* __restrict__ out) {
  const int64_t q = blockIdx.x;
  const int m = members[q];
  const int e0 = ys_ptr[m], e1 = ys_ptr[m + 1];
  int* o = out + (pptr[q] - shift);
  for (int e = e0 + (int)threadIdx.x; e < e1; e += (int)blockDim.x) o[e - e0] = ys_idx[e];
}

}  // namespace

template <class T>
int launch_scatter_rows(const T* src, int64_t lds, int64_t nrows, int64_t ncols, const int* dst_rows, T* dst,
                        int64_t ldd) {
  if (nrows <= 0 || ncols <= 0) return SS_OK;
  const bool vec = ((reinterpret_cast<uintptr_t>(src) | reinterpret_cast<uintptr_t>(dst)) & 15) == 0 &&
                   ((lds * (int64_t)sizeof(T)) & 15) == 0 && ((ldd * (int64_t)sizeof(T)) & 15) == 0;
  const int64_t items = vec ? ncols * (int64_t)sizeof(T) / 16 + 1 : ncols;
  const int threads = items <= 64 ? 64 : 256;
  int64_t gx = ceil_div(items, threads);
  if (gx > 64) gx = 64;
  for (int64_t r0 = 0; r0 < nrows; r0 += 65535) {
    const int64_t nb = nrows - r0 < 65535 ? nrows - r0 : 65535;
    hipLaunchKernelGGL(scatter_rows_kernel<T>, dim3((unsigned)gx, (unsigned)nb), dim3(threads), 0, ctx().stream,
                       src + r0 * lds, lds, ncols, dst_rows + r0, dst, ldd, vec ? 1 : 0);
    SS_LAUNCH_CHECK();
  }
  return SS_OK;
}

int launch_gather_labels(const int* ys_ptr, const int* ys_idx, const int* members, int64_t nrows, const int64_t* pptr,
                         int64_t shift, int* out) {
  if (nrows <= 0) return SS_OK;
  hipLaunchKernelGGL(gather_labels_kernel, dim3((unsigned)nrows), dim3(64), 0, ctx().stream, ys_ptr, ys_idx, members,
                     pptr, shift, out);
  SS_LAUNCH_CHECK();
  return SS_OK;
}

template int launch_scatter_rows<float>(const float*, int64_t, int64_t, int64_t, const int*, float*, int64_t);
template int launch_scatter_rows<double>(const double*, int64_t, int64_t, int64_t, const int*, double*, int64_t);

}  // namespace ss
