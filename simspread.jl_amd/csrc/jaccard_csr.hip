// Thresholded weighted Jaccard (Ruzicka) similarity of real-valued feature rows, produced straight as CSR: the
// featurize cutoff (src/core.jl:106-112) applied to `1 .- pairwise(Jaccard(), X, dims=1)`
// (docs/src/tutorial/fishers-flowers.jl:66,95-96), without the dense n x n similarity ever existing.
//
//   smin = smax = +0; for k = 0 .. d-1 in order, in T: smin += min(a_k, b_k), smax += max(a_k, b_k)
//   s = smax == 0 ? 1 : smin / smax                                          (one correctly rounded division in T)
//   keep (i, j) iff s >= alpha and v != 0 with v = weighted ? s : 1          (keep_entry of assemble.hip)
//
// This is jaccard_kernel (kernels.hip) pair for pair: the two sums run sequentially over k in T, nothing is
// reassociated or split, and the quotient is the plain division (the Makefile builds without fast-math), so the CSR is
// bitwise equal to the dense route followed by the cutoff.  v_min / v_max stand in for the compare-and-select of the
// dense kernel: for non-NaN inputs they differ only in the sign of a zero, and adding -0 instead of +0 to a sum that
// started at +0 changes nothing.  NaN features are refused before anything is written.
//
// Two passes over 128 x 128 tiles of (row, column) pairs, the skeleton of fingerprint.hip (pair_csr.hip):
//   count  per (column tile, row): the number of kept entries -> counts[jt * rows + i]; per tile: any kept -> tile_nz
//   fill   the tiles that kept something, again, each slot written at ptr[i] + its offset in column order.
// Register blocks: fp32 8 x 8 pairs per thread (256 threads, 128 accumulator VGPRs), fp64 4 x 8 (512 threads, the
// same 128 VGPRs).  In symmetric mode (Fb = Fa) only the tiles on and above the diagonal run; an off-diagonal tile
// emits its pairs for its rows and, mirrored, for its columns.  No atomics decide any position.
#include <algorithm>
#include <hip/hip_runtime.h>

#include "graph.hpp"

namespace ss {

#define SS_LAUNCH_CHECK()                                                                              \
  do {                                                                                                 \
    hipError_t _e = hipGetLastError();                                                                 \
    if (_e != hipSuccess)                                                                              \
      return fail(SS_EHIP, "%s:%d kernel launch: %s", __FILE__, __LINE__, hipGetErrorString(_e));      \
  } while (0)

namespace {

constexpr int TILE = 128;  // rows and columns per workgroup tile
constexpr int BK = 16;     // feature columns staged per step
constexpr int RC = 8;      // columns per thread
constexpr int NTX = TILE / RC;  // 16 thread columns

template <class T>
struct Block;
template <>
struct Block<float> {
  static constexpr int RA = 8;  // rows per thread
};
template <>
struct Block<double> {
  static constexpr int RA = 4;
};

__device__ __forceinline__ float vmin(float a, float b) { return __builtin_fminf(a, b); }
__device__ __forceinline__ float vmax(float a, float b) { return __builtin_fmaxf(a, b); }
__device__ __forceinline__ double vmin(double a, double b) { return __builtin_fmin(a, b); }
__device__ __forceinline__ double vmax(double a, double b) { return __builtin_fmax(a, b); }

template <class T>
__device__ __forceinline__ bool jaccard_keep(T smin, T smax, T alpha, bool weighted, T& v) {
  const T s = smax == T(0) ? T(1) : smin / smax;
  v = weighted ? s : T(1);
  return s >= alpha && v != T(0);
}

// tile (it, jt) of the upper triangle (it <= jt) from its linear index t (the enumeration of fingerprint.hip)
__device__ __forceinline__ void triangle_tile(int64_t t, int64_t nt, int64_t& it, int64_t& jt) {
  const double b = 2.0 * (double)nt + 1.0;
  int64_t r = (int64_t)((b - sqrt(b * b - 8.0 * (double)t)) * 0.5);
  if (r < 0) r = 0;
  if (r > nt - 1) r = nt - 1;
  while (r > 0 && r * nt - r * (r - 1) / 2 > t) --r;
  while (r + 1 < nt && (r + 1) * nt - (r + 1) * r / 2 <= t) ++r;
  it = r;
  jt = r + (t - (r * nt - r * (r - 1) / 2));
}

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

// FILL == false: write the per-(tile, row) counts and the tile flag.  FILL == true: write the entries of the tiles that
// kept something (counts then hold in-row offsets).
template <class T, bool SYM, bool FILL>
__global__ void __launch_bounds__(NTX * (TILE / Block<T>::RA)) jaccard_tile_kernel(
    const T* __restrict__ Fa, int64_t na, int64_t lda, const T* __restrict__ Fb, int64_t nb, int64_t ldb, int64_t d,
    T alpha, int weighted, int64_t ntiles, int* __restrict__ counts, int* __restrict__ tile_nz,
    const int64_t* __restrict__ ptr, int* __restrict__ oidx, T* __restrict__ oval, int* __restrict__ not_binary) {
  constexpr int RA = Block<T>::RA;
  constexpr int NTY = TILE / RA;       // thread rows
  constexpr int NT = NTX * NTY;        // threads
  __shared__ __attribute__((aligned(16))) T As[BK][TILE];
  __shared__ __attribute__((aligned(16))) T Bs[BK][TILE];
  __shared__ int rc[TILE][NTX + 1];  // [row][tx]: kept entries of the row in the columns of thread column tx -> offsets
  __shared__ int cc[TILE][NTY + 1];  // [column][ty]: the same for the mirror (SYM, off-diagonal tiles)

  const int64_t tlin = SYM ? (int64_t)blockIdx.x : (int64_t)blockIdx.y * gridDim.x + blockIdx.x;
  if (FILL && tile_nz[tlin] == 0) return;  // uniform over the block
  int64_t it, jt;
  if (SYM) {
    triangle_tile(blockIdx.x, ntiles, it, jt);
  } else {
    it = blockIdx.y;
    jt = blockIdx.x;
  }
  const int64_t i0 = it * TILE, j0 = jt * TILE;
  const int tid = threadIdx.x, tx = tid % NTX, ty = tid / NTX;
  const bool mirror = SYM && it != jt;

  // acc[a][b] = (smin, smax) of one pair: the two sums sit in adjacent registers, so that fp32 adds them with one
  // v_pk_add_f32 (lane-wise, each lane one correctly rounded add -- the same two adds)
  typedef T T2 __attribute__((ext_vector_type(2)));
  T2 acc[RA][RC];
#pragma unroll
  for (int a = 0; a < RA; ++a)
#pragma unroll
    for (int b = 0; b < RC; ++b) acc[a][b] = T2{T(0), T(0)};

  // staging: BK feature columns of the tile's 128 rows of each side; consecutive threads read consecutive rows of one
  // column (coalesced).  Past d or past the last row the value is 0: a padded k adds +0 to both sums, which changes
  // nothing, and padded rows / columns are masked below.
  constexpr int PER = BK * TILE / NT;
  T ra[PER], rb[PER];
  auto load = [&](int64_t k0) {
#pragma unroll
    for (int q = 0; q < PER; ++q) {
      const int e = tid + q * NT;
      const int kk = e / TILE, r = e % TILE;
      const int64_t k = k0 + kk;
      ra[q] = (k < d && i0 + r < na) ? Fa[i0 + r + k * lda] : T(0);
      rb[q] = (k < d && j0 + r < nb) ? Fb[j0 + r + k * ldb] : T(0);
    }
  };
  if (d > 0) load(0);
  for (int64_t k0 = 0; k0 < d; k0 += BK) {
#pragma unroll
    for (int q = 0; q < PER; ++q) {
      const int e = tid + q * NT;
      As[e / TILE][e % TILE] = ra[q];
      Bs[e / TILE][e % TILE] = rb[q];
    }
    __syncthreads();
    if (k0 + BK < d) load(k0 + BK);  // the next step's loads are in flight during this step's arithmetic
#pragma unroll
    for (int kk = 0; kk < BK; ++kk) {
      T av[RA], bv[RC];
#pragma unroll
      for (int a = 0; a < RA; ++a) av[a] = As[kk][RA * ty + a];
#pragma unroll
      for (int b = 0; b < RC; ++b) bv[b] = Bs[kk][RC * tx + b];
#pragma unroll
      for (int a = 0; a < RA; ++a)
#pragma unroll
        for (int b = 0; b < RC; ++b) acc[a][b] += T2{vmin(av[a], bv[b]), vmax(av[a], bv[b])};
    }
    __syncthreads();
  }

  // which pairs are kept: bit b of rmask[a] = bit a of cmask[b] = pair (row RA*ty + a, column RC*tx + b)
  uint32_t rmask[RA], cmask[RC];
#pragma unroll
  for (int b = 0; b < RC; ++b) cmask[b] = 0;
  const bool wgt = weighted != 0;
#pragma unroll
  for (int a = 0; a < RA; ++a) {
    rmask[a] = 0;
    const bool va = i0 + RA * ty + a < na;
#pragma unroll
    for (int b = 0; b < RC; ++b) {
      T v;
      const bool k = va && j0 + RC * tx + b < nb && jaccard_keep<T>(acc[a][b].x, acc[a][b].y, alpha, wgt, v);
      rmask[a] |= (k ? 1u : 0u) << b;
      cmask[b] |= (k ? 1u : 0u) << a;
    }
  }
  bool any = false;
#pragma unroll
  for (int a = 0; a < RA; ++a) {
    rc[RA * ty + a][tx] = __popc(rmask[a]);
    any |= rmask[a] != 0;
  }
  if (mirror) {
#pragma unroll
    for (int b = 0; b < RC; ++b) cc[RC * tx + b][ty] = __popc(cmask[b]);
  }
  any = __syncthreads_or(any);
  if (!FILL && tid == 0) tile_nz[tlin] = any ? 1 : 0;
  // exclusive scans: threads 0..127 over the NTX thread columns of row tid, threads 128..255 over the NTY thread rows
  // of column tid - 128
  if (tid < TILE) {
    int run = 0;
#pragma unroll
    for (int q = 0; q < NTX; ++q) {
      const int c = rc[tid][q];
      rc[tid][q] = run;
      run += c;
    }
    if (!FILL && i0 + tid < na) counts[jt * na + i0 + tid] = run;
  } else if (tid < 2 * TILE && mirror) {
    const int r = tid - TILE;
    int run = 0;
#pragma unroll
    for (int q = 0; q < NTY; ++q) {
      const int c = cc[r][q];
      cc[r][q] = run;
      run += c;
    }
    if (!FILL && j0 + r < nb) counts[it * na + j0 + r] = run;  // SYM: na == nb
  }
  if (!FILL) return;
  __syncthreads();

  bool nb_flag = false;
#pragma unroll
  for (int a = 0; a < RA; ++a) {
    if (!rmask[a]) continue;
    const int64_t i = i0 + RA * ty + a;
    int64_t o = ptr[i] + counts[jt * na + i] + rc[RA * ty + a][tx];
#pragma unroll
    for (int b = 0; b < RC; ++b) {
      if (!((rmask[a] >> b) & 1u)) continue;
      T v;
      (void)jaccard_keep<T>(acc[a][b].x, acc[a][b].y, alpha, wgt, v);
      oidx[o] = (int)(j0 + RC * tx + b);
      if (oval) oval[o] = v;
      nb_flag |= (v != T(1));
      ++o;
    }
  }
  if (mirror) {
#pragma unroll
    for (int b = 0; b < RC; ++b) {
      if (!cmask[b]) continue;
      const int64_t j = j0 + RC * tx + b;
      int64_t o = ptr[j] + counts[it * na + j] + cc[RC * tx + b][ty];
#pragma unroll
      for (int a = 0; a < RA; ++a) {
        if (!((cmask[b] >> a) & 1u)) continue;
        T v;
        (void)jaccard_keep<T>(acc[a][b].x, acc[a][b].y, alpha, wgt, v);
        oidx[o] = (int)(i0 + RA * ty + a);
        if (oval) oval[o] = v;
        ++o;
      }
    }
  }
  if (nb_flag) *not_binary = 1;
}

template <class T>
constexpr int threads() {
  return NTX * (TILE / Block<T>::RA);
}

}  // namespace

template <class T>
int launch_feature_nan_scan(const T* F, int64_t n, int64_t ld, int64_t d, int* flag) {
  if (n == 0 || d == 0) return SS_OK;
  const int64_t blocks = std::min<int64_t>(ceil_div(n * d, 256), 4096);
  hipLaunchKernelGGL(nan_scan_kernel<T>, dim3((unsigned)blocks), dim3(256), 0, ctx().stream, F, n, ld, d, flag);
  SS_LAUNCH_CHECK();
  return SS_OK;
}
template int launch_feature_nan_scan<float>(const float*, int64_t, int64_t, int64_t, int*);
template int launch_feature_nan_scan<double>(const double*, int64_t, int64_t, int64_t, int*);

template <class T>
int JaccardCsr<T>::count(const T* Fa_, int64_t na_, int64_t lda_, const T* Fb_, int64_t nb_, int64_t ldb_, int64_t d_,
                         T alpha_, bool weighted_) {
  hipStream_t st = ctx().stream;
  what = "jaccard";
  sym = (Fb_ == nullptr);
  Fa = Fa_;
  Fb = sym ? Fa_ : Fb_;
  lda = lda_;
  ldb = sym ? lda_ : ldb_;
  d = d_;
  alpha = alpha_;
  weighted = weighted_;
  if (alpha != alpha) return fail(SS_EINVAL, "jaccard: alpha is NaN");
  // NaN features: refused before anything (the row pointers included) is written
  {
    DevBuf<int> flag;
    SS_TRY(flag.alloc(1));
    SS_HIP(hipMemsetAsync(flag.p, 0, sizeof(int), st));
    SS_TRY(launch_feature_nan_scan<T>(Fa, na_, lda, d, flag.p));
    if (!sym) SS_TRY(launch_feature_nan_scan<T>(Fb, nb_, ldb, d, flag.p));
    int bad = 0;
    SS_HIP(hipMemcpyAsync(&bad, flag.p, sizeof(int), hipMemcpyDeviceToHost, st));
    SS_HIP(hipStreamSynchronize(st));
    if (bad) return fail(SS_EINVAL, "jaccard: the features hold a NaN");
  }
  SS_TRY(this->begin(na_, sym ? na_ : nb_, TILE));
  if (na == 0 || nb == 0) return SS_OK;
  const int64_t nti = ceil_div(na, TILE);
  const int64_t nblocks = sym ? nti * (nti + 1) / 2 : nti * ntj;
  if (sym ? nblocks >= (1LL << 31) : (ntj >= (1LL << 31) || nti > 65535))
    return fail(SS_EUNSUPPORTED, "jaccard: %lld x %lld pairs need more tiles than one launch holds", (long long)na,
                (long long)nb);
  SS_TRY(counts.alloc((size_t)ntj * (size_t)na));
  SS_TRY(tile_nz.alloc((size_t)nblocks));
  if (sym) {
    hipLaunchKernelGGL((jaccard_tile_kernel<T, true, false>), dim3((unsigned)nblocks), dim3(threads<T>()), 0, st, Fa,
                       na, lda, Fb, nb, ldb, d, alpha, weighted ? 1 : 0, nti, counts.p, tile_nz.p,
                       (const int64_t*)nullptr, (int*)nullptr, (T*)nullptr, (int*)nullptr);
  } else {
    hipLaunchKernelGGL((jaccard_tile_kernel<T, false, false>), dim3((unsigned)ntj, (unsigned)nti), dim3(threads<T>()), 0,
                       st, Fa, na, lda, Fb, nb, ldb, d, alpha, weighted ? 1 : 0, ntj, counts.p, tile_nz.p,
                       (const int64_t*)nullptr, (int*)nullptr, (T*)nullptr, (int*)nullptr);
  }
  SS_LAUNCH_CHECK();
  return this->scan();
}

template <class T>
int JaccardCsr<T>::fill(int* idx, T* val, bool* binary) {
  hipStream_t st = ctx().stream;
  if (binary) *binary = true;
  if (nnz == 0) return SS_OK;
  DevBuf<int> flag;
  SS_TRY(flag.alloc(1));
  SS_HIP(hipMemsetAsync(flag.p, 0, sizeof(int), st));
  const int64_t nti = ceil_div(na, TILE);
  if (sym) {
    hipLaunchKernelGGL((jaccard_tile_kernel<T, true, true>), dim3((unsigned)(nti * (nti + 1) / 2)), dim3(threads<T>()),
                       0, st, Fa, na, lda, Fb, nb, ldb, d, alpha, weighted ? 1 : 0, nti, counts.p, tile_nz.p, ptr.p, idx,
                       val, flag.p);
  } else {
    hipLaunchKernelGGL((jaccard_tile_kernel<T, false, true>), dim3((unsigned)ntj, (unsigned)nti), dim3(threads<T>()), 0,
                       st, Fa, na, lda, Fb, nb, ldb, d, alpha, weighted ? 1 : 0, ntj, counts.p, tile_nz.p, ptr.p, idx,
                       val, flag.p);
  }
  SS_LAUNCH_CHECK();
  int notbin = 0;
  SS_HIP(hipMemcpyAsync(&notbin, flag.p, sizeof(int), hipMemcpyDeviceToHost, st));
  SS_HIP(hipStreamSynchronize(st));
  if (binary) *binary = (notbin == 0);
  return SS_OK;
}

template struct JaccardCsr<float>;
template struct JaccardCsr<double>;

}  // namespace ss
