// Thresholded Tanimoto similarity of packed binary fingerprints, produced straight as CSR: the featurize cutoff
// (src/core.jl:106-112) applied to `1 .- pairwise(Jaccard(), F, dims=1)` (docs/src/tutorial/fishers-flowers.jl:66) on
// 0/1 rows, without the dense n x n similarity ever existing.
//
//   c = popcount(a & b), u = popcount(a) + popcount(b) - c, s = u == 0 ? 1 : T(c) / T(u)
//   keep (i, j) iff s >= alpha and v != 0 with v = weighted ? s : 1          (keep_entry of assemble.hip)
//
// The counts are exact integers and the quotient is one correctly rounded division, the same one jaccard_kernel
// (kernels.hip) performs on the float sums of min / max, so the CSR is bitwise equal to the dense route.
//
// Two passes over 128 x 128 tiles of (row, column) pairs, 256 threads, an 8 x 8 block of pairs per thread:
//   count  per (column tile, row): the number of kept entries          -> counts[jt * rows + i]
//   (per row: in-row exclusive offsets of the slots and the row total; a 64-bit scan of the totals gives ptr, and the
//    nnz >= 2^31 refusal happens there, before any output exists)
//   fill   the same tiles again, each slot written at ptr[i] + its offset in column order.
// In symmetric mode (Fb = Fa) only the tiles on and above the diagonal run (1-D grid over the triangle); an
// off-diagonal tile emits its pairs for its rows and, mirrored, for its columns.  No atomics decide any position,
// so the output is bitwise repeatable.
#include <cstdlib>
#include <cstring>
#include <hip/hip_runtime.h>
#include <rocprim/rocprim.hpp>

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
constexpr int BK = 16;     // 32-bit fingerprint words staged per step (8 uint64 words)
constexpr int RB = 8;      // rows / columns per thread

__global__ void popcount_rows_kernel(const uint64_t* __restrict__ F, int64_t n, int64_t nwords, int* __restrict__ pop) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const uint64_t* row = F + i * nwords;
  int c = 0;
  for (int64_t w = 0; w < nwords; ++w) c += __popcll(row[w]);
  pop[i] = c;
}

template <class T>
__device__ __forceinline__ bool tanimoto_keep(int c, int pa, int pb, T alpha, bool weighted, T& v) {
  const int u = pa + pb - c;
  const T s = u == 0 ? T(1) : T(c) / T(u);
  v = weighted ? s : T(1);
  return s >= alpha && v != T(0);
}

// tile (it, jt) of the upper triangle (it <= jt) from its linear index t: rows of the triangle hold nt, nt-1, ... tiles
__device__ __forceinline__ void triangle_tile(int64_t t, int64_t nt, int64_t& it, int64_t& jt) {
  // first tile of row r: r * nt - r * (r - 1) / 2
  const double b = 2.0 * (double)nt + 1.0;
  int64_t r = (int64_t)((b - sqrt(b * b - 8.0 * (double)t)) * 0.5);
  if (r < 0) r = 0;
  if (r > nt - 1) r = nt - 1;
  while (r > 0 && r * nt - r * (r - 1) / 2 > t) --r;
  while (r + 1 < nt && (r + 1) * nt - (r + 1) * r / 2 <= t) ++r;
  it = r;
  jt = r + (t - (r * nt - r * (r - 1) / 2));
}

// FILL == false: write the per-(tile, row) counts.  FILL == true: write the entries (counts then hold in-row offsets).
template <class T, bool SYM, bool FILL>
__global__ void __launch_bounds__(256) tanimoto_tile_kernel(
    const uint64_t* __restrict__ Fa, int64_t na, const uint64_t* __restrict__ Fb, int64_t nb, int64_t nwords,
    const int* __restrict__ pop_a, const int* __restrict__ pop_b, T alpha, int weighted, int64_t ntiles,
    int* __restrict__ counts, const int64_t* __restrict__ ptr, int* __restrict__ oidx, T* __restrict__ oval,
    int* __restrict__ not_binary) {
  __shared__ __attribute__((aligned(16))) uint32_t As[BK][TILE];
  __shared__ __attribute__((aligned(16))) uint32_t Bs[BK][TILE];
  __shared__ int rc[TILE][17];  // [row][tx]: kept entries of the row in the columns of thread column tx -> offsets
  __shared__ int cc[TILE][17];  // [column][ty]: the same for the mirror (SYM, off-diagonal tiles)

  int64_t it, jt;
  if (SYM) {
    triangle_tile(blockIdx.x, ntiles, it, jt);
  } else {
    it = blockIdx.y;
    jt = blockIdx.x;
  }
  const int64_t i0 = it * TILE, j0 = jt * TILE;
  const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
  const bool mirror = SYM && it != jt;

  uint32_t acc[RB][RB];
#pragma unroll
  for (int a = 0; a < RB; ++a)
#pragma unroll
    for (int b = 0; b < RB; ++b) acc[a][b] = 0;

  for (int64_t w0 = 0; w0 < nwords; w0 += BK / 2) {
    // stage 8 uint64 words of 128 rows of each side: consecutive threads read consecutive words of a row
#pragma unroll
    for (int e = tid; e < TILE * (BK / 2); e += 256) {
      const int r = e >> 3, w = e & 7;
      const int64_t k = w0 + w;
      const int64_t ia = i0 + r, jb = j0 + r;
      const uint64_t x = (k < nwords && ia < na) ? Fa[ia * nwords + k] : 0ull;
      const uint64_t y = (k < nwords && jb < nb) ? Fb[jb * nwords + k] : 0ull;
      As[2 * w][r] = (uint32_t)x;
      As[2 * w + 1][r] = (uint32_t)(x >> 32);
      Bs[2 * w][r] = (uint32_t)y;
      Bs[2 * w + 1][r] = (uint32_t)(y >> 32);
    }
    __syncthreads();
#pragma unroll
    for (int kk = 0; kk < BK; ++kk) {
      const uint4 a0 = *reinterpret_cast<const uint4*>(&As[kk][RB * ty]);
      const uint4 a1 = *reinterpret_cast<const uint4*>(&As[kk][RB * ty + 4]);
      const uint4 b0 = *reinterpret_cast<const uint4*>(&Bs[kk][RB * tx]);
      const uint4 b1 = *reinterpret_cast<const uint4*>(&Bs[kk][RB * tx + 4]);
      const uint32_t av[RB] = {a0.x, a0.y, a0.z, a0.w, a1.x, a1.y, a1.z, a1.w};
      const uint32_t bv[RB] = {b0.x, b0.y, b0.z, b0.w, b1.x, b1.y, b1.z, b1.w};
#pragma unroll
      for (int a = 0; a < RB; ++a)
#pragma unroll
        for (int b = 0; b < RB; ++b) acc[a][b] += __popc(av[a] & bv[b]);
    }
    __syncthreads();
  }

  // which of the 64 pairs are kept: bit b of rmask[a] = bit a of cmask[b] = pair (row RB*ty + a, column RB*tx + b)
  int pa[RB], pb[RB];
#pragma unroll
  for (int a = 0; a < RB; ++a) {
    const int64_t i = i0 + RB * ty + a;
    pa[a] = i < na ? pop_a[i] : -1;
  }
#pragma unroll
  for (int b = 0; b < RB; ++b) {
    const int64_t j = j0 + RB * tx + b;
    pb[b] = j < nb ? pop_b[j] : -1;
  }
  uint32_t rmask[RB], cmask[RB];
#pragma unroll
  for (int b = 0; b < RB; ++b) cmask[b] = 0;
  const bool wgt = weighted != 0;
#pragma unroll
  for (int a = 0; a < RB; ++a) {
    rmask[a] = 0;
#pragma unroll
    for (int b = 0; b < RB; ++b) {
      T v;
      const bool k = pa[a] >= 0 && pb[b] >= 0 && tanimoto_keep<T>((int)acc[a][b], pa[a], pb[b], alpha, wgt, v);
      rmask[a] |= (k ? 1u : 0u) << b;
      cmask[b] |= (k ? 1u : 0u) << a;
    }
  }
#pragma unroll
  for (int a = 0; a < RB; ++a) rc[RB * ty + a][tx] = __popc(rmask[a]);
  if (mirror) {
#pragma unroll
    for (int b = 0; b < RB; ++b) cc[RB * tx + b][ty] = __popc(cmask[b]);
  }
  __syncthreads();
  // exclusive scans: threads 0..127 over the 16 thread columns of row tid, threads 128..255 over the 16 thread rows
  // of column tid - 128
  {
    int(*tab)[17] = tid < TILE ? rc : cc;
    const int r = tid & (TILE - 1);
    if (tid < TILE || mirror) {
      int run = 0;
#pragma unroll
      for (int q = 0; q < 16; ++q) {
        const int c = tab[r][q];
        tab[r][q] = run;
        run += c;
      }
      if (!FILL) {
        if (tid < TILE) {
          if (i0 + r < na) counts[jt * na + i0 + r] = run;
        } else if (j0 + r < nb) {
          counts[it * na + j0 + r] = run;  // SYM: na == nb
        }
      }
    }
  }
  if (!FILL) return;
  __syncthreads();

  bool nb_flag = false;
#pragma unroll
  for (int a = 0; a < RB; ++a) {
    if (!rmask[a]) continue;
    const int64_t i = i0 + RB * ty + a;
    int64_t o = ptr[i] + counts[jt * na + i] + rc[RB * ty + a][tx];
#pragma unroll
    for (int b = 0; b < RB; ++b) {
      if (!((rmask[a] >> b) & 1u)) continue;
      T v;
      (void)tanimoto_keep<T>((int)acc[a][b], pa[a], pb[b], alpha, wgt, v);
      oidx[o] = (int)(j0 + RB * tx + b);
      if (oval) oval[o] = v;
      nb_flag |= (v != T(1));
      ++o;
    }
  }
  if (mirror) {
#pragma unroll
    for (int b = 0; b < RB; ++b) {
      if (!cmask[b]) continue;
      const int64_t j = j0 + RB * tx + b;
      int64_t o = ptr[j] + counts[it * na + j] + cc[RB * tx + b][ty];
#pragma unroll
      for (int a = 0; a < RB; ++a) {
        if (!((cmask[b] >> a) & 1u)) continue;
        T v;
        (void)tanimoto_keep<T>((int)acc[a][b], pa[a], pb[b], alpha, wgt, v);
        oidx[o] = (int)(i0 + RB * ty + a);
        if (oval) oval[o] = v;
        ++o;
      }
    }
  }
  if (nb_flag) *not_binary = 1;
}

}  // namespace

template <class T>
int TanimotoCsr<T>::count(const uint64_t* Fa_, int64_t na_, const uint64_t* Fb_, int64_t nb_, int64_t nwords_, T alpha_,
                          bool weighted_) {
  hipStream_t st = ctx().stream;
  what = "tanimoto";
  sym = (Fb_ == nullptr);
  Fa = Fa_;
  Fb = sym ? Fa_ : Fb_;
  nwords = nwords_;
  alpha = alpha_;
  weighted = weighted_;
  SS_TRY(this->begin(na_, sym ? na_ : nb_, TILE));
  if (na == 0 || nb == 0) return SS_OK;
  const int64_t nti = ceil_div(na, TILE);
  const int64_t nblocks = sym ? nti * (nti + 1) / 2 : nti * ntj;
  if (sym ? nblocks >= (1LL << 31) : (ntj >= (1LL << 31) || nti > 65535))
    return fail(SS_EUNSUPPORTED, "tanimoto: %lld x %lld pairs need more tiles than one launch holds", (long long)na,
                (long long)nb);
  SS_TRY(pop_a.alloc(na));
  hipLaunchKernelGGL(popcount_rows_kernel, dim3((unsigned)ceil_div(na, 256)), dim3(256), 0, st, Fa, na, nwords, pop_a.p);
  SS_LAUNCH_CHECK();
  if (!sym) {
    SS_TRY(pop_b.alloc(nb));
    hipLaunchKernelGGL(popcount_rows_kernel, dim3((unsigned)ceil_div(nb, 256)), dim3(256), 0, st, Fb, nb, nwords,
                       pop_b.p);
    SS_LAUNCH_CHECK();
  }
  SS_TRY(counts.alloc((size_t)ntj * (size_t)na));
  if (sym) {
    hipLaunchKernelGGL((tanimoto_tile_kernel<T, true, false>), dim3((unsigned)nblocks), dim3(256), 0, st, Fa, na, Fb, nb,
                       nwords, pop_a.p, pop_a.p, alpha, weighted ? 1 : 0, nti, counts.p, (const int64_t*)nullptr,
                       (int*)nullptr, (T*)nullptr, (int*)nullptr);
  } else {
    hipLaunchKernelGGL((tanimoto_tile_kernel<T, false, false>), dim3((unsigned)ntj, (unsigned)nti), dim3(256), 0, st, Fa,
                       na, Fb, nb, nwords, pop_a.p, pop_b.p, alpha, weighted ? 1 : 0, ntj, counts.p,
                       (const int64_t*)nullptr, (int*)nullptr, (T*)nullptr, (int*)nullptr);
  }
  SS_LAUNCH_CHECK();
  return this->scan();
}

template <class T>
int TanimotoCsr<T>::fill(int* idx, T* val, bool* binary) {
  hipStream_t st = ctx().stream;
  if (binary) *binary = true;
  if (nnz == 0) return SS_OK;
  DevBuf<int> flag;
  SS_TRY(flag.alloc(1));
  SS_HIP(hipMemsetAsync(flag.p, 0, sizeof(int), st));
  const int64_t nti = ceil_div(na, TILE);
  if (sym) {
    hipLaunchKernelGGL((tanimoto_tile_kernel<T, true, true>), dim3((unsigned)(nti * (nti + 1) / 2)), dim3(256), 0, st, Fa,
                       na, Fb, nb, nwords, pop_a.p, pop_a.p, alpha, weighted ? 1 : 0, nti, counts.p, ptr.p, idx, val,
                       flag.p);
  } else {
    hipLaunchKernelGGL((tanimoto_tile_kernel<T, false, true>), dim3((unsigned)ntj, (unsigned)nti), dim3(256), 0, st, Fa,
                       na, Fb, nb, nwords, pop_a.p, pop_b.p, alpha, weighted ? 1 : 0, ntj, counts.p, ptr.p, idx, val,
                       flag.p);
  }
  SS_LAUNCH_CHECK();
  int notbin = 0;
  SS_HIP(hipMemcpyAsync(&notbin, flag.p, sizeof(int), hipMemcpyDeviceToHost, st));
  SS_HIP(hipStreamSynchronize(st));
  if (binary) *binary = (notbin == 0);
  return SS_OK;
}

template struct TanimotoCsr<float>;
template struct TanimotoCsr<double>;

}  // namespace ss
