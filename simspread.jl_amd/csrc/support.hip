// Support lists: which sources carry a score.  A score is Yhat[r,t] = sum_s T[r,s] * Ys[s,t] with T[r,:] the transfer
// row stage 1 hands to stage 2; the support of the pair (r, t) is the set of sources s with a stored Ys[s,t] and
// c_s = T[r,s] * Ys[s,t] != 0 (one rounded multiply in T; a pattern-only label block multiplies by 1), ordered by c_s
// descending as Julia's isless orders floats, ties by ascending s.  Per pair the kernel gives the size of the support
// and its first M entries (M <= 64).
//
// One wave per pair, SUPPORT_WAVES pairs per workgroup.  The wave streams row t of Ys' once: every step its lanes load
// 64 consecutive entries (idx, and val unless the block is pattern-only: coalesced), gather T[slot][s] and form the
// order-preserving unsigned key of c (tl_key's rule, target_topl.hip).  The M best so far live in registers, entry j in
// lane j, sorted; a step's entries are filtered against the current M-th entry with one ballot, and the survivors are
// inserted one by one: the insert position is the popcount of a ballot ("my entry ranks before the candidate"), the tail
// moves up by one lane with a shuffle.  The list is the exact top M under a total order (key descending, s ascending; s
// is unique inside a row of Ys'), so neither the lane a candidate sat in nor the order of the inserts can reach the
// output: it is bitwise repeatable without atomics.  Waves never wait for one another (no workgroup barrier: the rows
// of a workgroup's pairs have different lengths) and no LDS is used.
//
// Bytes per pair: kt * (4 + sizeof(T) + 4) -- the index, the value and the gathered T entry of every stored label --
// and sizeof(T) less per entry for a pattern-only block; the outputs are M * (4 + sizeof(T)) + 4.
#include <hip/hip_runtime.h>

#include "graph.hpp"

namespace ss {

namespace {

constexpr int SUPPORT_WAVES = 4;  // pairs per workgroup
constexpr int SUPPORT_THREADS = 64 * SUPPORT_WAVES;
constexpr int SUPPORT_EMPTY = 0x7fffffff;  // source id of an unused list slot (key 0: ranks after every entry)

__device__ inline uint32_t sp_key(float v) {
  const uint32_t u = __float_as_uint(v);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ inline uint64_t sp_key(double v) {
  const uint64_t u = (uint64_t)__double_as_longlong(v);
  return (u >> 63) ? ~u : (u | (1ULL << 63));
}
__device__ inline float sp_value(uint32_t k) { return __uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k); }
__device__ inline double sp_value(uint64_t k) {
  return __longlong_as_double((long long)((k >> 63) ? (k & ~(1ULL << 63)) : ~k));
}

__device__ inline uint32_t sp_shfl(uint32_t v, int lane) { return (uint32_t)__shfl((int)v, lane, 64); }
__device__ inline uint64_t sp_shfl(uint64_t v, int lane) {
  const uint32_t lo = (uint32_t)__shfl((int)(uint32_t)v, lane, 64);
  const uint32_t hi = (uint32_t)__shfl((int)(uint32_t)(v >> 32), lane, 64);
  return ((uint64_t)hi << 32) | lo;
}
__device__ inline uint32_t sp_shfl_up(uint32_t v) { return (uint32_t)__shfl_up((int)v, 1, 64); }
__device__ inline uint64_t sp_shfl_up(uint64_t v) {
  const uint32_t lo = (uint32_t)__shfl_up((int)(uint32_t)v, 1, 64);
  const uint32_t hi = (uint32_t)__shfl_up((int)(uint32_t)(v >> 32), 1, 64);
  return ((uint64_t)hi << 32) | lo;
}

// (ka, sa) ranks strictly before (kb, sb)
template <class K>
__device__ inline bool sp_before(K ka, int sa, K kb, int sb) {
  return ka > kb || (ka == kb && sa < sb);
}

// pairs [0, npairs): pair p reads transfer row slot[p] of Trows (leading dimension ldt) and row tgt[p] of Ys' and
// writes entry pos[p] of the outputs
template <class T, bool BINARY>
__global__ void __launch_bounds__(SUPPORT_THREADS)
support_kernel(const int* __restrict__ yptr, const int* __restrict__ yidx, const T* __restrict__ yval,
               const T* __restrict__ Trows, int64_t ldt, const int* __restrict__ slot, const int* __restrict__ tgt,
               const int* __restrict__ pos, int64_t npairs, int M, int* __restrict__ src, T* __restrict__ contrib,
               int* __restrict__ nsupp) {
  using K = pool_key_t<T>;
  const int lane = threadIdx.x & 63;
  const int64_t p = (int64_t)blockIdx.x * SUPPORT_WAVES + (threadIdx.x >> 6);
  if (p >= npairs) return;  // the whole wave leaves
  const int t = tgt[p];
  const T* __restrict__ trow = Trows + (int64_t)slot[p] * ldt;
  const int b = yptr[t], e = yptr[t + 1];

  K mykey = 0;               // entry `lane` of the list (lanes >= M: never read)
  int mys = SUPPORT_EMPTY;
  K thk = 0;                 // entry M - 1: what a candidate has to beat
  int ths = SUPPORT_EMPTY;
  int n = 0;                 // size of the support
  for (int q0 = b; q0 < e; q0 += 64) {
    const int q = q0 + lane;
    const bool have = q < e;
    int s = 0;
    T c = T(0);
    if (have) {
      s = yidx[q];
      c = trow[s];
      if (!BINARY) c = c * yval[q];
    }
    const bool nz = have && c != T(0);
    n += __popcll(__ballot(nz));
    const K k = sp_key(c);
    unsigned long long m = __ballot(nz && sp_before<K>(k, s, thk, ths));
    while (m) {
      const int l = __ffsll((long long)m) - 1;
      m &= m - 1;
      const K ck = sp_shfl(k, l);
      const int cs = __shfl(s, l, 64);
      if (!sp_before<K>(ck, cs, thk, ths)) continue;  // an earlier insert of this step raised the bar (uniform)
      const int at = __popcll(__ballot(lane < M && sp_before<K>(mykey, mys, ck, cs)));
      const K upk = sp_shfl_up(mykey);
      const int ups = __shfl_up(mys, 1, 64);
      if (lane == at) {
        mykey = ck;
        mys = cs;
      } else if (lane > at) {
        mykey = upk;
        mys = ups;
      }
      thk = sp_shfl(mykey, M - 1);
      ths = __shfl(mys, M - 1, 64);
    }
  }
  const int64_t o = (int64_t)pos[p];
  if (lane < M) {
    const bool used = mys != SUPPORT_EMPTY;
    src[o * M + lane] = used ? mys : -1;
    contrib[o * M + lane] = used ? sp_value(mykey) : T(0);
  }
  if (lane == 0) nsupp[o] = n;
}

}  // namespace

template <class T>
int launch_support(const DevCsr<T>& YsT, const T* Trows, int64_t ldt, const int* slot, const int* tgt, const int* pos,
                   int64_t npairs, int M, int* src, T* contrib, int* nsupp) {
  if (npairs <= 0) return SS_OK;
  if (M < 1 || M > 64) return fail(SS_EINVAL, "support: M = %d outside 1..64", M);
  const int64_t grid = ceil_div(npairs, SUPPORT_WAVES);
  if (grid >= (1LL << 31)) return fail(SS_EUNSUPPORTED, "support: too many pairs for one launch");
  auto kernel = YsT.binary ? support_kernel<T, true> : support_kernel<T, false>;
  hipLaunchKernelGGL(kernel, dim3((unsigned)grid), dim3(SUPPORT_THREADS), 0, ctx().stream, YsT.ptr.p, YsT.idx.p,
                     YsT.val.p, Trows, ldt, slot, tgt, pos, npairs, M, src, contrib, nsupp);
  SS_LAUNCH_CHECK();
  return SS_OK;
}

template int launch_support<float>(const DevCsr<float>&, const float*, int64_t, const int*, const int*, const int*,
                                   int64_t, int, int*, float*, int*);
template int launch_support<double>(const DevCsr<double>&, const double*, int64_t, const int*, const int*, const int*,
                                    int64_t, int, int*, double*, int*);

}  // namespace ss
