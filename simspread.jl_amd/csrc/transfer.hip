// Stage 1 of the SimSpread resource-spreading pass: rows of the transfer block T = (L D1^-1) Mt D2^-1 (the sparse x
// sparse -> dense product hidden in the reference's W*W, src/core.jl:413).  transfer_kernel is the default (one
// single-wave workgroup per row and column chunk; also leave-one-out, k-fold, two-term and accumulating rows; COEF: the
// coefficients of a neighbour group from a table the handle keeps, transfer_coef_rows_kernel, not gathered); the
// block family (transfer_block / _qflat / _wide / _wide2_kernel: NW rows of L per workgroup on one chunk, opt-in with
// SS_TRANSFER_V=2) is the measured record behind DESIGN.md 4.1.  Shared: BlockLayout, quad_fetch, quad_fold (all that
// have them), block_prologue (block, qflat), block_row (qflat), fixed_scale (block, wide, wide2), fixed_store (block, qflat,
// wide2), raw_load (wide), subrows_fold_any, tails_begin / tails_finish (single-wave, block).  A piece is used only where the kernel's loop compiles to the parent
// layout's instructions with it; where it did not, the kernel keeps its own text and says so.
// Wavefront = 64 lanes.  No float atomics: every sum has a fixed order or is an integer sum, so results are bitwise
// reproducible from run to run.
#include <type_traits>

#include "graph.hpp"

namespace ss {

template <class T>
struct ChunkedView {
  const int* off;            // [nchunks*rows + 1]
  const unsigned short* idx; // chunk-local column
  const T* val;
  int64_t rows;
};
template <class T>
static inline ChunkedView<T> view(const DevChunked<T>& m) {
  return ChunkedView<T>{m.off.p, m.idx.p, m.val.p, m.rows};
}

template <class T>
struct TransferArgs {
  int nterms;
  CsrView<T> L[2];
  const T* inv1[2];
  const T* coef[2];  // COEF kernels: the coefficient of entry q of L[t], ready made (transfer_coef_build)
  ChunkedView<T> M[2];
  const T* inv2;
  const int* kf;  // LOO: integer degrees
  const int* ks;
  int64_t row_begin;
  const int* row_ids;  // optional: row of L handled by workgroup-row r is row_ids[row_begin + r] (k-fold members)
  int64_t nj;
  int SC;       // columns of T per workgroup (= chunk of the Mt operands)
  int nchunks;
  T* out;
  int64_t ld;
  int accumulate;  // add to what `out` already holds (dense regime: the feature path came from the GEMM)
  float xmax;      // FIX: largest |value| of the Mt operand
  int chunk_interleave;  // SS_TRANSFER_ORDER=0: rows take all their chunks in turn (the order of rounds 1-2)
};
template <class T>
__device__ __forceinline__ bool chunks_in_turn(const TransferArgs<T>& p) { return p.chunk_interleave != 0; }

// ---------------------------------------------------------------- launch helpers
// A runtime bool / one of a small set of integers becomes a compile-time constant: f is a generic lambda that reads
// decltype(arg)::value.  dispatch_int fails with SS_EINVAL when v is none of Vs.
template <class F>
static int dispatch_bool(bool b, F&& f) {
  return b ? f(std::true_type{}) : f(std::false_type{});
}
template <int... Vs, class F>
static int dispatch_int(int v, F&& f) {
  int rc = SS_OK;
  const bool hit = ((v == Vs && ((rc = f(std::integral_constant<int, Vs>{})), true)) || ...);
  return hit ? rc : fail(SS_EINVAL, "dispatch_int: no kernel for the value %d", v);
}

// Launch of a kernel whose dynamic LDS may exceed 64 KiB: the attribute is set once per kernel.
template <auto Kernel, class... Args>
static int launch_lds(unsigned grid, int block, size_t lds, Args... args) {
  static std::atomic<bool> attr_done{false};
  if (!attr_done) {
    SS_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(Kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                               160 * 1024));
    attr_done = true;
  }
  hipLaunchKernelGGL(Kernel, dim3(grid), dim3(block), lds, ctx().stream, args...);
  SS_LAUNCH_CHECK();
  return SS_OK;
}

// ---------------------------------------------------------------- sub-rows, U at a time
// One single-wave workgroup per (row r of L, column chunk c of T); c = blockIdx % nchunks so that,
// with the dispatcher dealing workgroups round-robin over the 8 XCDs, chunk c is always served by
// the same XCD and the sub-rows of Mt it touches stay in that XCD's L2 (speed only -- any placement
// is correct).  acc[j] (LDS, owned by this one wave) collects sum_a L[r,a]*inv1[a]*Mt[a][c*SC + j].
// The wave takes U neighbours a of r at a time, issues all their global loads, then folds the
// sub-rows in one after the other with plain LDS read-add-write: the columns inside one sub-row are
// distinct and LDS operations of one wave execute in order, so no atomics are needed and the sum
// order is fixed (bitwise reproducible).  Measured on MI355X: ds_add_f32 costs ~193 clk per
// wave-instruction (lanes serialised), ds_add_f64 ~27, a plain read-add-write pair ~17
// (tools/lds_atomic_bench.hip) -- which is why this is not an LDS-atomic kernel.
constexpr int TRANSFER_THREADS = 64;

template <class T> struct BitsOf;
template <> struct BitsOf<float> {
  static __device__ __forceinline__ float bcast(float v, int src) {
    return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), src));
  }
  // lane i's value goes to lane to4 / 4; lane i takes the value of lane from4 / 4
  static __device__ __forceinline__ float push(int to4, float v) {
    return __int_as_float(__builtin_amdgcn_ds_permute(to4, __float_as_int(v)));
  }
  static __device__ __forceinline__ float pull(int from4, float v) {
    return __int_as_float(__builtin_amdgcn_ds_bpermute(from4, __float_as_int(v)));
  }
};
template <> struct BitsOf<double> {
  static __device__ __forceinline__ double join(int lo, int hi) {
    return __longlong_as_double(((long long)hi << 32) | (unsigned int)lo);
  }
  static __device__ __forceinline__ double bcast(double v, int src) {
    const long long b = __double_as_longlong(v);
    const int lo = __builtin_amdgcn_readlane((int)(b & 0xffffffffll), src);
    const int hi = __builtin_amdgcn_readlane((int)(b >> 32), src);
    return join(lo, hi);
  }
  static __device__ __forceinline__ double push(int to4, double v) {
    const long long b = __double_as_longlong(v);
    return join(__builtin_amdgcn_ds_permute(to4, (int)(b & 0xffffffffll)), __builtin_amdgcn_ds_permute(to4, (int)(b >> 32)));
  }
  static __device__ __forceinline__ double pull(int from4, double v) {
    const long long b = __double_as_longlong(v);
    return join(__builtin_amdgcn_ds_bpermute(from4, (int)(b & 0xffffffffll)), __builtin_amdgcn_ds_bpermute(from4, (int)(b >> 32)));
  }
};

// U sub-rows: scalar bounds + coefficient, and the (unconditional) loads of their first 64 entries (the heads).
// The operand arrays carry 256 entries of slack, so lanes past the end of a sub-row read valid memory;
// such lanes are steered to a per-lane dummy accumulator behind the chunk.
template <class T, int U>
struct SubRows {
  int n[U];
  unsigned b[U];
  T cf[U];
  unsigned short j[U];
  T v[U];
};

// The same loads as buffer instructions: resource descriptor (SGPRs) + scalar byte offset of the sub-row + a 32-bit lane
// offset.  A global_load with per-lane 64-bit addresses hands the texture addresser 512 bytes of address per
// wave-instruction, the buffer form 256; stage 1 is bound by that unit (TA busy 92 % of the kernel at ~7 clk per load,
// profiles/r03_stage1_mem_pmc.txt).
template <int U, bool BINM>
__device__ __forceinline__ void subrows_load_buf(SubRows<float, U>& s, int first, int b_l, int n_l, float cf_l,
                                                 __amdgpu_buffer_rsrc_t ridx, __amdgpu_buffer_rsrc_t rval, int lane) {
#pragma unroll
  for (int u = 0; u < U; ++u) {
    const int src = first + u;
    s.b[u] = (unsigned)__builtin_amdgcn_readlane(b_l, src);
    s.n[u] = __builtin_amdgcn_readlane(n_l, src);
    s.cf[u] = BitsOf<float>::bcast(cf_l, src);
    s.j[u] = __builtin_amdgcn_raw_buffer_load_b16(ridx, lane * 2, (int)(s.b[u] * 2u), 0);
    s.v[u] = BINM ? 1.f : __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rval, lane * 4, (int)(s.b[u] * 4u), 0));
    __builtin_amdgcn_sched_barrier(0);
  }
}

template <class T, int U, bool BINM>
__device__ __forceinline__ void subrows_load(SubRows<T, U>& s, int first, int b_l, int n_l, T cf_l,
                                             const unsigned short* __restrict__ midx, const T* __restrict__ mval,
                                             int lane) {
#pragma unroll
  for (int u = 0; u < U; ++u) {
    const int src = first + u;  // < 64 by construction
    s.b[u] = (unsigned)__builtin_amdgcn_readlane(b_l, src);
    s.n[u] = __builtin_amdgcn_readlane(n_l, src);
    s.cf[u] = BitsOf<T>::bcast(cf_l, src);
    const unsigned short* pi = midx + s.b[u];
    const T* pv = mval + s.b[u];
    s.j[u] = pi[lane];
    s.v[u] = BINM ? T(1) : pv[lane];  // unweighted features: every stored value is 1, two thirds of the bytes vanish
    // the loads leave in the order the fold takes them (it waits for them one by one): without the fence the
    // scheduler is free to issue sub-row 0 last, and the fold of a batch then waits for all of it
    __builtin_amdgcn_sched_barrier(0);
  }
}

// DUAL: two copies of the accumulators (acc and acc + astride); sub-rows 2i and 2i+1 of a batch go to different
// copies, so their read-add-write pairs are independent and both LDS reads are in flight together (with one copy
// every pair waits for the previous pair's LDS round trip).  The copies are added when T is written out: the sum
// order is still fixed.  (Tails and rests go to the first copy.)
template <class T, int U, bool DUAL>
__device__ __forceinline__ void subrows_fold(const SubRows<T, U>& s, T* __restrict__ acc, int astride, int dummy, int lane) {
  if constexpr (DUAL) {
    T* __restrict__ acc1 = acc + astride;
#pragma unroll
    for (int u = 0; u < U; u += 2) {
      const int ja = lane < s.n[u] ? (int)s.j[u] : dummy;
      const int jb = lane < s.n[u + 1] ? (int)s.j[u + 1] : dummy;
      const T ra = acc[ja], rb = acc1[jb];
      acc[ja] = fma(s.cf[u], s.v[u], ra);
      acc1[jb] = fma(s.cf[u + 1], s.v[u + 1], rb);
    }
  } else {
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int j = lane < s.n[u] ? (int)s.j[u] : dummy;
      acc[j] = fma(s.cf[u], s.v[u], acc[j]);
    }
  }
}

// Fixed-point fold (fp32 graphs): the product cf * v is scaled by 2^k (k per row of L, see fixed_scale),
// rounded to an integer and added with ds_add_u32.  An LDS integer atomic costs ~8 clk per wave-instruction on random
// addresses where the plain read-add-write pair costs ~15 (tools/lds_atomic_bench.hip) -- and stage 1 runs at exactly
// the LDS rate of its scatter -- it returns nothing (no wait, no dependent chain through the LDS round trip) and integer
// addition commutes: the sums do not depend on any order, so the result is bitwise reproducible by construction.
// Lanes past the end of a sub-row add 0 to whatever valid column they happened to read.
__device__ __forceinline__ int cvt_rpi(float x) {
  int r;
  asm("v_cvt_rpi_i32_f32 %0, %1" : "=v"(r) : "v"(x));   // floor(x + 0.5)
  return r;
}
template <int U>
__device__ __forceinline__ void subrows_fold_fixed(const SubRows<float, U>& s, unsigned* __restrict__ acc, int lane) {
#pragma unroll
  for (int u = 0; u < U; ++u) {
    const float v = lane < s.n[u] ? s.v[u] : 0.f;
    atomicAdd(&acc[s.j[u]], (unsigned)cvt_rpi(s.cf[u] * v));
  }
}

// the heads of one batch into the wave's sums: fixed point or plain read-add-write
template <class T, int U, bool DUAL, bool FIX>
__device__ __forceinline__ void subrows_fold_any(const SubRows<T, U>& s, T* acc, int astride, int dummy, int lane) {
  if constexpr (FIX) subrows_fold_fixed<U>(s, reinterpret_cast<unsigned*>(acc), lane);
  else subrows_fold<T, U, DUAL>(s, acc, astride, dummy, lane);
}

// ---------------------------------------------------------------- tails: entries 64.. of the long sub-rows of a group
// With the chunk sized for a mean sub-row of ~60 entries, ~40 % of the sub-rows are longer than one wave, by ~6 entries.
// Their entries 64..79 are taken once per group of 64 neighbours, after the heads, FOUR sub-rows to a load pair AND to a
// read-add-write pair.  What keeps the four apart is the operand (assemble.hip, "class-pure tails"): the tail of the
// sub-row of operand row a holds only columns j with (j & 3) == (a & 3) -- or sentinels on the first dummy word -- so
// tails of four different classes a & 3 have pairwise distinct columns.  The group's long sub-rows are compacted by
// class (four ballots and one lane permutation of start, length and coefficient per group: no scalar work per
// sub-row): the k-th long sub-row of class c, in neighbour order, goes to slot 4k + c; round r serves slots 4r .. 4r+3,
// lane group g = lane >> 4 the slot 4r + g, i.e. a sub-row of class g, with its 16 lanes.  Rounds = the largest class
// count.  A group without a long sub-row (sub-rows of ~40 entries, C3) pays one ballot and one branch.  Lanes past the
// end of the tail or of a slot that no sub-row took (length forced to 0: the permutation's result in a lane nobody
// writes is not relied on) go to their dummy word; the fixed-point fold adds the round in one integer atomic.  Entries
// from position 80 on (~1 % of the sub-rows at 62.5 +- 7.7 entries) take the rest loop, bounds re-read by lane index;
// so does, from position 64, a long sub-row beyond the 16th of its class in the group (overflow).
// Order of a column's sums inside a group: heads in neighbour order; tails in neighbour order (a column only meets
// tails of its own class, one per round); then the rests and the overflowing sub-rows in neighbour order -- a fixed
// function of the row's neighbour list.
// AHEAD rounds are fetched together; the first AHEAD of a group fly while its heads are folded: 4 with pattern-only
// operands (one register a round), 3 with values (2 in the opt-in DUAL / FIX / BUF and block kernels, as before the classes).  By class a group has ~8.9 rounds where it had 6.6, so with values
// one more round per flight pays (C2 stage 1: 1.273 ms with 2, 1.265 ms with 3, profiles/stage1_tail_classes_time.json)
// and fits: the U = 8 kernel holds 78 registers with 3 (6 waves per SIMD) and 81 with 4 (5 waves; before the classes
// 4 rounds measured 1.39 instead of 1.33 ms, profiles/stage1_tails_time.json).
template <class T, int AHEAD>
struct Tails {
  static constexpr int TAIL_AHEAD = AHEAD;
  int nr;                  // rounds of the group (wave-uniform); 0: no long sub-row
  unsigned long long ovf;  // long sub-rows without a slot (wave-uniform)
  int cb, cn;              // lane s: start and length of the sub-row in slot s; length 0 in an empty slot
  T ccf;
  unsigned short tj[TAIL_AHEAD];
  T tv[TAIL_AHEAD];
};

// rounds r0 .. r0 + TAIL_AHEAD - 1 that exist; ld(entry, index&, value&) reads one operand entry
template <class T, int TAIL_AHEAD, class LD>
__device__ __forceinline__ void tails_fetch(Tails<T, TAIL_AHEAD>& t, int r0, int lane, LD&& ld) {
#pragma unroll
  for (int i = 0; i < TAIL_AHEAD; ++i) {
    if (r0 + i >= t.nr) break;
    const unsigned b = (unsigned)__builtin_amdgcn_ds_bpermute((4 * (r0 + i) + (lane >> 4)) * 4, t.cb);
    ld(b + 64u + (unsigned)(lane & 15), t.tj[i], t.tv[i]);   // (any start + 80 is inside the operand and its slack)
    __builtin_amdgcn_sched_barrier(0);
  }
}

// compaction of the group's long sub-rows by class (a_l: the lane's operand row), and the loads of the first rounds
template <class T, int TAIL_AHEAD, class LD>
__device__ __forceinline__ void tails_begin(Tails<T, TAIL_AHEAD>& t, int a_l, int b_l, int n_l, T cf_l, int lane, LD&& ld) {
  const bool lng = n_l > 64;
  const unsigned long long longs = __ballot(lng);
  t.nr = 0;
  if (longs == 0ull) return;
  const int cls = a_l & 3;
  int k = 0, rounds = 0, fewest = 16, spare = 0, taken = 0;
#pragma unroll
  for (int c = 0; c < 4; ++c) {
    const unsigned long long mc = __ballot(lng && cls == c);
    const int kc = (int)__builtin_amdgcn_mbcnt_hi((unsigned)(mc >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)mc, 0u));
    int cc = __builtin_popcountll(mc);
    cc = cc < 16 ? cc : 16;
    k = cls == c ? kc : k;
    rounds = cc > rounds ? cc : rounds;
    if (cc < fewest) { fewest = cc; spare = 4 * cc + c; }   // a slot nobody takes (none only when all 64 are taken)
    taken = (lane & 3) == c ? cc : taken;                   // slot s is taken when (s >> 2) < count of class s & 3
  }
  const bool placed = lng && k < 16;
  t.nr = rounds;
  t.ovf = __ballot(lng && k >= 16);
  const int to4 = (placed ? 4 * k + cls : spare) * 4;       // every lane without a slot writes the spare one
  const bool mine = (lane >> 2) < taken;
  const int pb = __builtin_amdgcn_ds_permute(to4, b_l), pn = __builtin_amdgcn_ds_permute(to4, n_l);
  t.cb = mine ? pb : 0;
  t.cn = mine ? pn : 0;
  t.ccf = BitsOf<T>::push(to4, cf_l);
  tails_fetch(t, 0, lane, ld);
}

template <class T, bool BINM, bool FIX, int TAIL_AHEAD, class LD>
__device__ __forceinline__ void tails_finish(Tails<T, TAIL_AHEAD>& t, int b_l, int n_l, T cf_l, T* __restrict__ acc, int dummy,
                                             const unsigned short* __restrict__ midx, const T* __restrict__ mval, int lane,
                                             LD&& ld) {
  if (t.nr == 0) return;
  for (int r0 = 0; r0 < t.nr; r0 += TAIL_AHEAD) {
    if (r0 > 0) tails_fetch(t, r0, lane, ld);
#pragma unroll
    for (int i = 0; i < TAIL_AHEAD; ++i) {
      if (r0 + i >= t.nr) break;
      const int from4 = (4 * (r0 + i) + (lane >> 4)) * 4;
      const int tn = __builtin_amdgcn_ds_bpermute(from4, t.cn) - 64;   // entries past position 64 (<= 0: none); may exceed 16
      const T tcf = BitsOf<T>::pull(from4, t.ccf);
      const bool live = (lane & 15) < tn;
      if constexpr (FIX) {
        atomicAdd(reinterpret_cast<unsigned*>(acc) + (live ? (int)t.tj[i] : dummy),
                  (unsigned)cvt_rpi(live ? (float)(tcf * t.tv[i]) : 0.f));
      } else {
        const int j = live ? (int)t.tj[i] : dummy;   // the four tails of the round: four classes, distinct columns
        acc[j] = fma(tcf, t.tv[i], acc[j]);
      }
    }
  }
  // rests from position 80; overflowing sub-rows whole from position 64
  unsigned long long m = __ballot(n_l > 80) | t.ovf;
  while (m != 0ull) {
    const int src = __builtin_ctzll(m);
    m &= m - 1ull;
    const int n = __builtin_amdgcn_readlane(n_l, src);
    const unsigned b = (unsigned)__builtin_amdgcn_readlane(b_l, src);
    const T cf = BitsOf<T>::bcast(cf_l, src);
    for (int x = (((t.ovf >> src) & 1ull) ? 64 : 80) + lane; x < n; x += 64) {
      const int j = midx[b + x];
      const T v = BINM ? T(1) : mval[b + x];
      if constexpr (FIX) atomicAdd(reinterpret_cast<unsigned*>(acc) + j, (unsigned)cvt_rpi((float)(cf * v)));
      else acc[j] = fma(cf, v, acc[j]);
    }
  }
}

// Scale 2^k of one row's fixed-point sums.  Every sum is bounded by bound = (sum_a |coef[a]|) * xmax (xmax = largest
// |value| of the operand); bound < 2^e, so with k = 30 - e all sums stay below 2^30, the roundings (one unit per term
// at most) below 2^24: no overflow in 32 bits, resolution bound * 2^-30.  abs_coef(q) is |coefficient| of entry q of
// the row.  The order of the sum (stride 64 per lane, then the xor butterfly from 32 down) decides the bits of e.
struct FixedScale {
  float scale, unscale;   // 2^k, 2^-k
};
template <class F>
__device__ __forceinline__ FixedScale fixed_scale(int lb, int le, int lane, float xmax, F&& abs_coef) {
  float sabs = 0.f;
  for (int q = lb + lane; q < le; q += 64) sabs += abs_coef(q);
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) sabs += __shfl_xor(sabs, o);
  int e = 0;
  (void)frexpf(sabs * xmax, &e);
  if (!(sabs * xmax > 0.f)) e = 0;
  e = e < -90 ? -90 : (e > 120 ? 120 : e);
  return FixedScale{ldexpf(1.f, 30 - e), ldexpf(1.f, e - 30)};
}

// ---------------------------------------------------------------- the single-wave kernel
// COEF (default family only: no DUAL / FIX / BUF): a group's coefficients come from p.coef[t][q], one coalesced load
// issued together with L.idx[q], instead of L.val[q] and the 64-lane gather inv1[a] (LOO: kf[a]); the gather of the
// sub-row bounds no longer waits for the coefficient: it is unconditional and a zero coefficient zeroes the length.
template <class T, bool LOO, int U, bool BINM, bool DUAL, bool FIX = false, bool BUF = false, bool COEF = false>
__global__ void __launch_bounds__(TRANSFER_THREADS) transfer_kernel(TransferArgs<T> p) {
  static_assert(64 % (2 * U) == 0, "U must divide 32");
  static_assert(!COEF || (!DUAL && !FIX && !BUF), "coefficient tables serve the default family only");
  extern __shared__ __align__(16) unsigned char smem_raw[];
  T* acc = reinterpret_cast<T*>(smem_raw);                        // [SC] sums + [64] per-lane dummies (x2 when DUAL)
  const int astride = p.SC + 64;
  constexpr int NCOPY = DUAL ? 2 : 1;
  unsigned* bits = reinterpret_cast<unsigned*>(acc + NCOPY * astride);  // LOO only: source owns the dropped feature
  const int lane = threadIdx.x;
  // Workgroup i runs on XCD i % 8 and chunk c on XCD c % 8 (the chunk count is a multiple of 8).  With more than 8
  // chunks the groups of 8 chunks are walked ONE AFTER THE OTHER over all rows (round 3; before: every row took all its
  // chunks in turn): what the 8 XCDs re-read from row to row is then 8 chunk slices of X' instead of all of it -- at
  // C3 200 MB instead of 600 MB, i.e. inside the 256 MB Infinity Cache instead of in HBM.  8 chunks (C2): same order as before.
  int c;
  int64_t r;
  if (p.nchunks > 8 && p.nchunks % 8 == 0 && !chunks_in_turn(p)) {
    const int64_t nrows = (int64_t)gridDim.x / p.nchunks, per = nrows * 8;
    const int64_t grp = blockIdx.x / per, rem = blockIdx.x - grp * per;
    r = rem >> 3;
    c = (int)(grp * 8 + (rem & 7));
  } else {
    c = blockIdx.x % p.nchunks;
    r = blockIdx.x / p.nchunks;
  }
  const int64_t gr = p.row_ids ? (int64_t)p.row_ids[p.row_begin + r] : p.row_begin + r;
  const int64_t j0 = (int64_t)c * p.SC;
  const int jn = (int)((p.nj - j0 < p.SC) ? (p.nj - j0) : p.SC);
  const int dummy = p.SC + lane;

  for (int j = lane; j < NCOPY * astride; j += 64) acc[j] = T(0);
  if (LOO)
    for (int j = lane; j < (p.SC + 31) / 32; j += 64) bits[j] = 0u;
  __syncthreads();

  float fix_unscale = 1.f;
  for (int t = 0; t < p.nterms; ++t) {
    const CsrView<T> L = p.L[t];
    const ChunkedView<T> M = p.M[t];
    const int* __restrict__ off = M.off + (int64_t)c * M.rows;
    const unsigned short* __restrict__ midx = M.idx;
    const T* __restrict__ mval = M.val;
    const int lb = L.ptr[gr], le = L.ptr[gr + 1];
    float scale = 1.f;
    if constexpr (FIX) {   // (experiment: fixed-point sums in the single-wave kernel; one term, not LOO)
      float sabs = 0.f;   // (fixed_scale's text: as a call it reschedules this kernel)
      for (int q = lb + lane; q < le; q += 64) sabs += fabsf((float)(L.val[q] * p.inv1[t][L.idx[q]]));
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) sabs += __shfl_xor(sabs, o);
      int e = 0;
      (void)frexpf(sabs * p.xmax, &e);
      if (!(sabs * p.xmax > 0.f)) e = 0;
      e = e < -90 ? -90 : (e > 120 ? 120 : e);
      scale = ldexpf(1.f, 30 - e);
      fix_unscale = ldexpf(1.f, e - 30);
    }
    for (int g0 = lb; g0 < le; g0 += 64) {
      // ---- the next 64 neighbours a of r, one per lane: coefficient and sub-row bounds
      const int q = g0 + lane;
      int a_l = 0, b_l = 0, n_l = 0;   // a_l: the neighbour, i.e. the operand row (its class cuts the tails)
      T cf_l = T(0);
      if constexpr (COEF) {
        if (q < le) {
          const int a = a_l = L.idx[q];
          cf_l = p.coef[t][q];
          const int o0 = off[a], o1 = off[a + 1];
          b_l = o0;
          n_l = cf_l != T(0) ? o1 - o0 : 0;
        }
      } else if (q < le) {
        const int a = a_l = L.idx[q];
        const T lv = L.val[q];
        if (LOO) {
          const int d = p.kf[a] - 1;  // the query leaves every feature column it touched
          cf_l = (a != (int)gr && d > 0) ? lv * (T(1) / T(d)) : T(0);  // a == gr: the dropped feature
        } else {
          cf_l = lv * p.inv1[t][a];
          if constexpr (FIX) cf_l = (T)((float)cf_l * scale);
        }
        if (cf_l != T(0)) { b_l = off[a]; n_l = off[a + 1] - b_l; }
      }
      const int cnt = __builtin_amdgcn_readfirstlane((le - g0 < 64) ? (le - g0) : 64);
      // ---- fold the sub-rows in, U at a time; the loads of the next U are in flight meanwhile
      // (this loop is also transfer_block_kernel's: as a shared function it changes the instructions of both)
      SubRows<T, U> A, B;
      auto load = [&](SubRows<T, U>& sr, int first) __attribute__((always_inline)) {
        if constexpr (BUF) {
          const __amdgpu_buffer_rsrc_t ridx = __builtin_amdgcn_make_buffer_rsrc((void*)midx, 0, -1, 0x00020000);
          const __amdgpu_buffer_rsrc_t rval = __builtin_amdgcn_make_buffer_rsrc((void*)mval, 0, -1, 0x00020000);
          subrows_load_buf<U, BINM>(sr, first, b_l, n_l, cf_l, ridx, rval, lane);
        } else {
          subrows_load<T, U, BINM>(sr, first, b_l, n_l, cf_l, midx, mval, lane);
        }
      };
      auto tail_ld = [&](unsigned e, unsigned short& j, T& v) __attribute__((always_inline)) {
        if constexpr (BUF) {
          const __amdgpu_buffer_rsrc_t ridx = __builtin_amdgcn_make_buffer_rsrc((void*)midx, 0, -1, 0x00020000);
          const __amdgpu_buffer_rsrc_t rval = __builtin_amdgcn_make_buffer_rsrc((void*)mval, 0, -1, 0x00020000);
          j = __builtin_amdgcn_raw_buffer_load_b16(ridx, (int)(e * 2u), 0, 0);
          v = BINM ? 1.f : __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rval, (int)(e * 4u), 0, 0));
        } else {
          j = midx[e];
          v = BINM ? T(1) : mval[e];
        }
      };
      Tails<T, (BINM ? 4 : (DUAL || FIX || BUF) ? 2 : 3)> tails;   // (3 was measured on the default family only)
      tails_begin(tails, a_l, b_l, n_l, cf_l, lane, tail_ld);
      load(A, 0);
      for (int u0 = 0; u0 < cnt; u0 += 2 * U) {
        if (u0 + U < cnt) load(B, u0 + U);
        subrows_fold_any<T, U, DUAL, FIX>(A, acc, astride, dummy, lane);
        if (u0 + U < cnt) {
          if (u0 + 2 * U < cnt) load(A, u0 + 2 * U);
          subrows_fold_any<T, U, DUAL, FIX>(B, acc, astride, dummy, lane);
        }
      }
      tails_finish<T, BINM, FIX>(tails, b_l, n_l, cf_l, acc, dummy, midx, mval, lane, tail_ld);
    }
  }
  if (LOO) {
    // sources that own the dropped feature column f_i: their degree is one lower in this fold
    const ChunkedView<T> M = p.M[0];
    const int* off = M.off + (int64_t)c * M.rows;
    for (int x = off[gr] + lane; x < off[gr + 1]; x += 64) {
      const int j = M.idx[x];
      if (j < p.SC) atomicOr(&bits[j >> 5], 1u << (j & 31));   // (not a tail's sentinel)
    }
  }
  __syncthreads();

  T* orow = p.out + r * p.ld + j0;
  for (int j = lane; j < jn; j += 64) {
    T z;
    T sum = DUAL ? acc[j] + acc[astride + j] : acc[j];
    if constexpr (FIX) sum = (T)((float)reinterpret_cast<const int*>(acc)[j] * fix_unscale);
    if (LOO) {
      const int d = p.ks[j0 + j] - (int)((bits[j >> 5] >> (j & 31)) & 1u);
      z = (d > 0 && (j0 + j) != gr) ? sum * (T(1) / T(d)) : T(0);
    } else {
      z = sum * p.inv2[j0 + j];
      if (p.accumulate) z += orow[j];
    }
    orow[j] = z;
  }
}

constexpr int TRANSFER_U = 8;

// SS_TRANSFER_DUAL=0/1: one or two copies of the LDS accumulators (see subrows_fold)
static bool transfer_dual() { return env_int("SS_TRANSFER_DUAL", 0) != 0; }

// sub-rows in flight per wave: 8.  Until the tails left the batch small weighted operands took 4, which
// reached 30 instead of 20 single-wave workgroups per CU (55 instead of 90 registers); now U = 8 holds 78 registers
// (24 workgroups per CU) and measures faster everywhere: C2 weighted 1.33 vs 1.37 ms, pattern-only 1.15 vs 1.19 ms
// (profiles/stage1_tails_time.json).  SS_TRANSFER_U overrides.
static int transfer_u() {
  const int u = (int)env_int("SS_TRANSFER_U", TRANSFER_U);
  return (u == 4 || u == 16) ? u : 8;
}

// ================================================================ query-block workgroups (round 3)
// Same product, same per-wave loop (U sub-rows in flight, plain LDS read-add-write), different workgroup: NW waves,
// one row of L per wave, all on chunk c.  What the single-wave kernel fetched per (row, feature) from L2 besides the
// sub-row itself -- off[a], off[a+1] (one 64-byte sector for 8 bytes) and inv1[a] (another sector for 4 bytes), i.e.
// ~130 of the ~600 bytes of L2 -> L1 traffic per sub-row visit -- is gone: the chunk's sub-row offsets ((rows+1) ints)
// are staged once per workgroup in LDS and read from there, and the coefficients L[r,a] * inv1[a] come from a
// coalesced array written by transfer_coef_kernel (one pass over L per launch).  The operand may be cut with
// sub-rows padded to 32 entries (64-byte index runs, 128-byte value runs: every sub-row starts on an L2 sector).
template <class T>
__global__ void transfer_coef_kernel(const int* __restrict__ ptr, const int* __restrict__ idx, const T* __restrict__ val,
                                     const T* __restrict__ inv1, int64_t row_begin, int64_t nrows, T* __restrict__ coef) {
  const int lo = ptr[row_begin], hi = ptr[row_begin + nrows];
  for (int64_t e = (int64_t)lo + (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < hi; e += (int64_t)gridDim.x * blockDim.x)
    coef[e] = val[e] * inv1[idx[e]];
}

// ---------------------------------------------------------------- what the block family shares
// LDS of a block-family workgroup: [offs: (rows + 1) ints, units of `align`] [lens: rows exact 16-bit lengths, the
// three kernels that walk exact lengths] [shared: wide's 64-byte identity list] then per wave [accumulators]
// [tables / lists of the wide kernels].  The launch sizes the workgroup from it, the kernel places its pointers with it.
enum { TB_PLAIN, TB_QFLAT, TB_WIDE, TB_WIDE2 };
constexpr int WIDE_META = 64 * 12;   // wide, bytes per wave: (start quad, length, coefficient) of 64 features
constexpr int WIDE_LIST = 64;        // wide, bytes per wave: features with entries left (one byte each)
constexpr int W2_TBL = 64 * 12;      // wide2: one table as above; a wave has two, and two x (list 1 [64], list 2 [64])
template <int KIND, class T>
struct BlockLayout {
  static constexpr bool EXACT = KIND != TB_PLAIN;
  static constexpr int shared_bytes = KIND == TB_WIDE ? 64 : 0;
  __host__ __device__ static int64_t offs_bytes(int64_t mrows) { return (((mrows + 1) * 4 + 15) / 16) * 16; }
  __host__ __device__ static int64_t lens_bytes(int64_t mrows) { return EXACT ? ((mrows * 2 + 15) / 16) * 16 : 0; }
  // a wave's sums: SC columns + 64 per-lane dummies, or (wide kernels) + the padding column SC, zero entries point at it
  __host__ __device__ static int acc_elems(int SC) { return SC + 64; }   // plain, qflat: in units of T
  __host__ __device__ static int acc_bytes(int SC) {
    return KIND == TB_WIDE || KIND == TB_WIDE2 ? (((SC + 4) * 4 + 15) / 16) * 16 : acc_elems(SC) * (int)sizeof(T);
  }
  __host__ __device__ static int per_wave(int SC) {
    return acc_bytes(SC) + (KIND == TB_WIDE ? WIDE_META + WIDE_LIST : KIND == TB_WIDE2 ? 2 * W2_TBL + 4 * 64 : 0);
  }
  // the region of wave `wave`, given the sizes of offs and lens the launch passed
  __device__ static unsigned char* wave_base(unsigned char* smem, int offs_b, int lens_b, int wave, int SC) {
    return smem + offs_b + lens_b + shared_bytes + (size_t)wave * (size_t)per_wave(SC);
  }
};

// What a wave knows after the prologue: its chunk c and columns j0 .. j0 + jn, its row r of the launch (gr of L) and
// that row's entries lb .. le.
struct BlockWave {
  int lane, c, jn, lb, le;
  int64_t r, gr, j0;
};

// Workgroup prologue: c = blockIdx % nchunks, row r = (blockIdx / nchunks) * nw + wave; the chunk's sub-row offsets
// (and exact lengths, EXACT) go to LDS, the wave's `nacc` accumulators are zeroed; then the only barrier.  Returns
// whether the wave has a row: one without leaves (the exit stays the kernel's own branch: inside this function it
// changes the block order of the kernels).
template <bool EXACT, class T, class A>
__device__ __forceinline__ bool block_prologue(BlockWave& w, const TransferArgs<T>& p, int64_t nrows, int wave, int* offs,
                                               unsigned short* lens, const unsigned short* glen, A* acc, int nacc) {
  const int nw = blockDim.x >> 6;
  w.lane = threadIdx.x & 63;
  w.c = blockIdx.x % p.nchunks;
  w.r = (int64_t)(blockIdx.x / p.nchunks) * nw + wave;
  const ChunkedView<T> M = p.M[0];
  {
    const int* __restrict__ off = M.off + (int64_t)w.c * M.rows;
    for (int64_t i = threadIdx.x; i <= M.rows; i += blockDim.x) offs[i] = off[i];
    if constexpr (EXACT) {
      const unsigned short* __restrict__ gl = glen + (int64_t)w.c * M.rows;
      for (int64_t i = threadIdx.x; i < M.rows; i += blockDim.x) lens[i] = gl[i];
    }
  }
  for (int j = w.lane; j < nacc; j += 64) acc[j] = A(0);
  __syncthreads();
  return w.r < nrows;
}
// ... and its row's bounds, in scalar registers (qflat; the block kernel reads them as vector values, the way it always
// did, and the two wide kernels keep their own prologue text)
template <class T>
__device__ __forceinline__ void block_row(BlockWave& w, const TransferArgs<T>& p) {
  w.gr = p.row_begin + w.r;
  w.j0 = (int64_t)w.c * p.SC;
  w.jn = (int)((p.nj - w.j0 < p.SC) ? (p.nj - w.j0) : p.SC);
  const int* lptr = p.L[0].ptr;
  w.lb = __builtin_amdgcn_readfirstlane(lptr[w.gr]);
  w.le = __builtin_amdgcn_readfirstlane(lptr[w.gr + 1]);
}

// fixed-point epilogue: the wave's integer sums back to T, times inv2 (the wave's own LDS operations execute in order:
// no barrier needed before it reads its sums back)
template <class T>
__device__ __forceinline__ void fixed_store(const TransferArgs<T>& p, int64_t r, int64_t j0, int jn, int lane, const void* acc,
                                            float unscale) {
  T* orow = p.out + r * p.ld + j0;
  const int* iacc = reinterpret_cast<const int*>(acc);
  for (int j = lane; j < jn; j += 64) orow[j] = (T)((float)iacc[j] * unscale) * p.inv2[j0 + j];
}

// ---- quads: 4 consecutive entries of a sub-row, one 8-byte index load + one 16-byte value load per lane
typedef float f4 __attribute__((ext_vector_type(4)));
typedef unsigned u2 __attribute__((ext_vector_type(2)));

// One ring slot: the coefficient, the index quad and the value quad.  Pattern-only operand (BINM): the values are not
// read, so the padding of a sub-row's last quad is masked here from `rem`, the entries of the sub-row in this quad (a
// stored padding value is 0, an implied one would be 1 -- added to the padding's column SC).
template <bool BINM>
__device__ __forceinline__ void quad_fetch(const u2* midx4, const f4* mval4, int quad, float cfv, int rem, u2& oj, f4& ov,
                                           float& ocf) {
  ocf = cfv;
  oj = midx4[quad];
  if constexpr (BINM) ov = f4{rem > 0 ? 1.f : 0.f, rem > 1 ? 1.f : 0.f, rem > 2 ? 1.f : 0.f, rem > 3 ? 1.f : 0.f};
  else ov = mval4[quad];
}
// Columns of different sub-rows may coincide inside one instruction, which only atomics get right.
__device__ __forceinline__ void quad_fold(unsigned* acc, u2 j, f4 v, float cf) {
  atomicAdd(acc + (j.x & 0xffffu), (unsigned)cvt_rpi(cf * v.x));
  atomicAdd(acc + (j.x >> 16), (unsigned)cvt_rpi(cf * v.y));
  atomicAdd(acc + (j.y & 0xffffu), (unsigned)cvt_rpi(cf * v.z));
  atomicAdd(acc + (j.y >> 16), (unsigned)cvt_rpi(cf * v.w));
}

// raw (feature, coefficient) pair of this lane in group g of the row; lanes past the end of the row get coefficient 0
__device__ __forceinline__ void raw_load(const int* lidx, const float* coef, int lb, int le, int lane, int g, int& a, float& cf) {
  const int q = lb + g * 64 + lane;
  a = 0;
  cf = 0.f;
  if (q < le) { a = lidx[q]; cf = coef[q]; }
}

// ---------------------------------------------------------------- the block kernel
template <class T, int U, bool BINM, bool FIX>
__global__ void __launch_bounds__(1024) transfer_block_kernel(TransferArgs<T> p, const T* __restrict__ coef, int64_t nrows,
                                                              int align, int offs_bytes, float xmax) {
  using Lay = BlockLayout<TB_PLAIN, T>;
  extern __shared__ __align__(16) unsigned char smem_raw[];
  int* offs = reinterpret_cast<int*>(smem_raw);                               // [rows + 1] sub-row offsets of chunk c
  const int wave = threadIdx.x >> 6;
  const int astride = p.SC + 64;
  T* acc = reinterpret_cast<T*>(smem_raw + offs_bytes) + (size_t)wave * Lay::acc_elems(p.SC);  // this wave's sums + per-lane dummies
  BlockWave w;
  if (!block_prologue<false>(w, p, nrows, wave, offs, nullptr, nullptr, acc, astride)) return;   // (after the only barrier)
  w.gr = p.row_begin + w.r;
  w.j0 = (int64_t)w.c * p.SC;
  w.jn = (int)((p.nj - w.j0 < p.SC) ? (p.nj - w.j0) : p.SC);
  const int lane = w.lane, lb = p.L[0].ptr[w.gr], le = p.L[0].ptr[w.gr + 1];
  const int dummy = p.SC + lane;
  const CsrView<T> L = p.L[0];
  const unsigned short* __restrict__ midx = p.M[0].idx;
  const T* __restrict__ mval = p.M[0].val;
  float scale = 1.f, unscale = 1.f;
  if constexpr (FIX) {
    const FixedScale fs = fixed_scale(lb, le, lane, xmax, [&](int q) __attribute__((always_inline)) { return fabsf((float)coef[q]); });
    scale = fs.scale;
    unscale = fs.unscale;
  }
  for (int g0 = lb; g0 < le; g0 += 64) {
    const int q = g0 + lane;
    int a_l = 0, b_l = 0, n_l = 0;
    T cf_l = T(0);
    if (q < le) {
      const int a = a_l = L.idx[q];
      cf_l = coef[q];
      if constexpr (FIX) cf_l = (T)((float)cf_l * scale);   // exact: a power of two
      if (cf_l != T(0)) {
        const int o0 = offs[a], o1 = offs[a + 1];
        b_l = o0 * align;
        n_l = (o1 - o0) * align;
      }
    }
    const int cnt = __builtin_amdgcn_readfirstlane((le - g0 < 64) ? (le - g0) : 64);
    SubRows<T, U> A, B;
    auto load = [&](SubRows<T, U>& sr, int first) __attribute__((always_inline)) {
      subrows_load<T, U, BINM>(sr, first, b_l, n_l, cf_l, midx, mval, lane);
    };
    auto tail_ld = [&](unsigned e, unsigned short& j, T& v) __attribute__((always_inline)) {
      j = midx[e];
      v = BINM ? T(1) : mval[e];
    };
    Tails<T, (BINM ? 4 : 2)> tails;
    tails_begin(tails, a_l, b_l, n_l, cf_l, lane, tail_ld);
    load(A, 0);
    for (int u0 = 0; u0 < cnt; u0 += 2 * U) {
      if (u0 + U < cnt) load(B, u0 + U);
      subrows_fold_any<T, U, false, FIX>(A, acc, astride, dummy, lane);
      if (u0 + U < cnt) {
        if (u0 + 2 * U < cnt) load(A, u0 + 2 * U);
        subrows_fold_any<T, U, false, FIX>(B, acc, astride, dummy, lane);
      }
    }
    tails_finish<T, BINM, FIX>(tails, b_l, n_l, cf_l, acc, dummy, midx, mval, lane, tail_ld);
  }
  if constexpr (FIX) {
    fixed_store(p, w.r, w.j0, w.jn, lane, acc, unscale);
  } else {
    T* orow = p.out + w.r * p.ld + w.j0;
    for (int j = lane; j < w.jn; j += 64) orow[j] = acc[j] * p.inv2[w.j0 + j];
  }
}

// ---------------------------------------------------------------- stage 1, flat stream of quads (round 3, measured variant)
// Workgroup as in transfer_block_kernel (NW waves = NW rows of L on chunk c; the chunk's sub-row offsets AND exact
// sub-row lengths staged in LDS; coefficients precomputed).  The entries of the 64 sub-rows of a feature group are walked
// as ONE stream of QUADS (4 consecutive entries of a sub-row, the last quad of a sub-row padded with zero entries) in
// steps of 64 quads = 256 entries ~ four 62-entry sub-rows: lane l of step t takes stream position 64 t + l, whichever
// sub-row it falls into -- no half-empty second halves.  One global_load_dwordx4 (values) + one global_load_dwordx2
// (indices) per step; a step holds entries of several features, whose columns can coincide: only safe because the sums
// are integer atomics (ds_add_u32 on 2^k-scaled fixed-point products, see subrows_fold_fixed).  Per step: the owner of
// the first lane (popcount of a ballot), then one select per sub-row boundary inside the step, all from wave-uniform
// broadcasts.  Steps run through a ring of D slots, every load unconditional.  Measured (C2): 2.04 ms -- the boundary
// loop's readlane -> scalar -> select chains make a step ~1900 clk per wave.
template <class T, int D, bool BINM>
__global__ void __launch_bounds__(1024) transfer_qflat_kernel(TransferArgs<T> p, const T* __restrict__ coef, int64_t nrows,
                                                             int align, int offs_bytes, int lens_bytes, float xmax,
                                                             const unsigned short* __restrict__ glen) {
  static_assert(std::is_same<T, float>::value, "fixed-point sums: fp32 graphs only");
  extern __shared__ __align__(16) unsigned char smem_raw[];
  int* offs = reinterpret_cast<int*>(smem_raw);                                        // [rows + 1], units of `align`
  unsigned short* lens = reinterpret_cast<unsigned short*>(smem_raw + offs_bytes);     // [rows] exact entries
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int astride = p.SC + 64;
  unsigned* acc = reinterpret_cast<unsigned*>(BlockLayout<TB_QFLAT, T>::wave_base(smem_raw, offs_bytes, lens_bytes, wave, p.SC));
  BlockWave w;
  if (!block_prologue<true>(w, p, nrows, wave, offs, lens, glen, acc, astride)) return;
  block_row(w, p);
  const ChunkedView<T> M = p.M[0];
  const CsrView<T> L = p.L[0];
  const int64_t r = w.r, j0 = w.j0;
  const int jn = w.jn, lb = w.lb, le = w.le;
  const unsigned short* __restrict__ midx = M.idx;
  const T* __restrict__ mval = M.val;
  // (own text of fixed_scale and raw_load: as calls they change this kernel's step loop)
  // scale 2^k of the row's sums: bound = (sum |coef|) * xmax < 2^e, k = 30 - e (see transfer_block_kernel)
  float scale, unscale;
  {
    float sabs = 0.f;
    for (int q = lb + lane; q < le; q += 64) sabs += fabsf(coef[q]);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) sabs += __shfl_xor(sabs, o);
    int e = 0;
    (void)frexpf(sabs * xmax, &e);
    if (!(sabs * xmax > 0.f)) e = 0;
    e = e < -90 ? -90 : (e > 120 ? 120 : e);
    scale = ldexpf(1.f, 30 - e);
    unscale = ldexpf(1.f, e - 30);
  }
  const int ngroups = (le - lb + 63) >> 6;
  auto raw_load = [&](int g, int& a, float& cf) __attribute__((always_inline)) {
    const int q = lb + g * 64 + lane;
    a = 0;
    cf = 0.f;
    if (q < le) { a = L.idx[q]; cf = coef[q]; }
  };
  // sub-row of feature a in this chunk: start (entries) and exact length, from LDS; nothing for a zero coefficient
  auto meta = [&](int a, float cf, int& b_l, int& n_l, float& cf_l) __attribute__((always_inline)) {
    cf_l = cf * scale;   // exact: a power of two
    b_l = 0;
    n_l = 0;
    if (cf_l != 0.f) {
      b_l = (offs[a] * align) >> 2;        // start in quads (sub-rows start on 32-entry boundaries)
      n_l = ((int)lens[a] + 3) >> 2;       // length in quads; the last quad is padded with zero entries
    }
  };
  // current group: per lane i the stream start P_i of its sub-row, delta_i = start in memory - P_i, coefficient
  int Pc = 0, dc = 0, ra, bn, nn;
  float cc = 0.f, cn, rc;
  int total = 0, nst = 0, t = 0, gcur = -1;
  raw_load(0, ra, rc); meta(ra, rc, bn, nn, cn);
  raw_load(1, ra, rc);
  bool done = false;
  auto switch_group = [&]() __attribute__((always_inline)) {
    // the prepared next group becomes current: exclusive prefix sum of the lengths over the 64 lanes
    ++gcur;
    int incl = nn;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const int up = __shfl_up(incl, o);
      if (lane >= o) incl += up;
    }
    Pc = incl - nn;
    dc = bn - Pc;
    cc = cn;
    total = __builtin_amdgcn_readlane(incl, 63);
    nst = (total + 63) >> 6;
    t = 0;
    meta(ra, rc, bn, nn, cn);            // group gcur + 1 (its raw pairs were requested a group ago)
    raw_load(gcur + 2, ra, rc);
  };
  u2 sj[D];
  f4 sv[D];
  float sc[D];
  const f4* __restrict__ mval4 = reinterpret_cast<const f4*>(mval);
  const u2* __restrict__ midx4 = reinterpret_cast<const u2*>(midx);
  auto next_step = [&](u2& oj, f4& ov, float& ocf) __attribute__((always_inline)) {
    if (t >= nst) {
      if (gcur + 1 < ngroups) switch_group();   // (may land on a group without entries: a null step, next call moves on)
      else done = true;
    }
    float cfv = 0.f;
    int addr = lane;   // lanes without work add 0 to different columns (same-address atomics serialise)
    if (t < nst) {
      const int lo = t << 6;
      const int pos = lo + lane;
      const unsigned long long le_mask = __ballot(Pc <= lo);
      const int own0 = __builtin_popcountll(le_mask) - 1;                 // last sub-row that starts at or before lo
      unsigned long long m = __ballot(Pc > lo && Pc <= lo + 63);          // sub-rows that start inside the step
      cfv = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(cc), own0));
      int dlv = __builtin_amdgcn_readlane(dc, own0);
      while (m != 0ull) {
        const int i = __builtin_ctzll(m);
        m &= m - 1ull;
        const int Pi = __builtin_amdgcn_readlane(Pc, i);
        const float cfi = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(cc), i));
        const int dli = __builtin_amdgcn_readlane(dc, i);
        const bool in = pos >= Pi;
        cfv = in ? cfi : cfv;
        dlv = in ? dli : dlv;
      }
      const bool valid = pos < total;
      cfv = valid ? cfv : 0.f;
      addr = valid ? pos + dlv : lane;
      ++t;
    }
    quad_fetch<BINM>(midx4, mval4, addr, cfv, 4, oj, ov, ocf);   // (the padding of a last quad is in memory: no mask)
  };
#pragma unroll
  for (int i = 0; i < D; ++i) next_step(sj[i], sv[i], sc[i]);
  while (!done) {
#pragma unroll
    for (int i = 0; i < D; ++i) {
      quad_fold(acc, sj[i], sv[i], sc[i]);
      next_step(sj[i], sv[i], sc[i]);
    }
  }
#pragma unroll
  for (int i = 0; i < D; ++i) quad_fold(acc, sj[i], sv[i], sc[i]);
  fixed_store(p, r, j0, jn, lane, acc, unscale);
}

// ---------------------------------------------------------------- stage 1, wide loads + fixed-point sums (round 3)
// What the counters of the single-wave kernel say (profiles/r03_stage1_mem_pmc.txt): its 2- and 4-byte-per-lane loads
// cost the vector L1 ~6 accesses each (TCP_TOTAL_CACHE_ACCESSES ~0.8 per cycle and CU, TA busy 92 %), its LDS
// read-add-write pairs keep the LDS 64 % busy, and a wave needs ~400 clk per sub-row (readlane -> scalar -> address
// chains, one LDS round trip per fold).  This kernel removes all three:
//  * 16 bytes per lane: 16 lanes share a sub-row, lane e takes its entries 4e .. 4e+3 -- ONE global_load_dwordx4
//    (values) + ONE global_load_dwordx2 (indices) fetch the first 64 entries of FOUR sub-rows;
//  * sums are 2^k-scaled integers added with ds_add_u32 (half the LDS cycles of the pair, no return value, no wait;
//    columns of different sub-rows may coincide inside one instruction, which only atomics get right; integer sums do
//    not depend on any order);
//  * no per-sub-row scalar work: a wave writes (start, length, coefficient) of its 64 current features to a small LDS
//    table once per group and every lane reads its sub-row's triple from there (one ds_read per step).
// Entries past the first 64 of a sub-row (40 % of the sub-rows have some, ~8 on average) are taken afterwards, 4 lanes
// (16 entries) per sub-row and step, through a list of the features that still have entries left.
// Workgroup = NW waves = NW rows of L on chunk c; sub-row offsets and exact lengths of the chunk staged in LDS;
// coefficients precomputed (transfer_coef_kernel); steps run through a ring of D slots, every load unconditional.
template <int D, bool BINM>
__global__ void __launch_bounds__(1024) transfer_wide_kernel(TransferArgs<float> p, const float* __restrict__ coef,
                                                             int64_t nrows, int align, int offs_bytes, int lens_bytes,
                                                             float xmax, const unsigned short* __restrict__ glen) {
  extern __shared__ __align__(16) unsigned char smem_raw[];
  int* offs = reinterpret_cast<int*>(smem_raw);
  unsigned short* lens = reinterpret_cast<unsigned short*>(smem_raw + offs_bytes);
  unsigned char* ident = smem_raw + offs_bytes + lens_bytes;                 // [64] identity list (first 64 entries: all features)
  const int lane = threadIdx.x & 63, nw = blockDim.x >> 6;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  using Lay = BlockLayout<TB_WIDE, float>;
  const int accb = Lay::acc_bytes(p.SC);
  unsigned char* mine = Lay::wave_base(smem_raw, offs_bytes, lens_bytes, wave, p.SC);
  unsigned* acc = reinterpret_cast<unsigned*>(mine);
  unsigned char* metab = mine + accb;                                        // [64][12]
  unsigned char* list = metab + WIDE_META;                                   // [64]
  // (own text of block_prologue / block_row and, at the end, fixed_store: as calls they change the D = 4 loop)
  const int c = blockIdx.x % p.nchunks;
  const int64_t r = (int64_t)(blockIdx.x / p.nchunks) * nw + wave;
  const ChunkedView<float> M = p.M[0];
  const CsrView<float> L = p.L[0];
  {
    const int* __restrict__ off = M.off + (int64_t)c * M.rows;
    const unsigned short* __restrict__ gl = glen + (int64_t)c * M.rows;
    for (int64_t i = threadIdx.x; i <= M.rows; i += blockDim.x) offs[i] = off[i];
    for (int64_t i = threadIdx.x; i < M.rows; i += blockDim.x) lens[i] = gl[i];
    if (threadIdx.x < 64) ident[threadIdx.x] = (unsigned char)threadIdx.x;
  }
  for (int j = lane; j < p.SC; j += 64) acc[j] = 0u;
  __syncthreads();
  if (r >= nrows) return;
  const int64_t gr = p.row_begin + r;
  const int64_t j0 = (int64_t)c * p.SC;
  const int jn = (int)((p.nj - j0 < p.SC) ? (p.nj - j0) : p.SC);
  const int lb = __builtin_amdgcn_readfirstlane(L.ptr[gr]), le = __builtin_amdgcn_readfirstlane(L.ptr[gr + 1]);
  const FixedScale fs = fixed_scale(lb, le, lane, xmax, [&](int q) __attribute__((always_inline)) { return fabsf(coef[q]); });
  const float scale = fs.scale, unscale = fs.unscale;
  const int ngroups = (le - lb + 63) >> 6;
  const f4* __restrict__ mval4 = reinterpret_cast<const f4*>(M.val);
  const u2* __restrict__ midx4 = reinterpret_cast<const u2*>(M.idx);
  // ---- generator state (wave-uniform): group, level (0: entries 0..63, 16 lanes per sub-row; h >= 1: entries
  // 64 + 16 (h-1) .. +15, 4 lanes per sub-row), step inside the level
  int gcur = -1, level = 0, st = 0, nst = 0, nlist = 0, qoff = 0;
  int ncur = 0;            // lane i: length of the sub-row of feature i of the current group
  int ra;
  float rc;
  raw_load(L.idx, coef, lb, le, lane, 0, ra, rc);
  bool done = false;
  auto open_group = [&]() __attribute__((always_inline)) {
    // the raw (feature, coefficient) pairs of this group are here; those of the next group are requested now
    ++gcur;
    const float cf = rc * scale;   // exact: a power of two
    int b = 0, n = 0;
    if (cf != 0.f) { b = (offs[ra] * align) >> 2; n = (int)lens[ra]; }
    raw_load(L.idx, coef, lb, le, lane, gcur + 1, ra, rc);
    ncur = n;
    unsigned* m = reinterpret_cast<unsigned*>(metab + lane * 12);
    m[0] = (unsigned)b; m[1] = (unsigned)n; m[2] = __float_as_uint(cf);
    level = 0;
    st = 0;
    qoff = 0;
    const int cnt = (le - lb - gcur * 64 < 64) ? (le - lb - gcur * 64) : 64;
    nlist = cnt;
    nst = (cnt + 3) >> 2;          // four sub-rows per step
  };
  auto next_level = [&]() __attribute__((always_inline)) {
    // features that still have entries: level 1 starts at entry 64, each further level 16 entries on
    const int covered = 64 + 16 * level;
    ++level;
    qoff = covered >> 2;
    const bool more = ncur > covered;
    const unsigned long long mk = __ballot(more);
    nlist = __builtin_popcountll(mk);
    if (more) list[__builtin_amdgcn_mbcnt_hi((unsigned)(mk >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)mk, 0u))] = (unsigned char)lane;
    st = 0;
    nst = (nlist + 15) >> 4;       // sixteen sub-rows per step
  };
  u2 sj[D];
  f4 sv[D];
  float sc[D];
  auto next_step = [&](u2& oj, f4& ov, float& ocf) __attribute__((always_inline)) {
    if (st >= nst) {
      if (gcur >= 0 && nlist > 0) next_level();          // (an empty level: nst = 0, handled by the next call)
      else if (gcur + 1 < ngroups) open_group();
      else done = true;
    }
    float cfv = 0.f;
    int quad = lane;   // lanes without work add 0 to 64 DIFFERENT columns (64 lanes adding to one LDS word serialise)
    int rem = 0;       // entries of the sub-row in this lane's quad (the last quad of a sub-row ends in padding)
    if (st < nst) {
      const int sh = level == 0 ? 4 : 2;                 // log2(lanes per sub-row)
      const int pos = (st << (6 - sh)) + (lane >> sh);   // position in the list of features of this level
      const int e = lane & ((1 << sh) - 1);
      const unsigned char* lst = level == 0 ? ident : list;
      const int fi = pos < nlist ? (int)lst[pos] : 0;
      const unsigned* m = reinterpret_cast<const unsigned*>(metab + fi * 12);
      const int b = (int)m[0], n = (int)m[1];
      const float cf = __uint_as_float(m[2]);
      const int qe = qoff + e;                           // quad of the sub-row this lane takes
      const bool valid = pos < nlist && 4 * qe < n;
      cfv = valid ? cf : 0.f;
      quad = valid ? b + qe : lane;
      rem = n - 4 * qe;
      ++st;
    }
    quad_fetch<BINM>(midx4, mval4, quad, cfv, rem, oj, ov, ocf);
  };
#pragma unroll
  for (int i = 0; i < D; ++i) next_step(sj[i], sv[i], sc[i]);
  while (!done) {
#pragma unroll
    for (int i = 0; i < D; ++i) {
      quad_fold(acc, sj[i], sv[i], sc[i]);
      next_step(sj[i], sv[i], sc[i]);
    }
  }
#pragma unroll
  for (int i = 0; i < D; ++i) quad_fold(acc, sj[i], sv[i], sc[i]);
  float* orow = p.out + r * p.ld + j0;
  const int* iacc = reinterpret_cast<const int*>(acc);
  for (int j = lane; j < jn; j += 64) orow[j] = ((float)iacc[j] * unscale) * p.inv2[j0 + j];
}

// ---------------------------------------------------------------- stage 1, wide loads, static schedule (round 3)
// transfer_wide_kernel without its step generator (whose scalar control flow cost ~45 instructions and two dependent LDS
// reads per step: 1.2 ms of the 1.8 ms with loads and atomics removed).  A group of 64 features is ALWAYS 20 steps:
//   steps  0..15  entries  0..63 of features 4s .. 4s+3        (16 lanes x 4 entries per sub-row)
//   steps 16..18  entries 64..79 of the features that have them (4 lanes per sub-row, 16 features per step, from list 1)
//   step  19      entries 80..95 of the features that have them (list 2)
// so the whole row is one straight-line software pipeline: the loop body is one group, completely unrolled, LDS table
// reads use immediate offsets, a ring of 4 slots carries the loads across steps and across groups (the table of the
// next group is written -- into the other of two buffers -- four steps before the current group ends), every load is
// unconditional and the waits are exact counts.  What the 20 steps cannot hold (a 49th feature longer than 64 entries,
// a 17th longer than 80, entries past 96; ~1e-4 of the sub-rows at a mean of 62) is added by the owning lane itself,
// entry by entry, when the table is written.
constexpr int W2_STEPS = 20;
constexpr int W2_D = 4;
template <bool BINM>
__global__ void __launch_bounds__(1024) transfer_wide2_kernel(TransferArgs<float> p, const float* __restrict__ coef,
                                                              int64_t nrows, int align, int offs_bytes, int lens_bytes,
                                                              float xmax, const unsigned short* __restrict__ glen) {
  extern __shared__ __align__(16) unsigned char smem_raw[];
  int* offs = reinterpret_cast<int*>(smem_raw);
  unsigned short* lens = reinterpret_cast<unsigned short*>(smem_raw + offs_bytes);
  const int lane = threadIdx.x & 63, nw = blockDim.x >> 6;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  using Lay = BlockLayout<TB_WIDE2, float>;
  const int accb = Lay::acc_bytes(p.SC);
  unsigned char* mine = Lay::wave_base(smem_raw, offs_bytes, lens_bytes, wave, p.SC);
  unsigned* acc = reinterpret_cast<unsigned*>(mine);
  unsigned char* tbl0 = mine + accb;                      // two tables [64][12]: (start quad, length, coefficient)
  unsigned char* lst0 = tbl0 + 2 * W2_TBL;                // two x (list 1 [64], list 2 [64])
  // (own text of block_prologue / block_row, and raw_load below in its clamped form)
  const int c = blockIdx.x % p.nchunks;
  const int64_t r = (int64_t)(blockIdx.x / p.nchunks) * nw + wave;
  const ChunkedView<float> M = p.M[0];
  const CsrView<float> L = p.L[0];
  {
    const int* __restrict__ off = M.off + (int64_t)c * M.rows;
    const unsigned short* __restrict__ gl = glen + (int64_t)c * M.rows;
    for (int64_t i = threadIdx.x; i <= M.rows; i += blockDim.x) offs[i] = off[i];
    for (int64_t i = threadIdx.x; i < M.rows; i += blockDim.x) lens[i] = gl[i];
  }
  for (int j = lane; j < p.SC; j += 64) acc[j] = 0u;
  __syncthreads();
  if (r >= nrows) return;
  const int64_t gr = p.row_begin + r;
  const int64_t j0 = (int64_t)c * p.SC;
  const int jn = (int)((p.nj - j0 < p.SC) ? (p.nj - j0) : p.SC);
  const int lb = __builtin_amdgcn_readfirstlane(L.ptr[gr]), le = __builtin_amdgcn_readfirstlane(L.ptr[gr + 1]);
  const FixedScale fs = fixed_scale(lb, le, lane, xmax, [&](int q) __attribute__((always_inline)) { return fabsf(coef[q]); });
  const float scale = fs.scale, unscale = fs.unscale;
  const int ngroups = (le - lb + 63) >> 6;
  const f4* __restrict__ mval4 = reinterpret_cast<const f4*>(M.val);
  const u2* __restrict__ midx4 = reinterpret_cast<const u2*>(M.idx);
  const unsigned short* __restrict__ midx = M.idx;
  const float* __restrict__ mval = M.val;
  const int lastq = le > lb ? le - 1 : lb;   // (an empty row never dereferences: ngroups == 0)
  // raw (feature, coefficient) pair of this lane in group g; lanes past the end of the row get coefficient 0.
  // Unconditional loads from a clamped position: no branch, exact wait counts.
  auto raw_load = [&](int g, int& a, float& cf) __attribute__((always_inline)) {
    const int q = lb + g * 64 + lane;
    const int qc = q < le ? q : lastq;
    a = L.idx[qc];
    const float x = coef[qc];
    cf = q < le ? x : 0.f;
  };
  // write the table + lists of group g (its raw pair is in (ra, rc)) into buffer g & 1; request the raw pair of g + 1
  int ra = 0;
  float rc = 0.f;
  auto open_group = [&](int g) __attribute__((always_inline)) {
    unsigned char* tb = tbl0 + (g & 1) * W2_TBL;
    unsigned char* l1 = lst0 + (g & 1) * 128;
    unsigned char* l2 = l1 + 64;
    const float cf = (g < ngroups) ? rc * scale : 0.f;   // exact: a power of two
    int b = 0, n = 0;
    if (cf != 0.f) { b = (offs[ra] * align) >> 2; n = (int)lens[ra]; }
    raw_load(g + 1, ra, rc);                            // (clamped past the end of the row: always safe, never a branch)
    unsigned* m = reinterpret_cast<unsigned*>(tb + lane * 12);
    m[0] = (unsigned)b; m[1] = (unsigned)n; m[2] = __float_as_uint(cf);
    // list 1 holds the first 48 features longer than 64 entries (steps 16..18), list 2 the first 16 of THOSE that are
    // longer than 80 (step 19): a feature that found no place in list 1 must not appear in list 2 -- its owner adds
    // everything past entry 64 itself, and step 19 would add entries 80..95 a second time
    const unsigned long long m1 = __ballot(n > 64);
    const int r1 = __builtin_amdgcn_mbcnt_hi((unsigned)(m1 >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)m1, 0u));
    const bool in1 = n > 64 && r1 < 48;
    const unsigned long long m2 = __ballot(in1 && n > 80);
    const int r2 = __builtin_amdgcn_mbcnt_hi((unsigned)(m2 >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)m2, 0u));
    const bool in2 = in1 && n > 80 && r2 < 16;
    l1[lane] = 255; l2[lane] = 255;                      // 255 = no feature at this list position
    if (in1) l1[r1] = (unsigned char)lane;
    if (in2) l2[r2] = (unsigned char)lane;
    // the rare rest: entries the 20 steps do not reach, added by the owning lane
    const int cov = in2 ? 96 : (in1 ? 80 : 64);
    if (__ballot(n > cov) != 0ull) {
      for (int x = cov; x < n; ++x) {
        const int at = 4 * b + x;
        atomicAdd(acc + midx[at], (unsigned)cvt_rpi(cf * (BINM ? 1.f : mval[at])));
      }
    }
  };
  // ---- the ring
  u2 sj[W2_D];
  f4 sv[W2_D];
  float sc[W2_D];
  // step s (compile-time after unrolling) of the group whose table sits in buffer `par`
  auto gen = [&](int s, int par, u2& oj, f4& ov, float& ocf) __attribute__((always_inline)) {
    const unsigned char* tb = tbl0 + par * W2_TBL;
    int fi, e, qoff;
    bool have = true;
    if (s < 16) {
      fi = 4 * s + (lane >> 4);
      e = lane & 15;
      qoff = 0;
    } else {
      const unsigned char* lst = lst0 + par * 128 + (s < 19 ? 0 : 64);
      const int pos = (s < 19 ? 16 * (s - 16) : 0) + (lane >> 2);
      fi = (int)lst[pos];
      have = fi != 255;
      fi = have ? fi : 0;
      e = lane & 3;
      qoff = s < 19 ? 16 : 20;
    }
    const unsigned* m = reinterpret_cast<const unsigned*>(tb + fi * 12);
    const int b = (int)m[0], n = (int)m[1];
    const float cf = __uint_as_float(m[2]);
    const int qe = qoff + e;
    const bool valid = have && 4 * qe < n;
    // lanes without work add 0 to 64 DIFFERENT columns (many lanes adding to one LDS word serialise)
    quad_fetch<BINM>(midx4, mval4, valid ? b + qe : lane, valid ? cf : 0.f, n - 4 * qe, oj, ov, ocf);
  };
  if (ngroups > 0) {
    raw_load(0, ra, rc);
    open_group(0);
#pragma unroll
    for (int i = 0; i < W2_D; ++i) gen(i, 0, sj[i], sv[i], sc[i]);
    for (int g = 0; g < ngroups; ++g) {
      const int par = g & 1;
#pragma unroll
      for (int s = 0; s < W2_STEPS; ++s) {
        if (s == W2_STEPS - W2_D) open_group(g + 1);     // (past the last group: an empty table, all steps idle)
        quad_fold(acc, sj[s % W2_D], sv[s % W2_D], sc[s % W2_D]);
        if (s + W2_D < W2_STEPS) gen(s + W2_D, par, sj[s % W2_D], sv[s % W2_D], sc[s % W2_D]);
        else gen(s + W2_D - W2_STEPS, par ^ 1, sj[s % W2_D], sv[s % W2_D], sc[s % W2_D]);
      }
    }
    // the ring now holds the first steps of the (empty) group past the end: nothing left to add
  }
  fixed_store(p, r, j0, jn, lane, acc, unscale);
}

// ================================================================ launches
// waves per workgroup of a block-family kernel that fit next to the chunk's tables: 0 = does not fit (fall back)
template <int KIND, class T>
static int transfer_block_waves(int64_t mrows, int SC) {
  using Lay = BlockLayout<KIND, T>;
  const int64_t fixed_bytes = Lay::offs_bytes(mrows) + Lay::lens_bytes(mrows) + Lay::shared_bytes;
  const int64_t room = (int64_t)ctx().lds_per_block - fixed_bytes;
  int64_t nw = room > 0 ? room / Lay::per_wave(SC) : 0;
  if (nw > 16) nw = 16;
  nw = env_int_in("SS_TRANSFER_NW", 1, nw, nw);
  return nw >= 8 ? (int)nw : 0;
}

template <class T>
bool transfer_block_fits(int64_t mrows, int SC) {
  return transfer_block_waves<TB_PLAIN, T>(mrows, SC) > 0;
}

// nw rows of L per workgroup, LDS from the kernel's layout
template <int KIND, auto Kernel, class T>
static int launch_block_kernel(const TransferArgs<T>& p, const DevChunked<T>& Mt, const T* coef, int64_t nrows, int nw,
                               float xmax) {
  using Lay = BlockLayout<KIND, T>;
  const int offs_bytes = (int)Lay::offs_bytes(Mt.rows), lens_bytes = (int)Lay::lens_bytes(Mt.rows);
  const unsigned grid = (unsigned)(ceil_div(nrows, (int64_t)nw) * p.nchunks);
  const size_t lds = (size_t)offs_bytes + (size_t)lens_bytes + Lay::shared_bytes + (size_t)nw * (size_t)Lay::per_wave(p.SC);
  if constexpr (Lay::EXACT)
    return launch_lds<Kernel>(grid, 64 * nw, lds, p, coef, nrows, Mt.align, offs_bytes, lens_bytes, xmax,
                              (const unsigned short*)Mt.len.p);
  else
    return launch_lds<Kernel>(grid, 64 * nw, lds, p, coef, nrows, Mt.align, offs_bytes, xmax);
}

template <class T>
int launch_transfer_block(const DevCsr<T>& L, const T* inv1, const DevChunked<T>& Mt, const T* inv2, int64_t row_begin,
                          int64_t nrows, int64_t nj, T* out, int64_t ld, T* coef, float xmax, bool fixed) {
  if (nrows <= 0 || nj <= 0) return SS_OK;
  const int nw = transfer_block_waves<TB_PLAIN, T>(Mt.rows, Mt.SC);
  if (nw == 0) return fail(SS_EUNSUPPORTED, "transfer_block: offsets + accumulators do not fit in LDS");
  TransferArgs<T> p{};
  p.nterms = 1;
  p.L[0] = view(L);
  p.M[0] = view(Mt);
  p.inv2 = inv2;
  p.row_begin = row_begin;
  p.nj = nj;
  p.SC = Mt.SC;
  p.nchunks = Mt.nchunks;
  p.out = out;
  p.ld = ld;
  if (ceil_div(nrows, (int64_t)nw) * p.nchunks >= (1LL << 31))
    return fail(SS_EUNSUPPORTED, "transfer grid too large; lower SS_TRANSFER_BYTES");
  path_add("transfer_block");
  hipLaunchKernelGGL(transfer_coef_kernel<T>, dim3(grid_1d(L.nnz > 0 ? L.nnz : 1, 256, 256 * 8)), dim3(256), 0, ctx().stream,
                     L.ptr.p, L.idx.p, L.val.p, inv1, row_begin, nrows, coef);
  SS_LAUNCH_CHECK();
  constexpr bool CANFIX = std::is_same<T, float>::value;
  const bool fx = CANFIX && fixed;
  if (fx) path_add("fixed_point");
  const bool binm = Mt.binary;
  if constexpr (CANFIX) {
    // the fixed-point kernels with 16 bytes per lane: they walk exact sub-row lengths (operand cut with align 32).
    // wide2 over wide over qflat; the one asked for runs if >= 8 of its waves fit, else the block kernel below.
    const int wide2 = (int)env_int("SS_TRANSFER_WIDE2", 0), wide = (int)env_int("SS_TRANSFER_WIDE", 0),
              qflat = (int)env_int("SS_TRANSFER_QFLAT", 0);
    if ((wide2 > 0 || wide > 0 || qflat > 0) && fixed && Mt.align == 32 && Mt.len_ok) {
      if (wide2 > 0) {
        if (const int n = transfer_block_waves<TB_WIDE2, T>(Mt.rows, Mt.SC)) {
          path_add("wide2");
          return dispatch_bool(binm, [&](auto B) {
            return launch_block_kernel<TB_WIDE2, transfer_wide2_kernel<decltype(B)::value>>(p, Mt, coef, nrows, n, xmax);
          });
        }
      } else if (wide > 0) {
        if (const int n = transfer_block_waves<TB_WIDE, T>(Mt.rows, Mt.SC)) {
          path_add("wide");
          return dispatch_int<2, 4>(wide == 2 ? 2 : 4, [&](auto D) {
            return dispatch_bool(binm, [&](auto B) {
              return launch_block_kernel<TB_WIDE, transfer_wide_kernel<decltype(D)::value, decltype(B)::value>>(
                  p, Mt, coef, nrows, n, xmax);
            });
          });
        }
      } else if (const int n = transfer_block_waves<TB_QFLAT, T>(Mt.rows, Mt.SC)) {
        path_add("qflat");
        return dispatch_bool(binm, [&](auto B) {
          return launch_block_kernel<TB_QFLAT, transfer_qflat_kernel<float, 4, decltype(B)::value>>(p, Mt, coef, nrows, n, xmax);
        });
      }
    }
  }
  return dispatch_int<4, 8>(transfer_u() == 4 ? 4 : 8, [&](auto U) {
    return dispatch_bool(binm, [&](auto B) {
      return dispatch_bool(fx, [&](auto F) {
        constexpr bool FIX = CANFIX && decltype(F)::value;   // (fx is never set for fp64)
        return launch_block_kernel<TB_PLAIN, transfer_block_kernel<T, decltype(U)::value, decltype(B)::value, FIX>>(
            p, Mt, coef, nrows, nw, xmax);
      });
    });
  });
}

// ---------------------------------------------------------------- coefficient tables of the single-wave kernel
// One workgroup per row of L (the leave-one-out coefficient needs the row of an entry), entries 256 at a time: every
// load but the degree gather is coalesced.  The expressions are transfer_kernel's own, so the bits are too.
template <class T, bool LOO>
__global__ void __launch_bounds__(256) transfer_coef_rows_kernel(CsrView<T> L, const T* __restrict__ inv1,
                                                                 const int* __restrict__ kf, int64_t nrows,
                                                                 T* __restrict__ coef) {
  for (int64_t r = blockIdx.x; r < nrows; r += gridDim.x) {
    const int lb = L.ptr[r], le = L.ptr[r + 1];
    for (int q = lb + (int)threadIdx.x; q < le; q += 256) {
      const int a = L.idx[q];
      const T lv = L.val[q];
      if (LOO) {
        const int d = kf[a] - 1;
        coef[q] = (a != (int)r && d > 0) ? lv * (T(1) / T(d)) : T(0);
      } else {
        coef[q] = lv * inv1[a];
      }
    }
  }
}

template <class T>
int transfer_coef_build(const DevCsr<T>& L, const T* inv1, const int* kf_loo, T* coef) {
  if (L.rows <= 0 || L.nnz <= 0) return SS_OK;
  const unsigned grid = (unsigned)(L.rows < 65536 ? L.rows : 65536);
  if (kf_loo)
    hipLaunchKernelGGL((transfer_coef_rows_kernel<T, true>), dim3(grid), dim3(256), 0, ctx().stream, view(L), inv1, kf_loo,
                       L.rows, coef);
  else
    hipLaunchKernelGGL((transfer_coef_rows_kernel<T, false>), dim3(grid), dim3(256), 0, ctx().stream, view(L), inv1, kf_loo,
                       L.rows, coef);
  SS_LAUNCH_CHECK();
  return SS_OK;
}

// SS_TRANSFER_COEF: 0 = gather the coefficients (the kernels before the tables), unset / 1 = tables, 2 = tables and the
// tag coef_table in the path note
static int transfer_coef_mode() {
  const int m = (int)env_int("SS_TRANSFER_COEF", 1);
  return m == 0 ? 0 : (m == 2 ? 2 : 1);
}

// The single-wave kernel, by (U, BINM, DUAL); fp32 query / source rows with one accumulator copy also by FIX
// (SS_TRANSFER_FIX1=1: a single term that does not accumulate) and BUF (SS_TRANSFER_LD=1), where U is 4 or 8.  The
// default family (U 4 or 8, none of DUAL / FIX / BUF) reads coefficient tables when the caller passed one per term.
template <class T, bool LOO>
static int launch_transfer_variant(const TransferArgs<T>& p, unsigned grid, size_t lds, bool binm, bool dual) {
  auto launch = [&](auto kernel) {
    hipLaunchKernelGGL(kernel, dim3(grid), dim3(TRANSFER_THREADS), lds, ctx().stream, p);
    SS_LAUNCH_CHECK();
    return (int)SS_OK;
  };
  const int u = transfer_u();
  // the default family with a table for every term; else the gather kernels below
  bool coef = !dual && (u == 4 || u == 8) && transfer_coef_mode() != 0 && p.row_ids == nullptr;   // (row_ids: k-fold)
  if constexpr (std::is_same<T, float>::value && !LOO)
    coef = coef && env_int("SS_TRANSFER_LD", 0) != 1 && env_int("SS_TRANSFER_FIX1", 0) != 1;
  for (int t = 0; t < p.nterms; ++t) coef = coef && p.coef[t] != nullptr;
  if (coef) {
    if (transfer_coef_mode() == 2) path_add("coef_table");
    return dispatch_int<4, 8>(u, [&](auto U) {
      return dispatch_bool(binm, [&](auto B) {
        return launch(transfer_kernel<T, LOO, decltype(U)::value, decltype(B)::value, false, false, false, true>);
      });
    });
  }
  if constexpr (std::is_same<T, float>::value && !LOO) {
    const bool buf = !dual && env_int("SS_TRANSFER_LD", 0) == 1;
    const bool fix = !dual && env_int("SS_TRANSFER_FIX1", 0) == 1 && p.nterms == 1 && !p.accumulate;
    if (buf) path_add("buffer_loads");
    if (fix) path_add("fixed_point");
    if (buf || fix)
      return dispatch_int<4, 8>(u == 4 ? 4 : 8, [&](auto U) {
        return dispatch_bool(binm, [&](auto B) {
          return dispatch_bool(fix, [&](auto F) {
            return dispatch_bool(buf, [&](auto BF) {
              return launch(transfer_kernel<T, LOO, decltype(U)::value, decltype(B)::value, false, decltype(F)::value,
                                            decltype(BF)::value>);
            });
          });
        });
      });
  }
  return dispatch_int<4, 8, 16>(u, [&](auto U) {
    return dispatch_bool(binm, [&](auto B) {
      return dispatch_bool(dual, [&](auto D) {
        return launch(transfer_kernel<T, LOO, decltype(U)::value, decltype(B)::value, decltype(D)::value>);
      });
    });
  });
}

template <class T>
int launch_transfer(int nterms, const DevCsr<T>* L[2], const T* inv1[2], const DevChunked<T>* Mt[2],
                    const T* inv2, int64_t row_begin, int64_t nrows, int64_t nj, T* out, int64_t ld,
                    const int* row_ids, bool accumulate, const T* const* coef) {
  if (nrows <= 0 || nj <= 0) return SS_OK;
  TransferArgs<T> p{};
  p.nterms = nterms;
  for (int t = 0; t < nterms; ++t) {
    p.L[t] = view(*L[t]);
    p.M[t] = view(*Mt[t]);
    p.inv1[t] = inv1[t];
    p.coef[t] = coef ? coef[t] : nullptr;
    if (Mt[t]->SC != Mt[0]->SC || Mt[t]->nchunks != Mt[0]->nchunks)
      return fail(SS_EINVAL, "transfer operands were cut with different chunk sizes");
  }
  p.inv2 = inv2;
  p.row_begin = row_begin;
  p.row_ids = row_ids;
  p.nj = nj;
  p.SC = Mt[0]->SC;
  p.nchunks = Mt[0]->nchunks;
  p.out = out;
  p.ld = ld;
  p.accumulate = accumulate ? 1 : 0;
  p.xmax = 1.0f;
  p.chunk_interleave = env_off("SS_TRANSFER_ORDER") ? 1 : 0;
  bool binm = true;
  for (int t = 0; t < nterms; ++t) binm = binm && Mt[t]->binary;
  const int64_t grid = nrows * p.nchunks;
  if (grid >= (1LL << 31)) return fail(SS_EUNSUPPORTED, "transfer grid too large; lower SS_TRANSFER_BYTES");
  const bool dual = transfer_dual();
  path_add("transfer");
  const size_t lds = (size_t)(p.SC + 64) * sizeof(T) * (dual ? 2 : 1);
  return launch_transfer_variant<T, false>(p, (unsigned)grid, lds, binm, dual);
}

template <class T>
int launch_transfer_loo(const DevCsr<T>& X, const DevChunked<T>& XT, const int* kf, const int* ks,
                        int64_t i_begin, int64_t nrows, T* out, int64_t ld, const T* coef) {
  if (nrows <= 0) return SS_OK;
  TransferArgs<T> p{};
  p.nterms = 1;
  p.L[0] = view(X);
  p.M[0] = view(XT);
  p.kf = kf;
  p.ks = ks;
  p.coef[0] = coef;
  p.row_begin = i_begin;
  p.nj = X.rows;
  p.SC = XT.SC;
  p.nchunks = XT.nchunks;
  p.out = out;
  p.ld = ld;
  p.chunk_interleave = env_off("SS_TRANSFER_ORDER") ? 1 : 0;
  const int64_t grid = nrows * p.nchunks;
  if (grid >= (1LL << 31)) return fail(SS_EUNSUPPORTED, "transfer grid too large; lower SS_TRANSFER_BYTES");
  const bool dual = transfer_dual();
  path_add("transfer_loo");
  const size_t lds = (size_t)(p.SC + 64) * sizeof(T) * (dual ? 2 : 1) + (size_t)((p.SC + 31) / 32) * 4;
  return launch_transfer_variant<T, true>(p, (unsigned)grid, lds, XT.binary, dual);
}

#define SS_INSTANTIATE(T)                                                                                   \
  template int launch_transfer<T>(int, const DevCsr<T>*[2], const T*[2], const DevChunked<T>*[2], const T*, \
                                  int64_t, int64_t, int64_t, T*, int64_t, const int*, bool, const T* const*);     \
  template int transfer_coef_build<T>(const DevCsr<T>&, const T*, const int*, T*);                          \
  template int launch_transfer_block<T>(const DevCsr<T>&, const T*, const DevChunked<T>&, const T*, int64_t, int64_t, \
                                        int64_t, T*, int64_t, T*, float, bool);                               \
  template bool transfer_block_fits<T>(int64_t, int);                                                        \
  template int launch_transfer_loo<T>(const DevCsr<T>&, const DevChunked<T>&, const int*, const int*,       \
                                      int64_t, int64_t, T*, int64_t, const T*);
SS_INSTANTIATE(float)
SS_INSTANTIATE(double)

}  // namespace ss
