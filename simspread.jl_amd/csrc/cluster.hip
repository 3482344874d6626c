// Taylor-Butina clustering of a neighbour pattern on the device, and what goes with a leave-cluster-out split
// (include/simspread_hip_clusters.h states the rule).
//
//   symmetrise   (i,j) and (j,i) of every off-diagonal stored entry as 64-bit keys, radix sort, distinct keys flagged and
//                scanned: a sorted symmetric CSR without duplicates; its row lengths are the degrees d_i
//   rounds       one byte of state per source (undecided, centre, member); an undecided row that sees a centre among its
//                neighbours becomes a member, one that sees no undecided neighbour of earlier priority becomes a centre
//   assign       every member takes its earliest-priority centre neighbour; centres are ranked by priority for `label`
//
// Priority: key(i) = (d_i << 32) | (0xFFFFFFFF - i), larger is earlier.
//
// Why the rounds may update the state bytes in place.  A decision is written once and never changed, and every decision
// that is written is the sequential rule's (induction over the priority order): a row turns centre only after it has
// read every earlier-priority neighbour as a member, which is when the sequential visit finds it unassigned; it turns
// member only after it has read a centre among its neighbours, and a neighbour of a centre is not a centre.  Two
// adjacent undecided rows cannot both turn centre in one launch: the later one would have to read the earlier one as a
// member.  A read that misses a write of the same launch sees "undecided", which only postpones a decision.  Launch
// boundaries make all writes visible, and the earliest-priority undecided row decides in every round, so at most n
// rounds run.  No workgroup waits for another inside a launch.
#include "graph.hpp"

#include <rocprim/rocprim.hpp>

#include <algorithm>
#include <queue>

namespace ss {

namespace {

constexpr int BLK = 256;
constexpr int ROUNDS_PER_READ = 8;  // rounds enqueued between two readbacks of the undecided counters
constexpr int SHORT_ROW = 64;       // rows up to a wave's width: a lane per row; above: a wave per row
enum : unsigned char { UNDECIDED = 0, CENTRE = 1, MEMBER = 2 };
typedef unsigned long long u64;

__device__ __forceinline__ u64 prio_key(int deg, int i) {
  return ((u64)(unsigned)deg << 32) | (u64)(0xFFFFFFFFu - (unsigned)i);
}
__device__ __forceinline__ int key_row(u64 key) { return (int)(0xFFFFFFFFu - (unsigned)(key & 0xFFFFFFFFull)); }
__device__ __forceinline__ unsigned char load_state(const unsigned char* s) {
  return __atomic_load_n(s, __ATOMIC_RELAXED);
}
__device__ __forceinline__ void store_state(unsigned char* s, unsigned char v) {
  __atomic_store_n(s, v, __ATOMIC_RELAXED);
}

// wave per row; status bits: 1 a row's pointers leave [0, nnz_in] or decrease, 2 an index outside 0..n-1.  The indices
// of a row with bad pointers are not read.
__global__ void pattern_check_kernel(const int64_t* __restrict__ ptr, const int32_t* __restrict__ idx, int64_t n,
                                     int base, int64_t nnz_in, int* __restrict__ status) {
  const int lane = threadIdx.x & 63;
  const int64_t wave0 = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
  const int64_t nwaves = ((int64_t)gridDim.x * blockDim.x) >> 6;
  for (int64_t r = wave0; r < n; r += nwaves) {
    const int64_t b = ptr[r] - base, e = ptr[r + 1] - base;
    if (b < 0 || e < b || e > nnz_in) {
      if (lane == 0) atomicOr(status, 1);
      continue;
    }
    bool bad = false;
    for (int64_t x = b + lane; x < e; x += 64) {
      const int64_t c = (int64_t)idx[x] - base;
      bad |= (c < 0 || c >= n);
    }
    if (bad) atomicOr(status, 2);
  }
}

// status bit 4: a fold id outside 0..nfolds-1
__global__ void fold_check_kernel(const int32_t* __restrict__ fold, int64_t n, int nfolds, int* __restrict__ status) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n && (fold[i] < 0 || fold[i] >= nfolds)) atomicOr(status, 4);
}

// keys[2x], keys[2x+1] = (i,j), (j,i) of stored entry x = (i,j); a diagonal entry gives two keys of row n, which sort
// behind every real key and are never flagged.  Only after pattern_check_kernel passed.
__global__ void stack_pairs_kernel(const int64_t* __restrict__ ptr, const int32_t* __restrict__ idx, int64_t n, int base,
                                   u64* __restrict__ keys) {
  const int lane = threadIdx.x & 63;
  const int64_t wave0 = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
  const int64_t nwaves = ((int64_t)gridDim.x * blockDim.x) >> 6;
  const u64 none = (u64)n << 32;
  for (int64_t r = wave0; r < n; r += nwaves) {
    const int64_t b = ptr[r] - base, e = ptr[r + 1] - base;
    for (int64_t x = b + lane; x < e; x += 64) {
      const int64_t c = (int64_t)idx[x] - base;
      const bool diag = (c == r);
      keys[2 * x] = diag ? none : (((u64)r << 32) | (u64)c);
      keys[2 * x + 1] = diag ? none : (((u64)c << 32) | (u64)r);
    }
  }
}

__global__ void flag_distinct_kernel(const u64* __restrict__ keys, int64_t m, int64_t n, int* __restrict__ flag) {
  const int64_t x = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (x >= m) return;
  const u64 k = keys[x];
  flag[x] = ((int64_t)(k >> 32) < n && (x == 0 || keys[x - 1] != k)) ? 1 : 0;
}

// pos: the exclusive scan of flag, pos[m] the total
__global__ void scatter_distinct_kernel(const u64* __restrict__ keys, const int* __restrict__ flag,
                                        const int* __restrict__ pos, int64_t m, int* __restrict__ sidx) {
  const int64_t x = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (x < m && flag[x]) sidx[pos[x]] = (int)(keys[x] & 0xFFFFFFFFull);
}

// sptr[r] = distinct keys in front of the first key of row >= r (r = 0..n): a binary search, no atomics
__global__ void row_pointers_kernel(const u64* __restrict__ keys, const int* __restrict__ pos, int64_t m, int64_t n,
                                    int* __restrict__ sptr) {
  const int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (r > n) return;
  const u64 want = (u64)r << 32;
  int64_t lo = 0, hi = m;
  while (lo < hi) {
    const int64_t mid = (lo + hi) >> 1;
    if (keys[mid] < want) lo = mid + 1; else hi = mid;
  }
  sptr[r] = pos[lo];
}

__global__ void total_kernel(const int* __restrict__ in, int* __restrict__ out, int64_t m) {
  out[m] = out[m - 1] + in[m - 1];
}

struct IsLongRow {
  const int* sptr;
  __device__ bool operator()(int r) const { return sptr[r + 1] - sptr[r] > SHORT_ROW; }
};
struct IsCentre {
  const unsigned char* state;
  __device__ bool operator()(int r) const { return state[r] == CENTRE; }
};

// ---- rounds.  left[0] counts the rows this round leaves undecided (an integer count: its order does not matter).
__global__ void round_short_kernel(const int* __restrict__ sptr, const int* __restrict__ sidx, unsigned char* state,
                                   int n, int* __restrict__ left) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  bool still = false;
  if (i < n && load_state(state + i) == UNDECIDED) {
    const int b = sptr[i], e = sptr[i + 1];
    if (e - b <= SHORT_ROW) {
      const u64 mine = prio_key(e - b, (int)i);
      bool centre = false, blocked = false;
      for (int x = b; x < e; ++x) {
        const int j = sidx[x];
        const unsigned char s = load_state(state + j);
        if (s == CENTRE) {
          centre = true;
          break;
        }
        if (s == UNDECIDED && prio_key(sptr[j + 1] - sptr[j], j) > mine) blocked = true;
      }
      if (centre) store_state(state + i, MEMBER);
      else if (!blocked) store_state(state + i, CENTRE);
      else still = true;
    }
  }
  const u64 mask = __ballot(still);
  if ((threadIdx.x & 63) == 0 && mask) atomicAdd(left, __popcll(mask));
}

__global__ void round_long_kernel(const int* __restrict__ sptr, const int* __restrict__ sidx, unsigned char* state,
                                  const int* __restrict__ rows, int nrows, int* __restrict__ left) {
  const int lane = threadIdx.x & 63;
  const int64_t w = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
  if (w >= nrows) return;  // the whole wave
  const int i = rows[w];
  const int mystate = __shfl((int)load_state(state + i), 0);
  if (mystate != UNDECIDED) return;
  const int b = sptr[i], e = sptr[i + 1];
  const u64 mine = prio_key(e - b, i);
  bool centre = false, blocked = false;
  for (int x0 = b; x0 < e; x0 += 64) {
    const int x = x0 + lane;
    if (x < e) {
      const int j = sidx[x];
      const unsigned char s = load_state(state + j);
      centre |= (s == CENTRE);
      blocked |= (s == UNDECIDED && prio_key(sptr[j + 1] - sptr[j], j) > mine);
    }
    if (__ballot(centre)) break;
  }
  const bool any_centre = __ballot(centre) != 0, any_blocked = __ballot(blocked) != 0;
  if (lane == 0) {
    if (any_centre) store_state(state + i, MEMBER);
    else if (!any_blocked) store_state(state + i, CENTRE);
    else atomicAdd(left, 1);
  }
}

// ---- assign: centre[i] = i for a centre, else the centre neighbour of the largest key
__global__ void assign_short_kernel(const int* __restrict__ sptr, const int* __restrict__ sidx,
                                    const unsigned char* __restrict__ state, int n, int* __restrict__ centre) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const int b = sptr[i], e = sptr[i + 1];
  if (state[i] == CENTRE) {
    centre[i] = (int)i;
    return;
  }
  if (e - b > SHORT_ROW) return;
  u64 best = 0;
  for (int x = b; x < e; ++x) {
    const int j = sidx[x];
    if (state[j] == CENTRE) {
      const u64 k = prio_key(sptr[j + 1] - sptr[j], j);
      best = k > best ? k : best;
    }
  }
  centre[i] = key_row(best);  // a member has a centre neighbour, so best != 0
}

__global__ void assign_long_kernel(const int* __restrict__ sptr, const int* __restrict__ sidx,
                                   const unsigned char* __restrict__ state, const int* __restrict__ rows, int nrows,
                                   int* __restrict__ centre) {
  const int lane = threadIdx.x & 63;
  const int64_t w = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
  if (w >= nrows) return;
  const int i = rows[w];
  if (state[i] == CENTRE) return;  // assign_short_kernel wrote it
  const int b = sptr[i], e = sptr[i + 1];
  u64 best = 0;
  for (int x = b + lane; x < e; x += 64) {
    const int j = sidx[x];
    if (state[j] == CENTRE) {
      const u64 k = prio_key(sptr[j + 1] - sptr[j], j);
      best = k > best ? k : best;
    }
  }
  for (int o = 32; o > 0; o >>= 1) {
    const u64 other = __shfl_xor(best, o);
    best = other > best ? other : best;
  }
  if (lane == 0) centre[i] = key_row(best);
}

__global__ void centre_keys_kernel(const int* __restrict__ sptr, const int* __restrict__ clist, int nc,
                                   u64* __restrict__ ckeys) {
  const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (p < nc) {
    const int i = clist[p];
    ckeys[p] = prio_key(sptr[i + 1] - sptr[i], i);
  }
}
// sorted: the centres' keys, largest first; rank[i] = position of centre i
__global__ void centre_rank_kernel(const u64* __restrict__ sorted, int nc, int* __restrict__ rank) {
  const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (p < nc) rank[key_row(sorted[p])] = (int)p;
}
// size (nullable, zeroed): a histogram of the labels; integer counts, so the order of the atomics does not matter
__global__ void label_kernel(const int* __restrict__ centre, const int* __restrict__ rank, int n,
                             int* __restrict__ label, int* __restrict__ size) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const int c = centre[i];
  const int l = (c >= 0 && c < n) ? rank[c] : -1;  // every source has a centre; a defect must not become an address
  label[i] = l;
  if (size && l >= 0) atomicAdd(size + l, 1);
}

// wave per row: count[f] += stored off-diagonal entries (i, j) with fold[i] == f != fold[j].  Only after the pattern and
// the folds passed their checks.
__global__ void cross_edges_kernel(const int64_t* __restrict__ ptr, const int32_t* __restrict__ idx, int64_t n, int base,
                                   const int32_t* __restrict__ fold, u64* __restrict__ count) {
  const int lane = threadIdx.x & 63;
  const int64_t wave0 = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
  const int64_t nwaves = ((int64_t)gridDim.x * blockDim.x) >> 6;
  for (int64_t r = wave0; r < n; r += nwaves) {
    const int64_t b = ptr[r] - base, e = ptr[r + 1] - base;
    const int f = fold[r];
    long long c = 0;
    for (int64_t x = b + lane; x < e; x += 64) {
      const int64_t j = (int64_t)idx[x] - base;
      c += (j != r && fold[j] != f) ? 1 : 0;
    }
    for (int o = 32; o > 0; o >>= 1) c += __shfl_xor(c, o);
    if (lane == 0 && c) atomicAdd(count + f, (u64)c);
  }
}

int grid_rows(int64_t n) { return (int)std::max<int64_t>(1, ceil_div(n, BLK)); }   // a thread per item, all of them
int grid_waves(int64_t n) { return (int)std::max<int64_t>(1, ceil_div(n * 64, BLK)); }  // a wave per item

int read_ints(const int* dev, int* host, int count) {
  SS_HIP(hipMemcpyAsync(host, dev, (size_t)count * sizeof(int), hipMemcpyDeviceToHost, ctx().stream));
  SS_HIP(hipStreamSynchronize(ctx().stream));
  return SS_OK;
}

// out[0..m) = exclusive scan of in, out[m] = total; m >= 1
int scan_flags(const int* in, int* out, int64_t m) {
  hipStream_t st = ctx().stream;
  size_t bytes = 0;
  SS_HIP(rocprim::exclusive_scan(nullptr, bytes, in, out, 0, (size_t)m, rocprim::plus<int>(), st));
  DevBuf<unsigned char> tmp;
  SS_TRY(tmp.alloc(bytes));
  SS_HIP(rocprim::exclusive_scan(tmp.p, bytes, in, out, 0, (size_t)m, rocprim::plus<int>(), st));
  hipLaunchKernelGGL(total_kernel, dim3(1), dim3(1), 0, st, in, out, m);
  SS_LAUNCH_CHECK();
  SS_HIP(hipStreamSynchronize(st));  // tmp is freed on return
  return SS_OK;
}

// rows 0..n-1 that satisfy pred, ascending, into list; *count on the host
template <class Pred>
int select_rows(int64_t n, Pred pred, int* list, int* count) {
  hipStream_t st = ctx().stream;
  DevBuf<int> dcount;
  SS_TRY(dcount.alloc(1));
  rocprim::counting_iterator<int> rows(0);
  size_t bytes = 0;
  SS_HIP(rocprim::select(nullptr, bytes, rows, list, dcount.p, (size_t)n, pred, st));
  DevBuf<unsigned char> tmp;
  SS_TRY(tmp.alloc(bytes));
  SS_HIP(rocprim::select(tmp.p, bytes, rows, list, dcount.p, (size_t)n, pred, st));
  return read_ints(dcount.p, count, 1);  // synchronises: tmp is freed on return
}

int bit_length(uint64_t v) {
  int b = 0;
  while (v) { ++b; v >>= 1; }
  return b;
}

struct Span {  // a stage of ss_timing_last between two events on the stream
  int stage;
  hipEvent_t a = nullptr;
  bool ok;
  explicit Span(int s) : stage(s) { ok = timing_mark(&a) == SS_OK; }
  void stop() {
    hipEvent_t b;
    if (ok && timing_mark(&b) == SS_OK) timing_span(stage, a, b);
    ok = false;
  }
  ~Span() { stop(); }
};

}  // namespace

int pattern_check(int64_t n, const int64_t* ptr, const int32_t* idx, int base, int64_t nnz_in, const int32_t* fold,
                  int nfolds) {
  hipStream_t st = ctx().stream;
  DevBuf<int> status;
  SS_TRY(status.alloc(1));
  SS_HIP(hipMemsetAsync(status.p, 0, sizeof(int), st));
  hipLaunchKernelGGL(pattern_check_kernel, dim3(grid_1d(n * 64, BLK)), dim3(BLK), 0, st, ptr, idx, n, base, nnz_in,
                     status.p);
  SS_LAUNCH_CHECK();
  if (fold) {
    hipLaunchKernelGGL(fold_check_kernel, dim3(grid_rows(n)), dim3(BLK), 0, st, fold, n, nfolds, status.p);
    SS_LAUNCH_CHECK();
  }
  int s = 0;
  SS_TRY(read_ints(status.p, &s, 1));
  if (s & 1) return fail(SS_EINVAL, "row pointers are not monotone / exceed the entry count");
  if (s & 2) return fail(SS_EINVAL, "column index out of range");
  if (s & 4) return fail(SS_EINVAL, "fold id outside 0..nfolds-1");
  return SS_OK;
}

int butina_csr(int64_t n, const int64_t* ptr, const int32_t* idx, int base, int64_t nnz_in, bool validate, int* centre,
               int* label, int* size, int64_t* nclusters, int64_t* rounds) {
  hipStream_t st = ctx().stream;
  *nclusters = 0;
  *rounds = 0;
  if (n == 0) return SS_OK;
  if (nnz_in >= (1LL << 30))
    return fail(SS_EUNSUPPORTED, "butina: %lld stored entries (>= 2^30)", (long long)nnz_in);
  if (validate) SS_TRY(pattern_check(n, ptr, idx, base, nnz_in, nullptr, 0));

  // ---- symmetrise and deduplicate
  Span t_sym(ST_TRANSFER);
  const int64_t m = 2 * nnz_in;
  DevBuf<int> sptr, sidx;
  SS_TRY(sptr.alloc(n + 1));
  if (m == 0) {
    SS_HIP(hipMemsetAsync(sptr.p, 0, (size_t)(n + 1) * sizeof(int), st));
    SS_TRY(sidx.alloc(0));
  } else {
    DevBuf<u64> keys, sorted;
    DevBuf<int> flag, pos;
    SS_TRY(keys.alloc(m));
    SS_TRY(sorted.alloc(m));
    hipLaunchKernelGGL(stack_pairs_kernel, dim3(grid_1d(n * 64, BLK)), dim3(BLK), 0, st, ptr, idx, n, base, keys.p);
    SS_LAUNCH_CHECK();
    const unsigned end_bit = 32u + (unsigned)bit_length((uint64_t)n);  // rows 0..n, n being the diagonal's "no key"
    size_t bytes = 0;
    SS_HIP(rocprim::radix_sort_keys(nullptr, bytes, keys.p, sorted.p, (size_t)m, 0u, end_bit, st));
    DevBuf<unsigned char> tmp;
    SS_TRY(tmp.alloc(bytes));
    SS_HIP(rocprim::radix_sort_keys(tmp.p, bytes, keys.p, sorted.p, (size_t)m, 0u, end_bit, st));
    SS_TRY(flag.alloc(m));
    SS_TRY(pos.alloc(m + 1));
    hipLaunchKernelGGL(flag_distinct_kernel, dim3(grid_rows(m)), dim3(BLK), 0, st, sorted.p, m, n, flag.p);
    SS_LAUNCH_CHECK();
    SS_TRY(scan_flags(flag.p, pos.p, m));
    int total = 0;
    SS_TRY(read_ints(pos.p + m, &total, 1));
    SS_TRY(sidx.alloc(total));
    hipLaunchKernelGGL(scatter_distinct_kernel, dim3(grid_rows(m)), dim3(BLK), 0, st, sorted.p, flag.p, pos.p, m,
                       sidx.p);
    SS_LAUNCH_CHECK();
    hipLaunchKernelGGL(row_pointers_kernel, dim3(grid_rows(n + 1)), dim3(BLK), 0, st, sorted.p, pos.p, m, n, sptr.p);
    SS_LAUNCH_CHECK();
    SS_HIP(hipStreamSynchronize(st));  // keys, sorted, flag, pos and tmp are freed here
  }
  DevBuf<int> long_rows;
  int nlong = 0;
  SS_TRY(long_rows.alloc(n));
  SS_TRY(select_rows(n, IsLongRow{sptr.p}, long_rows.p, &nlong));
  t_sym.stop();

  // ---- rounds: at most n of them, ROUNDS_PER_READ between two looks at the counters
  Span t_rounds(ST_SPMM);
  DevBuf<unsigned char> state;
  DevBuf<int> left;
  SS_TRY(state.alloc(n));
  SS_TRY(left.alloc(ROUNDS_PER_READ));
  SS_HIP(hipMemsetAsync(state.p, UNDECIDED, (size_t)n, st));
  int64_t done_after = 0;
  for (int64_t r0 = 0; r0 < n && !done_after; r0 += ROUNDS_PER_READ) {
    SS_HIP(hipMemsetAsync(left.p, 0, ROUNDS_PER_READ * sizeof(int), st));
    for (int r = 0; r < ROUNDS_PER_READ; ++r) {
      hipLaunchKernelGGL(round_short_kernel, dim3(grid_rows(n)), dim3(BLK), 0, st, sptr.p, sidx.p, state.p, (int)n,
                         left.p + r);
      SS_LAUNCH_CHECK();
      if (nlong > 0) {
        hipLaunchKernelGGL(round_long_kernel, dim3(grid_waves(nlong)), dim3(BLK), 0, st, sptr.p, sidx.p, state.p,
                           long_rows.p, nlong, left.p + r);
        SS_LAUNCH_CHECK();
      }
    }
    int host_left[ROUNDS_PER_READ];
    SS_TRY(read_ints(left.p, host_left, ROUNDS_PER_READ));
    for (int r = 0; r < ROUNDS_PER_READ && !done_after; ++r)
      if (host_left[r] == 0) done_after = r0 + r + 1;
  }
  if (!done_after || done_after > n)
    return fail(SS_EINTERNAL, "butina: rows were still undecided after %lld rounds", (long long)n);
  *rounds = done_after;
  t_rounds.stop();

  // ---- assign and label
  Span t_assign(ST_EPILOGUE);
  hipLaunchKernelGGL(assign_short_kernel, dim3(grid_rows(n)), dim3(BLK), 0, st, sptr.p, sidx.p, state.p, (int)n, centre);
  SS_LAUNCH_CHECK();
  if (nlong > 0) {
    hipLaunchKernelGGL(assign_long_kernel, dim3(grid_waves(nlong)), dim3(BLK), 0, st, sptr.p, sidx.p, state.p,
                       long_rows.p, nlong, centre);
    SS_LAUNCH_CHECK();
  }
  DevBuf<int> clist, rank;
  int nc = 0;
  SS_TRY(clist.alloc(n));
  SS_TRY(rank.alloc(n));
  SS_TRY(select_rows(n, IsCentre{state.p}, clist.p, &nc));
  DevBuf<u64> ckeys, csorted;
  SS_TRY(ckeys.alloc(nc));
  SS_TRY(csorted.alloc(nc));
  hipLaunchKernelGGL(centre_keys_kernel, dim3(grid_rows(nc)), dim3(BLK), 0, st, sptr.p, clist.p, nc, ckeys.p);
  SS_LAUNCH_CHECK();
  size_t bytes = 0;
  SS_HIP(rocprim::radix_sort_keys_desc(nullptr, bytes, ckeys.p, csorted.p, (size_t)nc, 0u, 64u, st));
  DevBuf<unsigned char> tmp;
  SS_TRY(tmp.alloc(bytes));
  SS_HIP(rocprim::radix_sort_keys_desc(tmp.p, bytes, ckeys.p, csorted.p, (size_t)nc, 0u, 64u, st));
  hipLaunchKernelGGL(centre_rank_kernel, dim3(grid_rows(nc)), dim3(BLK), 0, st, csorted.p, nc, rank.p);
  SS_LAUNCH_CHECK();
  if (size) SS_HIP(hipMemsetAsync(size, 0, (size_t)nc * sizeof(int), st));
  hipLaunchKernelGGL(label_kernel, dim3(grid_rows(n)), dim3(BLK), 0, st, centre, rank.p, (int)n, label, size);
  SS_LAUNCH_CHECK();
  t_assign.stop();
  SS_HIP(hipStreamSynchronize(st));
  *nclusters = nc;
  return SS_OK;
}

int cross_edges(int64_t n, const int64_t* ptr, const int32_t* idx, int base, int64_t nnz_in, const int32_t* fold,
                int nfolds, int64_t* count) {
  hipStream_t st = ctx().stream;
  SS_HIP(hipMemsetAsync(count, 0, (size_t)nfolds * sizeof(int64_t), st));
  if (n > 0) {
    SS_TRY(pattern_check(n, ptr, idx, base, nnz_in, fold, nfolds));
    hipLaunchKernelGGL(cross_edges_kernel, dim3(grid_1d(n * 64, BLK)), dim3(BLK), 0, st, ptr, idx, n, base, fold,
                       reinterpret_cast<u64*>(count));
    SS_LAUNCH_CHECK();
  }
  SS_HIP(hipStreamSynchronize(st));
  return SS_OK;
}

// Host code.  Clusters by size descending (ties: label ascending), each to the fold with the fewest sources so far
// (ties: the lowest fold id).
int cluster_folds(const int32_t* label, int64_t n, int64_t nclusters, int nfolds, int32_t* fold) {
  std::vector<int64_t> size((size_t)nclusters, 0);
  for (int64_t i = 0; i < n; ++i) {
    if (label[i] < 0 || label[i] >= nclusters)
      return fail(SS_EINVAL, "cluster folds: label %d of source %lld outside 0..%lld", (int)label[i], (long long)i,
                  (long long)nclusters - 1);
    ++size[(size_t)label[i]];
  }
  std::vector<int32_t> order((size_t)nclusters);
  for (int64_t c = 0; c < nclusters; ++c) order[(size_t)c] = (int32_t)c;
  std::stable_sort(order.begin(), order.end(), [&](int32_t a, int32_t b) { return size[(size_t)a] > size[(size_t)b]; });
  typedef std::pair<int64_t, int> Load;  // (sources so far, fold id): the smallest pair is the next fold
  std::priority_queue<Load, std::vector<Load>, std::greater<Load>> loads;
  for (int f = 0; f < nfolds; ++f) loads.push(Load(0, f));
  std::vector<int32_t> fold_of_cluster((size_t)nclusters, 0);
  for (int32_t c : order) {
    Load l = loads.top();
    loads.pop();
    fold_of_cluster[(size_t)c] = l.second;
    l.first += size[(size_t)c];
    loads.push(l);
  }
  for (int64_t i = 0; i < n; ++i) fold[i] = fold_of_cluster[(size_t)label[i]];
  return SS_OK;
}

}  // namespace ss
