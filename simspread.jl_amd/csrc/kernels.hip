// Hand-written gfx950 kernels of the SimSpread resource-spreading pass (stage 1, the transfer rows, is transfer.hip).
//
//   spmm_sell_kernel     stage 2, wide: F = W*R with an LDS-resident tile of QT columns of R,
//                        one lane per row of W, chunk-local 16-bit indices (the A*W^2 row
//                        gather of src/core.jl:413,421 restricted to the Nq x Nt corner)
//   spmm_csr_narrow      stage 2, narrow (B <= 64): CSR streamed once from HBM, wave per row,
//                        __shfl broadcast of (index,value) and __shfl_xor reduction
//   cutoff / row_degree / spread_dense   the element-wise pieces (src/core.jl:37-43,365-371,
//                        src/graphs.jl:9-11)
//
// Wavefront = 64 lanes everywhere.  No float atomics anywhere: every sum has a fixed order, so
// results are bitwise reproducible from run to run.
#include "graph.hpp"

namespace ss {

// ============================================================== element-wise
template <class T>
__global__ void cutoff_kernel(const T* __restrict__ X, int64_t rows, int64_t cols, int64_t ld, T alpha,
                              int weighted, T* __restrict__ out, int64_t ldo) {
  const int64_t total = rows * cols;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total;
       i += (int64_t)gridDim.x * blockDim.x) {
    const int64_t c = i / rows, r = i - c * rows;
    const T x = X[r + c * ld];
    out[r + c * ldo] = (x >= alpha) ? (weighted ? x : T(1)) : T(0);
  }
}

template <class T>
int launch_cutoff(const T* X, int64_t rows, int64_t cols, int64_t ld, T alpha, bool weighted, T* out, int64_t ldo) {
  if (rows * cols == 0) return SS_OK;
  hipLaunchKernelGGL(cutoff_kernel<T>, dim3(grid_1d(rows * cols, 256)), dim3(256), 0, ctx().stream, X, rows,
                     cols, ld, alpha, weighted ? 1 : 0, out, ldo);
  SS_LAUNCH_CHECK();
  return SS_OK;
}

// k(G): one thread per row, lanes walk the same column together (coalesced in column-major)
template <class T>
__global__ void row_degree_kernel(const T* __restrict__ G, int64_t rows, int64_t cols, int64_t ld,
                                  int* __restrict__ deg) {
  for (int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; r < rows;
       r += (int64_t)gridDim.x * blockDim.x) {
    int n = 0;
    for (int64_t c = 0; c < cols; ++c) n += (G[r + c * ld] != T(0)) ? 1 : 0;
    deg[r] = n;
  }
}

template <class T>
int launch_row_degree(const T* G, int64_t rows, int64_t cols, int64_t ld, int* deg) {
  if (rows == 0) return SS_OK;
  hipLaunchKernelGGL(row_degree_kernel<T>, dim3(grid_1d(rows, 64)), dim3(64), 0, ctx().stream, G, rows, cols,
                     ld, deg);
  SS_LAUNCH_CHECK();
  return SS_OK;
}

template <class T>
__global__ void spread_dense_kernel(const T* __restrict__ G, int64_t rows, int64_t cols, int64_t ld,
                                    const int* __restrict__ deg, T* __restrict__ W, int64_t ldw) {
  const int64_t total = rows * cols;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total;
       i += (int64_t)gridDim.x * blockDim.x) {
    const int64_t c = i / rows, r = i - c * rows;
    const int d = deg[r];
    W[r + c * ldw] = d > 0 ? G[r + c * ld] / T(d) : T(0);
  }
}

template <class T>
int launch_spread_dense(const T* G, int64_t rows, int64_t cols, int64_t ld, const int* deg, T* W, int64_t ldw) {
  if (rows * cols == 0) return SS_OK;
  hipLaunchKernelGGL(spread_dense_kernel<T>, dim3(grid_1d(rows * cols, 256)), dim3(256), 0, ctx().stream, G,
                     rows, cols, ld, deg, W, ldw);
  SS_LAUNCH_CHECK();
  return SS_OK;
}

// ============================================================== stage 2, wide: SELL x LDS tile
template <class T, int QT>
struct alignas(sizeof(T) * QT) Vec {
  T v[QT];
};

template <class T>
struct SellArgs {
  const int* off;
  const unsigned short* idx;
  const T* val;
  int nslices, nchunks, KC;
  int64_t K, M, B;
  const T* R;
  int64_t ldr;
  T* F;
  int64_t ldf;
  const int* clean_deg;
  const int* out_rows;  // optional: column b of R goes to row out_rows[b] of F (k-fold members -> source rows)
  const int* q1;        // 16-byte tile rows: slot lending (DevSell), per (chunk, slice) the quads before the lent ones ...
  const unsigned* rec;  // ... and per lane whose partial sums it collects, and whether it is a receiver
};

constexpr int SELL_THREADS = 1024;
constexpr int SELL_NB = 4;  // quads of W in flight per lane ahead of the gathers
static_assert(SELL_Q1_STEP == 2 * SELL_NB, "a lending slice's first part must end with a turn of the gather loop");
constexpr int SELL_QT_F32_DEFAULT = 4;
constexpr int SELL_ZERO_ROWS = 16;  // zero rows behind the tile: one per 16-byte slot class of the 256-byte LDS line
constexpr int SELL_STAGE_IT = 5;  // passes of SELL_THREADS per staging round (the largest tile, 10240 rows, takes two rounds)

// Workgroup = QT columns of R (QT queries).  Per chunk of KC columns of W: the tile
// R[b0..b0+QT)[k0..k0+KC) sits in LDS as [k][QT] so that one ds_read_b128 fetches the QT
// operands of a non-zero; waves walk the slices, lane = row of W, no cross-lane reduction.
// (16-bit half H of x) << sh in one VALU instruction (SDWA source select)
template <int H>
__device__ __forceinline__ unsigned half_shl(unsigned x, unsigned sh) {
  unsigned r;
  if (H == 0)
    asm("v_lshlrev_b32_sdwa %0, %1, %2 dst_sel:DWORD dst_unused:UNUSED_PAD src0_sel:DWORD src1_sel:WORD_0"
        : "=v"(r) : "v"(sh), "v"(x));
  else
    asm("v_lshlrev_b32_sdwa %0, %1, %2 dst_sel:DWORD dst_unused:UNUSED_PAD src0_sel:DWORD src1_sel:WORD_1"
        : "=v"(r) : "v"(sh), "v"(x));
  return r;
}

template <class T, int QT, bool BIN>
__global__ void __launch_bounds__(SELL_THREADS) spmm_sell_kernel(SellArgs<T> a) {
  // Tile rows of 16 bytes ((float,4), (double,2)), or of 32 bytes = two 16-byte pieces ((float,8), round 3): the index
  // stream of W, which every workgroup re-reads for its own columns, is then shared by twice as many columns.  It is what
  // bounds this kernel (measured by ablation: without it stage 2 takes 0.36 instead of 0.59 ms at C2, 7.4 instead of
  // 12.7 ms at C3; with half the LDS reads 0.55 / 12.1).  With two pieces a lane reads piece r ^ (lane & 1) in read r, so
  // that the 16 lanes of an LDS cycle are spread over 16 (slot class, piece) cells; the accumulators hold the columns in
  // that rotated order and are put back when they are stored.
  constexpr int RB = (int)sizeof(T) * QT, NP = RB / 16;
  // registers: two-piece rows stage fewer passes per round and (weighted) keep fewer quads in flight
  constexpr int STAGE_IT = NP == 2 ? 2 : SELL_STAGE_IT;
  constexpr int NBQ = NP == 2 ? 2 : SELL_NB;   // divides SELL_NB: the builder pads slices to groups of SELL_NB quads
  constexpr unsigned TSH = NP == 2 ? 5 : 4;  // log2(RB)
  static_assert(RB == 16 || (RB == 32 && sizeof(T) == 4), "tile row must be 16 bytes, or 32 bytes of fp32");
  extern __shared__ __align__(16) unsigned char smem_raw[];
  using V = Vec<T, QT>;
  // [KC + 16]: rows KC .. KC+15 stay zero -- one padding target per 16-byte slot class, so that the builder can point a
  // padding entry at a zero row whose slot no active lane of its LDS cycle uses (sell_fill_sched_kernel, assemble.hip)
  V* tile = reinterpret_cast<V*>(smem_raw);
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, nwaves = blockDim.x >> 6;
  const int64_t b0 = (int64_t)blockIdx.x * QT;
  const unsigned pid = NP == 2 ? (unsigned)(lane & 1) : 0u;   // which piece this lane reads first
  // (the gathers below use tile-relative LDS addresses: the dynamic LDS segment must start at LDS address 0, i.e. the
  // kernel must have no static __shared__ object -- launch_spmm_sell checks that on the host before the first launch)

  for (int c = 0; c < a.nchunks; ++c) {
    const int64_t k0 = (int64_t)c * a.KC;
    const int kn = (int)((a.K - k0 < a.KC) ? (a.K - k0) : a.KC);
    if (c) __syncthreads();
    // Stage the tile in rounds of SELL_STAGE_IT passes of 1024 threads: all loads of a round are requested before its
    // first LDS write (clamped, branch-free addresses) -- one memory latency per round (two for the largest tile)
    // instead of one per pass.  Nothing else runs on the CU meanwhile (one workgroup per CU): this latency is not hidden.
    for (int kb = 0; kb < a.KC + SELL_ZERO_ROWS; kb += STAGE_IT * SELL_THREADS) {
      T stg[STAGE_IT][QT];
      const int klast = kn > 0 ? kn - 1 : 0;
#pragma unroll
      for (int it = 0; it < STAGE_IT; ++it) {
        const int k = kb + tid + it * SELL_THREADS;
        const int kk = k < kn ? k : klast;
#pragma unroll
        for (int q = 0; q < QT; ++q) {
          const int64_t b = (b0 + q < a.B) ? b0 + q : a.B - 1;
          stg[it][q] = kn > 0 ? a.R[b * a.ldr + k0 + kk] : T(0);
        }
      }
#pragma unroll
      for (int it = 0; it < STAGE_IT; ++it) {
        const int k = kb + tid + it * SELL_THREADS;
        if (k < a.KC + SELL_ZERO_ROWS) {
          V v;
#pragma unroll
          for (int q = 0; q < QT; ++q) v.v[q] = (k < kn && b0 + q < a.B) ? stg[it][q] : T(0);
          tile[k] = v;
        }
      }
    }
    __syncthreads();

    const int* off = a.off + (int64_t)c * a.nslices;
    const bool last = (c == a.nchunks - 1);
    // few tiles (narrow R): the slices are also split over gridDim.y workgroups per tile
    for (int s = wave + nwaves * (int)blockIdx.y; s < a.nslices; s += nwaves * (int)gridDim.y) {
      const int o = __builtin_amdgcn_readfirstlane(off[s]);
      const int oe = __builtin_amdgcn_readfirstlane(off[s + 1]);
      T acc[QT];
#pragma unroll
      for (int q = 0; q < QT; ++q) acc[q] = T(0);
      // chunks after the first add to what is already in F: request those values now, they are needed only
      // after the gathers of this slice (otherwise every slice ends on an exposed global-load latency)
      const int64_t m = (int64_t)s * 64 + lane;
      T fprev[QT];
#pragma unroll
      for (int q = 0; q < QT; ++q) {
        fprev[q] = T(0);
        if (NP == 1 && c && m < a.M && b0 + q < a.B)   // (two-piece rows: read when the slice is done -- registers)
          fprev[q] = a.F[(a.out_rows ? (int64_t)a.out_rows[b0 + q] : b0 + q) * a.ldf + m];
      }
      // slot lending (DevSell): quads q1 .. nq-1 of a receiver lane hold entries of another row of the slice
      int q1 = oe - o;
      unsigned rec = SELL_REC_NONE;
      if (NP == 1) {
        q1 = __builtin_amdgcn_readfirstlane(a.q1[(int64_t)c * a.nslices + s]);
        rec = a.rec[((int64_t)c * a.nslices + s) * 64 + lane];
      }
      const ushort4* ip = reinterpret_cast<const ushort4*>(a.idx) + (int64_t)o * 64 + lane;
      const Vec<T, 4>* vp = reinterpret_cast<const Vec<T, 4>*>(a.val) + (int64_t)o * 64 + lane;
      // NB quads of indices (and values) are fetched ahead of the LDS gathers they feed: the index stream comes
      // from L2 at several hundred cycles per access, the loop must not wait per quad.  The builder pads every
      // slice to whole groups of NB quads and leaves two groups of slack behind the last slice, so the loads need
      // neither clamps nor pad selects nor branches: with branches around them hipcc waits vmcnt(0) right after
      // issuing the next group, i.e. nothing would be in flight while the current group is gathered.  The group
      // past the end of a slice is loaded and never used.  Two register sets (A/B) alternate, nothing is copied.
      const uint2* ipw = reinterpret_cast<const uint2*>(ip);
      const int nq = oe - o;
      uint2 ia[NBQ], ib[NBQ];
      Vec<T, 4> wa[NBQ], wb[NBQ];
      auto fetch = [&](uint2 (&iq)[NBQ], Vec<T, 4> (&wq)[NBQ], int base) __attribute__((always_inline)) {
#pragma unroll
        for (int j = 0; j < NBQ; ++j) {
          iq[j] = ipw[(int64_t)(base + j) * 64];
          if (!BIN) wq[j] = vp[(int64_t)(base + j) * 64];
        }
      };
      auto gather = [&](const uint2 (&iq)[NBQ], const Vec<T, 4> (&wq)[NBQ], int cnt) __attribute__((always_inline)) {
        // LDS address of tile[k] = k * 16: one SDWA shift per 16-bit index, used as the address itself (the tile
        // is the only LDS object of this kernel and starts at LDS address 0 -- checked once at kernel entry;
        // going through the generic tile pointer costs one more VALU add per non-zero)
        constexpr int PV = 16 / (int)sizeof(T);   // values per 16-byte piece
        typedef T NV __attribute__((ext_vector_type(PV)));
        using LV = const __attribute__((address_space(3))) NV*;
        const unsigned lb = pid << 4;
        auto row = [&](unsigned addr) __attribute__((always_inline)) {
          V r;
          if (NP == 1) {
            const NV n = *(LV)(uintptr_t)addr;
#pragma unroll
            for (int q = 0; q < PV; ++q) r.v[q] = n[q];
          } else {
            const unsigned a0 = addr | lb;
            const NV n0 = *(LV)(uintptr_t)a0;
            const NV n1 = *(LV)(uintptr_t)(a0 ^ 16u);
#pragma unroll
            for (int q = 0; q < PV; ++q) { r.v[q] = n0[q]; r.v[PV + q] = n1[q]; }
          }
          return r;
        };
#pragma unroll
        for (int j = 0; j < NBQ; ++j) {
          if (j >= cnt) break;   // wave-uniform; cnt == NBQ inside the loop (folds away), smaller only for a slice's tail
          const V t0 = row(half_shl<0>(iq[j].x, TSH));
          const V t1 = row(half_shl<1>(iq[j].x, TSH));
          const V t2 = row(half_shl<0>(iq[j].y, TSH));
          const V t3 = row(half_shl<1>(iq[j].y, TSH));
          if (BIN) {
#pragma unroll
            for (int q = 0; q < QT; ++q) acc[q] += (t0.v[q] + t1.v[q]) + (t2.v[q] + t3.v[q]);
          } else {
#pragma unroll
            for (int q = 0; q < QT; ++q) {
              acc[q] = fma(wq[j].v[0], t0.v[q], acc[q]);
              acc[q] = fma(wq[j].v[1], t1.v[q], acc[q]);
              acc[q] = fma(wq[j].v[2], t2.v[q], acc[q]);
              acc[q] = fma(wq[j].v[3], t3.v[q], acc[q]);
            }
          }
          // two-piece rows: one quad's eight reads at a time (all of a group's at once would need 128 registers)
          if (NP == 2) __builtin_amdgcn_sched_barrier(0);
        }
      };
      // (both gathers of the loop body are unconditional on purpose: a gather under `if` lets the compiler sink
      // its loads into the branch, right in front of their use)
      // Measured and not kept (round 3): a third register set (two groups of quads in flight while one is gathered; the
      // gathers split in two by a compiler barrier so that it fits in 123 registers): 0.605 vs 0.594 ms at C2, 12.8 vs
      // 12.6 ms at C3 -- the index stream is bound by the bytes through the CU's vector-memory path, not by its latency.
      //
      // Two register sets, both requested before the first gather; a slice is a whole number of QUADS (not of groups, since
      // round 3): the last one or two groups are consumed quad by quad under wave-uniform conditions, outside the loop.
      // Requests run up to two groups past the slice (the next slice, or the slack behind the last one).
      //
      // A slice that lends (q1 < nq; q1 is a multiple of 2 * NBQ, so it ends a turn of the loop): where its first part
      // ends the receivers put their own sums aside and start from zero -- one wave-uniform test per turn, away from the
      // loads and the gathers; every other lane carries on in one chain, so its sums are those of the plain layout.  After
      // the last quad a lane adds the partial sums of the lanes its record lists (ds_bpermute: the LDS crossbar, no LDS
      // storage), in list order, and the receivers take their own sums back.  (q1 == 0: the receivers' own sums are 0.)
      fetch(ia, wa, 0);
      fetch(ib, wb, NBQ);
      const bool recv = NP == 1 && ((rec >> 24) & 1u);
      T own[QT];
#pragma unroll
      for (int q = 0; q < QT; ++q) own[q] = T(0);
      int u = 0;
      for (; u + 2 * NBQ <= nq; u += 2 * NBQ) {
        gather(ia, wa, NBQ);
        fetch(ia, wa, u + 2 * NBQ);
        gather(ib, wb, NBQ);
        fetch(ib, wb, u + 3 * NBQ);
        if (NP == 1 && u + 2 * NBQ == q1) {
#pragma unroll
          for (int q = 0; q < QT; ++q) { own[q] = recv ? acc[q] : own[q]; acc[q] = recv ? T(0) : acc[q]; }
        }
      }
      {
        const int rest = nq - u;   // 0 .. 2 * NBQ - 1 quads; ia holds quads u .., ib quads u + NBQ ..
        if (rest > 0) gather(ia, wa, rest < NBQ ? rest : NBQ);
        if (rest > NBQ) gather(ib, wb, rest - NBQ);
      }
      if (NP == 1 && q1 < nq) {
        constexpr int NW = (int)(sizeof(T) * QT / 4);
        int lent[NW];
        __builtin_memcpy(lent, acc, sizeof(lent));
#pragma unroll
        for (int r = 0; r < SELL_LEND_R; ++r) {
          const unsigned src = (rec >> (8 * r)) & 0xffu;
          if (__ballot(src != 0xffu) == 0ull) break;   // (the lists are filled from byte 0 on)
          // a lane with nothing to collect reads itself: every lane reading one lane would serialise in the crossbar
          const int from = (int)((src != 0xffu ? src : (unsigned)lane) << 2);
          int got[NW];
#pragma unroll
          for (int w = 0; w < NW; ++w) got[w] = __builtin_amdgcn_ds_bpermute(from, lent[w]);
          T add[QT];
          __builtin_memcpy(add, got, sizeof(got));
#pragma unroll
          for (int q = 0; q < QT; ++q) acc[q] = src != 0xffu ? acc[q] + add[q] : acc[q];
        }
#pragma unroll
        for (int q = 0; q < QT; ++q) acc[q] = recv ? own[q] : acc[q];
      }
      if (m < a.M) {
        const bool flag = last && a.clean_deg != nullptr && a.clean_deg[m] == 0;
#pragma unroll
        for (int q = 0; q < QT; ++q) {
          if (b0 + q < a.B) {
            T* f = a.F + (a.out_rows ? (int64_t)a.out_rows[b0 + q] : b0 + q) * a.ldf + m;
            // two-piece rows: odd lanes read the pieces in the order 1, 0 -- their accumulators q and q ^ 4 are swapped
            const T mine = NP == 2 ? (pid ? acc[q ^ (QT / 2)] : acc[q]) : acc[q];
            const T r = mine + ((NP == 2 && c) ? *f : fprev[q]);
            *f = flag ? T(-99) : r;
          }
        }
      }
    }
  }
}

// fp32: 8 columns per tile row since round 3 (SS_SELL_QT=4: the 16-byte rows of rounds 1-2)
template <> int sell_tile_width<float>() {
  const int v = (int)env_int("SS_SELL_QT", 0);
  if (v == 4 || v == 8) return v;
  return SELL_QT_F32_DEFAULT;
}
template <> int sell_tile_width<double>() { return 2; }

template <class T>
int sell_max_chunk(int qt) {
  // (KC + 16) * qt * sizeof(T) <= 160 KiB and KC + 15 <= 65535 (16-bit local indices; KC .. KC+15 are the zero rows)
  int64_t kc = (int64_t)(160 * 1024) / ((int64_t)qt * (int64_t)sizeof(T)) - SELL_ZERO_ROWS;
  if (kc > 65535 - (SELL_ZERO_ROWS - 1)) kc = 65535 - (SELL_ZERO_ROWS - 1);
  return (int)kc;
}

template <class T>
int launch_spmm_sell(const DevSell<T>& W, const T* R, int64_t ldr, int64_t B, T* F, int64_t ldf,
                     const int* clean_deg, const int* out_rows) {
  if (B <= 0 || W.rows <= 0) return SS_OK;
  path_add(W.sorted ? "spmm_sell_sorted" : "spmm_sell");
  const int QT = W.qt > 0 ? W.qt : (sizeof(T) == 4 ? 4 : 2);
  SellArgs<T> a{};
  a.off = W.off.p;
  a.idx = W.idx.p;
  a.val = W.val.p;
  a.nslices = W.nslices;
  a.nchunks = W.nchunks;
  a.KC = W.KC;
  a.K = W.cols;
  a.M = W.sorted ? W.vrows : W.rows;
  a.B = B;
  a.R = R;
  a.ldr = ldr;
  a.F = F;
  a.ldf = ldf;
  a.clean_deg = clean_deg;
  a.out_rows = out_rows;
  a.q1 = W.q1.p;
  a.rec = W.rec.p;
  if (W.lends) path_add("sell_lend");
  const size_t lds = (size_t)(W.KC + SELL_ZERO_ROWS) * QT * sizeof(T);
  if (lds > (size_t)160 * 1024) return fail(SS_EINVAL, "SELL chunk does not fit the LDS tile of %d columns", QT);
  const unsigned gx = (unsigned)ceil_div(B, QT);
  unsigned gy = 1;
  if ((int)gx < 2 * ctx().num_cu) {
    gy = (unsigned)ceil_div(2 * ctx().num_cu, (int64_t)gx);
    const unsigned maxy = (unsigned)ceil_div(W.nslices, SELL_THREADS / 64);
    if (gy > maxy) gy = maxy > 0 ? maxy : 1;
  }
  const dim3 grid(gx, gy);
  // first launch of an instantiation: raise its dynamic-LDS limit and check, on the host, what the kernel's LDS
  // addressing relies on -- no static LDS in the code object's kernel, so that the dynamic segment starts at 0.
  // (A violated assumption is an error code for the caller, never a device-side abort.)
  auto prepare = [](const void* fn) -> int {
    hipFuncAttributes fa{};
    SS_HIP(hipFuncGetAttributes(&fa, fn));
    if (fa.sharedSizeBytes != 0)
      return fail(SS_EUNSUPPORTED, "spmm_sell_kernel was built with %zu bytes of static LDS: its tile-relative LDS "
                  "addresses need the dynamic segment at LDS address 0", (size_t)fa.sharedSizeBytes);
    SS_HIP(hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
    return SS_OK;
  };
#define SS_SELL_LAUNCH(QTV, BINV, SLOT)                                                                      \
  do {                                                                                                       \
    static std::atomic<bool> attr_done{false};                                                               \
    if (!attr_done) {                                                                                        \
      SS_TRY(prepare(reinterpret_cast<const void*>(&spmm_sell_kernel<T, QTV, BINV>)));                       \
      attr_done = true;                                                                                      \
    }                                                                                                        \
    hipLaunchKernelGGL((spmm_sell_kernel<T, QTV, BINV>), grid, dim3(SELL_THREADS), lds, ctx().stream, a);    \
  } while (0)
  if constexpr (sizeof(T) == 4) {
    if (QT == 8) { if (W.binary) SS_SELL_LAUNCH(8, true, 0); else SS_SELL_LAUNCH(8, false, 1); }
    else if (QT == 4) { if (W.binary) SS_SELL_LAUNCH(4, true, 2); else SS_SELL_LAUNCH(4, false, 3); }
    else return fail(SS_EINVAL, "SELL tile width must be 4 or 8 (fp32)");
  } else {
    if (QT != 2) return fail(SS_EINVAL, "SELL tile width must be 2 (fp64)");
    if (W.binary) SS_SELL_LAUNCH(2, true, 0); else SS_SELL_LAUNCH(2, false, 1);
  }
#undef SS_SELL_LAUNCH
  SS_LAUNCH_CHECK();
  return SS_OK;
}

// ============================================================== stage 2, narrow, HBM-bound: R chunk in LDS
// F = W*R for B <= 4 columns.  W is cut into column chunks of KC (all of R's rows k0..k0+KC for the B
// columns fit in LDS), stored chunk-major with 16-bit local indices, sub-rows padded to 4 entries so
// that a lane streams 8 B of indices + 16 B of values per step; workgroup (c, slot) keeps chunk c of R
// in LDS and strides over the rows, GL lanes per sub-row, __shfl_xor to fold the lanes.
// Every non-zero of W is read exactly once from HBM (6 B instead of CSR's 8 B); partial sums per chunk
// are combined in fixed order by narrow_reduce_kernel.
template <class T>
struct NarrowArgs {
  const int* off;
  const unsigned short* idx;
  const T* val;
  int64_t M, K;
  int KC, nchunks, B;
  const T* R;
  int64_t ldr;
  T* F;       // direct output when nchunks == 1
  int64_t ldf;
  T* P;       // [nchunks][M][BV] otherwise
};

constexpr int NARROW_THREADS = 1024;

// Sum over each group of GL consecutive lanes (GL = 8, 16, 32, 64) with DPP moves only -- no LDS traffic, where
// __shfl_xor compiles to one ds_bpermute_b32 per step (at B = 4 the 5 x 4 permutes per row group were 0.07 ms of LDS
// time in a 0.18 ms launch).  quad_perm swaps inside quads, row_half_mirror / row_mirror fold 8 and 16 lanes (after the
// quad steps every lane of a quad holds the quad's sum, so the reversed order does not matter), row_bcast15 adds lane
// 15 of rows 0 and 2 to rows 1 and 3, row_bcast31 lane 31 to rows 2 and 3.  The order of the additions is fixed.
// The sum of a group is valid in its LAST lane (for GL <= 16 in all its lanes).
template <int CTRL, int ROW_MASK = 0xF>
__device__ __forceinline__ float dpp_add(float v) {
  return v + __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), CTRL, ROW_MASK, 0xF, false));
}
template <int CTRL, int ROW_MASK = 0xF>
__device__ __forceinline__ double dpp_add(double v) {
  const long long b = __double_as_longlong(v);
  const int lo = __builtin_amdgcn_update_dpp(0, (int)(b & 0xffffffffll), CTRL, ROW_MASK, 0xF, false);
  const int hi = __builtin_amdgcn_update_dpp(0, (int)(b >> 32), CTRL, ROW_MASK, 0xF, false);
  return v + __longlong_as_double(((long long)hi << 32) | (unsigned int)lo);
}
template <int GL, class T>
__device__ __forceinline__ T lane_group_sum(T v) {
  static_assert(GL == 8 || GL == 16 || GL == 32 || GL == 64, "group of 8, 16, 32 or 64 lanes");
  v = dpp_add<0xB1>(v);                       // quad_perm [1,0,3,2]
  v = dpp_add<0x4E>(v);                       // quad_perm [2,3,0,1]
  v = dpp_add<0x141>(v);                      // row_half_mirror
  if constexpr (GL >= 16) v = dpp_add<0x140>(v);        // row_mirror
  if constexpr (GL >= 32) v = dpp_add<0x142, 0xA>(v);   // row_bcast15 into rows 1 and 3
  if constexpr (GL >= 64) v = dpp_add<0x143, 0xC>(v);   // row_bcast31 into rows 2 and 3
  return v;
}

// VEC = columns (1, 2 or 4); GL = lanes that share one sub-row (64, 32, 16 or 8), so a wave streams 64/GL rows at once;
// UR row groups per step; NBQ quads requested per lane and row.
template <class T, int VEC, int GL, int UR, int NBQ>
__global__ void __launch_bounds__(NARROW_THREADS) spmm_chunked_narrow_kernel(NarrowArgs<T> a) {
  constexpr int BV = VEC;
  extern __shared__ __align__(16) unsigned char smem_raw[];
  T* tile = reinterpret_cast<T*>(smem_raw);  // [KC + 1][BV]; row KC stays zero (padding target)
  using V = Vec<T, VEC>;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, nwaves = blockDim.x >> 6;
  const int c = blockIdx.x % a.nchunks;
  const int slot = blockIdx.x / a.nchunks, nslots = gridDim.x / a.nchunks;
  const int64_t k0 = (int64_t)c * a.KC;
  const int kn = (int)((a.K - k0 < a.KC) ? (a.K - k0) : a.KC);

  // 32-byte tile rows (two 16-byte halves per non-zero): all lanes fetch the same half at the same time, so with
  // a plain layout only every other 16-byte slot of the 256-byte LDS line is ever hit (a fixed 2-way conflict);
  // half h of row k is stored at h ^ ((k >> 3) & 1), which spreads random k over all 16 slots
  constexpr bool SWZ = (BV * sizeof(T) == 32);
  constexpr int HB = 16 / (int)sizeof(T);  // values per 16-byte half
  // rows of R packed without gaps (ldr == B == BV) and a 16-byte aligned chunk: the tile is a plain copy, moved in
  // 16-byte pieces (KC is a multiple of 4 by construction); otherwise element by element
  constexpr int PW16 = 16 / (int)sizeof(T);
  const bool packed = a.ldr == BV && a.B == BV &&
                      ((reinterpret_cast<uintptr_t>(a.R + k0 * a.ldr) & 15) == 0) && ((a.KC * BV) % PW16 == 0);
  if (packed) {
    using P16 = Vec<T, PW16>;
    const P16* __restrict__ src = reinterpret_cast<const P16*>(a.R + k0 * a.ldr);
    P16* dst = reinterpret_cast<P16*>(tile);
    const int npieces = ((a.KC + 1) * BV + PW16 - 1) / PW16, nfull = (kn * BV) / PW16;
    for (int i = tid; i < npieces; i += blockDim.x) {
      P16 v;
      if (i < nfull) {
        v = src[i];
      } else {
#pragma unroll
        for (int e = 0; e < PW16; ++e) {
          const int x = i * PW16 + e;   // element of the tile; row x / BV
          v.v[e] = (x < kn * BV) ? a.R[k0 * a.ldr + x] : T(0);
        }
      }
      if ((i + 1) * PW16 <= (a.KC + 1) * BV) {
        // 32-byte tile rows: half h of row k sits at h ^ ((k >> 3) & 1) (see below), i.e. piece i at i ^ ((i >> 4) & 1)
        dst[SWZ ? (i ^ ((i >> 4) & 1)) : i] = v;
      } else {
#pragma unroll
        for (int e = 0; e < PW16; ++e)
          if (i * PW16 + e < (a.KC + 1) * BV) tile[i * PW16 + e] = v.v[e];
      }
    }
  } else {
    for (int e = tid; e < (a.KC + 1) * BV; e += blockDim.x) {
      const int k = e / BV, b = e - k * BV;
      const T v = (k < kn && b < a.B) ? a.R[(k0 + k) * a.ldr + b] : T(0);
      if constexpr (SWZ) tile[k * BV + ((((b / HB) ^ (k >> 3)) & 1) * HB) + (b % HB)] = v;
      else tile[e] = v;
    }
  }
  __syncthreads();
  auto tile_row = [&](int k) __attribute__((always_inline)) {
    V r;
    if constexpr (SWZ) {
      using H = Vec<T, HB>;
      const int s = (k >> 3) & 1;
      const H lo = *reinterpret_cast<const H*>(&tile[k * BV + s * HB]);
      const H hi = *reinterpret_cast<const H*>(&tile[k * BV + (s ^ 1) * HB]);
#pragma unroll
      for (int i = 0; i < HB; ++i) { r.v[i] = lo.v[i]; r.v[HB + i] = hi.v[i]; }
    } else {
      r = *reinterpret_cast<const V*>(&tile[k * BV]);
    }
    return r;
  };

  const int* __restrict__ off = a.off + (int64_t)c * a.M;
  {
    constexpr int RPS = 64 / GL;  // rows per wave-step
    const int sub = lane / GL, gl = lane % GL;
    const ushort4* __restrict__ ip = reinterpret_cast<const ushort4*>(a.idx);
    const Vec<T, 4>* __restrict__ vp = reinterpret_cast<const Vec<T, 4>*>(a.val);
    const int64_t stride = (int64_t)nslots * nwaves * RPS * UR;
    // Software pipeline over the row groups of this wave: while group i is gathered, the quads of group i+1 are in
    // flight and the sub-row bounds of group i+2 are being read, so the W stream never waits for a dependent load.
    // Every lane requests NBQ quads per row unconditionally (q, q + GL, ...; clamped to a valid quad, masked below):
    // loads stay out of branches and their waits stay counted.  Rows longer than NBQ * GL quads take the rolled tail.
    struct Bounds { int lo[UR], hi[UR]; };   // raw off[m], off[m + 1] (row clamped; validity is applied at use)
    // quads in flight for one row group; mask bit u*NBQ + nb: this lane's quad nb of row u is inside the sub-row,
    // bit 31: some row of the group is longer than NBQ * GL quads
    struct Quads { ushort4 iv[UR][NBQ]; Vec<T, 4> w[UR][NBQ]; unsigned mask; };
    auto bounds = [&](int64_t mb, Bounds& b) __attribute__((always_inline)) {
#pragma unroll
      for (int u = 0; u < UR; ++u) {
        const int64_t m = mb + u * RPS + sub;
        const int64_t mm = m < a.M ? m : a.M - 1;
        b.lo[u] = off[mm];
        b.hi[u] = off[mm + 1];
      }
    };
    auto issue = [&](int64_t mb, const Bounds& b, Quads& x) __attribute__((always_inline)) {
      unsigned mask = 0;
#pragma unroll
      for (int u = 0; u < UR; ++u) {
        const int oe = (mb + u * RPS + sub < a.M) ? b.hi[u] : b.lo[u];
#pragma unroll
        for (int nb = 0; nb < NBQ; ++nb) {
          const int q = b.lo[u] + gl + nb * GL;
          const bool in = q < oe;
          const int qq = in ? q : b.lo[u];
          {
            // W is read exactly once per launch: non-temporal loads keep the stream from displacing the tile of R and the
            // partial sums in L2 (100k x 100k, 1 %: B = 1 0.124 -> 0.115 ms, B = 2 0.136 -> 0.120 ms, B = 4 0.185 -> 0.178 ms)
            typedef unsigned nt_u2 __attribute__((ext_vector_type(2)));
            typedef T nt_t4 __attribute__((ext_vector_type(4)));
            const nt_u2 ii = __builtin_nontemporal_load(reinterpret_cast<const nt_u2*>(&ip[qq]));
            const nt_t4 ww = __builtin_nontemporal_load(reinterpret_cast<const nt_t4*>(&vp[qq]));
            x.iv[u][nb] = ushort4((unsigned short)(ii.x & 0xffffu), (unsigned short)(ii.x >> 16), (unsigned short)(ii.y & 0xffffu),
                                  (unsigned short)(ii.y >> 16));
            x.w[u][nb].v[0] = ww.x; x.w[u][nb].v[1] = ww.y; x.w[u][nb].v[2] = ww.z; x.w[u][nb].v[3] = ww.w;
          }
          mask |= in ? (1u << (u * NBQ + nb)) : 0u;
        }
        mask |= (b.lo[u] + NBQ * GL < oe) ? 0x80000000u : 0u;
      }
      x.mask = mask;
    };
    auto quad = [&](T (&acc)[VEC], const ushort4 jv, const Vec<T, 4> x) __attribute__((always_inline)) {
      const V r0 = tile_row((int)jv.x);
      const V r1 = tile_row((int)jv.y);
      const V r2 = tile_row((int)jv.z);
      const V r3 = tile_row((int)jv.w);
#pragma unroll
      for (int i = 0; i < VEC; ++i) {
        acc[i] = fma(x.v[0], r0.v[i], acc[i]);
        acc[i] = fma(x.v[1], r1.v[i], acc[i]);
        acc[i] = fma(x.v[2], r2.v[i], acc[i]);
        acc[i] = fma(x.v[3], r3.v[i], acc[i]);
      }
    };
    int64_t mb = ((int64_t)slot * nwaves + wave) * RPS * UR;
    Bounds bn;
    Quads xa, xb;
    if (mb < a.M) {
      Bounds b0;
      bounds(mb, b0);
      bounds(mb + stride < a.M ? mb + stride : mb, bn);
      issue(mb, b0, xa);
    }
    // one row group: request the quads of the next group (its bounds arrived a step ago) and the bounds of the one
    // after, then gather the current group.  Two copies of the step alternate the quad registers (a copy of a
    // register with a load in flight would wait for it); only the bounds, long arrived, are moved.
    auto step = [&](const int64_t mb, const Quads& xc, Quads& xn) __attribute__((always_inline)) {
      // unconditional (the last group re-requests itself): no load sits in a branch
      const int64_t mb1 = mb + stride < a.M ? mb + stride : mb;
      const int64_t mb2 = mb + 2 * stride < a.M ? mb + 2 * stride : mb;
      Bounds bnn;
      bounds(mb2, bnn);
      issue(mb1, bn, xn);
      __builtin_amdgcn_sched_barrier(0);  // the requests go out BEFORE the gathers of the current group (hipcc sinks them otherwise)
      T acc[UR][VEC];
#pragma unroll
      for (int u = 0; u < UR; ++u) {
#pragma unroll
        for (int i = 0; i < VEC; ++i) acc[u][i] = T(0);
#pragma unroll
        for (int nb = 0; nb < NBQ; ++nb) {
          // lanes past the end of the sub-row hold a clamped (valid) quad: gather it with zero weights
          const bool has = (xc.mask >> (u * NBQ + nb)) & 1u;
          Vec<T, 4> w = xc.w[u][nb];
#pragma unroll
          for (int e = 0; e < 4; ++e) w.v[e] = has ? w.v[e] : T(0);
          quad(acc[u], xc.iv[u][nb], w);
        }
      }
      if (__any((int)(xc.mask >> 31))) {
        // rows longer than the NBQ * GL quads requested ahead (rare by the choice of GL): bounds re-read, rolled loop
#pragma unroll
        for (int u = 0; u < UR; ++u) {
          const int64_t m = mb + u * RPS + sub;
          if (m < a.M) {
            const int lo = off[m], hi = off[m + 1];
            for (int q = lo + gl + NBQ * GL; q < hi; q += GL) quad(acc[u], ip[q], vp[q]);
          }
        }
      }
#pragma unroll
      for (int u = 0; u < UR; ++u) {
#pragma unroll
        for (int i = 0; i < VEC; ++i) acc[u][i] = lane_group_sum<GL>(acc[u][i]);
        const int64_t m = mb + u * RPS + sub;
        if (gl == GL - 1 && m < a.M) {   // the group's sum sits in its last lane
          if (a.P) {
            T* p = a.P + ((int64_t)c * a.M + m) * BV;
#pragma unroll
            for (int i = 0; i < VEC; ++i) p[i] = acc[u][i];
          } else {
#pragma unroll
            for (int i = 0; i < VEC; ++i)
              if (i < a.B) a.F[m * a.ldf + i] = acc[u][i];
          }
        }
      }
      bn = bnn;
    };
    while (mb < a.M) {
      step(mb, xa, xb);
      mb += stride;
      if (mb >= a.M) break;
      step(mb, xb, xa);
      mb += stride;
    }
  }
}

// F[m][0..B) = sum of the per-chunk partial sums, in chunk order (one thread per row: BV <= 4 values)
template <class T, int BV>
__global__ void narrow_reduce_kernel(const T* __restrict__ P, int nchunks, int64_t M, int B, T* __restrict__ F,
                                     int64_t ldf) {
  using PV = Vec<T, BV>;
  for (int64_t m = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; m < M; m += (int64_t)gridDim.x * blockDim.x) {
    PV s = *reinterpret_cast<const PV*>(P + m * BV);
    for (int c = 1; c < nchunks; ++c) {
      const PV t = *reinterpret_cast<const PV*>(P + ((int64_t)c * M + m) * BV);
#pragma unroll
      for (int e = 0; e < BV; ++e) s.v[e] += t.v[e];
    }
#pragma unroll
    for (int e = 0; e < BV; ++e)
      if (e < B) F[m * ldf + e] = s.v[e];
  }
}

template <class T>
int narrow_chunk_cols(int bv) {
  int64_t kc = (int64_t)(160 * 1024) / ((int64_t)bv * (int64_t)sizeof(T)) - 1;
  if (kc > 65535) kc = 65535;
  kc &= ~3LL;  // chunks of R start on 16-byte boundaries (vector staging of the tile)
  return (int)kc;
}

template <class T, int VEC, int GL, int UR, int NBQ = 1>
static int launch_narrow_variant(const NarrowArgs<T>& a, unsigned grid, size_t lds) {
  static std::atomic<bool> attr_set{false};
  if (!attr_set) {
    SS_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(&spmm_chunked_narrow_kernel<T, VEC, GL, UR, NBQ>),
                               hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
    attr_set = true;
  }
  hipLaunchKernelGGL((spmm_chunked_narrow_kernel<T, VEC, GL, UR, NBQ>), dim3(grid), dim3(NARROW_THREADS), lds,
                     ctx().stream, a);
  SS_LAUNCH_CHECK();
  return SS_OK;
}

// Row groups per step (UR) such that two sets of quads in flight (UR * NBQ quads of 8 + 4*sizeof(T) bytes per lane and
// set), the UR * VEC accumulators, four gathered tile rows and the bounds stay inside the 128 registers a lane has at 16
// waves per CU.
constexpr int narrow_ur(int elem, int vec, int nbq) {
  const int per_quad = 2 + elem;  // registers
  int ur = 4;
  while (ur > 1 && 2 * ur * nbq * per_quad + (ur + 4) * vec * (elem / 4) + 4 * ur + 24 > 124) ur >>= 1;
  return ur;
}

template <class T, int VEC>
static int launch_narrow_width(const NarrowArgs<T>& a, unsigned grid, size_t lds, double mean_quads) {
  constexpr int E = (int)sizeof(T);
  // GL lanes per row, one request per lane (two above 64 quads): the smallest capacity about 10 % above the mean
  // sub-row length in quads.  Measured (100k x 100k, 1 %): lanes past the end of a sub-row are not free (a step is
  // bound by the latency of its requests, so rows per step count: B = 4, mean 25 quads, 32 vs 64 lanes per row
  // 0.20 vs 0.35 ms), while the rolled tail for the few longer rows costs little
  const double need = 1.1 * mean_quads + 1.0;
  if (need > 64.0) return launch_narrow_variant<T, VEC, 64, narrow_ur(E, VEC, 2), 2>(a, grid, lds);
  if (need > 32.0) return launch_narrow_variant<T, VEC, 64, narrow_ur(E, VEC, 1)>(a, grid, lds);
  if (need > 16.0) return launch_narrow_variant<T, VEC, 32, narrow_ur(E, VEC, 1)>(a, grid, lds);
  if (need > 8.0) return launch_narrow_variant<T, VEC, 16, narrow_ur(E, VEC, 1)>(a, grid, lds);
  return launch_narrow_variant<T, VEC, 8, narrow_ur(E, VEC, 1)>(a, grid, lds);
}

template <class T>
int launch_spmm_chunked_narrow(const DevChunked<T>& W, int bv, const T* R, int64_t ldr, int B, T* F, int64_t ldf,
                               DevBuf<T>& partial) {
  if (W.rows <= 0 || B <= 0) return SS_OK;
  if (W.align != 4) return fail(SS_EINVAL, "narrow operand must be quad-aligned");
  path_add("spmm_chunked_narrow");
  NarrowArgs<T> a{};
  a.off = W.off.p; a.idx = W.idx.p; a.val = W.val.p;
  a.M = W.rows; a.K = W.cols; a.KC = W.SC; a.nchunks = W.nchunks; a.B = B;
  a.R = R; a.ldr = ldr; a.F = F; a.ldf = ldf; a.P = nullptr;
  if (W.nchunks > 1) {
    const size_t need = (size_t)W.nchunks * (size_t)W.rows * (size_t)bv;
    if (partial.n < need) SS_TRY(partial.alloc(need));
    a.P = partial.p;
  }
  // one resident round: the 160 KB tile allows one workgroup per CU, and every workgroup strides over
  // all rows of its chunk, so a partial second round would only add idle CUs
  int nslots = ctx().num_cu / W.nchunks;
  const int64_t max_slots = ceil_div(W.rows, NARROW_THREADS / 64);
  if (nslots > max_slots) nslots = (int)max_slots;
  if (nslots < 1) nslots = 1;
  const unsigned grid = (unsigned)(W.nchunks * nslots);
  const size_t lds = (size_t)(W.SC + 1) * bv * sizeof(T);
  const double mean_quads = (double)W.stored / 4.0 / ((double)W.rows * (double)W.nchunks);
  int rc;
  switch (bv) {
    case 1: rc = launch_narrow_width<T, 1>(a, grid, lds, mean_quads); break;
    case 2: rc = launch_narrow_width<T, 2>(a, grid, lds, mean_quads); break;
    case 4: rc = launch_narrow_width<T, 4>(a, grid, lds, mean_quads); break;
    default: return fail(SS_EINVAL, "narrow width must be 1, 2 or 4");
  }
  SS_TRY(rc);
  if (W.nchunks > 1) {
    const dim3 rg(grid_1d(W.rows, 256)), rb(256);
    switch (bv) {
      case 1: hipLaunchKernelGGL((narrow_reduce_kernel<T, 1>), rg, rb, 0, ctx().stream, partial.p, W.nchunks, W.rows, B, F, ldf); break;
      case 2: hipLaunchKernelGGL((narrow_reduce_kernel<T, 2>), rg, rb, 0, ctx().stream, partial.p, W.nchunks, W.rows, B, F, ldf); break;
      default: hipLaunchKernelGGL((narrow_reduce_kernel<T, 4>), rg, rb, 0, ctx().stream, partial.p, W.nchunks, W.rows, B, F, ldf); break;
    }
    SS_LAUNCH_CHECK();
  }
  return SS_OK;
}

// ============================================================== transpose (layout conversion)
// in: rows x cols, element (r,c) at in[r*ldin + c]; out: (c,r) at out[c*ldout + r]
template <class T>
__global__ void __launch_bounds__(256) transpose_kernel(const T* __restrict__ in, int64_t rows, int64_t cols,
                                                        int64_t ldin, T* __restrict__ out, int64_t ldout) {
  __shared__ T tile[64][65];
  const int64_t c0 = (int64_t)blockIdx.x * 64, r0 = (int64_t)blockIdx.y * 64;
  const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
  for (int i = ty; i < 64; i += 4) {
    const int64_t r = r0 + i, c = c0 + tx;
    tile[i][tx] = (r < rows && c < cols) ? in[r * ldin + c] : T(0);
  }
  __syncthreads();
  for (int i = ty; i < 64; i += 4) {
    const int64_t c = c0 + i, r = r0 + tx;
    if (r < rows && c < cols) out[c * ldout + r] = tile[tx][i];
  }
}

template <class T>
int launch_transpose(const T* in, int64_t rows, int64_t cols, int64_t ldin, T* out, int64_t ldout) {
  if (rows <= 0 || cols <= 0) return SS_OK;
  dim3 grid((unsigned)ceil_div(cols, 64), (unsigned)ceil_div(rows, 64));
  hipLaunchKernelGGL(transpose_kernel<T>, grid, dim3(256), 0, ctx().stream, in, rows, cols, ldin, out, ldout);
  SS_LAUNCH_CHECK();
  return SS_OK;
}

// ============================================================== unpermute (skew-sorted SELL results)
template <class T>
__global__ void unpermute_kernel(const T* __restrict__ in, int64_t ldin, int64_t nrows, int64_t nt,
                                 const int* __restrict__ vfirst, const int* __restrict__ inv,
                                 const int* __restrict__ clean_deg, T* __restrict__ out, int64_t ldout) {
  const int64_t r = blockIdx.y;
  const T* src = in + r * ldin;
  T* dst = out + r * ldout;
  for (int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; t < nt; t += (int64_t)gridDim.x * blockDim.x) {
    T v = T(0);
    for (int x = vfirst[t]; x < vfirst[t + 1]; ++x) v += src[inv[x]];  // the row of `in` sits in L2 meanwhile
    dst[t] = (clean_deg != nullptr && clean_deg[t] == 0) ? T(-99) : v;
  }
}

template <class T>
int launch_unpermute(const T* in, int64_t ldin, int64_t nrows, int64_t nt, const int* vfirst, const int* inv,
                     const int* clean_deg, T* out, int64_t ldout) {
  if (nrows <= 0 || nt <= 0) return SS_OK;
  for (int64_t r0 = 0; r0 < nrows; r0 += 65535) {
    const int64_t nb = nrows - r0 < 65535 ? nrows - r0 : 65535;
    dim3 grid((unsigned)grid_1d(nt, 256, 64), (unsigned)nb);
    hipLaunchKernelGGL(unpermute_kernel<T>, grid, dim3(256), 0, ctx().stream, in + r0 * ldin, ldin, nb, nt, vfirst,
                       inv, clean_deg, out + r0 * ldout, ldout);
    SS_LAUNCH_CHECK();
  }
  return SS_OK;
}

// ============================================================== k-fold: degrees of the graph without a fold's members
// construct(y, X, queries) (src/core.jl:148-201) drops the query rows from the sources and the feature
// columns named after them: kf[f] loses one per member row with X[g,f] != 0, ks[s] one per member feature
// column with X[s,g] != 0, kt[t] one per member with Y[g,t] != 0.  One wave per member; integer atomics.
__global__ void fold_degrees_kernel(const int* __restrict__ xptr, const int* __restrict__ xidx,
                                    const int* __restrict__ tptr, const int* __restrict__ tidx,
                                    const int* __restrict__ yptr, const int* __restrict__ yidx,
                                    const int* __restrict__ members, int64_t nmembers, int* __restrict__ kf,
                                    int* __restrict__ ks, int* __restrict__ kt) {
  const int lane = threadIdx.x & 63;
  const int64_t wave0 = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
  const int64_t nwaves = ((int64_t)gridDim.x * blockDim.x) >> 6;
  for (int64_t m = wave0; m < nmembers; m += nwaves) {
    const int g = members[m];
    for (int x = xptr[g] + lane; x < xptr[g + 1]; x += 64) atomicSub(&kf[xidx[x]], 1);
    for (int x = tptr[g] + lane; x < tptr[g + 1]; x += 64) atomicSub(&ks[tidx[x]], 1);
    for (int x = yptr[g] + lane; x < yptr[g + 1]; x += 64) atomicSub(&kt[yidx[x]], 1);
  }
}

template <class T>
int launch_fold_degrees(const DevCsr<T>& X, const DevCsr<T>& XT, const DevCsr<T>& Y, const int* members,
                        int64_t nmembers, int* kf, int* ks, int* kt) {
  if (nmembers <= 0) return SS_OK;
  hipLaunchKernelGGL(fold_degrees_kernel, dim3(grid_1d(nmembers * 64, 256)), dim3(256), 0, ctx().stream, X.ptr.p,
                     X.idx.p, XT.ptr.p, XT.idx.p, Y.ptr.p, Y.idx.p, members, nmembers, kf, ks, kt);
  SS_LAUNCH_CHECK();
  return SS_OK;
}

// reciprocal degrees of the fold's graph; members are neither features nor sources in it (-> 0)
template <class T>
__global__ void fold_inverse_kernel(const int* __restrict__ kf, const int* __restrict__ ks,
                                    const int* __restrict__ fold, int phi, int64_t nf, int64_t ns,
                                    T* __restrict__ inv_kf, T* __restrict__ inv_ks) {
  const int64_t n = nf > ns ? nf : ns;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    const bool member = fold[i] == phi;
    if (i < nf) inv_kf[i] = (!member && kf[i] > 0) ? T(1) / T(kf[i]) : T(0);
    if (i < ns) inv_ks[i] = (!member && ks[i] > 0) ? T(1) / T(ks[i]) : T(0);
  }
}

template <class T>
int launch_fold_inverse(const int* kf, const int* ks, const int* fold, int phi, int64_t nf, int64_t ns, T* inv_kf,
                        T* inv_ks) {
  const int64_t n = nf > ns ? nf : ns;
  if (n <= 0) return SS_OK;
  hipLaunchKernelGGL(fold_inverse_kernel<T>, dim3(grid_1d(n, 256)), dim3(256), 0, ctx().stream, kf, ks, fold, phi, nf,
                     ns, inv_kf, inv_ks);
  SS_LAUNCH_CHECK();
  return SS_OK;
}

// ============================================================== top-L per row (ranked evaluation on the device)
// One workgroup per row.  Radix select (4 passes of 8 bits over an order-preserving integer image of the
// float) finds the L-th largest key; elements above it are collected, ties at the threshold are taken in
// ascending column order (what a stable descending sortperm does), then the L pairs are bitonic-sorted in LDS.
__device__ __forceinline__ unsigned float_key(float f) {
  const unsigned u = __float_as_uint(f);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);  // larger float <=> larger key
}

constexpr int TOPL_THREADS = 256;
constexpr int TOPL_MAX = 1024;

// `only_flagged`: second launch after topl_bound_kernel -- serve only the rows it marked (oidx[row*L] == -1)
__global__ void __launch_bounds__(TOPL_THREADS) topl_kernel(const float* __restrict__ scores, int64_t ncols, int64_t ld,
                                                            int L, int* __restrict__ oidx, float* __restrict__ oval,
                                                            int only_flagged) {
  if (only_flagged && oidx[(int64_t)blockIdx.x * L] != -1) return;
  __shared__ unsigned hist[256];
  __shared__ unsigned long long sel[TOPL_MAX];  // (key << 32) | ~column : descending sort = score desc, column asc
  __shared__ unsigned s_prefix, s_need, s_count, s_base;
  const int tid = threadIdx.x;
  const float* row = scores + (int64_t)blockIdx.x * ld;
  if (tid == 0) { s_prefix = 0; s_need = (unsigned)L; }
  __syncthreads();
  // ---- radix select: after the loop s_prefix is the key of the L-th largest element,
  //      s_need how many elements equal to it are wanted
  for (int pass = 0; pass < 4; ++pass) {
    const int shift = 24 - 8 * pass;
    hist[tid] = 0;
    __syncthreads();
    const unsigned prefix = s_prefix;
    const unsigned himask = pass == 0 ? 0u : (0xFFFFFFFFu << (shift + 8));
    for (int64_t c = tid; c < ncols; c += TOPL_THREADS) {
      const unsigned k = float_key(row[c]);
      if ((k & himask) == prefix) atomicAdd(&hist[(k >> shift) & 255u], 1u);
    }
    __syncthreads();
    if (tid == 0) {
      unsigned need = s_need, b = 255;
      for (;; --b) {  // buckets from the largest digit down
        if (hist[b] >= need) break;
        need -= hist[b];
        if (b == 0) break;
      }
      s_prefix = prefix | (b << shift);
      s_need = need;
    }
    __syncthreads();
  }
  const unsigned kth = s_prefix;
  const unsigned need_eq = s_need;
  if (tid == 0) { s_count = 0; s_base = 0; }
  __syncthreads();
  // ---- strictly above the threshold: any order (sorted afterwards)
  for (int64_t c = tid; c < ncols; c += TOPL_THREADS) {
    const unsigned k = float_key(row[c]);
    if (k > kth) {
      const unsigned p = atomicAdd(&s_count, 1u);
      sel[p] = ((unsigned long long)k << 32) | (unsigned)(~(unsigned)c);
    }
  }
  __syncthreads();
  const unsigned above = s_count;
  // ---- ties at the threshold: the first need_eq in column order (block-wide ordered compaction)
  for (int64_t c0 = 0; c0 < ncols && s_base < need_eq; c0 += TOPL_THREADS) {
    const int64_t c = c0 + tid;
    const bool eq = c < ncols && float_key(row[c]) == kth;
    // ordered rank of this thread among the equal ones of the chunk: wave ballots + per-wave offsets in hist[]
    const unsigned long long m = __ballot(eq);
    const int lane = tid & 63, w = tid >> 6;
    if (lane == 0) hist[w] = (unsigned)__popcll(m);
    __syncthreads();
    unsigned before = s_base;
    for (int i = 0; i < w; ++i) before += hist[i];
    const unsigned r = before + (unsigned)__popcll(m & ((1ull << lane) - 1ull));
    if (eq && r < need_eq) sel[above + r] = ((unsigned long long)kth << 32) | (unsigned)(~(unsigned)c);
    __syncthreads();
    if (tid == 0) s_base += hist[0] + hist[1] + hist[2] + hist[3];
    __syncthreads();
  }
  // ---- sort the L pairs descending (bitonic on the next power of two, padding with 0 = smallest)
  int P = 1;
  while (P < L) P <<= 1;
  for (int i = L + tid; i < P; i += TOPL_THREADS) sel[i] = 0ull;
  __syncthreads();
  for (int k = 2; k <= P; k <<= 1)
    for (int j = k >> 1; j > 0; j >>= 1) {
      for (int i = tid; i < P; i += TOPL_THREADS) {
        const int ixj = i ^ j;
        if (ixj > i) {
          const unsigned long long a = sel[i], b = sel[ixj];
          const bool desc = (i & k) == 0;
          if (desc ? (a < b) : (a > b)) { sel[i] = b; sel[ixj] = a; }
        }
      }
      __syncthreads();
    }
  for (int i = tid; i < L; i += TOPL_THREADS) {
    const unsigned long long e = sel[i];
    const unsigned c = ~(unsigned)(e & 0xFFFFFFFFull);
    oidx[(int64_t)blockIdx.x * L + i] = (int)c;
    oval[(int64_t)blockIdx.x * L + i] = row[c];
  }
}

// Fast path (two reads of the row instead of six, no per-element histogram): every thread takes the maximum key of its
// strided share; the L-th largest of those 1024 maxima is a lower bound of the L-th largest element (they are L
// distinct elements), so only elements at or above it can be among the top L.  They are collected as (key, ~column)
// pairs -- unique, and their descending order IS score descending / column ascending, so ties need no special case --
// and bitonic-sorted in LDS.  A row with more than TOPL2_CAP candidates (long runs of equal scores at the bound:
// e.g. mostly zeros) is marked with oidx = -1 and left to the radix-select kernel above.
constexpr int TOPL2_THREADS = 1024;
constexpr int TOPL2_CAP = 4096;

__global__ void __launch_bounds__(TOPL2_THREADS) topl_bound_kernel(const float* __restrict__ scores, int64_t ncols,
                                                                   int64_t ld, int L, int* __restrict__ oidx,
                                                                   float* __restrict__ oval) {
  __shared__ unsigned long long cand[TOPL2_CAP];
  __shared__ unsigned hist[256];
  __shared__ unsigned s_prefix, s_need, s_count;
  const int tid = threadIdx.x, lane = tid & 63;
  const float* row = scores + (int64_t)blockIdx.x * ld;
  unsigned mx = 0;  // smaller than the key of any float
  for (int64_t c = tid; c < ncols; c += TOPL2_THREADS) {
    const unsigned k = float_key(row[c]);
    mx = k > mx ? k : mx;
  }
  if (tid == 0) { s_prefix = 0; s_need = (unsigned)L; s_count = 0; }
  __syncthreads();
  // radix select of the L-th largest thread maximum (L <= 1024 = number of maxima; threads without elements hold 0)
  for (int pass = 0; pass < 4; ++pass) {
    const int shift = 24 - 8 * pass;
    if (tid < 256) hist[tid] = 0;
    __syncthreads();
    const unsigned prefix = s_prefix;
    const unsigned himask = pass == 0 ? 0u : (0xFFFFFFFFu << (shift + 8));
    if ((mx & himask) == prefix) atomicAdd(&hist[(mx >> shift) & 255u], 1u);
    __syncthreads();
    if (tid == 0) {
      unsigned need = s_need, b = 255;
      for (;; --b) {
        if (hist[b] >= need) break;
        need -= hist[b];
        if (b == 0) break;
      }
      s_prefix = prefix | (b << shift);
      s_need = need;
    }
    __syncthreads();
  }
  const unsigned bound = s_prefix;
  // candidates: one counter update per wave (ballot), order irrelevant (sorted below)
  for (int64_t c0 = 0; c0 < ncols; c0 += TOPL2_THREADS) {
    const int64_t c = c0 + tid;
    const unsigned k = c < ncols ? float_key(row[c]) : 0u;
    const bool in = c < ncols && k >= bound;
    const unsigned long long m = __ballot(in);
    if (m) {
      unsigned base = 0;
      if (lane == 0) base = atomicAdd(&s_count, (unsigned)__popcll(m));
      base = __shfl(base, 0);
      const unsigned p = base + (unsigned)__popcll(m & ((1ull << lane) - 1ull));
      if (in && p < (unsigned)TOPL2_CAP) cand[p] = ((unsigned long long)k << 32) | (unsigned)(~(unsigned)c);
    }
  }
  __syncthreads();
  const unsigned n = s_count;
  if (n > (unsigned)TOPL2_CAP) {
    if (tid == 0) oidx[(int64_t)blockIdx.x * L] = -1;
    return;
  }
  int P = 1;
  while (P < (int)n) P <<= 1;   // n >= L
  for (int i = (int)n + tid; i < P; i += TOPL2_THREADS) cand[i] = 0ull;
  __syncthreads();
  for (int k = 2; k <= P; k <<= 1)
    for (int j = k >> 1; j > 0; j >>= 1) {
      for (int i = tid; i < P; i += TOPL2_THREADS) {
        const int ixj = i ^ j;
        if (ixj > i) {
          const unsigned long long a = cand[i], b = cand[ixj];
          const bool desc = (i & k) == 0;
          if (desc ? (a < b) : (a > b)) { cand[i] = b; cand[ixj] = a; }
        }
      }
      __syncthreads();
    }
  for (int i = tid; i < L; i += TOPL2_THREADS) {
    const unsigned long long e = cand[i];
    const unsigned c = ~(unsigned)(e & 0xFFFFFFFFull);
    oidx[(int64_t)blockIdx.x * L + i] = (int)c;
    oval[(int64_t)blockIdx.x * L + i] = row[c];
  }
}

int launch_topl(const float* scores, int64_t nrows, int64_t ncols, int64_t ld, int L, int* oidx, float* oval) {
  if (nrows <= 0) return SS_OK;
  if (L < 1 || L > TOPL_MAX || L > ncols) return fail(SS_EINVAL, "top-L needs 1 <= L <= min(%d, ncols)", TOPL_MAX);
  const bool fast = !env_off("SS_TOPL_BOUND");
  for (int64_t r0 = 0; r0 < nrows; r0 += (1 << 30)) {
    const int64_t nb = nrows - r0 < (1 << 30) ? nrows - r0 : (1 << 30);
    if (fast) {
      hipLaunchKernelGGL(topl_bound_kernel, dim3((unsigned)nb), dim3(TOPL2_THREADS), 0, ctx().stream, scores + r0 * ld,
                         ncols, ld, L, oidx + r0 * L, oval + r0 * L);
      SS_LAUNCH_CHECK();
    }
    hipLaunchKernelGGL(topl_kernel, dim3((unsigned)nb), dim3(TOPL_THREADS), 0, ctx().stream, scores + r0 * ld, ncols, ld,
                       L, oidx + r0 * L, oval + r0 * L, fast ? 1 : 0);
    SS_LAUNCH_CHECK();
  }
  return SS_OK;
}

// ============================================================== LOO clean! fix-up
// In fold i target t has degree kt[t] - [Y[i,t] != 0] (src/core.jl:479): the kt == 0 columns are
// flagged by the SpMM epilogue, here the columns whose single edge belongs to the query itself.
template <class T>
__global__ void loo_clean_fix_kernel(const int* __restrict__ tptr, const int* __restrict__ tidx,
                                     const int* __restrict__ kt, int64_t nt, int64_t i_begin, int64_t nrows,
                                     T* __restrict__ out, int64_t ld) {
  for (int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; t < nt; t += (int64_t)gridDim.x * blockDim.x) {
    if (kt[t] == 1) {
      const int64_t s = tidx[tptr[t]];
      if (s >= i_begin && s < i_begin + nrows) out[(s - i_begin) * ld + t] = T(-99);
    }
  }
}

template <class T>
int launch_loo_clean_fix(const DevCsr<T>& YsT, const int* kt, int64_t i_begin, int64_t nrows, T* out, int64_t ld) {
  if (YsT.rows <= 0 || nrows <= 0) return SS_OK;
  hipLaunchKernelGGL(loo_clean_fix_kernel<T>, dim3(grid_1d(YsT.rows, 256)), dim3(256), 0, ctx().stream,
                     YsT.ptr.p, YsT.idx.p, kt, YsT.rows, i_begin, nrows, out, ld);
  SS_LAUNCH_CHECK();
  return SS_OK;
}

// ============================================================== explicit instantiations
// ============================================================== similarity producer (the step before featurize)
// S[i][j] = sum_k min(F[i,k], F[j,k]) / sum_k max(F[i,k], F[j,k]): the weighted Jaccard (Ruzicka) similarity of
// the reference's tutorial, `1 .- pairwise(Jaccard(), X, dims=1)` (docs/src/tutorial/fishers-flowers.jl:66;
// Distances.jl: distance 0 when both rows are all zero).  F: n x d column-major; S: n x n column-major.
// 64 x 64 tile per workgroup, 4 x 4 pairs per thread, feature columns staged 16 at a time through LDS; only the
// tiles on and above the diagonal are computed, the mirror image is written with them.
template <class T>
__global__ void __launch_bounds__(256) jaccard_kernel(const T* __restrict__ F, int64_t n, int64_t d, int64_t ld,
                                                      T* __restrict__ S, int64_t lds_) {
  constexpr int TS = 64, BK = 16;
  if (blockIdx.y < blockIdx.x) return;  // lower triangle comes from the mirror write
  __shared__ T A[BK][TS + 1];
  __shared__ T B[BK][TS + 1];
  const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
  const int64_t i0 = (int64_t)blockIdx.x * TS, j0 = (int64_t)blockIdx.y * TS;
  T smin[4][4], smax[4][4];
#pragma unroll
  for (int a = 0; a < 4; ++a)
#pragma unroll
    for (int b = 0; b < 4; ++b) { smin[a][b] = T(0); smax[a][b] = T(0); }
  for (int64_t k0 = 0; k0 < d; k0 += BK) {
    for (int e = tid; e < BK * TS; e += 256) {
      const int kk = e / TS, r = e % TS;
      const int64_t k = k0 + kk;
      A[kk][r] = (k < d && i0 + r < n) ? F[i0 + r + k * ld] : T(0);
      B[kk][r] = (k < d && j0 + r < n) ? F[j0 + r + k * ld] : T(0);
    }
    __syncthreads();
#pragma unroll
    for (int kk = 0; kk < BK; ++kk) {
      T av[4], bv[4];
#pragma unroll
      for (int a = 0; a < 4; ++a) av[a] = A[kk][tx + 16 * a];
#pragma unroll
      for (int b = 0; b < 4; ++b) bv[b] = B[kk][ty + 16 * b];
#pragma unroll
      for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int b = 0; b < 4; ++b) {
          smin[a][b] += av[a] < bv[b] ? av[a] : bv[b];
          smax[a][b] += av[a] < bv[b] ? bv[b] : av[a];
        }
    }
    __syncthreads();
  }
#pragma unroll
  for (int a = 0; a < 4; ++a)
#pragma unroll
    for (int b = 0; b < 4; ++b) {
      const int64_t i = i0 + tx + 16 * a, j = j0 + ty + 16 * b;
      if (i < n && j < n) {
        const T v = smax[a][b] == T(0) ? T(1) : smin[a][b] / smax[a][b];
        S[i + j * lds_] = v;
        S[j + i * lds_] = v;
      }
    }
}

template <class T>
int launch_jaccard(const T* F, int64_t n, int64_t d, int64_t ld, T* S, int64_t lds_) {
  if (n <= 0) return SS_OK;
  const unsigned g = (unsigned)ceil_div(n, 64);
  hipLaunchKernelGGL(jaccard_kernel<T>, dim3(g, g), dim3(256), 0, ctx().stream, F, n, d, ld, S, lds_);
  SS_LAUNCH_CHECK();
  return SS_OK;
}

#define SS_INSTANTIATE(T)                                                                                   \
  template int launch_cutoff<T>(const T*, int64_t, int64_t, int64_t, T, bool, T*, int64_t);                 \
  template int launch_jaccard<T>(const T*, int64_t, int64_t, int64_t, T*, int64_t);                        \
  template int launch_row_degree<T>(const T*, int64_t, int64_t, int64_t, int*);                             \
  template int launch_spread_dense<T>(const T*, int64_t, int64_t, int64_t, const int*, T*, int64_t);        \
  template int launch_fold_degrees<T>(const DevCsr<T>&, const DevCsr<T>&, const DevCsr<T>&, const int*,     \
                                      int64_t, int*, int*, int*);                                           \
  template int launch_fold_inverse<T>(const int*, const int*, const int*, int, int64_t, int64_t, T*, T*);   \
  template int sell_max_chunk<T>(int);                                                                      \
  template int launch_spmm_sell<T>(const DevSell<T>&, const T*, int64_t, int64_t, T*, int64_t, const int*,  \
                                   const int*);                                                             \
  template int narrow_chunk_cols<T>(int);                                                                   \
  template int launch_spmm_chunked_narrow<T>(const DevChunked<T>&, int, const T*, int64_t, int, T*, int64_t, \
                                             DevBuf<T>&);                                                   \
  template int launch_transpose<T>(const T*, int64_t, int64_t, int64_t, T*, int64_t);                       \
  template int launch_unpermute<T>(const T*, int64_t, int64_t, int64_t, const int*, const int*, const int*, T*, \
                                   int64_t);                                                                \
  template int launch_loo_clean_fix<T>(const DevCsr<T>&, const int*, int64_t, int64_t, T*, int64_t);
SS_INSTANTIATE(float)
SS_INSTANTIATE(double)

}  // namespace ss
