// extern "C" surface of libsimspread_hip.so (see include/simspread_hip.h for the contract and the
// reference methods each entry point stands behind).  Host-side orchestration only: argument
// checks, staging of caller buffers, the stage-1 / stage-2 launch sequence, event timing.
#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <mutex>
#include <new>
#include <shared_mutex>
#include <type_traits>

#include "graph.hpp"
#include "pair_tile.hpp"  // PROFILE_CUTS_MAX

namespace ss {

// ------------------------------------------------------------------ errors / context
std::string& last_error() {
  static thread_local std::string msg;
  return msg;
}

int fail(int code, const char* fmt, ...) {
  char buf[1024];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof(buf), fmt, ap);
  va_end(ap);
  last_error() = buf;
  return code;
}

Ctx& ctx() {
  static Ctx c;
  return c;
}

int require_init() {
  if (!ctx().inited) return fail(SS_ENODEV, "ss_init(device) has not been called (the HIP path has no CPU fallback)");
  return SS_OK;
}

// registry of the per-thread Timing objects (their hipEvent pools): ss_shutdown destroys every thread's events, not
// only the calling thread's; a thread that exits destroys its own.  The mutex orders the two.
static std::mutex& timing_reg_mu() {
  static std::mutex m;
  return m;
}
static std::vector<Timing*>& timing_reg() {
  static std::vector<Timing*> v;
  return v;
}
Timing::Timing() {
  std::lock_guard<std::mutex> lk(timing_reg_mu());
  timing_reg().push_back(this);
}
Timing::~Timing() {
  std::lock_guard<std::mutex> lk(timing_reg_mu());
  auto& v = timing_reg();
  for (size_t i = 0; i < v.size(); ++i)
    if (v[i] == this) {
      v[i] = v.back();
      v.pop_back();
      break;
    }
  if (ctx().inited && generation == ctx().generation)
    for (hipEvent_t e : pool) (void)hipEventDestroy(e);
}

Timing& timing() {
  static thread_local Timing t;
  if (t.generation != ctx().generation) {  // the context these events belonged to is gone
    t.pool.clear();
    t.spans.clear();
    t.used = 0;
    t.hold = false;
    t.generation = ctx().generation;
  }
  return t;
}

std::string& path_note() {
  static thread_local std::string s;
  return s;
}
void path_add(const char* tag) {
  std::string& s = path_note();
  if (s.find(tag) != std::string::npos) return;
  if (!s.empty()) s += ",";
  s += tag;
}

void timing_begin_call() {
  Timing& t = timing();
  if (!t.hold) path_note().clear();
  t.dirty = true;
  if (t.hold) return;  // accumulate: the spans of this call join those already recorded
  t.used = 0;
  t.spans.clear();
  for (double& e : t.extra) e = 0;
  t.dirty = true;
}

int timing_mark(hipEvent_t* ev) {
  Timing& t = timing();
  if (t.used == t.pool.size()) {
    hipEvent_t e;
    SS_HIP(hipEventCreate(&e));
    t.pool.push_back(e);
  }
  *ev = t.pool[t.used++];
  SS_HIP(hipEventRecord(*ev, ctx().stream));
  return SS_OK;
}

void timing_span(int stage, hipEvent_t a, hipEvent_t b) { timing().spans.push_back({stage, a, b}); }
void timing_count(int stage, double inc) { timing().extra[stage] += inc; }

static int check_mem(int mem) {
  if (mem != SS_MEM_HOST && mem != SS_MEM_DEVICE) return fail(SS_EINVAL, "mem must be SS_MEM_HOST or SS_MEM_DEVICE");
  return SS_OK;
}
static int check_layout(int layout) {
  if (layout != SS_LAYOUT_ROWMAJOR && layout != SS_LAYOUT_COLMAJOR) return fail(SS_EINVAL, "unknown layout");
  return SS_OK;
}

// RAII marks: a span of one stage on the stream
struct StageTimer {
  int stage;
  hipEvent_t a = nullptr;
  bool ok = false;
  explicit StageTimer(int s) : stage(s) { ok = timing_mark(&a) == SS_OK; }
  void stop() {
    hipEvent_t b;
    if (ok && timing_mark(&b) == SS_OK) timing_span(stage, a, b);
    ok = false;
  }
  ~StageTimer() { stop(); }
};

// ------------------------------------------------------------------ element-wise entry points
template <class T>
static int cutoff_impl(const T* X, int64_t rows, int64_t cols, int64_t ld, T alpha, int weighted, T* out,
                       int64_t ldo, int mem) {
  SS_TRY(require_init());
  SS_TRY(check_mem(mem));
  if (rows < 0 || cols < 0 || ld < rows || ldo < rows) return fail(SS_EINVAL, "cutoff: bad shape / leading dimension");
  if (rows * cols == 0) return SS_OK;
  if (!X || !out) return fail(SS_EINVAL, "cutoff: NULL buffer");
  hipStream_t st = ctx().stream;
  if (mem == SS_MEM_DEVICE) {
    SS_TRY(launch_cutoff<T>(X, rows, cols, ld, alpha, weighted != 0, out, ldo));
    return SS_OK;
  }
  DevBuf<T> din, dout;
  SS_TRY(din.alloc((size_t)rows * cols));
  SS_TRY(dout.alloc((size_t)rows * cols));
  SS_HIP(hipMemcpy2DAsync(din.p, rows * sizeof(T), X, ld * sizeof(T), rows * sizeof(T), cols, hipMemcpyHostToDevice, st));
  SS_TRY(launch_cutoff<T>(din.p, rows, cols, rows, alpha, weighted != 0, dout.p, rows));
  SS_HIP(hipMemcpy2DAsync(out, ldo * sizeof(T), dout.p, rows * sizeof(T), rows * sizeof(T), cols, hipMemcpyDeviceToHost, st));
  SS_HIP(hipStreamSynchronize(st));
  return SS_OK;
}

template <class T>
static int row_degree_impl(const T* G, int64_t rows, int64_t cols, int64_t ld, int64_t* deg, int mem) {
  SS_TRY(require_init());
  SS_TRY(check_mem(mem));
  if (rows < 0 || cols < 0 || ld < rows) return fail(SS_EINVAL, "k: bad shape / leading dimension");
  if (rows == 0) return SS_OK;
  if (!deg || (cols > 0 && !G)) return fail(SS_EINVAL, "k: NULL buffer");
  hipStream_t st = ctx().stream;
  DevBuf<T> din;
  const T* src = G;
  int64_t sld = ld;
  if (mem == SS_MEM_HOST && cols > 0) {
    SS_TRY(din.alloc((size_t)rows * cols));
    SS_HIP(hipMemcpy2DAsync(din.p, rows * sizeof(T), G, ld * sizeof(T), rows * sizeof(T), cols, hipMemcpyHostToDevice, st));
    src = din.p;
    sld = rows;
  }
  DevBuf<int> d;
  SS_TRY(d.alloc(rows));
  SS_TRY(launch_row_degree<T>(src, rows, cols, sld, d.p));
  std::vector<int> h(rows);
  SS_HIP(hipMemcpyAsync(h.data(), d.p, rows * sizeof(int), hipMemcpyDeviceToHost, st));
  SS_HIP(hipStreamSynchronize(st));
  if (mem == SS_MEM_HOST) {
    for (int64_t i = 0; i < rows; ++i) deg[i] = h[i];
  } else {
    std::vector<int64_t> h64(h.begin(), h.end());
    SS_HIP(hipMemcpy(deg, h64.data(), rows * sizeof(int64_t), hipMemcpyHostToDevice));
  }
  return SS_OK;
}

template <class T>
static int spread_impl(const T* G, int64_t rows, int64_t cols, int64_t ld, T* W, int64_t ldw, int mem) {
  SS_TRY(require_init());
  SS_TRY(check_mem(mem));
  if (rows < 0 || cols < 0 || ld < rows || ldw < rows) return fail(SS_EINVAL, "spread: bad shape / leading dimension");
  if (rows * cols == 0) return SS_OK;
  if (!G || !W) return fail(SS_EINVAL, "spread: NULL buffer");
  hipStream_t st = ctx().stream;
  DevBuf<T> din, dout;
  DevBuf<int> deg;
  SS_TRY(deg.alloc(rows));
  const T* src = G;
  T* dst = W;
  int64_t sld = ld, dld = ldw;
  if (mem == SS_MEM_HOST) {
    SS_TRY(din.alloc((size_t)rows * cols));
    SS_TRY(dout.alloc((size_t)rows * cols));
    SS_HIP(hipMemcpy2DAsync(din.p, rows * sizeof(T), G, ld * sizeof(T), rows * sizeof(T), cols, hipMemcpyHostToDevice, st));
    src = din.p; dst = dout.p; sld = rows; dld = rows;
  }
  SS_TRY(launch_row_degree<T>(src, rows, cols, sld, deg.p));
  SS_TRY(launch_spread_dense<T>(src, rows, cols, sld, deg.p, dst, dld));
  if (mem == SS_MEM_HOST)
    SS_HIP(hipMemcpy2DAsync(W, ldw * sizeof(T), dout.p, rows * sizeof(T), rows * sizeof(T), cols, hipMemcpyDeviceToHost, st));
  SS_HIP(hipStreamSynchronize(st));
  return SS_OK;
}

// ------------------------------------------------------------------ graph handles
// Every handle starts with its precision tag and its own lock: an entry point holds the handle's lock while it
// works on it (operands are cut lazily, workspaces live in the handle), so calls on DIFFERENT handles overlap
// and calls on the same handle queue up.
struct HandleHead {
  int dtype;  // 4 or 8 = sizeof(T), guards against mixing _f32/_f64 entry points
  std::mutex mu;
};
// every graph box carries an identity of its own (never reused, unlike its address): what a query set is bound to
static uint64_t next_graph_id() {
  static std::atomic<uint64_t> n{0};
  return ++n;
}
template <class T>
struct GraphBox : HandleHead {
  uint64_t id = next_graph_id();
  Graph<T> g;
};
// a query set: an nq x nf block of query rows that belongs to the graph with identity graph_id
template <class T>
struct QueriesBox : HandleHead {
  uint64_t graph_id = 0;
  DevCsr<T> Xq;
  CoefTable<T> coef;   // Xq * inv_kf of its graph, from the first prediction on
};
template <class T>
struct SpMatBox : HandleHead {
  SpMat<T> m;
};

template <class T>
static int graph_check(const void* h, Graph<T>** out) {
  if (!h) return fail(SS_EINVAL, "graph handle is NULL");
  GraphBox<T>* b = const_cast<GraphBox<T>*>(reinterpret_cast<const GraphBox<T>*>(h));
  if (b->dtype != (int)sizeof(T)) return fail(SS_EINVAL, "graph handle was created with the other precision");
  *out = &b->g;
  return SS_OK;
}

// a query set used with the graph handle h (already checked): its precision, and that it was created for that graph
template <class T>
static int queries_check(const void* qh, const void* h, const DevCsr<T>** out, CoefTable<T>** tab = nullptr) {
  QueriesBox<T>* q = const_cast<QueriesBox<T>*>(reinterpret_cast<const QueriesBox<T>*>(qh));
  if (q->dtype != (int)sizeof(T)) return fail(SS_EINVAL, "query set was created with the other precision");
  if (q->graph_id != reinterpret_cast<const GraphBox<T>*>(h)->id)
    return fail(SS_EINVAL, "query set was created for another graph");
  *out = &q->Xq;
  if (tab) *tab = &q->coef;   // (the caller holds the query set's lock)
  return SS_OK;
}

template <class T>
static int graph_create_csr_impl(int64_t nq, int64_t ns, int64_t nf, int64_t nt, const int64_t* xq_ptr,
                                 const int32_t* xq_idx, const T* xq_val, const int64_t* xs_ptr, const int32_t* xs_idx,
                                 const T* xs_val, const int64_t* ys_ptr, const int32_t* ys_idx, const T* ys_val,
                                 int index_base, int mem, ss_graph** out) {
  SS_TRY(require_init());
  SS_TRY(check_mem(mem));
  if (!out) return fail(SS_EINVAL, "out handle pointer is NULL");
  *out = nullptr;
  if (nq < 0 || ns < 0 || nf < 0 || nt < 0) return fail(SS_EINVAL, "negative node count");
  GraphBox<T>* box = new (std::nothrow) GraphBox<T>();
  if (!box) return fail(SS_ENOMEM, "host allocation failed");
  box->dtype = (int)sizeof(T);
  Graph<T>& g = box->g;
  g.nq = nq; g.ns = ns; g.nf = nf; g.nt = nt;
  int rc = csr_from_user<T>(nq, nf, xq_ptr, xq_idx, xq_val, index_base, mem, g.Xq);
  if (rc == SS_OK) rc = csr_from_user<T>(ns, nf, xs_ptr, xs_idx, xs_val, index_base, mem, g.Xs);
  if (rc == SS_OK) rc = csr_from_user<T>(ns, nt, ys_ptr, ys_idx, ys_val, index_base, mem, g.Ys);
  if (rc == SS_OK) rc = graph_finalize<T>(g);
  if (rc != SS_OK) { delete box; return rc; }
  *out = reinterpret_cast<ss_graph*>(box);
  return SS_OK;
}

template <class T>
static int graph_create_dense_impl(int64_t nq, int64_t ns, int64_t nf, int64_t nt, const T* Sq, int64_t ldq,
                                   const T* Ss, int64_t lds, const T* Y, int64_t ldy, int apply_cutoff, T alpha,
                                   int weighted, int mem, ss_graph** out) {
  SS_TRY(require_init());
  SS_TRY(check_mem(mem));
  if (!out) return fail(SS_EINVAL, "out handle pointer is NULL");
  *out = nullptr;
  if (nq < 0 || ns < 0 || nf < 0 || nt < 0) return fail(SS_EINVAL, "negative node count");
  GraphBox<T>* box = new (std::nothrow) GraphBox<T>();
  if (!box) return fail(SS_ENOMEM, "host allocation failed");
  box->dtype = (int)sizeof(T);
  Graph<T>& g = box->g;
  g.nq = nq; g.ns = ns; g.nf = nf; g.nt = nt;
  int rc = csr_from_dense<T>(Sq, nq, nf, ldq, apply_cutoff != 0, alpha, weighted != 0, mem, g.Xq);
  if (rc == SS_OK) rc = csr_from_dense<T>(Ss, ns, nf, lds, apply_cutoff != 0, alpha, weighted != 0, mem, g.Xs);
  if (rc == SS_OK) rc = csr_from_dense<T>(Y, ns, nt, ldy, false, T(0), true, mem, g.Ys);
  if (rc == SS_OK) rc = graph_finalize<T>(g);
  if (rc != SS_OK) { delete box; return rc; }
  *out = reinterpret_cast<ss_graph*>(box);
  return SS_OK;
}

template <class T>
static int graph_create_general_impl(int64_t n, int64_t nr, int64_t nc, const int64_t* l_ptr, const int32_t* l_idx,
                                     const T* l_val, const int64_t* b_ptr, const int32_t* b_idx, const T* b_val,
                                     const int64_t* w_ptr, const int32_t* w_idx, const T* w_val, int index_base,
                                     int mem, ss_graph** out) {
  SS_TRY(require_init());
  SS_TRY(check_mem(mem));
  if (!out) return fail(SS_EINVAL, "out handle pointer is NULL");
  *out = nullptr;
  if (n < 0 || nr < 0 || nc < 0) return fail(SS_EINVAL, "negative node count");
  GraphBox<T>* box = new (std::nothrow) GraphBox<T>();
  if (!box) return fail(SS_ENOMEM, "host allocation failed");
  box->dtype = (int)sizeof(T);
  Graph<T>& g = box->g;
  g.general = true;
  g.nq = nr; g.ns = n; g.nf = n; g.nt = nc;
  int rc = csr_from_user<T>(nr, n, l_ptr, l_idx, l_val, index_base, mem, g.Xq);
  if (rc == SS_OK) rc = csr_from_user<T>(n, n, b_ptr, b_idx, b_val, index_base, mem, g.XsT);
  if (rc == SS_OK) rc = csr_from_user<T>(nc, n, w_ptr, w_idx, w_val, index_base, mem, g.YsT);
  if (rc == SS_OK) rc = graph_finalize_general<T>(g);
  if (rc != SS_OK) { delete box; return rc; }
  *out = reinterpret_cast<ss_graph*>(box);
  return SS_OK;
}

// dense-similarity graph: raw similarities resident, labels sparse
template <class T>
static int graph_create_similarity_impl(int64_t nq, int64_t ns, int64_t nt, const T* Sq, int64_t ldq,
                                        const T* Ss, int64_t lds, const int64_t* y_ptr, const int32_t* y_idx,
                                        const T* y_val, int index_base, T alpha, int weighted, int mem,
                                        ss_graph** out) {
  SS_TRY(require_init());
  SS_TRY(check_mem(mem));
  if (!out) return fail(SS_EINVAL, "out handle pointer is NULL");
  *out = nullptr;
  if (nq < 0 || ns < 0 || nt < 0) return fail(SS_EINVAL, "negative node count");
  if ((nq > 0 && (!Sq || ldq < nq)) || (ns > 0 && (!Ss || lds < ns)))
    return fail(SS_EINVAL, "similarity block: NULL pointer or ld < rows");
  GraphBox<T>* box = new (std::nothrow) GraphBox<T>();
  if (!box) return fail(SS_ENOMEM, "host allocation failed");
  box->dtype = (int)sizeof(T);
  Graph<T>& g = box->g;
  g.nq = nq; g.ns = ns; g.nf = ns; g.nt = nt;
  DenseSim<T>& d = g.dense;
  d.on = true; d.nq = nq; d.ns = ns; d.nf = ns; d.alpha = alpha; d.weighted = weighted != 0;
  hipStream_t st = ctx().stream;
  auto stage = [&](const T* src, int64_t rows, int64_t ld, DevBuf<T>& dst) -> int {
    SS_TRY(dst.alloc((size_t)rows * (size_t)ns));
    if (rows == 0 || ns == 0) return SS_OK;
    SS_HIP(hipMemcpy2DAsync(dst.p, rows * sizeof(T), src, ld * sizeof(T), rows * sizeof(T), ns,
                            mem == SS_MEM_HOST ? hipMemcpyHostToDevice : hipMemcpyDeviceToDevice, st));
    return SS_OK;
  };
  int rc = stage(Sq, nq, ldq, d.Sq);
  if (rc == SS_OK) rc = stage(Ss, ns, lds, d.Ss);
  if (rc == SS_OK) rc = csr_from_user<T>(ns, nt, y_ptr, y_idx, y_val, index_base, mem, g.Ys);
  if (rc == SS_OK) rc = csr_transpose(g.Ys, g.YsT);
  if (rc == SS_OK) rc = graph_finalize_general_targets(g);
  if (rc == SS_OK) rc = dense_degrees(g);
  if (rc != SS_OK) { delete box; return rc; }
  *out = reinterpret_cast<ss_graph*>(box);
  return SS_OK;
}

// ------------------------------------------------------------------ binary fingerprints -> thresholded Tanimoto CSR
static int check_fingerprints(const char* what, const uint64_t* F, int64_t n, int64_t nwords) {
  if (n < 0) return fail(SS_EINVAL, "%s: negative fingerprint count", what);
  if (n >= (1LL << 31)) return fail(SS_EUNSUPPORTED, "%s: %lld fingerprints (>= 2^31)", what, (long long)n);
  if (n > 0 && !F) return fail(SS_EINVAL, "%s is NULL", what);
  return SS_OK;
}
static int check_nwords(int64_t nwords) {
  if (nwords < 1) return fail(SS_EINVAL, "nwords must be >= 1");
  // popcounts stay exact in fp32 (and fit the int accumulators) for d < 2^24 bits
  if (nwords > (1LL << 18)) return fail(SS_EUNSUPPORTED, "nwords > 2^18 (fingerprints of 2^24 bits or more)");
  return SS_OK;
}
// fingerprints on the device: the caller's buffer (SS_MEM_DEVICE) or a staged copy
static int stage_fingerprints(const uint64_t* F, int64_t n, int64_t nwords, int mem, DevBuf<uint64_t>& buf,
                              const uint64_t** dev) {
  if (mem == SS_MEM_DEVICE || n == 0) {
    *dev = F;
    return SS_OK;
  }
  SS_TRY(buf.alloc((size_t)n * (size_t)nwords));
  SS_TRY(upload(buf.p, F, (size_t)n * (size_t)nwords, mem));
  *dev = buf.p;
  return SS_OK;
}

// the size protocol of the fused producers, after their count pass: *nnz always; nnz >= 2^31 refused and capacity
// checked before anything is written; ptr, then (idx != NULL) idx and val (val may be NULL) in `mem`
template <class T>
static int emit_pair_csr(PairCsr<T>& pc, int64_t na, int64_t* ptr, int32_t* idx, T* val, int64_t capacity,
                         int64_t* nnz, int mem) {
  *nnz = pc.nnz;
  if (pc.nnz >= (1LL << 31))
    return fail(SS_EUNSUPPORTED, "%s: nnz = %lld >= 2^31 (use the dense-similarity graph)", pc.what,
                (long long)pc.nnz);
  if (idx && capacity < pc.nnz)
    return fail(SS_EINVAL, "%s: capacity %lld < nnz %lld", pc.what, (long long)capacity, (long long)pc.nnz);
  hipStream_t st = ctx().stream;
  const hipMemcpyKind back = mem == SS_MEM_HOST ? hipMemcpyDeviceToHost : hipMemcpyDeviceToDevice;
  SS_HIP(hipMemcpyAsync(ptr, pc.ptr.p, (size_t)(na + 1) * sizeof(int64_t), back, st));
  if (idx && pc.nnz > 0) {
    if (mem == SS_MEM_DEVICE) {
      SS_TRY(pc.fill(idx, val, nullptr));
    } else {
      DevBuf<int> di;
      DevBuf<T> dv;
      SS_TRY(di.alloc(pc.nnz));
      if (val) SS_TRY(dv.alloc(pc.nnz));
      SS_TRY(pc.fill(di.p, val ? dv.p : nullptr, nullptr));
      SS_HIP(hipMemcpyAsync(idx, di.p, (size_t)pc.nnz * sizeof(int), back, st));
      if (val) SS_HIP(hipMemcpyAsync(val, dv.p, (size_t)pc.nnz * sizeof(T), back, st));
      SS_HIP(hipStreamSynchronize(st));
    }
  }
  SS_HIP(hipStreamSynchronize(st));
  return SS_OK;
}

// the common head of the graph constructors below: the library and `mem` are usable, *out is cleared, the path note is
// emptied and nt is in range
static int graph_create_begin(int mem, int64_t nt, ss_graph** out) {
  SS_TRY(require_init());
  SS_TRY(check_mem(mem));
  if (!out) return fail(SS_EINVAL, "out handle pointer is NULL");
  *out = nullptr;
  path_note().clear();
  if (nt < 0) return fail(SS_EINVAL, "negative node count");
  if (nt >= (1LL << 31)) return fail(SS_EUNSUPPORTED, "dimension >= 2^31");
  return SS_OK;
}

// construct(y, X, ...) from two fused producers: Xs = count_s() (ns x ns, tag_s), Xq = count_q() (nq x ns, tag_q, noted
// when nq > 0), features named after the sources; Y and the finalisation as for the other graphs
template <class T, class Prod, class CountS, class CountQ>
static int graph_from_producers(int64_t nq, int64_t ns, int64_t nt, CountS count_s, CountQ count_q, const char* tag_s,
                                const char* tag_q, const int64_t* y_ptr, const int32_t* y_idx, const T* y_val,
                                int index_base, int mem, ss_graph** out) {
  GraphBox<T>* box = new (std::nothrow) GraphBox<T>();
  if (!box) return fail(SS_ENOMEM, "host allocation failed");
  box->dtype = (int)sizeof(T);
  Graph<T>& g = box->g;
  g.nq = nq; g.ns = ns; g.nf = ns; g.nt = nt;
  int rc = SS_OK;
  {
    Prod ps;
    rc = count_s(ps);
    if (rc == SS_OK) rc = ps.to_dev_csr(g.Xs);
    path_add(tag_s);
  }
  if (rc == SS_OK) {
    Prod pq;
    rc = count_q(pq);
    if (rc == SS_OK) rc = pq.to_dev_csr(g.Xq);
    if (nq > 0) path_add(tag_q);
  }
  if (rc == SS_OK) rc = csr_from_user<T>(ns, nt, y_ptr, y_idx, y_val, index_base, mem, g.Ys);
  if (rc == SS_OK) rc = graph_finalize<T>(g);
  if (rc != SS_OK) { delete box; return rc; }
  *out = reinterpret_cast<ss_graph*>(box);
  return SS_OK;
}

// The neighbour floor (include/simspread_hip_neighbours.h): k > 0 adds the per-row cut tau = tanimoto_kth(k) to the
// producer (TanimotoCsr::count); k == 0 is the plain producer, its kernels and its tags.
static const char* tanimoto_tag(bool sym, int k) {
  if (k > 0) return sym ? "tanimoto_csr_floor_sym" : "tanimoto_csr_floor_cross";
  return sym ? "tanimoto_csr_sym" : "tanimoto_csr_cross";
}
// what the floor entry points refuse before anything is written
template <class T>
static int check_floor(int k, T alpha) {
  if (k < 0 || k > NEIGHBOUR_K_MAX) return fail(SS_EINVAL, "neighbour floor: k = %d outside 0..%d", k, NEIGHBOUR_K_MAX);
  if (alpha != alpha) return fail(SS_EINVAL, "neighbour floor: alpha is NaN");
  return SS_OK;
}

template <class T>
static int tanimoto_csr_impl(const uint64_t* Fa, int64_t na, const uint64_t* Fb, int64_t nb, int64_t nwords, T alpha,
                             int weighted, int64_t* ptr, int32_t* idx, T* val, int64_t capacity, int64_t* nnz,
                             int mem, int k = 0) {
  SS_TRY(require_init());
  SS_TRY(check_mem(mem));
  path_note().clear();
  const bool sym = (Fb == nullptr);
  if (sym) nb = na;
  SS_TRY(check_nwords(nwords));
  SS_TRY(check_fingerprints("Fa", Fa, na, nwords));
  if (!sym) SS_TRY(check_fingerprints("Fb", Fb, nb, nwords));
  if (!ptr || !nnz) return fail(SS_EINVAL, "tanimoto: ptr and nnz must not be NULL");
  DevBuf<uint64_t> ba, bb;
  const uint64_t *da = nullptr, *db = nullptr;
  SS_TRY(stage_fingerprints(Fa, na, nwords, mem, ba, &da));
  if (!sym) SS_TRY(stage_fingerprints(Fb, nb, nwords, mem, bb, &db));
  TanimotoCsr<T> tc;
  SS_TRY(tc.count(da, na, sym ? nullptr : db, nb, nwords, alpha, weighted != 0, k));
  path_add(tanimoto_tag(sym, k));
  return emit_pair_csr<T>(tc, na, ptr, idx, val, capacity, nnz, mem);
}

// tau[na]: the k-th largest positive similarity of every row (neighbour_floor.hip)
template <class T>
static int tanimoto_kth_impl(const uint64_t* Fa, int64_t na, const uint64_t* Fb, int64_t nb, int64_t nwords, int k,
                             T* tau, int mem) {
  SS_TRY(require_init());
  SS_TRY(check_mem(mem));
  path_note().clear();
  const bool sym = (Fb == nullptr);
  if (sym) nb = na;
  if (k < 1 || k > NEIGHBOUR_K_MAX) return fail(SS_EINVAL, "tanimoto kth: k = %d outside 1..%d", k, NEIGHBOUR_K_MAX);
  SS_TRY(check_nwords(nwords));
  SS_TRY(check_fingerprints("Fa", Fa, na, nwords));
  if (!sym) SS_TRY(check_fingerprints("Fb", Fb, nb, nwords));
  if (na > 0 && !tau) return fail(SS_EINVAL, "tanimoto kth: tau must not be NULL");
  path_add("tanimoto_kth");
  if (na == 0) return SS_OK;
  DevBuf<uint64_t> ba, bb;
  const uint64_t *da = nullptr, *db = nullptr;
  SS_TRY(stage_fingerprints(Fa, na, nwords, mem, ba, &da));
  if (!sym) SS_TRY(stage_fingerprints(Fb, nb, nwords, mem, bb, &db));
  hipStream_t st = ctx().stream;
  DevBuf<T> dt;
  T* dtau = tau;
  if (mem == SS_MEM_HOST) {
    SS_TRY(dt.alloc(na));
    dtau = dt.p;
  }
  SS_TRY(tanimoto_kth<T>(da, na, sym ? nullptr : db, nb, nwords, nullptr, nullptr, k, dtau));
  if (mem == SS_MEM_HOST) SS_HIP(hipMemcpyAsync(tau, dtau, (size_t)na * sizeof(T), hipMemcpyDeviceToHost, st));
  SS_HIP(hipStreamSynchronize(st));
  return SS_OK;
}

// construct(y, X, ...) with X = featurize(Tanimoto(F), alpha, weighted): Xs = cut(T(Fs, Fs)), Xq = cut(T(Fq, Fs)),
// features named after the sources; the CSR blocks are produced on the device and finalised like the other graphs
template <class T>
static int graph_create_fingerprint_impl(int64_t nq, int64_t ns, int64_t nt, int64_t nwords, const uint64_t* Fq,
                                         const uint64_t* Fs, const int64_t* y_ptr, const int32_t* y_idx,
                                         const T* y_val, int index_base, T alpha, int weighted, int mem,
                                         ss_graph** out, int k = 0) {
  SS_TRY(graph_create_begin(mem, nt, out));
  SS_TRY(check_nwords(nwords));
  SS_TRY(check_fingerprints("Fq", Fq, nq, nwords));
  SS_TRY(check_fingerprints("Fs", Fs, ns, nwords));
  DevBuf<uint64_t> bq, bs;
  const uint64_t *dq = nullptr, *ds = nullptr;
  SS_TRY(stage_fingerprints(Fs, ns, nwords, mem, bs, &ds));
  SS_TRY(stage_fingerprints(Fq, nq, nwords, mem, bq, &dq));
  const bool wgt = weighted != 0;
  return graph_from_producers<T, TanimotoCsr<T>>(
      nq, ns, nt, [&](TanimotoCsr<T>& p) { return p.count(ds, ns, nullptr, ns, nwords, alpha, wgt, k); },
      [&](TanimotoCsr<T>& p) { return p.count(dq, nq, ds, ns, nwords, alpha, wgt, k); }, tanimoto_tag(true, k),
      tanimoto_tag(false, k), y_ptr, y_idx, y_val, index_base, mem, out);
}

// ------------------- real-valued rows -> thresholded weighted Jaccard CSR, or cosine / Tanimoto / Dice CSR (MFMA)
static int check_features(const char* what, const void* F, int64_t n, int64_t ld, int64_t d) {
  if (n < 0) return fail(SS_EINVAL, "%s: negative row count", what);
  if (n >= (1LL << 31)) return fail(SS_EUNSUPPORTED, "%s: %lld rows (>= 2^31)", what, (long long)n);
  if (ld < n) return fail(SS_EINVAL, "%s: leading dimension %lld < %lld rows", what, (long long)ld, (long long)n);
  if (n > 0 && d > 0 && !F) return fail(SS_EINVAL, "%s is NULL", what);
  return SS_OK;
}
// features on the device: the caller's buffer (SS_MEM_DEVICE) or a staged copy with ld = n
template <class T>
static int stage_features(const T* F, int64_t n, int64_t ld, int64_t d, int mem, DevBuf<T>& buf, const T** dev,
                          int64_t* dev_ld) {
  if (mem == SS_MEM_DEVICE || n == 0 || d == 0) {
    *dev = F;
    *dev_ld = ld;
    return SS_OK;
  }
  SS_TRY(buf.alloc((size_t)n * (size_t)d));
  SS_HIP(hipMemcpy2DAsync(buf.p, n * sizeof(T), F, ld * sizeof(T), n * sizeof(T), d, hipMemcpyHostToDevice,
                          ctx().stream));
  *dev = buf.p;
  *dev_ld = n;
  return SS_OK;
}

// What tells the fused producers of column-major feature rows apart on this level: how their messages start, their path
// tags, check(), the check of the producer's own arguments, and count(p, Fa, na, lda, Fb, nb, ldb), the count pass of
// producer p on device rows (Fb == NULL: symmetric).
struct FeatureNames {
  const char *msg, *tag_sym, *tag_cross;
  // the neighbour floor (include/simspread_hip_neighbours_real.h): the tags of the floor producer and of its tau
  const char *tag_floor_sym, *tag_floor_cross, *tag_kth;
  const char* tag(bool sym, int k) const {
    return k > 0 ? (sym ? tag_floor_sym : tag_floor_cross) : (sym ? tag_sym : tag_cross);
  }
};
static const FeatureNames jaccard_names = {"jaccard", "jaccard_csr_sym", "jaccard_csr_cross", "jaccard_csr_floor_sym",
                                           "jaccard_csr_floor_cross", "jaccard_kth"};
static const FeatureNames dot_names = {"dot_csr", "dot_csr_sym", "dot_csr_cross", "dot_csr_floor_sym",
                                       "dot_csr_floor_cross", "dot_kth"};

static int check_sim_metric(int metric) {
  if (metric != SS_SIM_COSINE && metric != SS_SIM_TANIMOTO && metric != SS_SIM_DICE)
    return fail(SS_EINVAL, "dot_csr: metric %d is not SS_SIM_COSINE, SS_SIM_TANIMOTO or SS_SIM_DICE", metric);
  return SS_OK;
}
template <class T>
static auto jaccard_count(int64_t d, T alpha, int weighted, int k = 0) {
  return [=](JaccardCsr<T>& p, const T* Fa, int64_t na, int64_t lda, const T* Fb, int64_t nb, int64_t ldb) {
    return p.count(Fa, na, lda, Fb, nb, ldb, d, alpha, weighted != 0, k);
  };
}
template <class T>
static auto dot_count(int64_t d, int metric, T alpha, int weighted, int k = 0) {
  return [=](DotCsr<T>& p, const T* Fa, int64_t na, int64_t lda, const T* Fb, int64_t nb, int64_t ldb) {
    return p.count(Fa, na, lda, Fb, nb, ldb, d, metric, alpha, weighted != 0, k);
  };
}

template <class T, class Check>
static int check_feature_args(const FeatureNames& nm, Check check, int64_t d, T alpha) {
  SS_TRY(check());
  if (d < 0) return fail(SS_EINVAL, "%s: negative feature count", nm.msg);
  if (alpha != alpha) return fail(SS_EINVAL, "%s: alpha is NaN", nm.msg);
  return SS_OK;
}

// Fa (na x d) against Fb (nb x d; NULL: Fa against itself) as CSR, under the size protocol of emit_pair_csr
template <class T, class Prod, class Check, class Count>
static int features_csr_impl(const FeatureNames& nm, Check check, Count count, const T* Fa, int64_t na, int64_t lda,
                             const T* Fb, int64_t nb, int64_t ldb, int64_t d, T alpha, int64_t* ptr, int32_t* idx,
                             T* val, int64_t capacity, int64_t* nnz, int mem, int k = 0) {
  SS_TRY(require_init());
  SS_TRY(check_mem(mem));
  path_note().clear();
  const bool sym = (Fb == nullptr);
  if (sym) {
    nb = na;
    ldb = lda;
  }
  SS_TRY(check_feature_args(nm, check, d, alpha));
  SS_TRY(check_features("Fa", Fa, na, lda, d));
  if (!sym) SS_TRY(check_features("Fb", Fb, nb, ldb, d));
  if (!ptr || !nnz) return fail(SS_EINVAL, "%s: ptr and nnz must not be NULL", nm.msg);
  DevBuf<T> ba, bb;
  const T *da = nullptr, *db = nullptr;
  int64_t la = 0, lb = 0;
  SS_TRY(stage_features(Fa, na, lda, d, mem, ba, &da, &la));
  if (!sym) SS_TRY(stage_features(Fb, nb, ldb, d, mem, bb, &db, &lb));
  Prod p;
  SS_TRY(count(p, da, na, la, sym ? nullptr : db, nb, lb));
  path_add(nm.tag(sym, k));
  return emit_pair_csr<T>(p, na, ptr, idx, val, capacity, nnz, mem);
}

// tau[na] (in `mem`): the k-th largest positive similarity of every row of Fa against Fb (real_floor.hip);
// kth(da, na, la, db, nb, lb, dtau) is the producer's selection on device rows (db == NULL: Fa against itself)
template <class T, class Check, class Kth>
static int features_kth_impl(const FeatureNames& nm, Check check, Kth kth, const T* Fa, int64_t na, int64_t lda,
                             const T* Fb, int64_t nb, int64_t ldb, int64_t d, int k, T* tau, int mem) {
  SS_TRY(require_init());
  SS_TRY(check_mem(mem));
  path_note().clear();
  const bool sym = (Fb == nullptr);
  if (sym) {
    nb = na;
    ldb = lda;
  }
  if (k < 1 || k > NEIGHBOUR_K_MAX) return fail(SS_EINVAL, "%s kth: k = %d outside 1..%d", nm.msg, k, NEIGHBOUR_K_MAX);
  SS_TRY(check());
  if (d < 0) return fail(SS_EINVAL, "%s kth: negative feature count", nm.msg);
  SS_TRY(check_features("Fa", Fa, na, lda, d));
  if (!sym) SS_TRY(check_features("Fb", Fb, nb, ldb, d));
  if (na > 0 && !tau) return fail(SS_EINVAL, "%s kth: tau must not be NULL", nm.msg);
  path_add(nm.tag_kth);
  if (na == 0) return SS_OK;
  DevBuf<T> ba, bb;
  const T *da = nullptr, *db = nullptr;
  int64_t la = 0, lb = 0;
  SS_TRY(stage_features(Fa, na, lda, d, mem, ba, &da, &la));
  if (!sym) SS_TRY(stage_features(Fb, nb, ldb, d, mem, bb, &db, &lb));
  SS_TRY(refuse_nan_rows<T>(nm.msg, da, na, la, sym ? nullptr : db, nb, lb, d));
  hipStream_t st = ctx().stream;
  DevBuf<T> dt;
  T* dtau = tau;
  if (mem == SS_MEM_HOST) {
    SS_TRY(dt.alloc(na));
    dtau = dt.p;
  }
  SS_TRY(kth(da, na, la, sym ? nullptr : db, nb, lb, dtau));
  if (mem == SS_MEM_HOST) SS_HIP(hipMemcpyAsync(tau, dtau, (size_t)na * sizeof(T), hipMemcpyDeviceToHost, st));
  SS_HIP(hipStreamSynchronize(st));
  return SS_OK;
}

// construct(y, X, ...) with X = featurize(S(F), alpha, weighted), S the producer's similarity of the feature rows:
// Xs = cut(S(Fs, Fs)), Xq = cut(S(Fq, Fs)), features named after the sources
template <class T, class Prod, class Check, class Count>
static int features_graph_impl(const FeatureNames& nm, Check check, Count count, int64_t nq, int64_t ns, int64_t nt,
                               int64_t d, const T* Fq, int64_t ldq, const T* Fs, int64_t lds_, const int64_t* y_ptr,
                               const int32_t* y_idx, const T* y_val, int index_base, T alpha, int mem, ss_graph** out,
                               int k = 0) {
  SS_TRY(graph_create_begin(mem, nt, out));
  SS_TRY(check_feature_args(nm, check, d, alpha));
  SS_TRY(check_features("Fq", Fq, nq, ldq, d));
  SS_TRY(check_features("Fs", Fs, ns, lds_, d));
  DevBuf<T> bq, bs;
  const T *dq = nullptr, *ds = nullptr;
  int64_t lq = 0, ls = 0;
  SS_TRY(stage_features(Fs, ns, lds_, d, mem, bs, &ds, &ls));
  SS_TRY(stage_features(Fq, nq, ldq, d, mem, bq, &dq, &lq));
  return graph_from_producers<T, Prod>(
      nq, ns, nt, [&](Prod& p) { return count(p, ds, ns, ls, nullptr, ns, ls); },
      [&](Prod& p) { return count(p, dq, nq, lq, ds, ns, ls); }, nm.tag(true, k), nm.tag(false, k), y_ptr, y_idx, y_val,
      index_base, mem, out);
}

static int no_check() { return SS_OK; }

template <class T>
static int jaccard_csr_impl(const T* Fa, int64_t na, int64_t lda, const T* Fb, int64_t nb, int64_t ldb, int64_t d,
                            T alpha, int weighted, int64_t* ptr, int32_t* idx, T* val, int64_t capacity, int64_t* nnz,
                            int mem, int k = 0) {
  return features_csr_impl<T, JaccardCsr<T>>(jaccard_names, no_check, jaccard_count<T>(d, alpha, weighted, k), Fa, na,
                                             lda, Fb, nb, ldb, d, alpha, ptr, idx, val, capacity, nnz, mem, k);
}
template <class T>
static int jaccard_kth_impl(const T* Fa, int64_t na, int64_t lda, const T* Fb, int64_t nb, int64_t ldb, int64_t d, int k,
                            T* tau, int mem) {
  return features_kth_impl<T>(
      jaccard_names, no_check,
      [=](const T* da, int64_t na_, int64_t la, const T* db, int64_t nb_, int64_t lb, T* dtau) {
        return jaccard_kth<T>(da, na_, la, db, nb_, lb, d, k, dtau);
      },
      Fa, na, lda, Fb, nb, ldb, d, k, tau, mem);
}
template <class T>
static int graph_create_features_impl(int64_t nq, int64_t ns, int64_t nt, int64_t d, const T* Fq, int64_t ldq,
                                      const T* Fs, int64_t lds_, const int64_t* y_ptr, const int32_t* y_idx,
                                      const T* y_val, int index_base, T alpha, int weighted, int mem, ss_graph** out,
                                      int k = 0) {
  return features_graph_impl<T, JaccardCsr<T>>(jaccard_names, no_check, jaccard_count<T>(d, alpha, weighted, k), nq, ns,
                                               nt, d, Fq, ldq, Fs, lds_, y_ptr, y_idx, y_val, index_base, alpha, mem, out,
                                               k);
}
template <class T>
static int dot_csr_impl(const T* Fa, int64_t na, int64_t lda, const T* Fb, int64_t nb, int64_t ldb, int64_t d,
                        int metric, T alpha, int weighted, int64_t* ptr, int32_t* idx, T* val, int64_t capacity,
                        int64_t* nnz, int mem, int k = 0) {
  return features_csr_impl<T, DotCsr<T>>(
      dot_names, [=] { return check_sim_metric(metric); }, dot_count<T>(d, metric, alpha, weighted, k), Fa, na, lda, Fb,
      nb, ldb, d, alpha, ptr, idx, val, capacity, nnz, mem, k);
}
template <class T>
static int dot_kth_impl(const T* Fa, int64_t na, int64_t lda, const T* Fb, int64_t nb, int64_t ldb, int64_t d, int metric,
                        int k, T* tau, int mem) {
  return features_kth_impl<T>(
      dot_names, [=] { return check_sim_metric(metric); },
      [=](const T* da, int64_t na_, int64_t la, const T* db, int64_t nb_, int64_t lb, T* dtau) {
        return dot_kth<T>(da, na_, la, db, nb_, lb, d, metric, nullptr, nullptr, k, dtau);
      },
      Fa, na, lda, Fb, nb, ldb, d, k, tau, mem);
}
template <class T>
static int graph_create_vectors_impl(int64_t nq, int64_t ns, int64_t nt, int64_t d, int metric, const T* Fq,
                                     int64_t ldq, const T* Fs, int64_t lds_, const int64_t* y_ptr, const int32_t* y_idx,
                                     const T* y_val, int index_base, T alpha, int weighted, int mem, ss_graph** out,
                                     int k = 0) {
  return features_graph_impl<T, DotCsr<T>>(
      dot_names, [=] { return check_sim_metric(metric); }, dot_count<T>(d, metric, alpha, weighted, k), nq, ns, nt, d, Fq,
      ldq, Fs, lds_, y_ptr, y_idx, y_val, index_base, alpha, mem, out, k);
}

// ------------------- 16-bit rows (include/simspread_hip_half.h): ROW-MAJOR bf16 / fp16 patterns -> DotCsrH16, fp32 CSR
static const char* h16_tag(bool sym) { return sym ? "dot_h16_sym" : "dot_h16_cross"; }
// what the 16-bit entry points refuse before anything is staged or written
static int check_h16_args(int storage, int metric, int64_t d, float alpha) {
  if (storage != SS_H16_BF16 && storage != SS_H16_F16)
    return fail(SS_EINVAL, "dot_h16: storage %d is not SS_H16_BF16 or SS_H16_F16", storage);
  if (metric != SS_SIM_COSINE && metric != SS_SIM_TANIMOTO && metric != SS_SIM_DICE)
    return fail(SS_EINVAL, "dot_h16: metric %d is not SS_SIM_COSINE, SS_SIM_TANIMOTO or SS_SIM_DICE", metric);
  if (d < 0) return fail(SS_EINVAL, "dot_h16: negative feature count");
  if (alpha != alpha) return fail(SS_EINVAL, "dot_h16: alpha is NaN");
  return SS_OK;
}
static int check_rows_h16(const char* what, const uint16_t* F, int64_t n, int64_t ld, int64_t d) {
  if (n < 0) return fail(SS_EINVAL, "%s: negative row count", what);
  if (n >= (1LL << 31)) return fail(SS_EUNSUPPORTED, "%s: %lld rows (>= 2^31)", what, (long long)n);
  if (ld < d) return fail(SS_EINVAL, "%s: leading dimension %lld < %lld features (16-bit rows are row-major)", what,
                          (long long)ld, (long long)d);
  if (n > 0 && d > 0 && !F) return fail(SS_EINVAL, "%s is NULL", what);
  return SS_OK;
}
// rows on the device: the caller's buffer (SS_MEM_DEVICE) or a staged copy with ld = d; of a host row only its d
// elements are read
static int stage_rows_h16(const uint16_t* F, int64_t n, int64_t ld, int64_t d, int mem, DevBuf<uint16_t>& buf,
                          const uint16_t** dev, int64_t* dev_ld) {
  if (mem == SS_MEM_DEVICE || n == 0 || d == 0) {
    *dev = F;
    *dev_ld = ld;
    return SS_OK;
  }
  SS_TRY(buf.alloc((size_t)n * (size_t)d));
  SS_HIP(hipMemcpy2DAsync(buf.p, d * sizeof(uint16_t), F, ld * sizeof(uint16_t), d * sizeof(uint16_t), n,
                          hipMemcpyHostToDevice, ctx().stream));
  *dev = buf.p;
  *dev_ld = d;
  return SS_OK;
}

static int dot_csr_h16_impl(const uint16_t* Fa, int64_t na, int64_t lda, const uint16_t* Fb, int64_t nb, int64_t ldb,
                            int64_t d, int storage, int metric, float alpha, int weighted, int64_t* ptr, int32_t* idx,
                            float* val, int64_t capacity, int64_t* nnz, int mem) {
  SS_TRY(require_init());
  SS_TRY(check_mem(mem));
  path_note().clear();
  const bool sym = (Fb == nullptr);
  if (sym) {
    nb = na;
    ldb = lda;
  }
  SS_TRY(check_h16_args(storage, metric, d, alpha));
  SS_TRY(check_rows_h16("Fa", Fa, na, lda, d));
  if (!sym) SS_TRY(check_rows_h16("Fb", Fb, nb, ldb, d));
  if (!ptr || !nnz) return fail(SS_EINVAL, "dot_h16: ptr and nnz must not be NULL");
  DevBuf<uint16_t> ba, bb;
  const uint16_t *da = nullptr, *db = nullptr;
  int64_t la = 0, lb = 0;
  SS_TRY(stage_rows_h16(Fa, na, lda, d, mem, ba, &da, &la));
  if (!sym) SS_TRY(stage_rows_h16(Fb, nb, ldb, d, mem, bb, &db, &lb));
  DotCsrH16 p;
  SS_TRY(p.count(da, na, la, sym ? nullptr : db, nb, lb, d, storage, metric, alpha, weighted != 0));
  path_add(h16_tag(sym));
  return emit_pair_csr<float>(p, na, ptr, idx, val, capacity, nnz, mem);
}

static int graph_create_vectors_h16_impl(int64_t nq, int64_t ns, int64_t nt, int64_t d, int storage, int metric,
                                         const uint16_t* Fq, int64_t ldq, const uint16_t* Fs, int64_t lds_,
                                         const int64_t* y_ptr, const int32_t* y_idx, const float* y_val, int index_base,
                                         float alpha, int weighted, int mem, ss_graph** out) {
  SS_TRY(graph_create_begin(mem, nt, out));
  SS_TRY(check_h16_args(storage, metric, d, alpha));
  SS_TRY(check_rows_h16("Fq", Fq, nq, ldq, d));
  SS_TRY(check_rows_h16("Fs", Fs, ns, lds_, d));
  DevBuf<uint16_t> bq, bs;
  const uint16_t *dq = nullptr, *ds = nullptr;
  int64_t lq = 0, ls = 0;
  SS_TRY(stage_rows_h16(Fs, ns, lds_, d, mem, bs, &ds, &ls));
  SS_TRY(stage_rows_h16(Fq, nq, ldq, d, mem, bq, &dq, &lq));
  const bool wgt = weighted != 0;
  return graph_from_producers<float, DotCsrH16>(
      nq, ns, nt, [&](DotCsrH16& p) { return p.count(ds, ns, ls, nullptr, ns, ls, d, storage, metric, alpha, wgt); },
      [&](DotCsrH16& p) { return p.count(dq, nq, lq, ds, ns, ls, d, storage, metric, alpha, wgt); }, h16_tag(true),
      h16_tag(false), y_ptr, y_idx, y_val, index_base, mem, out);
}

// ------------------- int8 rows (include/simspread_hip_int8.h): ROW-MAJOR signed bytes -> DotCsrI8, fp32 CSR
static const FeatureNames i8_names = {"dot_i8", "dot_i8_sym", "dot_i8_cross", "dot_i8_floor_sym", "dot_i8_floor_cross",
                                      "dot_i8_kth"};
constexpr int64_t I8_D_MAX = 131071;  // d * 2^14 <= 2^31 - 1: the three sums are exact in int32
// what the int8 entry points refuse before anything is read, staged or written (k_min: 0, or 1 for the selection alone)
static int check_i8_args(int metric, int64_t d, float alpha, int k, int k_min) {
  if (metric != SS_SIM_COSINE && metric != SS_SIM_TANIMOTO && metric != SS_SIM_DICE)
    return fail(SS_EINVAL, "dot_i8: metric %d is not SS_SIM_COSINE, SS_SIM_TANIMOTO or SS_SIM_DICE", metric);
  if (d < 0) return fail(SS_EINVAL, "dot_i8: negative feature count");
  if (d > I8_D_MAX)
    return fail(SS_EINVAL, "dot_i8: %lld features; the sums are exact in int32 up to d = %lld", (long long)d,
                (long long)I8_D_MAX);
  if (alpha != alpha) return fail(SS_EINVAL, "dot_i8: alpha is NaN");
  if (k < k_min || k > NEIGHBOUR_K_MAX)
    return fail(SS_EINVAL, "dot_i8: k = %d outside %d..%d", k, k_min, NEIGHBOUR_K_MAX);
  return SS_OK;
}
static int check_rows_i8(const char* what, const int8_t* F, int64_t n, int64_t ld, int64_t d) {
  if (n < 0) return fail(SS_EINVAL, "%s: negative row count", what);
  if (n >= (1LL << 31)) return fail(SS_EUNSUPPORTED, "%s: %lld rows (>= 2^31)", what, (long long)n);
  if (ld < d) return fail(SS_EINVAL, "%s: leading dimension %lld < %lld features (int8 rows are row-major)", what,
                          (long long)ld, (long long)d);
  if (n > 0 && d > 0 && !F) return fail(SS_EINVAL, "%s is NULL", what);
  return SS_OK;
}
// rows on the device: the caller's buffer (SS_MEM_DEVICE) or a staged copy with ld = d; of a host row only its d bytes
// are read
static int stage_rows_i8(const int8_t* F, int64_t n, int64_t ld, int64_t d, int mem, DevBuf<int8_t>& buf,
                         const int8_t** dev, int64_t* dev_ld) {
  if (mem == SS_MEM_DEVICE || n == 0 || d == 0) {
    *dev = F;
    *dev_ld = ld;
    return SS_OK;
  }
  SS_TRY(buf.alloc((size_t)n * (size_t)d));
  SS_HIP(hipMemcpy2DAsync(buf.p, d, F, ld, d, n, hipMemcpyHostToDevice, ctx().stream));
  *dev = buf.p;
  *dev_ld = d;
  return SS_OK;
}

static int dot_csr_i8_impl(const int8_t* Fa, int64_t na, int64_t lda, const int8_t* Fb, int64_t nb, int64_t ldb,
                           int64_t d, int metric, float alpha, int k, int weighted, int64_t* ptr, int32_t* idx,
                           float* val, int64_t capacity, int64_t* nnz, int mem) {
  SS_TRY(require_init());
  SS_TRY(check_mem(mem));
  path_note().clear();
  const bool sym = (Fb == nullptr);
  if (sym) {
    nb = na;
    ldb = lda;
  }
  SS_TRY(check_i8_args(metric, d, alpha, k, 0));
  SS_TRY(check_rows_i8("Fa", Fa, na, lda, d));
  if (!sym) SS_TRY(check_rows_i8("Fb", Fb, nb, ldb, d));
  if (!ptr || !nnz) return fail(SS_EINVAL, "dot_i8: ptr and nnz must not be NULL");
  DevBuf<int8_t> ba, bb;
  const int8_t *da = nullptr, *db = nullptr;
  int64_t la = 0, lb = 0;
  SS_TRY(stage_rows_i8(Fa, na, lda, d, mem, ba, &da, &la));
  if (!sym) SS_TRY(stage_rows_i8(Fb, nb, ldb, d, mem, bb, &db, &lb));
  DotCsrI8 p;
  SS_TRY(p.count(da, na, la, sym ? nullptr : db, nb, lb, d, metric, alpha, weighted != 0, k));
  path_add(i8_names.tag(sym, k));
  return emit_pair_csr<float>(p, na, ptr, idx, val, capacity, nnz, mem);
}

// the order of the checks and the empty inputs are those of features_kth_impl
static int dot_kth_i8_impl(const int8_t* Fa, int64_t na, int64_t lda, const int8_t* Fb, int64_t nb, int64_t ldb,
                           int64_t d, int metric, int k, float* tau, int mem) {
  SS_TRY(require_init());
  SS_TRY(check_mem(mem));
  path_note().clear();
  const bool sym = (Fb == nullptr);
  if (sym) {
    nb = na;
    ldb = lda;
  }
  SS_TRY(check_i8_args(metric, d, 0.0f, k, 1));
  SS_TRY(check_rows_i8("Fa", Fa, na, lda, d));
  if (!sym) SS_TRY(check_rows_i8("Fb", Fb, nb, ldb, d));
  if (na > 0 && !tau) return fail(SS_EINVAL, "dot_i8 kth: tau must not be NULL");
  path_add(i8_names.tag_kth);
  if (na == 0) return SS_OK;
  DevBuf<int8_t> ba, bb;
  const int8_t *da = nullptr, *db = nullptr;
  int64_t la = 0, lb = 0;
  SS_TRY(stage_rows_i8(Fa, na, lda, d, mem, ba, &da, &la));
  if (!sym) SS_TRY(stage_rows_i8(Fb, nb, ldb, d, mem, bb, &db, &lb));
  hipStream_t st = ctx().stream;
  DevBuf<float> dt;
  float* dtau = tau;
  if (mem == SS_MEM_HOST) {
    SS_TRY(dt.alloc(na));
    dtau = dt.p;
  }
  SS_TRY(dot_kth_i8(da, na, la, sym ? nullptr : db, nb, lb, d, metric, nullptr, nullptr, k, dtau));
  if (mem == SS_MEM_HOST) SS_HIP(hipMemcpyAsync(tau, dtau, (size_t)na * sizeof(float), hipMemcpyDeviceToHost, st));
  SS_HIP(hipStreamSynchronize(st));
  return SS_OK;
}

static int graph_create_vectors_i8_impl(int64_t nq, int64_t ns, int64_t nt, int64_t d, int metric, const int8_t* Fq,
                                        int64_t ldq, const int8_t* Fs, int64_t lds_, const int64_t* y_ptr,
                                        const int32_t* y_idx, const float* y_val, int index_base, float alpha, int k,
                                        int weighted, int mem, ss_graph** out) {
  SS_TRY(graph_create_begin(mem, nt, out));
  SS_TRY(check_i8_args(metric, d, alpha, k, 0));
  SS_TRY(check_rows_i8("Fq", Fq, nq, ldq, d));
  SS_TRY(check_rows_i8("Fs", Fs, ns, lds_, d));
  DevBuf<int8_t> bq, bs;
  const int8_t *dq = nullptr, *ds = nullptr;
  int64_t lq = 0, ls = 0;
  SS_TRY(stage_rows_i8(Fs, ns, lds_, d, mem, bs, &ds, &ls));
  SS_TRY(stage_rows_i8(Fq, nq, ldq, d, mem, bq, &dq, &lq));
  const bool wgt = weighted != 0;
  return graph_from_producers<float, DotCsrI8>(
      nq, ns, nt, [&](DotCsrI8& p) { return p.count(ds, ns, ls, nullptr, ns, ls, d, metric, alpha, wgt, k); },
      [&](DotCsrI8& p) { return p.count(dq, nq, lq, ds, ns, ls, d, metric, alpha, wgt, k); }, i8_names.tag(true, k),
      i8_names.tag(false, k), y_ptr, y_idx, y_val, index_base, mem, out);
}

// ------------------- cutoff profiles (include/simspread_hip_profile.h; the device path is cut_profile.hip).  The operand
// checks and the staging are the matching producer's; what is the profile's own is the check of the cuts and the
// delivery of total / rows.
template <class T>
static int check_cuts(const char* what, const T* cuts, int ncuts) {
  if (ncuts < 1 || ncuts > PROFILE_CUTS_MAX)
    return fail(SS_EINVAL, "%s: %d cuts outside 1..%d", what, ncuts, PROFILE_CUTS_MAX);
  if (!cuts) return fail(SS_EINVAL, "%s: cuts is NULL", what);
  for (int b = 0; b < ncuts; ++b) {
    if (cuts[b] != cuts[b]) return fail(SS_EINVAL, "%s: cut %d is NaN", what, b);
    if (b > 0 && cuts[b] < cuts[b - 1]) return fail(SS_EINVAL, "%s: the cuts decrease at %d", what, b);
  }
  return SS_OK;
}
// run(total, rows) fills device arrays; they are the caller's (SS_MEM_DEVICE) or copied to the caller afterwards, so a
// refusal of run leaves the caller's arrays as they were
template <class Run>
static int profile_deliver(const char* what, const char* tag, int64_t na, int ncuts, int64_t* total, int32_t* rows,
                           int mem, Run run) {
  if (!total) return fail(SS_EINVAL, "%s: total must not be NULL", what);
  DevBuf<int64_t> dt;
  DevBuf<int> dr;
  int64_t* t = total;
  int* r = rows;
  if (mem == SS_MEM_HOST) {
    SS_TRY(dt.alloc((size_t)ncuts));
    t = dt.p;
    if (rows) {
      SS_TRY(dr.alloc((size_t)na * (size_t)ncuts));
      r = dr.p;
    }
  }
  SS_TRY(run(t, r));
  path_add(tag);
  if (mem == SS_MEM_HOST) {
    hipStream_t st = ctx().stream;
    SS_HIP(hipMemcpyAsync(total, t, (size_t)ncuts * sizeof(int64_t), hipMemcpyDeviceToHost, st));
    if (rows && na > 0)
      SS_HIP(hipMemcpyAsync(rows, r, (size_t)na * (size_t)ncuts * sizeof(int), hipMemcpyDeviceToHost, st));
    SS_HIP(hipStreamSynchronize(st));
  }
  return SS_OK;
}

template <class T>
static int tanimoto_profile_impl(const uint64_t* Fa, int64_t na, const uint64_t* Fb, int64_t nb, int64_t nwords,
                                 const T* cuts, int ncuts, int weighted, int64_t* total, int32_t* rows, int mem) {
  SS_TRY(require_init());
  SS_TRY(check_mem(mem));
  path_note().clear();
  const bool sym = (Fb == nullptr);
  if (sym) nb = na;
  SS_TRY(check_cuts("tanimoto profile", cuts, ncuts));
  SS_TRY(check_nwords(nwords));
  SS_TRY(check_fingerprints("Fa", Fa, na, nwords));
  if (!sym) SS_TRY(check_fingerprints("Fb", Fb, nb, nwords));
  DevBuf<uint64_t> ba, bb;
  const uint64_t *da = nullptr, *db = nullptr;
  SS_TRY(stage_fingerprints(Fa, na, nwords, mem, ba, &da));
  if (!sym) SS_TRY(stage_fingerprints(Fb, nb, nwords, mem, bb, &db));
  return profile_deliver("tanimoto profile", "tanimoto_profile", na, ncuts, total, rows, mem, [&](int64_t* t, int* r) {
    return tanimoto_profile<T>(da, na, sym ? nullptr : db, nb, nwords, cuts, ncuts, weighted != 0, t, r);
  });
}

// the profile of a producer of column-major feature rows: run(da, na, la, db, nb, lb, total, rows) on device rows
template <class T, class Check, class Run>
static int features_profile_impl(const FeatureNames& nm, const char* tag, Check check, Run run, const T* Fa, int64_t na,
                                 int64_t lda, const T* Fb, int64_t nb, int64_t ldb, int64_t d, const T* cuts, int ncuts,
                                 int64_t* total, int32_t* rows, int mem) {
  SS_TRY(require_init());
  SS_TRY(check_mem(mem));
  path_note().clear();
  const bool sym = (Fb == nullptr);
  if (sym) {
    nb = na;
    ldb = lda;
  }
  SS_TRY(check_cuts(tag, cuts, ncuts));
  SS_TRY(check_feature_args(nm, check, d, cuts[0]));
  SS_TRY(check_features("Fa", Fa, na, lda, d));
  if (!sym) SS_TRY(check_features("Fb", Fb, nb, ldb, d));
  DevBuf<T> ba, bb;
  const T *da = nullptr, *db = nullptr;
  int64_t la = 0, lb = 0;
  SS_TRY(stage_features(Fa, na, lda, d, mem, ba, &da, &la));
  if (!sym) SS_TRY(stage_features(Fb, nb, ldb, d, mem, bb, &db, &lb));
  return profile_deliver(tag, tag, na, ncuts, total, rows, mem,
                         [&](int64_t* t, int* r) { return run(da, na, la, sym ? nullptr : db, nb, lb, t, r); });
}
template <class T>
static int jaccard_profile_impl(const T* Fa, int64_t na, int64_t lda, const T* Fb, int64_t nb, int64_t ldb, int64_t d,
                                const T* cuts, int ncuts, int weighted, int64_t* total, int32_t* rows, int mem) {
  return features_profile_impl<T>(
      jaccard_names, "jaccard_profile", no_check,
      [=](const T* da, int64_t na_, int64_t la, const T* db, int64_t nb_, int64_t lb, int64_t* t, int* r) {
        return jaccard_profile<T>(da, na_, la, db, nb_, lb, d, cuts, ncuts, weighted != 0, t, r);
      },
      Fa, na, lda, Fb, nb, ldb, d, cuts, ncuts, total, rows, mem);
}
template <class T>
static int dot_profile_impl(const T* Fa, int64_t na, int64_t lda, const T* Fb, int64_t nb, int64_t ldb, int64_t d,
                            int metric, const T* cuts, int ncuts, int weighted, int64_t* total, int32_t* rows, int mem) {
  return features_profile_impl<T>(
      dot_names, "dot_profile", [=] { return check_sim_metric(metric); },
      [=](const T* da, int64_t na_, int64_t la, const T* db, int64_t nb_, int64_t lb, int64_t* t, int* r) {
        return dot_profile<T>(da, na_, la, db, nb_, lb, d, metric, cuts, ncuts, weighted != 0, t, r);
      },
      Fa, na, lda, Fb, nb, ldb, d, cuts, ncuts, total, rows, mem);
}
static int dot_profile_h16_impl(const uint16_t* Fa, int64_t na, int64_t lda, const uint16_t* Fb, int64_t nb, int64_t ldb,
                                int64_t d, int storage, int metric, const float* cuts, int ncuts, int weighted,
                                int64_t* total, int32_t* rows, int mem) {
  SS_TRY(require_init());
  SS_TRY(check_mem(mem));
  path_note().clear();
  const bool sym = (Fb == nullptr);
  if (sym) {
    nb = na;
    ldb = lda;
  }
  SS_TRY(check_cuts("dot_h16_profile", cuts, ncuts));
  SS_TRY(check_h16_args(storage, metric, d, cuts[0]));
  SS_TRY(check_rows_h16("Fa", Fa, na, lda, d));
  if (!sym) SS_TRY(check_rows_h16("Fb", Fb, nb, ldb, d));
  DevBuf<uint16_t> ba, bb;
  const uint16_t *da = nullptr, *db = nullptr;
  int64_t la = 0, lb = 0;
  SS_TRY(stage_rows_h16(Fa, na, lda, d, mem, ba, &da, &la));
  if (!sym) SS_TRY(stage_rows_h16(Fb, nb, ldb, d, mem, bb, &db, &lb));
  return profile_deliver("dot_h16_profile", "dot_h16_profile", na, ncuts, total, rows, mem, [&](int64_t* t, int* r) {
    return dot_profile_h16(da, na, la, sym ? nullptr : db, nb, lb, d, storage, metric, cuts, ncuts, weighted != 0, t, r);
  });
}

// ------------------------------------------------------------------ Butina clusters, cluster folds, cross-fold edges
// (include/simspread_hip_clusters.h; the device path is cluster.hip)
struct ClusterOut {
  int32_t *centre, *label, *size;
  int64_t *nclusters, *rounds;
};
// the common head of the clustering entry points: nothing is written before these pass
static int cluster_begin(int64_t n, const ClusterOut& o, int mem) {
  SS_TRY(require_init());
  SS_TRY(check_mem(mem));
  path_note().clear();
  timing_begin_call();
  if (n < 0) return fail(SS_EINVAL, "butina: negative source count");
  if (n >= (1LL << 31) - 64) return fail(SS_EUNSUPPORTED, "butina: %lld sources (>= 2^31)", (long long)n);
  if (!o.nclusters) return fail(SS_EINVAL, "butina: nclusters must not be NULL");
  if (n > 0 && (!o.centre || !o.label)) return fail(SS_EINVAL, "butina: centre and label must not be NULL");
  return SS_OK;
}
// cluster the device pattern (dptr, didx) and deliver centre, label and size in `mem`
static int cluster_deliver(int64_t n, const int64_t* dptr, const int32_t* didx, int base, int64_t nnz_in, bool validate,
                           const ClusterOut& o, int mem) {
  hipStream_t st = ctx().stream;
  DevBuf<int> bc, bl, bs;
  int *dc = o.centre, *dl = o.label, *dsz = o.size;
  if (mem == SS_MEM_HOST || validate) {
    // a pattern that is still to be checked must not cost the caller's buffers their contents
    SS_TRY(bc.alloc(n));
    SS_TRY(bl.alloc(n));
    dc = bc.p;
    dl = bl.p;
    if (o.size) {
      SS_TRY(bs.alloc(n));
      dsz = bs.p;
    }
  }
  int64_t nc = 0, rounds = 0;
  StageTimer total(ST_TOTAL);
  SS_TRY(butina_csr(n, dptr, didx, base, nnz_in, validate, dc, dl, dsz, &nc, &rounds));
  total.stop();
  if (dc != o.centre) {
    const hipMemcpyKind back = mem == SS_MEM_HOST ? hipMemcpyDeviceToHost : hipMemcpyDeviceToDevice;
    SS_HIP(hipMemcpyAsync(o.centre, dc, (size_t)n * sizeof(int), back, st));
    SS_HIP(hipMemcpyAsync(o.label, dl, (size_t)n * sizeof(int), back, st));
    if (o.size) SS_HIP(hipMemcpyAsync(o.size, dsz, (size_t)nc * sizeof(int), back, st));
    SS_HIP(hipStreamSynchronize(st));
  }
  *o.nclusters = nc;
  if (o.rounds) *o.rounds = rounds;
  return SS_OK;
}

// a caller's n x n pattern on the device: ptr[0] == index_base and the entry count, read before anything is staged
struct UserPattern {
  DevBuf<int64_t> bptr;
  DevBuf<int32_t> bidx;
  const int64_t* ptr = nullptr;
  const int32_t* idx = nullptr;
  int64_t nnz_in = 0;
};
static int stage_pattern(const char* what, int64_t n, const int64_t* ptr, const int32_t* idx, int index_base, int mem,
                         UserPattern& u) {
  hipStream_t st = ctx().stream;
  if (index_base != 0 && index_base != 1) return fail(SS_EINVAL, "%s: index_base must be 0 or 1", what);
  if (!ptr) return fail(SS_EINVAL, "%s: row pointer array is NULL", what);
  int64_t first = 0, last = 0;
  if (mem == SS_MEM_HOST) {
    first = ptr[0];
    last = ptr[n];
  } else {
    SS_HIP(hipMemcpyAsync(&last, ptr + n, sizeof(int64_t), hipMemcpyDeviceToHost, st));
    SS_HIP(hipMemcpyAsync(&first, ptr, sizeof(int64_t), hipMemcpyDeviceToHost, st));
    SS_HIP(hipStreamSynchronize(st));
  }
  if (first != index_base) return fail(SS_EINVAL, "%s: row pointer does not start at index_base", what);
  u.nnz_in = last - index_base;
  if (u.nnz_in < 0) return fail(SS_EINVAL, "%s: negative entry count in row pointers", what);
  if (u.nnz_in >= (1LL << 31) - 64) return fail(SS_EUNSUPPORTED, "%s: %lld stored entries (>= 2^31)", what,
                                                (long long)u.nnz_in);
  if (u.nnz_in > 0 && !idx) return fail(SS_EINVAL, "%s: column index array is NULL", what);
  u.ptr = ptr;
  u.idx = idx;
  if (mem == SS_MEM_HOST) {
    SS_TRY(u.bptr.alloc(n + 1));
    SS_TRY(upload(u.bptr.p, ptr, n + 1, mem));
    SS_TRY(u.bidx.alloc(u.nnz_in));
    SS_TRY(upload(u.bidx.p, idx, u.nnz_in, mem));
    u.ptr = u.bptr.p;
    u.idx = u.bidx.p;
  }
  return SS_OK;
}

static int cluster_butina_csr_impl(int64_t n, const int64_t* ptr, const int32_t* idx, int index_base,
                                   const ClusterOut& o, int mem) {
  SS_TRY(cluster_begin(n, o, mem));
  path_add("butina_csr");
  if (n == 0) {
    *o.nclusters = 0;
    if (o.rounds) *o.rounds = 0;
    return SS_OK;
  }
  UserPattern u;
  SS_TRY(stage_pattern("butina", n, ptr, idx, index_base, mem, u));
  if (u.nnz_in >= (1LL << 30))
    return fail(SS_EUNSUPPORTED, "butina: %lld stored entries (>= 2^30)", (long long)u.nnz_in);
  return cluster_deliver(n, u.ptr, u.idx, index_base, u.nnz_in, true, o, mem);
}

// the plain self-similarity pattern of producer p (counted already): its indices, then the clustering, on the device
template <class T>
static int cluster_from_producer(PairCsr<T>& p, int64_t n, const ClusterOut& o, int mem) {
  if (p.nnz >= (1LL << 30))
    return fail(SS_EUNSUPPORTED, "butina: the %s pattern has %lld entries (>= 2^30): raise the cutoff", p.what,
                (long long)p.nnz);
  DevBuf<int> idx;
  SS_TRY(idx.alloc(p.nnz));
  if (p.nnz > 0) SS_TRY(p.fill(idx.p, nullptr, nullptr));
  return cluster_deliver(n, p.ptr.p, idx.p, 0, p.nnz, false, o, mem);
}
static int cluster_empty(const ClusterOut& o) {
  *o.nclusters = 0;
  if (o.rounds) *o.rounds = 0;
  return SS_OK;
}

template <class T>
static int cluster_butina_fingerprint_impl(const uint64_t* F, int64_t n, int64_t nwords, T cutoff, const ClusterOut& o,
                                           int mem) {
  SS_TRY(cluster_begin(n, o, mem));
  SS_TRY(check_nwords(nwords));
  SS_TRY(check_fingerprints("F", F, n, nwords));
  if (cutoff != cutoff) return fail(SS_EINVAL, "butina: cutoff is NaN");
  path_add("butina_csr");
  path_add(tanimoto_tag(true, 0));
  if (n == 0) return cluster_empty(o);
  DevBuf<uint64_t> bf;
  const uint64_t* df = nullptr;
  SS_TRY(stage_fingerprints(F, n, nwords, mem, bf, &df));
  TanimotoCsr<T> tc;
  SS_TRY(tc.count(df, n, nullptr, n, nwords, cutoff, false, 0));
  return cluster_from_producer<T>(tc, n, o, mem);
}

template <class T, class Prod, class Check, class Count>
static int cluster_butina_rows_impl(const FeatureNames& nm, Check check, Count count, const T* F, int64_t n, int64_t d,
                                    int64_t ld, T cutoff, const ClusterOut& o, int mem) {
  SS_TRY(cluster_begin(n, o, mem));
  SS_TRY(check_feature_args(nm, check, d, cutoff));
  SS_TRY(check_features("F", F, n, ld, d));
  path_add("butina_csr");
  path_add(nm.tag(true, 0));
  if (n == 0) return cluster_empty(o);
  DevBuf<T> bf;
  const T* df = nullptr;
  int64_t lf = 0;
  SS_TRY(stage_features(F, n, ld, d, mem, bf, &df, &lf));
  Prod p;
  SS_TRY(count(p, df, n, lf, nullptr, n, lf));
  return cluster_from_producer<T>(p, n, o, mem);
}
template <class T>
static int cluster_butina_features_impl(const T* F, int64_t n, int64_t d, int64_t ld, T cutoff, const ClusterOut& o,
                                        int mem) {
  return cluster_butina_rows_impl<T, JaccardCsr<T>>(jaccard_names, no_check, jaccard_count<T>(d, cutoff, 0), F, n, d, ld,
                                                    cutoff, o, mem);
}
template <class T>
static int cluster_butina_vectors_impl(int metric, const T* F, int64_t n, int64_t d, int64_t ld, T cutoff,
                                       const ClusterOut& o, int mem) {
  return cluster_butina_rows_impl<T, DotCsr<T>>(
      dot_names, [=] { return check_sim_metric(metric); }, dot_count<T>(d, metric, cutoff, 0), F, n, d, ld, cutoff, o,
      mem);
}

static int cluster_folds_impl(const int32_t* label, int64_t n, int64_t nclusters, int nfolds, int32_t* fold, int mem) {
  SS_TRY(check_mem(mem));
  if (mem == SS_MEM_DEVICE) SS_TRY(require_init());
  if (n < 0 || nclusters < 0) return fail(SS_EINVAL, "cluster folds: negative count");
  if (nfolds < 1) return fail(SS_EINVAL, "cluster folds: nfolds = %d < 1", nfolds);
  if (n == 0) return SS_OK;
  if (!label || !fold) return fail(SS_EINVAL, "cluster folds: NULL argument");
  if (mem == SS_MEM_HOST) {
    std::vector<int32_t> out((size_t)n);
    SS_TRY(cluster_folds(label, n, nclusters, nfolds, out.data()));
    std::copy(out.begin(), out.end(), fold);
    return SS_OK;
  }
  hipStream_t st = ctx().stream;
  std::vector<int32_t> in((size_t)n), out((size_t)n);
  SS_HIP(hipMemcpyAsync(in.data(), label, (size_t)n * sizeof(int32_t), hipMemcpyDeviceToHost, st));
  SS_HIP(hipStreamSynchronize(st));
  SS_TRY(cluster_folds(in.data(), n, nclusters, nfolds, out.data()));
  SS_HIP(hipMemcpyAsync(fold, out.data(), (size_t)n * sizeof(int32_t), hipMemcpyHostToDevice, st));
  SS_HIP(hipStreamSynchronize(st));
  return SS_OK;
}

static int cluster_cross_edges_impl(int64_t n, const int64_t* ptr, const int32_t* idx, int index_base,
                                    const int32_t* fold, int nfolds, int64_t* count, int mem) {
  SS_TRY(require_init());
  SS_TRY(check_mem(mem));
  path_note().clear();
  if (n < 0) return fail(SS_EINVAL, "cross edges: negative source count");
  if (n >= (1LL << 31) - 64) return fail(SS_EUNSUPPORTED, "cross edges: %lld sources (>= 2^31)", (long long)n);
  if (nfolds < 1) return fail(SS_EINVAL, "cross edges: nfolds = %d < 1", nfolds);
  if (!count || (n > 0 && !fold)) return fail(SS_EINVAL, "cross edges: NULL argument");
  path_add("cross_edges");
  hipStream_t st = ctx().stream;
  UserPattern u;
  DevBuf<int32_t> bfold;
  DevBuf<int64_t> bcount;
  const int32_t* dfold = fold;
  if (n > 0) {
    SS_TRY(stage_pattern("cross edges", n, ptr, idx, index_base, mem, u));
    if (mem == SS_MEM_HOST) {
      SS_TRY(bfold.alloc(n));
      SS_TRY(upload(bfold.p, fold, n, mem));
      dfold = bfold.p;
    }
  }
  // counted aside: a pattern or a fold vector that fails its check leaves `count` as it was
  SS_TRY(bcount.alloc(nfolds));
  SS_TRY(cross_edges(n, u.ptr, u.idx, index_base, u.nnz_in, dfold, nfolds, bcount.p));
  SS_HIP(hipMemcpyAsync(count, bcount.p, (size_t)nfolds * sizeof(int64_t),
                        mem == SS_MEM_HOST ? hipMemcpyDeviceToHost : hipMemcpyDeviceToDevice, st));
  SS_HIP(hipStreamSynchronize(st));
  return SS_OK;
}

// ------------------------------------------------------------------ cutoff sweeps: featurize on resident CSR
// an unstored zero passes an unweighted cutoff at alpha <= 0, which CSR cannot hold
template <class T>
static int check_cut_alpha(const char* what, T alpha) {
  if (!(alpha > T(0))) return fail(SS_EINVAL, "%s: alpha must be > 0 and not NaN (alpha <= 0 keeps unstored zeros)", what);
  return SS_OK;
}

template <class T>
static int cutoff_csr_impl(int64_t rows, int64_t cols, const int64_t* ptr, const int32_t* idx, const T* val,
                           int index_base, T alpha, int weighted, int64_t* optr, int32_t* oidx, T* oval,
                           int64_t capacity, int64_t* nnz, int mem) {
  SS_TRY(require_init());
  SS_TRY(check_mem(mem));
  path_note().clear();
  SS_TRY(check_cut_alpha("cutoff_csr", alpha));
  if (!optr || !nnz) return fail(SS_EINVAL, "cutoff_csr: optr and nnz must not be NULL");
  DevCsr<T> in;  // checked, 0-based, stored zeros dropped (they fail v >= alpha > 0 anyway)
  SS_TRY(csr_from_user<T>(rows, cols, ptr, idx, val, index_base, mem, in));
  CutCsr<T> cc;
  SS_TRY(cc.count(in, alpha, weighted != 0));
  path_add("cutoff_csr");
  return emit_pair_csr<T>(cc, rows, optr, oidx, oval, capacity, nnz, mem);
}

template <class T>
static int graph_recut_impl(const ss_graph* h, T alpha, int weighted, ss_graph** out) {
  if (!out) return fail(SS_EINVAL, "out handle pointer is NULL");
  *out = nullptr;
  Graph<T>* p = nullptr;
  SS_TRY(graph_check<T>(h, &p));
  path_note().clear();
  if (p->general) return fail(SS_EUNSUPPORTED, "recut: a general graph carries no featurize cutoff");
  if (p->dense.on)
    return fail(SS_EUNSUPPORTED, "recut: a dense-similarity graph re-thresholds in place, use ss_graph_set_cutoff_*");
  SS_TRY(check_cut_alpha("recut", alpha));
  GraphBox<T>* box = new (std::nothrow) GraphBox<T>();
  if (!box) return fail(SS_ENOMEM, "host allocation failed");
  box->dtype = (int)sizeof(T);
  const int rc = graph_recut<T>(*p, alpha, weighted != 0, box->g);
  if (rc != SS_OK) { delete box; return rc; }
  path_add("recut");
  *out = reinterpret_cast<ss_graph*>(box);
  return SS_OK;
}

// dense-similarity graph: the cutoff lives in the handle, the raw similarities stay where they are
template <class T>
static int graph_set_cutoff_impl(ss_graph* h, T alpha, int weighted) {
  Graph<T>* g = nullptr;
  SS_TRY(graph_check<T>(h, &g));
  if (!g->dense.on)
    return fail(SS_EUNSUPPORTED, "set_cutoff: only a dense-similarity graph holds raw similarities, use ss_graph_recut_*");
  DenseSim<T>& d = g->dense;
  d.alpha = alpha;
  d.weighted = weighted != 0;
  d.Bpl_np = 0;  // the bf16 planes of the thresholded source side are rebuilt by the next prediction
  return dense_degrees(*g);  // kf, ks, their reciprocals and 1/(kf-1); synchronises
}

// SELL chunk of the stage-2 operands for tile width qt; SS_SELL_CHUNK lowers it
template <class T>
static int sell_chunk(int qt) {
  const int kcmax = sell_max_chunk<T>(qt);
  return (int)env_int_in("SS_SELL_CHUNK", 64, kcmax, kcmax);
}

// stage-2 operand of a graph: W = Ys' cut for the tile width of this precision
template <class T>
static int graph_sell(Graph<T>& g) {
  const int qt = sell_tile_width<T>();
  if (g.W_qt == qt) return SS_OK;
  SS_TRY(sell_build<T>(g.YsT, sell_chunk<T>(qt), g.W));
  g.W_qt = qt;
  return SS_OK;
}

// Column chunk of a stage-1 operand mT (ns columns): sized so that an average sub-row fills one 64-lane load
// (SC ~ 64 * ns / mean row length), the chunk count a multiple of 8 so that chunk c always meets the same XCD's L2.
// honour_switch: SS_TRANSFER_CHUNK replaces the size before it is rounded.
template <class T>
static int transfer_chunk_cols(const DevCsr<T>& mT, int64_t ns, bool honour_switch) {
  if (ns < 1) ns = 1;
  const double mean_len = mT.rows > 0 ? (double)mT.nnz / (double)mT.rows : 0.0;
  int64_t sc = mean_len > 1.0 ? (int64_t)(64.0 * (double)ns / mean_len) : ns;
  // keep >= 8 single-wave workgroups per CU: (SC + 64) * sizeof(T) <= 20 KiB (measured at 100k x 100k, 1 %:
  // SC 6250 -> 7.7 ms, 4167 -> 4.5 ms, 3200 -> 5.9 ms for 2048 folds)
  const int64_t sc_max = (20 * 1024) / (int64_t)sizeof(T) - 64;
  if (sc > sc_max) sc = sc_max;
  if (sc < 256) sc = 256;
  if (honour_switch) sc = env_int_in("SS_TRANSFER_CHUNK", 16, 8193, sc);
  int64_t nch = ceil_div(ns, sc);
  if (nch > 1) nch = ceil_div(nch, 8) * 8;
  return (int)(ceil_div(ceil_div(ns, nch), 4) * 4);
}

// stage-1 operands cut into column chunks: Xs' of a sparse graph, and for source rows (need_y) Ys' with the same chunk.
// A dense-similarity graph has no Xs': the Ys' of its sparse target path is sized by itself (and never honoured
// SS_TRANSFER_CHUNK).
template <class T>
static int graph_chunked(Graph<T>& g, bool need_y) {
  if (!g.dense.on && g.XsTc.SC == 0)
    SS_TRY(chunked_build<T>(g.XsT, transfer_chunk_cols(g.XsT, g.ns, true), 1, g.XsTc));
  if (need_y && g.YsTc.SC == 0)
    SS_TRY(chunked_build<T>(g.YsT, g.dense.on ? transfer_chunk_cols(g.YsT, g.ns, false) : g.XsTc.SC, 1, g.YsTc));
  return SS_OK;
}

// rows of T held at once (stage-1 output, stage-2 input)
static int64_t transfer_batch_rows(int64_t nrows, int64_t nj, size_t elem) {
  int64_t cap_bytes = env_int("SS_TRANSFER_BYTES", 0);
  if (cap_bytes < (1 << 20)) cap_bytes = 2LL << 30;
  int64_t rb = cap_bytes / ((nj > 0 ? nj : 1) * (int64_t)elem);
  rb &= ~7LL;
  if (rb < 8) rb = 8;
  return rb < nrows ? rb : nrows;
}

// Dense-similarity stage 1 of rows [r0, r0 + nb) -- of members[] when that is given -- into dst.  fp64: the fp64 matrix
// instruction (dense_f64.hip, the reference's default precision).  fp32: the bf16 matrix cores on exact bf16 planes of
// the operands (dense_bf16.hip: 1.5x weighted, 3.2x unweighted at 50k); SS_DENSE_BF16=0 selects the fp32-input MFMA
// kernel of dense.hip, which gathers no member rows: the k-fold calls (members != NULL) never take it.
template <class T>
static int dense_transfer(Graph<T>& g, bool loo, const T* inv_kf, const T* inv_ks, const int* ks, int64_t r0, int64_t nb,
                          T* dst, int64_t ld, bool srcrows, const int* members) {
  if constexpr (std::is_same<T, float>::value) {
    if (!members && env_off("SS_DENSE_BF16"))
      return launch_transfer_dense(g.dense, loo, inv_kf, inv_ks, ks, r0, nb, dst, ld, srcrows);
    return launch_transfer_dense_bf16(g.dense, loo, inv_kf, inv_ks, ks, r0, nb, dst, ld, srcrows, members);
  } else {
    return launch_transfer_dense_f64(g.dense, loo, inv_kf, inv_ks, ks, r0, nb, dst, ld, srcrows, members);
  }
}

// Where stage 2 puts the score rows of a batch.  Row q of the batch goes to row
//   o + q              of dst: contiguous rows (row_map and host_rows NULL)
//   row_map[o + q]     device row map: fused into the SELL launch when the operand is unsorted, launch_scatter_rows
//                      after launch_unpermute when it is length-sorted
//   host_rows[o + q]   the same rows on the host, given next to row_map: a length-sorted operand's rows are then put in
//                      place by one copy each instead of the scatter (ss_predict_kfold_*: few folds x rows)
template <class T>
struct ScoreDest {
  T* dst;
  int64_t ld, o;
  const int* row_map;
  const int* host_rows;
};

// Stage 2 of nb score rows: F = R W' with the SELL operand W (ncols score columns), R row-major with leading dimension
// ldr.  A length-sorted operand gives its scores in sorted target order into the scratch buffer ws (sized for batches of
// rb rows, plus rb packed rows when the destination rows are not contiguous); launch_unpermute puts them back (+ clean!).
template <class T>
static int sell_rows(const DevSell<T>& W, const T* R, int64_t ldr, int64_t ncols, DevBuf<T>& ws, int64_t rb, int64_t nb,
                     const int* kt_clean, const ScoreDest<T>& d) {
  const int* rows = d.row_map ? d.row_map + d.o : nullptr;
  T* out = rows ? d.dst : d.dst + d.o * d.ld;
  if (!W.sorted) {
    StageTimer t2(ST_SPMM);
    SS_TRY(launch_spmm_sell<T>(W, R, ldr, nb, out, d.ld, kt_clean, rows));
    timing_count(ST_NSPMM, 1);
    return SS_OK;
  }
  const size_t nsorted = (size_t)rb * (size_t)W.vrows;
  const size_t need_s = nsorted + (rows ? (size_t)rb * (size_t)ncols : 0);
  if (ws.n < need_s) SS_TRY(ws.alloc(need_s));
  {
    StageTimer t2(ST_SPMM);
    SS_TRY(launch_spmm_sell<T>(W, R, ldr, nb, ws.p, W.vrows, nullptr));
    timing_count(ST_NSPMM, 1);
  }
  StageTimer t3(ST_EPILOGUE);
  T* packed = ws.p + nsorted;  // rows in batch order before they go to their places
  SS_TRY(launch_unpermute<T>(ws.p, W.vrows, nb, ncols, W.vfirst.p, W.inv.p, kt_clean, rows ? packed : out,
                             rows ? ncols : d.ld));
  if (d.host_rows) {
    for (int64_t q = 0; q < nb; ++q)
      SS_HIP(hipMemcpyAsync(d.dst + (int64_t)d.host_rows[d.o + q] * d.ld, packed + q * ncols, ncols * sizeof(T),
                            hipMemcpyDeviceToDevice, ctx().stream));
  } else if (rows) {
    SS_TRY(launch_scatter_rows<T>(packed, ncols, nb, ncols, rows, d.dst, d.ld));
  }
  return SS_OK;
}

// stage 2 of a graph's score rows: the nb rows of the transfer block g.Tws (batches of at most rb rows) through W = Ys'
template <class T>
static int stage2_rows(Graph<T>& g, int64_t rb, int64_t nb, const int* kt_clean, const ScoreDest<T>& d) {
  return sell_rows<T>(g.W, g.Tws.p, g.ns, g.nt, g.Sws, rb, nb, kt_clean, d);
}

// The coefficient table of left operand L of graph g, kept in tb (a member of g, or of a query set bound to g): built at
// the first prediction that wants it and again after g's degrees changed.  *out stays NULL -- the kernels gather -- with
// SS_TRANSFER_COEF=0 and for a table above SS_TRANSFER_COEF_BYTES (default 1 GiB).
template <class T>
static int coef_table(const Graph<T>& g, CoefTable<T>& tb, const DevCsr<T>& L, const T* inv1, const int* kf_loo,
                      const T** out) {
  *out = nullptr;
  if (env_off("SS_TRANSFER_COEF")) return SS_OK;
  const int64_t cap = env_int("SS_TRANSFER_COEF_BYTES", 1LL << 30);
  if (L.nnz * (int64_t)sizeof(T) > cap) return SS_OK;
  if (tb.epoch != g.coef_epoch) {
    tb.drop();
    SS_TRY(tb.c.alloc((size_t)L.nnz));
    SS_TRY(transfer_coef_build<T>(L, inv1, kf_loo, tb.c.p));
    tb.epoch = g.coef_epoch;
  }
  *out = tb.c.p;
  return SS_OK;
}

// run stage 1 + stage 2 over [row_begin, row_end) into dev_out (row-major nrows x nt, ld = ldo); Xq: the query block
// SS_ROWS_QUERY rows of a sparse graph are taken from (the graph's own, or a query set's, then with its table qtab)
template <class T>
static int predict_rows_device(Graph<T>& g, const DevCsr<T>& Xq, int kind, int64_t row_begin, int64_t row_end, int clean,
                               T* dev_out, int64_t ldo, CoefTable<T>* qtab = nullptr) {
  const int64_t nrows = row_end - row_begin;
  const int64_t nj = g.ns;
  SS_TRY(graph_sell(g));
  SS_TRY(graph_chunked(g, kind == SS_ROWS_SOURCE));
  const T* coef[2] = {nullptr, nullptr};
  if (!g.dense.on) {
    if (kind == 2) {
      SS_TRY(coef_table<T>(g, g.coef_loo, g.Xs, nullptr, g.kf.p, &coef[0]));
    } else if (kind == SS_ROWS_QUERY) {
      if (&Xq == &g.Xq) qtab = &g.coef_q;
      if (qtab) SS_TRY(coef_table<T>(g, *qtab, Xq, g.inv_kf.p, nullptr, &coef[0]));
    } else {
      SS_TRY(coef_table<T>(g, g.coef_s, g.Xs, g.inv_kf.p, nullptr, &coef[0]));
      SS_TRY(coef_table<T>(g, g.coef_y, g.Ys, g.inv_kt.p, nullptr, &coef[1]));
    }
  }
  const int64_t rb = transfer_batch_rows(nrows, nj, sizeof(T));
  // the transfer block lives in the handle so that repeated predictions do not re-allocate
  const size_t need = (size_t)rb * (size_t)(nj > 0 ? nj : 1);
  if (g.Tws.n < need) SS_TRY(g.Tws.alloc(need));
  DevBuf<T>& Tbuf = g.Tws;
  for (int64_t r0 = 0; r0 < nrows; r0 += rb) {
    const int64_t nb = (nrows - r0 < rb) ? (nrows - r0) : rb;
    {
      StageTimer t1(ST_TRANSFER);
      if (g.dense.on) {
        const bool loo = (kind == 2);
        const bool srcrows = (kind == SS_ROWS_SOURCE);  // feature path here, target path added below
        SS_TRY(dense_transfer<T>(g, loo, loo ? g.dense.inv_kf_m1.p : g.inv_kf.p, g.inv_ks.p, g.ks.p, row_begin + r0, nb,
                                 Tbuf.p, nj, srcrows, nullptr));
        if (srcrows) {
          // target path (Ys D_t^-1) Ys' D_s^-1 of the source rows: sparse, added to T
          const DevCsr<T>* L[2] = {&g.Ys, nullptr};
          const DevChunked<T>* M[2] = {&g.YsTc, nullptr};
          const T* inv1[2] = {g.inv_kt.p, nullptr};
          SS_TRY(launch_transfer<T>(1, L, inv1, M, g.inv_ks.p, row_begin + r0, nb, nj, Tbuf.p, nj, nullptr, true));
        }
      } else if (kind == 2) {
        SS_TRY(launch_transfer_loo<T>(g.Xs, g.XsTc, g.kf.p, g.ks.p, row_begin + r0, nb, Tbuf.p, nj, coef[0]));
      } else if (kind == SS_ROWS_QUERY) {
        // query rows: SS_TRANSFER_V=2 selects the query-block kernels (measured variants of round 3)
        // when the chunk's sub-row offsets fit in LDS next to >= 8 waves of accumulators; default: the single-wave kernel
        const bool want_block = env_int("SS_TRANSFER_V", 0) >= 2 && transfer_block_fits<T>(g.XsT.rows, g.XsTc.SC);
        if (want_block) {
          if (g.XsTb.SC == 0) {
            const int al = env_int("SS_TRANSFER_ALIGN", 32) == 1 ? 1 : 32;
            SS_TRY(chunked_build<T>(g.XsT, g.XsTc.SC, al, g.XsTb));
          }
          if (g.Cq.n < (size_t)(Xq.nnz > 0 ? Xq.nnz : 1)) SS_TRY(g.Cq.alloc((size_t)(Xq.nnz > 0 ? Xq.nnz : 1)));
          const bool fixed = !env_off("SS_TRANSFER_FIX");
          SS_TRY(launch_transfer_block<T>(Xq, g.inv_kf.p, g.XsTb, g.inv_ks.p, row_begin + r0, nb, nj, Tbuf.p, nj, g.Cq.p,
                                          g.XsTb.vmax, fixed));
        } else {
          const DevCsr<T>* L[2] = {&Xq, nullptr};
          const DevChunked<T>* M[2] = {&g.XsTc, nullptr};
          const T* inv1[2] = {g.inv_kf.p, nullptr};
          SS_TRY(launch_transfer<T>(1, L, inv1, M, g.inv_ks.p, row_begin + r0, nb, nj, Tbuf.p, nj, nullptr, false, coef));
        }
      } else {
        // source rows: feature path + target path
        const DevCsr<T>* L[2] = {&g.Xs, &g.Ys};
        const DevChunked<T>* M[2] = {&g.XsTc, &g.YsTc};
        const T* inv1[2] = {g.inv_kf.p, g.inv_kt.p};
        SS_TRY(launch_transfer<T>(2, L, inv1, M, g.inv_ks.p, row_begin + r0, nb, nj, Tbuf.p, nj, nullptr, false, coef));
      }
      timing_count(ST_NTRANSFER, 1);
    }
    SS_TRY(stage2_rows<T>(g, rb, nb, clean ? g.kt.p : nullptr, ScoreDest<T>{dev_out, ldo, r0, nullptr, nullptr}));
  }
  if (kind == 2 && clean) {
    StageTimer t3(ST_EPILOGUE);
    SS_TRY(launch_loo_clean_fix<T>(g.YsT, g.kt.p, row_begin, nrows, dev_out, ldo));
  }
  return SS_OK;
}

template <class T>
static int loo_graph_check(const Graph<T>& g) {
  if (g.general || (!g.dense.on && g.nq != 0) || g.ns != g.nf)
    return fail(SS_EINVAL, "leave-one-out needs a graph with nq == 0 and ns == nf (feature j named after source j)");
  return SS_OK;
}

// How score rows reach the caller.  begin() opens the call's timing and its ST_TOTAL span and yields the row-major device
// block the scores are computed into (dev_rm, ld_rm): the caller's own buffer when that is on the device and row-major,
// else a block this owns.  deliver() transposes for a column-major caller, closes the span and copies to a host caller.
// The copies are asynchronous and the staging buffers live as long as this does: a call that is not direct()
// synchronises the stream before it returns.
template <class T>
struct ScoreOut {
  T* out = nullptr;
  int64_t ld = 0, nrows = 0, nt = 0;
  int layout = SS_LAYOUT_ROWMAJOR, mem = SS_MEM_DEVICE;
  T* dev_rm = nullptr;
  int64_t ld_rm = 0;
  hipEvent_t e_begin = nullptr;
  DevBuf<T> scores;  // row-major nrows x nt
  DevBuf<T> cm;      // column-major staging when the caller is on the host

  bool direct() const { return mem == SS_MEM_DEVICE && layout == SS_LAYOUT_ROWMAJOR; }
  int begin(T* out_, int64_t ld_, int layout_, int mem_, int64_t nrows_, int64_t nt_) {
    out = out_; ld = ld_; layout = layout_; mem = mem_; nrows = nrows_; nt = nt_;
    timing_begin_call();
    SS_TRY(timing_mark(&e_begin));
    dev_rm = out;
    ld_rm = ld;
    if (!direct()) {
      SS_TRY(scores.alloc((size_t)nrows * nt));
      dev_rm = scores.p;
      ld_rm = nt;
    }
    return SS_OK;
  }
  int deliver() {
    if (layout == SS_LAYOUT_COLMAJOR) {
      StageTimer t3(ST_EPILOGUE);
      T* dst = out;
      int64_t dld = ld;
      if (mem == SS_MEM_HOST) {
        SS_TRY(cm.alloc((size_t)nrows * nt));
        dst = cm.p;
        dld = nrows;
      }
      SS_TRY(launch_transpose<T>(dev_rm, nrows, nt, ld_rm, dst, dld));
    }
    hipEvent_t e_end;
    SS_TRY(timing_mark(&e_end));
    timing_span(ST_TOTAL, e_begin, e_end);
    if (mem == SS_MEM_HOST) {
      StageTimer t5(ST_D2H);
      if (layout == SS_LAYOUT_ROWMAJOR) {
        SS_HIP(hipMemcpy2DAsync(out, ld * sizeof(T), dev_rm, ld_rm * sizeof(T), nt * sizeof(T), nrows,
                                hipMemcpyDeviceToHost, ctx().stream));
      } else {
        SS_HIP(hipMemcpy2DAsync(out, ld * sizeof(T), cm.p, nrows * sizeof(T), nrows * sizeof(T), nt,
                                hipMemcpyDeviceToHost, ctx().stream));
      }
    }
    return SS_OK;
  }
};

// kind: SS_ROWS_QUERY, SS_ROWS_SOURCE, or 2 (SS_ROWS_LOO) = leave-one-out; qh: the query set SS_ROWS_QUERY rows are taken
// from instead of the graph's own (ss_predict_queries_*)
template <class T>
static int predict_impl(ss_graph* h, int kind, int64_t row_begin, int64_t row_end, int clean, T* out, int64_t ld,
                        int layout, int mem, const ss_queries* qh = nullptr) {
  SS_TRY(require_init());
  SS_TRY(check_mem(mem));
  SS_TRY(check_layout(layout));
  Graph<T>* gp = nullptr;
  SS_TRY(graph_check<T>(h, &gp));
  Graph<T>& g = *gp;
  const DevCsr<T>* xq = &g.Xq;
  CoefTable<T>* qtab = nullptr;
  if (qh) SS_TRY(queries_check<T>(qh, h, &xq, &qtab));
  const int64_t limit = (kind == SS_ROWS_QUERY) ? (qh ? xq->rows : g.nq) : g.ns;
  if (g.general && kind != SS_ROWS_QUERY)
    return fail(SS_EINVAL, "a general graph serves SS_ROWS_QUERY only");
  if (kind == 2) {
    SS_TRY(loo_graph_check(g));  // a general graph was refused above
  } else if (kind != SS_ROWS_QUERY && kind != SS_ROWS_SOURCE) {
    return fail(SS_EINVAL, "rows_kind must be SS_ROWS_QUERY or SS_ROWS_SOURCE");
  }
  if (row_begin < 0 || row_end < row_begin || row_end > limit)
    return fail(SS_EINVAL, "row range [%lld,%lld) outside 0..%lld", (long long)row_begin, (long long)row_end,
                (long long)limit);
  const int64_t nrows = row_end - row_begin;
  const int64_t nt = g.nt;
  if (nrows == 0 || nt == 0) return SS_OK;
  if (!out) return fail(SS_EINVAL, "output buffer is NULL");
  const int64_t need_ld = (layout == SS_LAYOUT_ROWMAJOR) ? nt : nrows;
  if (ld < need_ld) return fail(SS_EINVAL, "leading dimension %lld < %lld", (long long)ld, (long long)need_ld);
  ScoreOut<T> so;
  SS_TRY(so.begin(out, ld, layout, mem, nrows, nt));
  SS_TRY(predict_rows_device<T>(g, *xq, kind, row_begin, row_end, clean, so.dev_rm, so.ld_rm, qtab));
  SS_TRY(so.deliver());
  // Staging buffers are released on return and host results must be complete: wait for the stream.  With the
  // scores written straight into the caller's device buffer there is nothing to release (the transfer block
  // lives in the handle), so the call returns as soon as the work is enqueued -- stream order, like a kernel
  // launch; ss_synchronize() or the caller's own stream synchronisation waits for it.
  if (!so.direct()) SS_HIP(hipStreamSynchronize(ctx().stream));
  return SS_OK;
}

// per-row ranking metrics (rank_rows.hip): argument checks shared by both entry points
static int check_rank_rows_shape(int64_t ncols, int L, double alpha) {
  if (ncols < 2 || ncols >= (1LL << 31) - 1)
    return fail(SS_EINVAL, "rank metrics rows: ncols = %lld outside [2, 2^31 - 1)", (long long)ncols);
  if (L < 1) return fail(SS_EINVAL, "Please use a list length greater than 0 (L > 0)");
  if ((int64_t)L >= ncols) return fail(SS_EINVAL, "Number of labels is less than length (L > y)");
  if (!(alpha > 0.0)) return fail(SS_EINVAL, "rank metrics rows: alpha must be positive");
  return SS_OK;
}

// ------------------------------------------------------------------ what the consumers of score rows share
// Caller-supplied score rows and their labels (CSR, index_base 0 or 1) as the row kernels take them: on the device,
// the row pointers on the host as well.  Host inputs are copied into buffers this owns, the label slice rebased to its
// first entry (row r's labels are didx[dptr[r] - shift .. dptr[r + 1] - shift), still carrying index_base).
template <class T>
struct StagedRows {
  std::vector<int64_t> hp;  // yptr[0 .. nrows]
  const int64_t* dptr = nullptr;
  const int* didx = nullptr;
  const T* dyhat = nullptr;
  int64_t shift = 0, dld = 0, nnz = 0;
  DevBuf<int64_t> bptr;
  DevBuf<int> bidx;
  DevBuf<T> bhat;
};

// Checks yptr on the host, begins the call's timing, stages host inputs and checks the labels on the device (sorted,
// unique, in range; syncs): a consumer writes nothing before this has passed.  what: the call's name in messages.
template <class T>
static int stage_label_rows(const char* what, const int64_t* yptr, const int32_t* yidx, int base, const T* yhat,
                            int64_t nrows, int64_t ncols, int64_t ld, int mem, StagedRows<T>& s) {
  hipStream_t st = ctx().stream;
  std::vector<int64_t>& hp = s.hp;
  hp.resize((size_t)nrows + 1);
  if (mem == SS_MEM_HOST) memcpy(hp.data(), yptr, hp.size() * sizeof(int64_t));
  else {
    SS_HIP(hipMemcpyAsync(hp.data(), yptr, hp.size() * sizeof(int64_t), hipMemcpyDeviceToHost, st));
    SS_HIP(hipStreamSynchronize(st));
  }
  if (hp[0] < base) return fail(SS_EINVAL, "%s: yptr[0] = %lld < index_base", what, (long long)hp[0]);
  for (int64_t r = 0; r < nrows; ++r)
    if (hp[r + 1] < hp[r] || hp[r + 1] - hp[r] > ncols)
      return fail(SS_EINVAL, "%s: row %lld has %lld labels (ncols %lld)", what, (long long)r,
                  (long long)(hp[r + 1] - hp[r]), (long long)ncols);
  s.nnz = hp[nrows] - hp[0];
  if (s.nnz > 0 && !yidx) return fail(SS_EINVAL, "%s: NULL label index buffer", what);
  timing_begin_call();
  s.dptr = yptr;
  s.didx = yidx;
  s.dyhat = yhat;
  s.dld = ld;
  s.shift = base;
  if (mem == SS_MEM_HOST) {
    SS_TRY(s.bptr.alloc((size_t)nrows + 1));
    SS_TRY(s.bidx.alloc((size_t)s.nnz));
    SS_TRY(s.bhat.alloc((size_t)nrows * ncols));
    SS_TRY(upload<int64_t>(s.bptr.p, hp.data(), (size_t)nrows + 1, SS_MEM_HOST));
    SS_TRY(upload<int>(s.bidx.p, yidx + (hp[0] - base), (size_t)s.nnz, SS_MEM_HOST));
    SS_HIP(hipMemcpy2DAsync(s.bhat.p, ncols * sizeof(T), yhat, ld * sizeof(T), ncols * sizeof(T), nrows,
                            hipMemcpyHostToDevice, st));
    s.dptr = s.bptr.p;
    s.didx = s.bidx.p;
    s.dyhat = s.bhat.p;
    s.dld = ncols;
    s.shift = hp[0];
  }
  return launch_rank_rows_validate<int64_t>(s.dptr, s.shift, s.didx, base, nrows, ncols);
}

static int range_check(int64_t i_begin, int64_t i_end, int64_t ns) {
  if (i_begin < 0 || i_end < i_begin || i_end > ns)
    return fail(SS_EINVAL, "row range [%lld,%lld) outside 0..%lld", (long long)i_begin, (long long)i_end,
                (long long)ns);
  return SS_OK;
}

static int check_block_rows(const char* what, int64_t block_rows) {
  if (block_rows < 0) return fail(SS_EINVAL, "%s: block_rows must be >= 0", what);
  return SS_OK;
}

// rows of scores a sweep holds at once: block_rows, or about 1 GiB of scores when that is 0
template <class T>
static int64_t sweep_block_rows(int64_t block_rows, int64_t nrows, int64_t nt) {
  int64_t rb = block_rows;
  if (rb == 0) {
    rb = (1LL << 30) / (nt * (int64_t)sizeof(T));
    if (rb < 1) rb = 1;
  }
  return rb > nrows ? nrows : rb;
}

// What a sweep (loo_blocks, kfold_blocks) hands its consumer per block: nb rows of scores and their labels, the rows of
// the graph's own Ys (checked sorted and unique when the graph was built), as CSR with index base 0: row r's labels are
// idx[ptr[r] - shift .. ptr[r + 1] - shift).
template <class T, class P>
struct SweepBlock {
  const P* ptr;         // device row pointers of the block, nb + 1 of them
  int64_t shift;
  const int* idx;
  int64_t nlab;         // labels in the block
  const P* hptr;        // ptr on the host
  const T* scores;      // row-major nb x nt, leading dimension nt
  int64_t nb, nt;
  int64_t r0;           // position of the block's first row in the sweep
  int64_t row0;         // without ids: row r is source row0 + r
  const int* ids;       // device; row r is source ids[r] (k-fold: the members in fold order)
  const int* out_rows;  // device; ids[r] - i_begin, the row of source order a result of row r belongs in (k-fold)
};

static int no_step() { return SS_OK; }

// The leave-one-out folds [i_begin, i_end) in blocks of rb through a score buffer owned by the call.  begin() runs once
// inside the call's ST_TOTAL span before the first block, each(block) after every block's scores under ST_EPILOGUE,
// finish() after the last block before the span closes; begin and finish time themselves.
template <class T, class Begin, class Each, class Finish>
static int loo_blocks(Graph<T>& g, int64_t i_begin, int64_t i_end, int clean, int64_t rb, Begin begin, Each each,
                      Finish finish) {
  hipStream_t st = ctx().stream;
  const int64_t nrows = i_end - i_begin, nt = g.nt;
  std::vector<int> hp((size_t)nrows + 1);
  SS_HIP(hipMemcpyAsync(hp.data(), g.Ys.ptr.p + i_begin, hp.size() * sizeof(int), hipMemcpyDeviceToHost, st));
  SS_HIP(hipStreamSynchronize(st));
  DevBuf<T> scores;
  SS_TRY(scores.alloc((size_t)rb * nt));
  timing_begin_call();
  hipEvent_t e_begin, e_end;
  SS_TRY(timing_mark(&e_begin));
  SS_TRY(begin());
  for (int64_t r0 = 0; r0 < nrows; r0 += rb) {
    const int64_t nb = nrows - r0 < rb ? nrows - r0 : rb;
    SS_TRY(predict_rows_device<T>(g, g.Xq, 2, i_begin + r0, i_begin + r0 + nb, clean, scores.p, nt));
    StageTimer t3(ST_EPILOGUE);
    SS_TRY(each(SweepBlock<T, int>{g.Ys.ptr.p + i_begin + r0, 0, g.Ys.idx.p, (int64_t)(hp[r0 + nb] - hp[r0]),
                                   hp.data() + r0, scores.p, nb, nt, r0, i_begin + r0, nullptr, nullptr}));
  }
  SS_TRY(finish());
  SS_TRY(timing_mark(&e_end));
  timing_span(ST_TOTAL, e_begin, e_end);
  return SS_OK;
}

template <class T>
static int rank_rows_impl(const int64_t* yptr, const int32_t* yidx, int base, const T* yhat, int64_t nrows,
                          int64_t ncols, int64_t ld, double alpha, int L, double* out, int mem) {
  SS_TRY(require_init());
  SS_TRY(check_mem(mem));
  if (base != 0 && base != 1) return fail(SS_EINVAL, "index_base must be 0 or 1");
  if (nrows < 0) return fail(SS_EINVAL, "rank metrics rows: negative row count");
  if (nrows == 0) return SS_OK;
  SS_TRY(check_rank_rows_shape(ncols, L, alpha));
  if (ld < ncols) return fail(SS_EINVAL, "rank metrics rows: leading dimension %lld < %lld", (long long)ld, (long long)ncols);
  if (!yptr || !yhat || !out) return fail(SS_EINVAL, "rank metrics rows: NULL buffer");
  hipStream_t st = ctx().stream;
  StagedRows<T> s;
  SS_TRY(stage_label_rows("rank metrics rows", yptr, yidx, base, yhat, nrows, ncols, ld, mem, s));
  double* dout = out;
  DevBuf<double> bout;
  if (mem == SS_MEM_HOST) {
    SS_TRY(bout.alloc((size_t)nrows * 6));
    dout = bout.p;
  }
  hipEvent_t e_begin, e_end;
  SS_TRY(timing_mark(&e_begin));
  SS_TRY((launch_rank_rows<T, int64_t>(s.dptr, s.shift, s.didx, base, s.hp.data(), s.dyhat, nrows, ncols, s.dld, alpha,
                                       L, dout)));
  SS_TRY(timing_mark(&e_end));
  timing_span(ST_TOTAL, e_begin, e_end);
  if (mem == SS_MEM_HOST)
    SS_HIP(hipMemcpyAsync(out, bout.p, (size_t)nrows * 6 * sizeof(double), hipMemcpyDeviceToHost, st));
  SS_HIP(hipStreamSynchronize(st));
  return SS_OK;
}

// leave-one-out folds evaluated where they are produced
template <class T>
static int evaluate_loo_impl(ss_graph* h, int64_t i_begin, int64_t i_end, int clean, double alpha, int L,
                             int64_t block_rows, double* out, int mem) {
  SS_TRY(require_init());
  SS_TRY(check_mem(mem));
  Graph<T>* gp = nullptr;
  SS_TRY(graph_check<T>(h, &gp));
  Graph<T>& g = *gp;
  SS_TRY(loo_graph_check(g));
  SS_TRY(range_check(i_begin, i_end, g.ns));
  SS_TRY(check_block_rows("evaluate_loo", block_rows));
  const int64_t nrows = i_end - i_begin, nt = g.nt;
  if (nrows == 0) return SS_OK;
  SS_TRY(check_rank_rows_shape(nt, L, alpha));
  if (!out) return fail(SS_EINVAL, "output buffer is NULL");
  hipStream_t st = ctx().stream;
  double* dout = out;
  DevBuf<double> bout;
  if (mem == SS_MEM_HOST) {
    SS_TRY(bout.alloc((size_t)nrows * 6));
    dout = bout.p;
  }
  SS_TRY(loo_blocks<T>(g, i_begin, i_end, clean, sweep_block_rows<T>(block_rows, nrows, nt), no_step,
                       [&](const SweepBlock<T, int>& k) {
                         return launch_rank_rows<T, int>(k.ptr, k.shift, k.idx, 0, k.hptr, k.scores, k.nb, nt, nt, alpha,
                                                         L, dout + k.r0 * 6);
                       },
                       no_step));
  if (mem == SS_MEM_HOST)
    SS_HIP(hipMemcpyAsync(out, bout.p, (size_t)nrows * 6 * sizeof(double), hipMemcpyDeviceToHost, st));
  SS_HIP(hipStreamSynchronize(st));
  return SS_OK;
}

// per-row binary prediction metrics (binary_rows.hip): 18 doubles per row
static int check_binary_rows_shape(int64_t ncols) {
  if (ncols < 1 || ncols >= (1LL << 31))
    return fail(SS_EINVAL, "binary metrics rows: ncols = %lld outside [1, 2^31)", (long long)ncols);
  return SS_OK;
}

template <class T>
static int binary_rows_impl(const int64_t* yptr, const int32_t* yidx, int base, const T* yhat, int64_t nrows,
                            int64_t ncols, int64_t ld, double* out, int mem) {
  SS_TRY(require_init());
  SS_TRY(check_mem(mem));
  if (base != 0 && base != 1) return fail(SS_EINVAL, "index_base must be 0 or 1");
  if (nrows < 0) return fail(SS_EINVAL, "binary metrics rows: negative row count");
  if (nrows == 0) return SS_OK;
  SS_TRY(check_binary_rows_shape(ncols));
  if (ld < ncols)
    return fail(SS_EINVAL, "binary metrics rows: leading dimension %lld < %lld", (long long)ld, (long long)ncols);
  if (!yptr || !yhat || !out) return fail(SS_EINVAL, "binary metrics rows: NULL buffer");
  hipStream_t st = ctx().stream;
  StagedRows<T> s;
  SS_TRY(stage_label_rows("binary metrics rows", yptr, yidx, base, yhat, nrows, ncols, ld, mem, s));
  double* dout = out;
  DevBuf<double> bout;
  if (mem == SS_MEM_HOST) {
    SS_TRY(bout.alloc((size_t)nrows * 18));
    dout = bout.p;
  }
  hipEvent_t e_begin, e_end;
  SS_TRY(timing_mark(&e_begin));
  SS_TRY((launch_binary_rows<T, int64_t>(s.dptr, s.shift, s.didx, base, s.dyhat, nrows, ncols, s.dld, dout)));
  SS_TRY(timing_mark(&e_end));
  timing_span(ST_TOTAL, e_begin, e_end);
  if (mem == SS_MEM_HOST)
    SS_HIP(hipMemcpyAsync(out, bout.p, (size_t)nrows * 18 * sizeof(double), hipMemcpyDeviceToHost, st));
  SS_HIP(hipStreamSynchronize(st));
  return SS_OK;
}

// leave-one-out folds judged by the binary metrics where they are produced
template <class T>
static int evaluate_loo_binary_impl(ss_graph* h, int64_t i_begin, int64_t i_end, int clean, int64_t block_rows,
                                    double* out, int mem) {
  SS_TRY(require_init());
  SS_TRY(check_mem(mem));
  Graph<T>* gp = nullptr;
  SS_TRY(graph_check<T>(h, &gp));
  Graph<T>& g = *gp;
  SS_TRY(loo_graph_check(g));
  SS_TRY(range_check(i_begin, i_end, g.ns));
  SS_TRY(check_block_rows("evaluate_loo_binary", block_rows));
  const int64_t nrows = i_end - i_begin, nt = g.nt;
  if (nrows == 0) return SS_OK;
  SS_TRY(check_binary_rows_shape(nt));
  if (!out) return fail(SS_EINVAL, "output buffer is NULL");
  hipStream_t st = ctx().stream;
  double* dout = out;
  DevBuf<double> bout;
  if (mem == SS_MEM_HOST) {
    SS_TRY(bout.alloc((size_t)nrows * 18));
    dout = bout.p;
  }
  SS_TRY(loo_blocks<T>(g, i_begin, i_end, clean, sweep_block_rows<T>(block_rows, nrows, nt), no_step,
                       [&](const SweepBlock<T, int>& k) {
                         return launch_binary_rows<T, int>(k.ptr, k.shift, k.idx, 0, k.scores, k.nb, nt, nt,
                                                           dout + k.r0 * 18);
                       },
                       no_step));
  if (mem == SS_MEM_HOST)
    SS_HIP(hipMemcpyAsync(out, bout.p, (size_t)nrows * 18 * sizeof(double), hipMemcpyDeviceToHost, st));
  SS_HIP(hipStreamSynchronize(st));
  return SS_OK;
}

// device side of a k-fold call: the assignment, the selected members, their output rows and one fold's degrees
template <class T>
struct KfoldWork {
  DevBuf<int> d_fold, d_order, d_sel, d_map, kf, ks, kt;
  DevBuf<T> inv_kf, inv_ks;
  int cur_seg = -1;  // segment whose degrees kf / ks / kt / inv_* hold
};

// the part every k-fold call needs: fold[i] of each source, the sources in fold order, room for one fold's degrees
template <class T>
static int kfold_work_folds(const Graph<T>& g, const int32_t* fold, const int* order, KfoldWork<T>& w) {
  hipStream_t st = ctx().stream;
  const int64_t ns = g.ns;
  SS_TRY(w.d_fold.alloc(ns)); SS_TRY(w.d_order.alloc(ns));
  SS_TRY(w.kf.alloc(g.nf)); SS_TRY(w.ks.alloc(ns)); SS_TRY(w.kt.alloc(g.nt));
  SS_TRY(w.inv_kf.alloc(g.nf)); SS_TRY(w.inv_ks.alloc(ns));
  SS_HIP(hipMemcpyAsync(w.d_fold.p, fold, ns * sizeof(int), hipMemcpyHostToDevice, st));
  SS_HIP(hipMemcpyAsync(w.d_order.p, order, ns * sizeof(int), hipMemcpyHostToDevice, st));
  w.cur_seg = -1;
  return SS_OK;
}

// Degrees of the graph without fold fold_id, whose n members are members[]: w.kf / ks / kt recounted from the graph's
// own, and the reciprocals stage 1 multiplies by (0 on the members' own feature columns and for the members as sources).
template <class T>
static int fold_degrees(const Graph<T>& g, KfoldWork<T>& w, const int* members, int64_t n, int fold_id) {
  hipStream_t st = ctx().stream;
  SS_HIP(hipMemcpyAsync(w.kf.p, g.kf.p, g.nf * sizeof(int), hipMemcpyDeviceToDevice, st));
  SS_HIP(hipMemcpyAsync(w.ks.p, g.ks.p, g.ns * sizeof(int), hipMemcpyDeviceToDevice, st));
  SS_HIP(hipMemcpyAsync(w.kt.p, g.kt.p, g.nt * sizeof(int), hipMemcpyDeviceToDevice, st));
  if (g.dense.on) SS_TRY(dense_fold_degrees<T>(g, members, n, w.kf.p, w.ks.p, w.kt.p));
  else SS_TRY(launch_fold_degrees<T>(g.Xs, g.XsT, g.Ys, members, n, w.kf.p, w.ks.p, w.kt.p));
  return launch_fold_inverse<T>(w.kf.p, w.ks.p, w.d_fold.p, fold_id, g.nf, g.ns, w.inv_kf.p, w.inv_ks.p);
}

// stage 1 of a fold's members [r0, r0 + nb) into the transfer block g.Tws, with the fold's degrees in w
template <class T>
static int kfold_transfer(Graph<T>& g, KfoldWork<T>& w, const int* members, int64_t r0, int64_t nb) {
  StageTimer t1(ST_TRANSFER);
  const int64_t ns = g.ns;
  if (g.dense.on) {
    // members' rows gathered into the query planes
    SS_TRY(dense_transfer<T>(g, false, w.inv_kf.p, w.inv_ks.p, nullptr, r0, nb, g.Tws.p, ns, false, members));
  } else {
    const DevCsr<T>* L[2] = {&g.Xs, nullptr};
    const DevChunked<T>* M[2] = {&g.XsTc, nullptr};
    const T* inv1[2] = {w.inv_kf.p, nullptr};
    SS_TRY(launch_transfer<T>(1, L, inv1, M, w.inv_ks.p, r0, nb, ns, g.Tws.p, ns, members));
  }
  timing_count(ST_NTRANSFER, 1);
  return SS_OK;
}

// k-fold: all folds of construct(y, X, members) + predict (+ clean!) from the resident graph
template <class T>
static int predict_kfold_impl(ss_graph* h, const int32_t* fold_of_source, int nfolds, int clean, T* out, int64_t ld,
                              int layout, int mem) {
  SS_TRY(require_init());
  SS_TRY(check_mem(mem));
  SS_TRY(check_layout(layout));
  Graph<T>* gp = nullptr;
  SS_TRY(graph_check<T>(h, &gp));
  Graph<T>& g = *gp;
  if (g.general || (!g.dense.on && g.nq != 0) || g.ns != g.nf)
    return fail(SS_EINVAL, "k-fold needs a graph with nq == 0 and ns == nf (feature j named after source j)");
  if (nfolds < 1 || !fold_of_source) return fail(SS_EINVAL, "k-fold: bad fold assignment");
  const int64_t ns = g.ns, nt = g.nt;
  if (ns == 0 || nt == 0) return SS_OK;
  if (!out) return fail(SS_EINVAL, "output buffer is NULL");
  const int64_t need_ld = (layout == SS_LAYOUT_ROWMAJOR) ? nt : ns;
  if (ld < need_ld) return fail(SS_EINVAL, "leading dimension %lld < %lld", (long long)ld, (long long)need_ld);
  hipStream_t st = ctx().stream;
  // members of each fold, in source order (stable counting sort on the host)
  std::vector<int32_t> fold(ns);
  if (mem == SS_MEM_HOST) memcpy(fold.data(), fold_of_source, ns * sizeof(int32_t));
  else SS_HIP(hipMemcpy(fold.data(), fold_of_source, ns * sizeof(int32_t), hipMemcpyDeviceToHost));
  std::vector<int> start(nfolds + 1, 0), order(ns);
  for (int64_t i = 0; i < ns; ++i) {
    if (fold[i] < 0 || fold[i] >= nfolds) return fail(SS_EINVAL, "fold_of_source[%lld] = %d outside 0..%d", (long long)i, fold[i], nfolds - 1);
    start[fold[i] + 1]++;
  }
  for (int f = 0; f < nfolds; ++f) start[f + 1] += start[f];
  {
    std::vector<int> cur(start.begin(), start.end() - 1);
    for (int64_t i = 0; i < ns; ++i) order[cur[fold[i]]++] = (int)i;
  }
  KfoldWork<T> w;
  SS_TRY(kfold_work_folds<T>(g, fold.data(), order.data(), w));
  SS_TRY(graph_sell(g));
  SS_TRY(graph_chunked(g, false));

  ScoreOut<T> so;
  SS_TRY(so.begin(out, ld, layout, mem, ns, nt));
  for (int phi = 0; phi < nfolds; ++phi) {
    const int64_t nm = start[phi + 1] - start[phi];
    if (nm == 0) continue;
    const int* members = w.d_order.p + start[phi];
    SS_TRY(fold_degrees<T>(g, w, members, nm, phi));
    const int64_t rb = transfer_batch_rows(nm, ns, sizeof(T));
    const size_t need = (size_t)rb * (size_t)ns;
    if (g.Tws.n < need) SS_TRY(g.Tws.alloc(need));
    for (int64_t r0 = 0; r0 < nm; r0 += rb) {
      const int64_t nb = (nm - r0 < rb) ? (nm - r0) : rb;
      SS_TRY(kfold_transfer<T>(g, w, members, r0, nb));
      // a member's scores go to its source row: on a length-sorted operand by row copies addressed from order[]
      SS_TRY(stage2_rows<T>(g, rb, nb, clean ? w.kt.p : nullptr,
                            ScoreDest<T>{so.dev_rm, so.ld_rm, start[phi] + r0, w.d_order.p, order.data()}));
    }
  }
  SS_TRY(so.deliver());
  SS_HIP(hipStreamSynchronize(st));
  return SS_OK;
}

// ------------------------------------------------------------------ k-fold row blocks
// A fold assignment checked whole (a fold's degrees depend on all of its members, wherever the asked rows lie).  The
// folds that have members are segments of `order` (sources by fold, source order inside a fold): segment s holds fold
// seg_fold[s], members order[seg_start[s] .. seg_start[s + 1]).  Folds without members have no segment.
struct KfoldPlan {
  std::vector<int32_t> fold;
  std::vector<int> order, seg_fold, seg_start;
};

static int kfold_plan(const int32_t* fold_of_source, int nfolds, int64_t ns, int mem, KfoldPlan& p) {
  if (nfolds < 1) return fail(SS_EINVAL, "k-fold: nfolds = %d, must be >= 1", nfolds);
  if (!fold_of_source) return fail(SS_EINVAL, "k-fold: fold_of_source is NULL");
  p.fold.resize((size_t)ns);
  if (ns > 0) {
    if (mem == SS_MEM_HOST) memcpy(p.fold.data(), fold_of_source, (size_t)ns * sizeof(int32_t));
    else {
      hipStream_t st = ctx().stream;
      SS_HIP(hipMemcpyAsync(p.fold.data(), fold_of_source, (size_t)ns * sizeof(int32_t), hipMemcpyDeviceToHost, st));
      SS_HIP(hipStreamSynchronize(st));
    }
  }
  for (int64_t i = 0; i < ns; ++i)
    if (p.fold[i] < 0 || p.fold[i] >= nfolds)
      return fail(SS_EINVAL, "fold_of_source[%lld] = %d outside 0..%d", (long long)i, p.fold[i], nfolds - 1);
  p.order.resize((size_t)ns);
  for (int64_t i = 0; i < ns; ++i) p.order[i] = (int)i;
  std::stable_sort(p.order.begin(), p.order.end(), [&](int a, int b) { return p.fold[a] < p.fold[b]; });
  p.seg_fold.clear();
  p.seg_start.clear();
  for (int64_t x = 0; x < ns; ++x)
    if (x == 0 || p.fold[p.order[x]] != p.fold[p.order[x - 1]]) {
      p.seg_fold.push_back(p.fold[p.order[x]]);
      p.seg_start.push_back((int)x);
    }
  p.seg_start.push_back((int)ns);
  return SS_OK;
}

// The sources [i_begin, i_end) in fold order: piece k is sel[pos[k] .. pos[k + 1]), the in-range members of segment
// seg[k] of the plan.
struct KfoldRange {
  std::vector<int> sel, seg;
  std::vector<int64_t> pos;
};

static void kfold_range(const KfoldPlan& p, int64_t i_begin, int64_t i_end, KfoldRange& r) {
  r.sel.clear();
  r.seg.clear();
  r.pos.assign(1, 0);
  for (size_t s = 0; s + 1 < p.seg_start.size(); ++s) {
    const auto b = p.order.begin() + p.seg_start[s], e = p.order.begin() + p.seg_start[s + 1];
    const auto lo = std::lower_bound(b, e, (int)i_begin), hi = std::lower_bound(b, e, (int)i_end);
    if (lo == hi) continue;
    r.sel.insert(r.sel.end(), lo, hi);
    r.seg.push_back((int)s);
    r.pos.push_back((int64_t)r.sel.size());
  }
}

// map[p]: output row of the p-th selected member (its source row relative to i_begin)
template <class T>
static int kfold_work_init(const Graph<T>& g, const KfoldPlan& p, const KfoldRange& r, const std::vector<int>& map,
                           KfoldWork<T>& w) {
  hipStream_t st = ctx().stream;
  SS_TRY(kfold_work_folds<T>(g, p.fold.data(), p.order.data(), w));
  SS_TRY(w.d_sel.alloc(r.sel.size())); SS_TRY(w.d_map.alloc(map.size()));
  if (!r.sel.empty())
    SS_HIP(hipMemcpyAsync(w.d_sel.p, r.sel.data(), r.sel.size() * sizeof(int), hipMemcpyHostToDevice, st));
  if (!map.empty()) SS_HIP(hipMemcpyAsync(w.d_map.p, map.data(), map.size() * sizeof(int), hipMemcpyHostToDevice, st));
  return SS_OK;
}

// Scores of the selected members at positions [p0, p1) (fold order), the same kernels and fold set-up as
// predict_kfold_impl: per fold the degrees are recounted once over all of its members, then its selected members go
// through stage 1 (gathered by member id) and stage 2 in batches bounded by transfer_batch_rows.  Position p goes to
// row row_map[p - p0] of dst, or to row p - p0 when row_map is NULL.
template <class T>
static int kfold_rows_device(Graph<T>& g, KfoldWork<T>& w, const KfoldPlan& plan, const KfoldRange& rg, int64_t p0,
                             int64_t p1, int clean, T* dst, int64_t ld, const int* row_map) {
  const int64_t ns = g.ns;
  for (size_t k = 0; k < rg.seg.size(); ++k) {
    const int64_t a = rg.pos[k] > p0 ? rg.pos[k] : p0, b = rg.pos[k + 1] < p1 ? rg.pos[k + 1] : p1;
    if (a >= b) continue;
    const int s = rg.seg[k];
    if (w.cur_seg != s) {
      SS_TRY(fold_degrees<T>(g, w, w.d_order.p + plan.seg_start[s], plan.seg_start[s + 1] - plan.seg_start[s],
                             plan.seg_fold[s]));
      w.cur_seg = s;
    }
    const int* members = w.d_sel.p + a;
    const int64_t nm = b - a;
    const int64_t rb = transfer_batch_rows(nm, ns, sizeof(T));
    const size_t need = (size_t)rb * (size_t)ns;
    if (g.Tws.n < need) SS_TRY(g.Tws.alloc(need));
    for (int64_t r0 = 0; r0 < nm; r0 += rb) {
      const int64_t nb = (nm - r0 < rb) ? (nm - r0) : rb;
      SS_TRY(kfold_transfer<T>(g, w, members, r0, nb));
      // a - p0 + r0: block row of the batch's first member
      SS_TRY(stage2_rows<T>(g, rb, nb, clean ? w.kt.p : nullptr, ScoreDest<T>{dst, ld, a - p0 + r0, row_map, nullptr}));
    }
  }
  return SS_OK;
}

template <class T>
static int kfold_graph_check(const Graph<T>& g) {
  if (g.general || (!g.dense.on && g.nq != 0) || g.ns != g.nf)
    return fail(SS_EINVAL, "k-fold needs a graph with nq == 0 and ns == nf (feature j named after source j)");
  return SS_OK;
}

// The k-fold rows [i_begin, i_end) in blocks of rb positions in fold order, with no row map (each block is contiguous),
// through a score buffer owned by the call; a block's labels are its members' Ys rows gathered in the same order.
// begin / each / finish as for loo_blocks.
template <class T, class Begin, class Each, class Finish>
static int kfold_blocks(Graph<T>& g, const KfoldPlan& plan, int64_t i_begin, int64_t i_end, int clean, int64_t rb,
                        Begin begin, Each each, Finish finish) {
  hipStream_t st = ctx().stream;
  const int64_t nrows = i_end - i_begin, nt = g.nt;
  KfoldRange rg;
  kfold_range(plan, i_begin, i_end, rg);
  std::vector<int> map(rg.sel.size());
  for (size_t p = 0; p < map.size(); ++p) map[p] = (int)(rg.sel[p] - i_begin);
  KfoldWork<T> w;
  SS_TRY(kfold_work_init<T>(g, plan, rg, map, w));
  // pptr = the int64 row pointers of the members' Ys rows over the whole range
  std::vector<int> hy((size_t)nrows + 1);
  SS_HIP(hipMemcpyAsync(hy.data(), g.Ys.ptr.p + i_begin, hy.size() * sizeof(int), hipMemcpyDeviceToHost, st));
  SS_HIP(hipStreamSynchronize(st));
  std::vector<int64_t> pptr((size_t)nrows + 1, 0);
  for (int64_t p = 0; p < nrows; ++p) pptr[p + 1] = pptr[p] + (hy[map[p] + 1] - hy[map[p]]);
  int64_t max_lab = 1;
  for (int64_t p0 = 0; p0 < nrows; p0 += rb) {
    const int64_t p1 = nrows - p0 < rb ? nrows : p0 + rb;
    if (pptr[p1] - pptr[p0] > max_lab) max_lab = pptr[p1] - pptr[p0];
  }
  DevBuf<int64_t> d_pptr;
  DevBuf<int> lab;
  DevBuf<T> scores;
  SS_TRY(d_pptr.alloc((size_t)nrows + 1));
  SS_TRY(lab.alloc((size_t)max_lab));
  SS_TRY(scores.alloc((size_t)rb * nt));
  SS_HIP(hipMemcpyAsync(d_pptr.p, pptr.data(), pptr.size() * sizeof(int64_t), hipMemcpyHostToDevice, st));
  SS_TRY(graph_sell(g));
  SS_TRY(graph_chunked(g, false));
  timing_begin_call();
  hipEvent_t e_begin, e_end;
  SS_TRY(timing_mark(&e_begin));
  SS_TRY(begin());
  for (int64_t p0 = 0; p0 < nrows; p0 += rb) {
    const int64_t nb = nrows - p0 < rb ? nrows - p0 : rb;
    SS_TRY(kfold_rows_device<T>(g, w, plan, rg, p0, p0 + nb, clean, scores.p, nt, nullptr));
    StageTimer t3(ST_EPILOGUE);
    SS_TRY(launch_gather_labels(g.Ys.ptr.p, g.Ys.idx.p, w.d_sel.p + p0, nb, d_pptr.p + p0, pptr[p0], lab.p));
    SS_TRY(each(SweepBlock<T, int64_t>{d_pptr.p + p0, pptr[p0], lab.p, pptr[p0 + nb] - pptr[p0], pptr.data() + p0,
                                       scores.p, nb, nt, p0, 0, w.d_sel.p + p0, w.d_map.p + p0}));
  }
  SS_TRY(finish());
  SS_TRY(timing_mark(&e_end));
  timing_span(ST_TOTAL, e_begin, e_end);
  return SS_OK;
}

// rows [i_begin, i_end) (source order) of predict_kfold_impl
template <class T>
static int predict_kfold_rows_impl(ss_graph* h, const int32_t* fold_of_source, int nfolds, int64_t i_begin,
                                   int64_t i_end, int clean, T* out, int64_t ld, int layout, int mem) {
  SS_TRY(require_init());
  SS_TRY(check_mem(mem));
  SS_TRY(check_layout(layout));
  Graph<T>* gp = nullptr;
  SS_TRY(graph_check<T>(h, &gp));
  Graph<T>& g = *gp;
  SS_TRY(kfold_graph_check(g));
  SS_TRY(range_check(i_begin, i_end, g.ns));
  KfoldPlan plan;
  SS_TRY(kfold_plan(fold_of_source, nfolds, g.ns, mem, plan));
  const int64_t nrows = i_end - i_begin, nt = g.nt;
  if (nrows == 0 || nt == 0) return SS_OK;
  if (!out) return fail(SS_EINVAL, "output buffer is NULL");
  const int64_t need_ld = (layout == SS_LAYOUT_ROWMAJOR) ? nt : nrows;
  if (ld < need_ld) return fail(SS_EINVAL, "leading dimension %lld < %lld", (long long)ld, (long long)need_ld);
  KfoldRange rg;
  kfold_range(plan, i_begin, i_end, rg);
  std::vector<int> map(rg.sel.size());
  for (size_t p = 0; p < map.size(); ++p) map[p] = (int)(rg.sel[p] - i_begin);
  KfoldWork<T> w;
  SS_TRY(kfold_work_init<T>(g, plan, rg, map, w));
  SS_TRY(graph_sell(g));
  SS_TRY(graph_chunked(g, false));

  ScoreOut<T> so;
  SS_TRY(so.begin(out, ld, layout, mem, nrows, nt));
  SS_TRY(kfold_rows_device<T>(g, w, plan, rg, 0, nrows, clean, so.dev_rm, so.ld_rm, w.d_map.p));
  SS_TRY(so.deliver());
  // the member lists and degree buffers of the call are released on return
  SS_HIP(hipStreamSynchronize(ctx().stream));
  return SS_OK;
}

// k-fold rows [i_begin, i_end) judged where they are produced; a block's metric rows are scattered to source order.
// binary: 18 doubles per row (launch_binary_rows), else 6 (launch_rank_rows).
template <class T>
static int evaluate_kfold_impl(ss_graph* h, const int32_t* fold_of_source, int nfolds, int64_t i_begin, int64_t i_end,
                               int clean, bool binary, double alpha, int L, int64_t block_rows, double* out, int mem) {
  SS_TRY(require_init());
  SS_TRY(check_mem(mem));
  Graph<T>* gp = nullptr;
  SS_TRY(graph_check<T>(h, &gp));
  Graph<T>& g = *gp;
  SS_TRY(kfold_graph_check(g));
  SS_TRY(range_check(i_begin, i_end, g.ns));
  SS_TRY(check_block_rows(binary ? "evaluate_kfold_binary" : "evaluate_kfold", block_rows));
  KfoldPlan plan;
  SS_TRY(kfold_plan(fold_of_source, nfolds, g.ns, mem, plan));
  const int64_t nrows = i_end - i_begin, nt = g.nt;
  if (nrows == 0) return SS_OK;
  SS_TRY(binary ? check_binary_rows_shape(nt) : check_rank_rows_shape(nt, L, alpha));
  if (!out) return fail(SS_EINVAL, "output buffer is NULL");
  const int nw = binary ? 18 : 6;
  hipStream_t st = ctx().stream;
  const int64_t rb = sweep_block_rows<T>(block_rows, nrows, nt);
  DevBuf<double> bres, bout;
  SS_TRY(bres.alloc((size_t)rb * nw));
  double* dout = out;
  if (mem == SS_MEM_HOST) {
    SS_TRY(bout.alloc((size_t)nrows * nw));
    dout = bout.p;
  }
  SS_TRY(kfold_blocks<T>(g, plan, i_begin, i_end, clean, rb, no_step,
                         [&](const SweepBlock<T, int64_t>& k) {
                           if (binary)
                             SS_TRY((launch_binary_rows<T, int64_t>(k.ptr, k.shift, k.idx, 0, k.scores, k.nb, nt, nt,
                                                                    bres.p)));
                           else
                             SS_TRY((launch_rank_rows<T, int64_t>(k.ptr, k.shift, k.idx, 0, k.hptr, k.scores, k.nb, nt,
                                                                  nt, alpha, L, bres.p)));
                           return launch_scatter_rows<double>(bres.p, nw, k.nb, nw, k.out_rows, dout, nw);
                         },
                         no_step));
  if (mem == SS_MEM_HOST)
    SS_HIP(hipMemcpyAsync(out, bout.p, (size_t)nrows * nw * sizeof(double), hipMemcpyDeviceToHost, st));
  SS_HIP(hipStreamSynchronize(st));
  return SS_OK;
}

// ------------------------------------------------------------------ pooled tables (pooled.hip)
// A pool handle: the levels of its table, its pair counts and the scratch reused across adds.  An add builds its table
// (and merges it into copies of the levels) before anything of the pool changes: on any error the pool is as it was.
constexpr uint32_t SS_POOL_MAGIC = 0x4c4f4f50u;
template <class T>
struct PoolBox : HandleHead {
  uint32_t magic = SS_POOL_MAGIC;
  std::vector<PoolTable<pool_key_t<T>>> lv;
  int64_t n = 0, npos = 0, max_entries = 0;
  PoolWork<pool_key_t<T>> w;
};

static int pool_dtype(const void* h, int* dtype) {
  if (!h) return fail(SS_EINVAL, "pool handle is NULL");
  const PoolBox<float>* b = reinterpret_cast<const PoolBox<float>*>(h);  // the head and the tag lie alike in both
  if (b->magic != SS_POOL_MAGIC || (b->dtype != 4 && b->dtype != 8)) return fail(SS_EINVAL, "not a pool handle");
  *dtype = b->dtype;
  return SS_OK;
}

template <class T>
static int pool_check(const void* h, PoolBox<T>** out) {
  int dt = 0;
  SS_TRY(pool_dtype(h, &dt));
  if (dt != (int)sizeof(T)) return fail(SS_EINVAL, "pool handle was created with the other precision");
  *out = const_cast<PoolBox<T>*>(reinterpret_cast<const PoolBox<T>*>(h));
  return SS_OK;
}

template <class T>
static int pool_create_impl(int64_t max_entries, ss_pool** out) {
  SS_TRY(require_init());
  if (!out) return fail(SS_EINVAL, "out handle pointer is NULL");
  *out = nullptr;
  if (max_entries < 0) return fail(SS_EINVAL, "pool: max_entries = %lld < 0", (long long)max_entries);
  if (max_entries == 0) {  // half the free device memory, each entry counted twice (a merge's double buffer)
    size_t fr = 0, tot = 0;
    SS_HIP(hipMemGetInfo(&fr, &tot));
    max_entries = (int64_t)(fr / 2 / (2 * (sizeof(pool_key_t<T>) + 2 * sizeof(int64_t))));
    if (max_entries < 1) max_entries = 1;
  }
  PoolBox<T>* box = new (std::nothrow) PoolBox<T>();
  if (!box) return fail(SS_ENOMEM, "host allocation failed");
  box->dtype = (int)sizeof(T);
  box->max_entries = max_entries;
  *out = reinterpret_cast<ss_pool*>(box);
  return SS_OK;
}

// one finished add (its levels) into the pool, all or nothing
template <class T>
static int pool_commit(PoolBox<T>& p, std::vector<PoolTable<pool_key_t<T>>>& loc, int64_t n, int64_t npos) {
  SS_TRY(pool_consolidate(loc, p.w));
  if (!loc.empty()) SS_TRY(pool_push(p.lv, std::move(loc[0]), 0, p.max_entries, p.w));
  p.n += n;
  p.npos += npos;
  return SS_OK;
}

template <class T>
static int pool_add_rows_impl(ss_pool* h, const int64_t* yptr, const int32_t* yidx, int base, const T* yhat,
                              int64_t nrows, int64_t ncols, int64_t ld, int mem) {
  SS_TRY(require_init());
  SS_TRY(check_mem(mem));
  PoolBox<T>* pp = nullptr;
  SS_TRY(pool_check<T>(h, &pp));
  PoolBox<T>& p = *pp;
  if (base != 0 && base != 1) return fail(SS_EINVAL, "index_base must be 0 or 1");
  if (nrows < 0) return fail(SS_EINVAL, "pool add rows: negative row count");
  if (nrows == 0) return SS_OK;
  SS_TRY(check_binary_rows_shape(ncols));
  if (nrows > ((int64_t)1 << 62) / ncols) return fail(SS_EINVAL, "pool add rows: nrows x ncols overflows");
  if (ld < ncols)
    return fail(SS_EINVAL, "pool add rows: leading dimension %lld < %lld", (long long)ld, (long long)ncols);
  if (!yptr || !yhat) return fail(SS_EINVAL, "pool add rows: NULL buffer");
  StagedRows<T> s;
  SS_TRY(stage_label_rows("pool add rows", yptr, yidx, base, yhat, nrows, ncols, ld, mem, s));
  hipEvent_t e_begin, e_end;
  SS_TRY(timing_mark(&e_begin));
  PoolTable<pool_key_t<T>> t;
  SS_TRY((pool_block_table<T, int64_t>(s.dptr, s.shift, s.didx, base, s.nnz, s.dyhat, nrows, ncols, s.dld, p.w, t)));
  SS_TRY(pool_push(p.lv, std::move(t), 0, p.max_entries, p.w));
  p.n += nrows * ncols;
  p.npos += s.nnz;
  SS_TRY(timing_mark(&e_end));
  timing_span(ST_TOTAL, e_begin, e_end);
  timing_span(ST_EPILOGUE, e_begin, e_end);
  SS_HIP(hipStreamSynchronize(ctx().stream));
  return SS_OK;
}

// A sweep into a pool: every block's table goes onto the add's own levels (the rows' order does not matter to a pool),
// which pool_commit puts into the pool after the last block.
template <class T>
struct PoolAdd {
  PoolBox<T>& p;
  std::vector<PoolTable<pool_key_t<T>>> loc;
  int64_t other, n = 0, npos = 0;
  explicit PoolAdd(PoolBox<T>& pool) : p(pool), other(pool_stored(pool.lv)) {}
  template <class P>
  int block(const SweepBlock<T, P>& k) {
    PoolTable<pool_key_t<T>> t;
    SS_TRY((pool_block_table<T, P>(k.ptr, k.shift, k.idx, 0, k.nlab, k.scores, k.nb, k.nt, k.nt, p.w, t)));
    SS_TRY(pool_push(loc, std::move(t), other, p.max_entries, p.w));
    n += k.nb * k.nt;
    npos += k.nlab;
    return SS_OK;
  }
  int commit() {
    StageTimer t3(ST_EPILOGUE);
    return pool_commit(p, loc, n, npos);
  }
};

// leave-one-out folds pooled where they are produced
template <class T>
static int pool_add_loo_impl(ss_pool* ph, ss_graph* h, int64_t i_begin, int64_t i_end, int clean, int64_t block_rows) {
  SS_TRY(require_init());
  PoolBox<T>* pp = nullptr;
  SS_TRY(pool_check<T>(ph, &pp));
  Graph<T>* gp = nullptr;
  SS_TRY(graph_check<T>(h, &gp));
  Graph<T>& g = *gp;
  SS_TRY(loo_graph_check(g));
  SS_TRY(range_check(i_begin, i_end, g.ns));
  SS_TRY(check_block_rows("pool add loo", block_rows));
  const int64_t nrows = i_end - i_begin, nt = g.nt;
  if (nrows == 0) return SS_OK;
  SS_TRY(check_binary_rows_shape(nt));
  PoolAdd<T> add(*pp);
  SS_TRY(loo_blocks<T>(g, i_begin, i_end, clean, sweep_block_rows<T>(block_rows, nrows, nt), no_step,
                       [&](const SweepBlock<T, int>& k) { return add.block(k); }, [&] { return add.commit(); }));
  SS_HIP(hipStreamSynchronize(ctx().stream));
  return SS_OK;
}

// k-fold rows pooled where they are produced
template <class T>
static int pool_add_kfold_impl(ss_pool* ph, ss_graph* h, const int32_t* fold_of_source, int nfolds, int64_t i_begin,
                               int64_t i_end, int clean, int64_t block_rows, int mem) {
  SS_TRY(require_init());
  SS_TRY(check_mem(mem));
  PoolBox<T>* pp = nullptr;
  SS_TRY(pool_check<T>(ph, &pp));
  Graph<T>* gp = nullptr;
  SS_TRY(graph_check<T>(h, &gp));
  Graph<T>& g = *gp;
  SS_TRY(kfold_graph_check(g));
  SS_TRY(range_check(i_begin, i_end, g.ns));
  SS_TRY(check_block_rows("pool add kfold", block_rows));
  KfoldPlan plan;
  SS_TRY(kfold_plan(fold_of_source, nfolds, g.ns, mem, plan));
  const int64_t nrows = i_end - i_begin, nt = g.nt;
  if (nrows == 0) return SS_OK;
  SS_TRY(check_binary_rows_shape(nt));
  PoolAdd<T> add(*pp);
  SS_TRY(kfold_blocks<T>(g, plan, i_begin, i_end, clean, sweep_block_rows<T>(block_rows, nrows, nt), no_step,
                         [&](const SweepBlock<T, int64_t>& k) { return add.block(k); }, [&] { return add.commit(); }));
  SS_HIP(hipStreamSynchronize(ctx().stream));
  return SS_OK;
}

template <class T>
static int pool_merge_impl(ss_pool* dh, const ss_pool* sh) {
  SS_TRY(require_init());
  PoolBox<T>* d = nullptr;
  PoolBox<T>* s = nullptr;
  SS_TRY(pool_check<T>(dh, &d));
  SS_TRY(pool_check<T>(sh, &s));
  timing_begin_call();
  PoolTable<pool_key_t<T>> u;
  SS_TRY(pool_union(s->lv, d->w, u));
  const int64_t n = s->n, npos = s->npos;  // read before d's counts change (d may be s)
  SS_TRY(pool_push(d->lv, std::move(u), 0, d->max_entries, d->w));
  d->n += n;
  d->npos += npos;
  SS_HIP(hipStreamSynchronize(ctx().stream));
  return SS_OK;
}

template <class T>
static int pool_export_impl(ss_pool* h, T* keys, int64_t* npos, int64_t* nneg, int64_t cap, int64_t* count, int mem) {
  SS_TRY(require_init());
  SS_TRY(check_mem(mem));
  PoolBox<T>* pp = nullptr;
  SS_TRY(pool_check<T>(h, &pp));
  PoolBox<T>& p = *pp;
  SS_TRY(pool_consolidate(p.lv, p.w));
  const int64_t E = p.lv.empty() ? 0 : p.lv[0].n;
  if (count) *count = E;
  if (!keys) return SS_OK;  // size query
  if (!npos || !nneg) return fail(SS_EINVAL, "pool export: NULL count buffer");
  if (cap < E) return fail(SS_EINVAL, "pool export: capacity %lld < %lld entries", (long long)cap, (long long)E);
  if (E == 0) return SS_OK;
  hipStream_t st = ctx().stream;
  const PoolTable<pool_key_t<T>>& t = p.lv[0];
  if (mem == SS_MEM_DEVICE) {
    SS_TRY(pool_export_table<T>(t, keys));
    SS_HIP(hipMemcpyAsync(npos, t.npos.p, (size_t)E * sizeof(int64_t), hipMemcpyDeviceToDevice, st));
    SS_HIP(hipMemcpyAsync(nneg, t.nneg.p, (size_t)E * sizeof(int64_t), hipMemcpyDeviceToDevice, st));
  } else {
    DevBuf<T> v;
    SS_TRY(v.alloc((size_t)E));
    SS_TRY(pool_export_table<T>(t, v.p));
    SS_HIP(hipMemcpyAsync(keys, v.p, (size_t)E * sizeof(T), hipMemcpyDeviceToHost, st));
    SS_HIP(hipMemcpyAsync(npos, t.npos.p, (size_t)E * sizeof(int64_t), hipMemcpyDeviceToHost, st));
    SS_HIP(hipMemcpyAsync(nneg, t.nneg.p, (size_t)E * sizeof(int64_t), hipMemcpyDeviceToHost, st));
  }
  SS_HIP(hipStreamSynchronize(st));
  return SS_OK;
}

template <class T>
static int pool_import_impl(ss_pool* h, const T* keys, const int64_t* npos, const int64_t* nneg, int64_t n, int mem) {
  SS_TRY(require_init());
  SS_TRY(check_mem(mem));
  PoolBox<T>* pp = nullptr;
  SS_TRY(pool_check<T>(h, &pp));
  PoolBox<T>& p = *pp;
  if (n < 0) return fail(SS_EINVAL, "pool import: n = %lld < 0", (long long)n);
  if (n == 0) return SS_OK;
  if (!keys || !npos || !nneg) return fail(SS_EINVAL, "pool import: NULL buffer");
  timing_begin_call();
  const T* dk = keys;
  const int64_t* dp = npos;
  const int64_t* dn = nneg;
  DevBuf<T> bk;
  DevBuf<int64_t> bp, bn;
  if (mem == SS_MEM_HOST) {
    SS_TRY(bk.alloc((size_t)n));
    SS_TRY(bp.alloc((size_t)n));
    SS_TRY(bn.alloc((size_t)n));
    SS_TRY(upload<T>(bk.p, keys, (size_t)n, SS_MEM_HOST));
    SS_TRY(upload<int64_t>(bp.p, npos, (size_t)n, SS_MEM_HOST));
    SS_TRY(upload<int64_t>(bn.p, nneg, (size_t)n, SS_MEM_HOST));
    dk = bk.p;
    dp = bp.p;
    dn = bn.p;
  }
  PoolTable<pool_key_t<T>> t;
  int64_t P = 0, N = 0;
  SS_TRY(pool_import_table<T>(dk, dp, dn, n, p.w, t, &P, &N));
  SS_TRY(pool_push(p.lv, std::move(t), 0, p.max_entries, p.w));
  p.n += P + N;
  p.npos += P;
  SS_HIP(hipStreamSynchronize(ctx().stream));
  return SS_OK;
}

template <class T>
static int pool_metrics_impl(PoolBox<T>& p, double* out) {
  if (p.n == 0) return fail(SS_EINVAL, "pool is empty");
  timing_begin_call();
  SS_TRY(pool_consolidate(p.lv, p.w));
  return pool_table_metrics(p.lv[0], p.npos, p.n - p.npos, p.w, out);
}

// ------------------------------------------------------------------ per-target top-L tables (target_topl.hip)
// A handle: the committed table, a second one every add builds in, the counts and the scratch reused across adds.  An
// add copies the table into the second buffer, streams its blocks into that copy and swaps the two only when every
// block has gone in and no score was NaN: on any error the handle is as it was.
constexpr uint32_t SS_TOPL_MAGIC = 0x4c504f54u;
template <class T>
struct TlBox : HandleHead {
  uint32_t magic = SS_TOPL_MAGIC;
  int64_t nt = 0, rows = 0, npos = 0;
  int L = 0;
  TlTable<pool_key_t<T>> t, nx;
  TlWork<pool_key_t<T>> w;
  int64_t fill() const { return rows < L ? rows : L; }
};

static int tl_dtype(const void* h, int* dtype) {
  if (!h) return fail(SS_EINVAL, "target top-L handle is NULL");
  const TlBox<float>* b = reinterpret_cast<const TlBox<float>*>(h);  // the head and the tag lie alike in both
  if (b->magic != SS_TOPL_MAGIC || (b->dtype != 4 && b->dtype != 8)) return fail(SS_EINVAL, "not a target top-L handle");
  *dtype = b->dtype;
  return SS_OK;
}

template <class T>
static int tl_check(const void* h, TlBox<T>** out) {
  int dt = 0;
  SS_TRY(tl_dtype(h, &dt));
  if (dt != (int)sizeof(T)) return fail(SS_EINVAL, "target top-L handle was created with the other precision");
  *out = const_cast<TlBox<T>*>(reinterpret_cast<const TlBox<T>*>(h));
  return SS_OK;
}

template <class T>
static int tl_create_impl(int64_t nt, int L, ss_target_topl** out) {
  SS_TRY(require_init());
  if (!out) return fail(SS_EINVAL, "out handle pointer is NULL");
  *out = nullptr;
  if (nt < 1 || nt >= (1LL << 31)) return fail(SS_EINVAL, "target top-L: nt = %lld outside [1, 2^31)", (long long)nt);
  if (L < 1 || L > 1024) return fail(SS_EINVAL, "target top-L: L = %d outside [1, 1024]", L);
  TlBox<T>* box = new (std::nothrow) TlBox<T>();
  if (!box) return fail(SS_ENOMEM, "host allocation failed");
  box->dtype = (int)sizeof(T);
  box->nt = nt;
  box->L = L;
  int rc = tl_alloc(box->t, nt, L);
  if (rc == SS_OK) rc = hipStreamSynchronize(ctx().stream) == hipSuccess ? SS_OK : fail(SS_EHIP, "stream sync failed");
  if (rc != SS_OK) {
    delete box;
    return rc;
  }
  *out = reinterpret_cast<ss_target_topl*>(box);
  return SS_OK;
}

// an add starts on a copy of the table ...
template <class T>
static int tl_start(TlBox<T>& b) {
  SS_TRY(tl_copy(b.t, b.nx, b.nt, b.L, b.fill()));
  return tl_begin(b.w, b.nt, b.L);
}

// ... which replaces the table once every block has gone in
template <class T>
static int tl_commit(TlBox<T>& b, int64_t nrows, int64_t npos) {
  SS_TRY(tl_finish(b.w));
  std::swap(b.t, b.nx);
  b.rows += nrows;
  b.npos += npos;
  return SS_OK;
}

template <class T>
static int tl_add_rows_impl(ss_target_topl* h, const int64_t* yptr, const int32_t* yidx, int base, const T* yhat,
                            int64_t nrows, int64_t ncols, int64_t ld, int64_t row_begin, int mem) {
  SS_TRY(require_init());
  SS_TRY(check_mem(mem));
  TlBox<T>* bp = nullptr;
  SS_TRY(tl_check<T>(h, &bp));
  TlBox<T>& b = *bp;
  if (base != 0 && base != 1) return fail(SS_EINVAL, "index_base must be 0 or 1");
  if (nrows < 0 || nrows >= (1LL << 31))
    return fail(SS_EINVAL, "target top-L add rows: nrows = %lld outside [0, 2^31)", (long long)nrows);
  if (ncols != b.nt)
    return fail(SS_EINVAL, "target top-L add rows: ncols = %lld, the handle has nt = %lld", (long long)ncols,
                (long long)b.nt);
  if (ld < ncols)
    return fail(SS_EINVAL, "target top-L add rows: leading dimension %lld < %lld", (long long)ld, (long long)ncols);
  if (row_begin < 0 || row_begin > INT64_MAX - nrows)
    return fail(SS_EINVAL, "target top-L add rows: row_begin = %lld out of range", (long long)row_begin);
  if (nrows == 0) return SS_OK;
  if (!yptr || !yhat) return fail(SS_EINVAL, "target top-L add rows: NULL buffer");
  StagedRows<T> s;
  SS_TRY(stage_label_rows("target top-L add rows", yptr, yidx, base, yhat, nrows, ncols, ld, mem, s));
  hipEvent_t e_begin, e_end;
  SS_TRY(timing_mark(&e_begin));
  SS_TRY(tl_start(b));
  SS_TRY((tl_add_block<T, int64_t>(b.nx, b.nt, b.L, b.fill(), s.dptr, s.shift, s.didx, base, s.nnz, s.dyhat, nrows,
                                   s.dld, row_begin, nullptr, b.w)));
  SS_TRY(timing_mark(&e_end));
  timing_span(ST_TOTAL, e_begin, e_end);
  timing_span(ST_EPILOGUE, e_begin, e_end);
  return tl_commit(b, nrows, s.nnz);
}

// A sweep into a top-L handle: tl_start before the first block, every block into the copy under its rows' source
// indices (fill follows the rows taken so far), tl_commit once the call's ST_TOTAL span is closed.
template <class T>
struct TlAdd {
  TlBox<T>& b;
  int64_t fill, nrows = 0, npos = 0;
  explicit TlAdd(TlBox<T>& box) : b(box), fill(box.fill()) {}
  int start() {
    StageTimer t3(ST_EPILOGUE);
    return tl_start(b);
  }
  template <class P>
  int block(const SweepBlock<T, P>& k) {
    SS_TRY((tl_add_block<T, P>(b.nx, b.nt, b.L, fill, k.ptr, k.shift, k.idx, 0, k.nlab, k.scores, k.nb, k.nt, k.row0,
                               k.ids, b.w)));
    fill = fill + k.nb < b.L ? fill + k.nb : b.L;
    nrows += k.nb;
    npos += k.nlab;
    return SS_OK;
  }
  int commit() { return tl_commit(b, nrows, npos); }
};

// leave-one-out folds into the table where they are produced
template <class T>
static int tl_add_loo_impl(ss_target_topl* th, ss_graph* h, int64_t i_begin, int64_t i_end, int clean,
                           int64_t block_rows) {
  SS_TRY(require_init());
  TlBox<T>* bp = nullptr;
  SS_TRY(tl_check<T>(th, &bp));
  Graph<T>* gp = nullptr;
  SS_TRY(graph_check<T>(h, &gp));
  Graph<T>& g = *gp;
  SS_TRY(loo_graph_check(g));
  SS_TRY(range_check(i_begin, i_end, g.ns));
  SS_TRY(check_block_rows("target top-L add loo", block_rows));
  if (g.nt != bp->nt)
    return fail(SS_EINVAL, "target top-L add loo: the graph has %lld targets, the handle %lld", (long long)g.nt,
                (long long)bp->nt);
  const int64_t nrows = i_end - i_begin, nt = g.nt;
  if (nrows == 0) return SS_OK;
  TlAdd<T> add(*bp);
  SS_TRY(loo_blocks<T>(g, i_begin, i_end, clean, sweep_block_rows<T>(block_rows, nrows, nt),
                       [&] { return add.start(); }, [&](const SweepBlock<T, int>& k) { return add.block(k); }, no_step));
  return add.commit();
}

// k-fold rows into the table where they are produced
template <class T>
static int tl_add_kfold_impl(ss_target_topl* th, ss_graph* h, const int32_t* fold_of_source, int nfolds, int64_t i_begin,
                             int64_t i_end, int clean, int64_t block_rows, int mem) {
  SS_TRY(require_init());
  SS_TRY(check_mem(mem));
  TlBox<T>* bp = nullptr;
  SS_TRY(tl_check<T>(th, &bp));
  Graph<T>* gp = nullptr;
  SS_TRY(graph_check<T>(h, &gp));
  Graph<T>& g = *gp;
  SS_TRY(kfold_graph_check(g));
  SS_TRY(range_check(i_begin, i_end, g.ns));
  SS_TRY(check_block_rows("target top-L add kfold", block_rows));
  if (g.nt != bp->nt)
    return fail(SS_EINVAL, "target top-L add kfold: the graph has %lld targets, the handle %lld", (long long)g.nt,
                (long long)bp->nt);
  KfoldPlan plan;
  SS_TRY(kfold_plan(fold_of_source, nfolds, g.ns, mem, plan));
  const int64_t nrows = i_end - i_begin, nt = g.nt;
  if (nrows == 0) return SS_OK;
  TlAdd<T> add(*bp);
  SS_TRY(kfold_blocks<T>(g, plan, i_begin, i_end, clean, sweep_block_rows<T>(block_rows, nrows, nt),
                         [&] { return add.start(); }, [&](const SweepBlock<T, int64_t>& k) { return add.block(k); },
                         no_step));
  return add.commit();
}

template <class T>
static int tl_merge_impl(ss_target_topl* dh, const ss_target_topl* sh) {
  SS_TRY(require_init());
  TlBox<T>* d = nullptr;
  TlBox<T>* s = nullptr;
  SS_TRY(tl_check<T>(dh, &d));
  SS_TRY(tl_check<T>(sh, &s));
  if (d->nt != s->nt || d->L != s->L)
    return fail(SS_EINVAL, "target top-L merge: nt / L differ (%lld, %d) vs (%lld, %d)", (long long)d->nt, d->L,
                (long long)s->nt, s->L);
  timing_begin_call();
  const int64_t rows = s->rows, npos = s->npos;  // read before d's counts change (d may be s)
  SS_TRY(tl_merge_tables(d->t, d->fill(), s->t, s->fill(), d->nt, d->L, d->nx));
  SS_HIP(hipStreamSynchronize(ctx().stream));
  std::swap(d->t, d->nx);
  d->rows += rows;
  d->npos += npos;
  return SS_OK;
}

template <class T>
static int tl_export_impl(ss_target_topl* h, T* vals, int64_t* rows, uint8_t* labels, int64_t* npos,
                          int64_t* rows_added, int mem) {
  SS_TRY(require_init());
  SS_TRY(check_mem(mem));
  TlBox<T>* bp = nullptr;
  SS_TRY(tl_check<T>(h, &bp));
  TlBox<T>& b = *bp;
  if (rows_added) *rows_added = b.rows;
  const int64_t fill = b.fill(), n = b.nt * fill;
  hipStream_t st = ctx().stream;
  if (mem == SS_MEM_DEVICE) {
    SS_TRY(tl_export_table<T>(b.t, b.nt, b.L, fill, vals, rows, labels));
    if (npos) SS_HIP(hipMemcpyAsync(npos, b.t.npos.p, (size_t)b.nt * sizeof(int64_t), hipMemcpyDeviceToDevice, st));
  } else {
    DevBuf<T> v;
    DevBuf<int64_t> r;
    DevBuf<uint8_t> l;
    if (vals) SS_TRY(v.alloc((size_t)n));
    if (rows) SS_TRY(r.alloc((size_t)n));
    if (labels) SS_TRY(l.alloc((size_t)n));
    SS_TRY(tl_export_table<T>(b.t, b.nt, b.L, fill, vals ? v.p : nullptr, rows ? r.p : nullptr, labels ? l.p : nullptr));
    if (vals && n) SS_HIP(hipMemcpyAsync(vals, v.p, (size_t)n * sizeof(T), hipMemcpyDeviceToHost, st));
    if (rows && n) SS_HIP(hipMemcpyAsync(rows, r.p, (size_t)n * sizeof(int64_t), hipMemcpyDeviceToHost, st));
    if (labels && n) SS_HIP(hipMemcpyAsync(labels, l.p, (size_t)n, hipMemcpyDeviceToHost, st));
    if (npos) SS_HIP(hipMemcpyAsync(npos, b.t.npos.p, (size_t)b.nt * sizeof(int64_t), hipMemcpyDeviceToHost, st));
    SS_HIP(hipStreamSynchronize(st));
  }
  SS_HIP(hipStreamSynchronize(st));
  return SS_OK;
}

template <class T>
static int tl_import_impl(ss_target_topl* h, const T* vals, const int64_t* rows, const uint8_t* labels,
                          const int64_t* npos, int64_t rows_added, int mem) {
  SS_TRY(require_init());
  SS_TRY(check_mem(mem));
  TlBox<T>* bp = nullptr;
  SS_TRY(tl_check<T>(h, &bp));
  TlBox<T>& b = *bp;
  if (rows_added < 0) return fail(SS_EINVAL, "target top-L import: rows_added = %lld < 0", (long long)rows_added);
  if (rows_added > INT64_MAX - b.rows) return fail(SS_EINVAL, "target top-L import: rows_added overflows");
  if (rows_added == 0) return SS_OK;
  const int64_t fill = rows_added < b.L ? rows_added : b.L, n = b.nt * fill;
  if (!vals || !rows || !labels || !npos) return fail(SS_EINVAL, "target top-L import: NULL buffer");
  timing_begin_call();
  const T* dv = vals;
  const int64_t* dr = rows;
  const uint8_t* dl = labels;
  const int64_t* dn = npos;
  DevBuf<T> bv;
  DevBuf<int64_t> br, bn;
  DevBuf<uint8_t> bl;
  if (mem == SS_MEM_HOST) {
    SS_TRY(bv.alloc((size_t)n));
    SS_TRY(br.alloc((size_t)n));
    SS_TRY(bl.alloc((size_t)n));
    SS_TRY(bn.alloc((size_t)b.nt));
    SS_TRY(upload<T>(bv.p, vals, (size_t)n, SS_MEM_HOST));
    SS_TRY(upload<int64_t>(br.p, rows, (size_t)n, SS_MEM_HOST));
    SS_TRY(upload<uint8_t>(bl.p, labels, (size_t)n, SS_MEM_HOST));
    SS_TRY(upload<int64_t>(bn.p, npos, (size_t)b.nt, SS_MEM_HOST));
    dv = bv.p;
    dr = br.p;
    dl = bl.p;
    dn = bn.p;
  }
  TlTable<pool_key_t<T>> src;
  int64_t P = 0;
  SS_TRY(tl_import_table<T>(dv, dr, dl, dn, b.nt, b.L, fill, src, &P));
  SS_TRY(tl_merge_tables(b.t, b.fill(), src, fill, b.nt, b.L, b.nx));
  SS_HIP(hipStreamSynchronize(ctx().stream));
  std::swap(b.t, b.nx);
  b.rows += rows_added;
  b.npos += P;
  return SS_OK;
}

template <class T>
static int tl_metrics_impl(TlBox<T>& b, int64_t* hits, int64_t* npos, double* out, int mem) {
  SS_TRY(check_mem(mem));
  if (b.rows <= b.L)
    return fail(SS_EINVAL, "target top-L metrics: %lld rows added, recall@L needs more than L = %d", (long long)b.rows,
                b.L);
  timing_begin_call();
  hipStream_t st = ctx().stream;
  const int64_t nt = b.nt;
  DevBuf<int64_t> dh;
  SS_TRY(dh.alloc((size_t)nt));
  SS_TRY(tl_hits(b.t, nt, b.L, b.fill(), dh.p));
  std::vector<int64_t> hh((size_t)nt), hn((size_t)nt);
  SS_HIP(hipMemcpyAsync(hh.data(), dh.p, (size_t)nt * sizeof(int64_t), hipMemcpyDeviceToHost, st));
  SS_HIP(hipMemcpyAsync(hn.data(), b.t.npos.p, (size_t)nt * sizeof(int64_t), hipMemcpyDeviceToHost, st));
  if (hits) SS_HIP(hipMemcpyAsync(hits, dh.p, (size_t)nt * sizeof(int64_t),
                                  mem == SS_MEM_HOST ? hipMemcpyDeviceToHost : hipMemcpyDeviceToDevice, st));
  if (npos) SS_HIP(hipMemcpyAsync(npos, b.t.npos.p, (size_t)nt * sizeof(int64_t),
                                  mem == SS_MEM_HOST ? hipMemcpyDeviceToHost : hipMemcpyDeviceToDevice, st));
  SS_HIP(hipStreamSynchronize(st));
  // sums in target order, as Julia's mean over the groups in first-seen order
  double rec = 0.0, prec = 0.0, rec_pos = 0.0;
  int64_t with_pos = 0;
  const double Ld = (double)b.L;
  for (int64_t t = 0; t < nt; ++t) {
    const double h = (double)hh[(size_t)t];
    const int64_t p = hn[(size_t)t];
    const double r = p > 0 ? h / (double)p : std::nan("");
    rec += r;
    prec += h / Ld;
    if (p > 0) {
      rec_pos += r;
      ++with_pos;
    }
  }
  out[0] = rec / (double)nt;
  out[1] = prec / (double)nt;
  out[2] = with_pos > 0 ? rec_pos / (double)with_pos : std::nan("");
  out[3] = (double)with_pos;
  return SS_OK;
}

// ------------------------------------------------------------------ per-target ranking metrics (target_rank.hip)
// A handle is a TrState.  Collect phase: an add appends behind the npos committed triples and only its commit moves
// npos and rows.  Count phase: an add accumulates into the state's delta and only its commit adds that to the counts.
// Either way the add's verdict (NaN, a positive that is not the sealed one) comes first, so a failed add leaves the
// handle as it was.
constexpr uint32_t SS_TRANK_MAGIC = 0x4b4e5254u;
template <class T>
struct TrBox : HandleHead {
  uint32_t magic = SS_TRANK_MAGIC;
  TrState<T> s;
};

static int tr_dtype(const void* h, int* dtype) {
  if (!h) return fail(SS_EINVAL, "target rank handle is NULL");
  const TrBox<float>* b = reinterpret_cast<const TrBox<float>*>(h);  // the head and the tag lie alike in both
  if (b->magic != SS_TRANK_MAGIC || (b->dtype != 4 && b->dtype != 8)) return fail(SS_EINVAL, "not a target rank handle");
  *dtype = b->dtype;
  return SS_OK;
}

template <class T>
static int tr_check(const void* h, TrBox<T>** out) {
  int dt = 0;
  SS_TRY(tr_dtype(h, &dt));
  if (dt != (int)sizeof(T)) return fail(SS_EINVAL, "target rank handle was created with the other precision");
  *out = const_cast<TrBox<T>*>(reinterpret_cast<const TrBox<T>*>(h));
  return SS_OK;
}

template <class T>
static int tr_create_impl(int64_t nt, ss_target_rank** out) {
  SS_TRY(require_init());
  if (!out) return fail(SS_EINVAL, "out handle pointer is NULL");
  *out = nullptr;
  if (nt < 1 || nt >= (1LL << 31)) return fail(SS_EINVAL, "target rank: nt = %lld outside [1, 2^31)", (long long)nt);
  TrBox<T>* box = new (std::nothrow) TrBox<T>();
  if (!box) return fail(SS_ENOMEM, "host allocation failed");
  box->dtype = (int)sizeof(T);
  box->s.nt = nt;
  *out = reinterpret_cast<ss_target_rank*>(box);
  return SS_OK;
}

// One add (a block of rows, or a whole sweep) into a handle: start before the first block, commit after the last.
template <class T>
struct TrAdd {
  TrState<T>& s;
  int64_t nrows = 0, npos = 0;
  explicit TrAdd(TrState<T>& st) : s(st) {}
  int start() {
    StageTimer t3(ST_EPILOGUE);
    return tr_begin(s);
  }
  template <class P>
  int rows(const P* ptr, int64_t shift, const int* idx, int base, int64_t nlab, const T* scores, int64_t nb, int64_t ld,
           int64_t row0, const int* ids) {
    if (s.phase == 0) {
      if (s.npos + npos + nlab >= (1LL << 31))
        return fail(SS_EUNSUPPORTED, "target rank: 2^31 or more positives in one handle");
      SS_TRY((tr_collect_block<T, P>(s, s.npos + npos, ptr, shift, idx, base, nlab, scores, nb, ld, row0, ids)));
    } else {
      SS_TRY((tr_count_block<T, P>(s, ptr, shift, idx, base, nlab, scores, nb, ld, row0, ids)));
    }
    nrows += nb;
    npos += nlab;
    return SS_OK;
  }
  template <class P>
  int block(const SweepBlock<T, P>& k) {
    return rows<P>(k.ptr, k.shift, k.idx, 0, k.nlab, k.scores, k.nb, k.nt, k.row0, k.ids);
  }
  int commit() {
    SS_TRY(tr_finish(s));
    if (s.phase == 0) {
      s.rows += nrows;
      s.npos += npos;
    } else {
      SS_TRY(tr_count_commit(s));
      s.rows_counted += nrows;
    }
    return SS_OK;
  }
};

template <class T>
static int tr_add_rows_impl(ss_target_rank* h, const int64_t* yptr, const int32_t* yidx, int base, const T* yhat,
                            int64_t nrows, int64_t ncols, int64_t ld, int64_t row_begin, int mem) {
  SS_TRY(require_init());
  SS_TRY(check_mem(mem));
  TrBox<T>* bp = nullptr;
  SS_TRY(tr_check<T>(h, &bp));
  TrState<T>& s = bp->s;
  if (base != 0 && base != 1) return fail(SS_EINVAL, "index_base must be 0 or 1");
  if (nrows < 0 || nrows >= (1LL << 31))
    return fail(SS_EINVAL, "target rank add rows: nrows = %lld outside [0, 2^31)", (long long)nrows);
  if (ncols != s.nt)
    return fail(SS_EINVAL, "target rank add rows: ncols = %lld, the handle has nt = %lld", (long long)ncols,
                (long long)s.nt);
  if (ld < ncols)
    return fail(SS_EINVAL, "target rank add rows: leading dimension %lld < %lld", (long long)ld, (long long)ncols);
  if (row_begin < 0 || row_begin + nrows > (1LL << 31))
    return fail(SS_EINVAL, "target rank add rows: rows %lld.. outside [0, 2^31)", (long long)row_begin);
  if (nrows == 0) return SS_OK;
  if (!yptr || !yhat) return fail(SS_EINVAL, "target rank add rows: NULL buffer");
  StagedRows<T> st;
  SS_TRY(stage_label_rows("target rank add rows", yptr, yidx, base, yhat, nrows, ncols, ld, mem, st));
  hipEvent_t e_begin, e_end;
  SS_TRY(timing_mark(&e_begin));
  TrAdd<T> add(s);
  SS_TRY(tr_begin(s));
  SS_TRY((add.template rows<int64_t>(st.dptr, st.shift, st.didx, base, st.nnz, st.dyhat, nrows, st.dld, row_begin,
                                     nullptr)));
  SS_TRY(timing_mark(&e_end));
  timing_span(ST_TOTAL, e_begin, e_end);
  timing_span(ST_EPILOGUE, e_begin, e_end);
  return add.commit();
}

template <class T>
static int tr_add_loo_impl(ss_target_rank* th, ss_graph* h, int64_t i_begin, int64_t i_end, int clean,
                           int64_t block_rows) {
  SS_TRY(require_init());
  TrBox<T>* bp = nullptr;
  SS_TRY(tr_check<T>(th, &bp));
  Graph<T>* gp = nullptr;
  SS_TRY(graph_check<T>(h, &gp));
  Graph<T>& g = *gp;
  SS_TRY(loo_graph_check(g));
  SS_TRY(range_check(i_begin, i_end, g.ns));
  SS_TRY(check_block_rows("target rank add loo", block_rows));
  if (g.nt != bp->s.nt)
    return fail(SS_EINVAL, "target rank add loo: the graph has %lld targets, the handle %lld", (long long)g.nt,
                (long long)bp->s.nt);
  const int64_t nrows = i_end - i_begin, nt = g.nt;
  if (nrows == 0) return SS_OK;
  TrAdd<T> add(bp->s);
  SS_TRY(loo_blocks<T>(g, i_begin, i_end, clean, sweep_block_rows<T>(block_rows, nrows, nt),
                       [&] { return add.start(); }, [&](const SweepBlock<T, int>& k) { return add.block(k); }, no_step));
  return add.commit();
}

template <class T>
static int tr_add_kfold_impl(ss_target_rank* th, ss_graph* h, const int32_t* fold_of_source, int nfolds, int64_t i_begin,
                             int64_t i_end, int clean, int64_t block_rows, int mem) {
  SS_TRY(require_init());
  SS_TRY(check_mem(mem));
  TrBox<T>* bp = nullptr;
  SS_TRY(tr_check<T>(th, &bp));
  Graph<T>* gp = nullptr;
  SS_TRY(graph_check<T>(h, &gp));
  Graph<T>& g = *gp;
  SS_TRY(kfold_graph_check(g));
  SS_TRY(range_check(i_begin, i_end, g.ns));
  SS_TRY(check_block_rows("target rank add kfold", block_rows));
  if (g.nt != bp->s.nt)
    return fail(SS_EINVAL, "target rank add kfold: the graph has %lld targets, the handle %lld", (long long)g.nt,
                (long long)bp->s.nt);
  KfoldPlan plan;
  SS_TRY(kfold_plan(fold_of_source, nfolds, g.ns, mem, plan));
  const int64_t nrows = i_end - i_begin, nt = g.nt;
  if (nrows == 0) return SS_OK;
  TrAdd<T> add(bp->s);
  SS_TRY(kfold_blocks<T>(g, plan, i_begin, i_end, clean, sweep_block_rows<T>(block_rows, nrows, nt),
                         [&] { return add.start(); }, [&](const SweepBlock<T, int64_t>& k) { return add.block(k); },
                         no_step));
  return add.commit();
}

template <class T>
static int tr_seal_impl(TrBox<T>& b) {
  SS_TRY(require_init());
  if (b.s.phase != 0) return fail(SS_EINVAL, "target rank seal: the handle is sealed already");
  timing_begin_call();
  return tr_seal(b.s);
}

template <class T>
static int tr_merge_impl(ss_target_rank* dh, const ss_target_rank* sh) {
  SS_TRY(require_init());
  TrBox<T>* d = nullptr;
  TrBox<T>* c = nullptr;
  SS_TRY(tr_check<T>(dh, &d));
  SS_TRY(tr_check<T>(sh, &c));
  TrState<T>& a = d->s;
  const TrState<T>& b = c->s;
  if (d == c) return fail(SS_EINVAL, "target rank merge: a handle cannot be merged into itself (its row ids would repeat)");
  if (a.nt != b.nt) return fail(SS_EINVAL, "target rank merge: nt differs (%lld vs %lld)", (long long)a.nt, (long long)b.nt);
  if (a.phase != b.phase) return fail(SS_EINVAL, "target rank merge: one handle collects, the other counts");
  timing_begin_call();
  if (a.phase == 0) {
    if (a.npos + b.npos >= (1LL << 31)) return fail(SS_EUNSUPPORTED, "target rank: 2^31 or more positives in one handle");
    const int64_t n = b.npos, rows = b.rows;
    SS_TRY(tr_append(a, b.ct.p, b.cr.p, b.cv.p, n, false));
    a.npos += n;
    a.rows += rows;
    return SS_OK;
  }
  bool same = false;
  SS_TRY(tr_same_table(a, b, &same));
  if (!same || a.rows != b.rows)
    return fail(SS_EINVAL, "target rank merge: the handles do not hold the same sealed positives");
  SS_TRY(tr_add_counts(a, b.counts.p, false));
  a.rows_counted += b.rows_counted;
  return SS_OK;
}

template <class T>
static int tr_export_positives_impl(ss_target_rank* h, int32_t* targets, int64_t* rows, T* scores, int64_t* rows_added,
                                    int mem) {
  SS_TRY(require_init());
  SS_TRY(check_mem(mem));
  TrBox<T>* bp = nullptr;
  SS_TRY(tr_check<T>(h, &bp));
  const TrState<T>& s = bp->s;
  if (rows_added) *rows_added = s.rows;
  hipStream_t st = ctx().stream;
  const hipMemcpyKind kind = mem == SS_MEM_HOST ? hipMemcpyDeviceToHost : hipMemcpyDeviceToDevice;
  const size_t n = (size_t)s.npos;
  if (n) {
    if (targets) SS_HIP(hipMemcpyAsync(targets, s.phase ? s.st.p : s.ct.p, n * sizeof(int), kind, st));
    if (rows) SS_HIP(hipMemcpyAsync(rows, s.phase ? s.sr.p : s.cr.p, n * sizeof(int64_t), kind, st));
    if (scores) SS_HIP(hipMemcpyAsync(scores, s.phase ? s.sv.p : s.cv.p, n * sizeof(T), kind, st));
  }
  SS_HIP(hipStreamSynchronize(st));
  return SS_OK;
}

template <class T>
static int tr_import_positives_impl(ss_target_rank* h, const int32_t* targets, const int64_t* rows, const T* scores,
                                    int64_t npos, int64_t rows_added, int mem) {
  SS_TRY(require_init());
  SS_TRY(check_mem(mem));
  TrBox<T>* bp = nullptr;
  SS_TRY(tr_check<T>(h, &bp));
  TrState<T>& s = bp->s;
  if (s.phase != 0) return fail(SS_EINVAL, "target rank import positives: the handle is sealed");
  if (npos < 0 || rows_added < 0) return fail(SS_EINVAL, "target rank import positives: negative size");
  if (s.npos + npos >= (1LL << 31)) return fail(SS_EUNSUPPORTED, "target rank: 2^31 or more positives in one handle");
  if (s.rows + rows_added > (1LL << 31)) return fail(SS_EINVAL, "target rank import positives: more than 2^31 rows");
  if (npos > 0 && (!targets || !rows || !scores)) return fail(SS_EINVAL, "target rank import positives: NULL buffer");
  timing_begin_call();
  const int* dt = targets;
  const int64_t* dr = rows;
  const T* dv = scores;
  DevBuf<int> bt;
  DevBuf<int64_t> br;
  DevBuf<T> bv;
  if (mem == SS_MEM_HOST && npos > 0) {
    SS_TRY(bt.alloc((size_t)npos));
    SS_TRY(br.alloc((size_t)npos));
    SS_TRY(bv.alloc((size_t)npos));
    SS_TRY(upload<int>(bt.p, targets, (size_t)npos, SS_MEM_HOST));
    SS_TRY(upload<int64_t>(br.p, rows, (size_t)npos, SS_MEM_HOST));
    SS_TRY(upload<T>(bv.p, scores, (size_t)npos, SS_MEM_HOST));
    dt = bt.p;
    dr = br.p;
    dv = bv.p;
  }
  SS_TRY(tr_append(s, dt, dr, dv, npos, true));
  SS_HIP(hipStreamSynchronize(ctx().stream));
  s.npos += npos;
  s.rows += rows_added;
  return SS_OK;
}

template <class T>
static int tr_export_counts_impl(TrBox<T>& b, int64_t* counts, int64_t* rows_counted, int mem) {
  SS_TRY(require_init());
  SS_TRY(check_mem(mem));
  const TrState<T>& s = b.s;
  if (s.phase != 1) return fail(SS_EINVAL, "target rank export counts: the handle is not sealed");
  if (rows_counted) *rows_counted = s.rows_counted;
  hipStream_t st = ctx().stream;
  if (counts)
    SS_HIP(hipMemcpyAsync(counts, s.counts.p, (size_t)s.counts_len() * sizeof(int64_t),
                          mem == SS_MEM_HOST ? hipMemcpyDeviceToHost : hipMemcpyDeviceToDevice, st));
  SS_HIP(hipStreamSynchronize(st));
  return SS_OK;
}

template <class T>
static int tr_import_counts_impl(TrBox<T>& b, const int64_t* counts, int64_t ncounts, int64_t rows_counted, int mem) {
  SS_TRY(require_init());
  SS_TRY(check_mem(mem));
  TrState<T>& s = b.s;
  if (s.phase != 1) return fail(SS_EINVAL, "target rank import counts: the handle is not sealed");
  if (ncounts != s.counts_len())
    return fail(SS_EINVAL, "target rank import counts: %lld counts, the handle's table has %lld", (long long)ncounts,
                (long long)s.counts_len());
  if (rows_counted < 0 || rows_counted > (1LL << 31) - s.rows_counted)
    return fail(SS_EINVAL, "target rank import counts: rows_counted = %lld out of range", (long long)rows_counted);
  if (!counts) return fail(SS_EINVAL, "target rank import counts: NULL buffer");
  timing_begin_call();
  const int64_t* dc = counts;
  DevBuf<int64_t> bc;
  if (mem == SS_MEM_HOST) {
    SS_TRY(bc.alloc((size_t)ncounts));
    SS_TRY(upload<int64_t>(bc.p, counts, (size_t)ncounts, SS_MEM_HOST));
    dc = bc.p;
  }
  SS_TRY(tr_add_counts(s, dc, true));
  s.rows_counted += rows_counted;
  return SS_OK;
}

template <class T>
static int tr_metrics_impl(TrBox<T>& b, double alpha, int L, double* out, int mem) {
  SS_TRY(require_init());
  SS_TRY(check_mem(mem));
  const TrState<T>& s = b.s;
  if (s.phase != 1) return fail(SS_EINVAL, "target rank metrics: the handle is not sealed (collect, seal, then count)");
  if (s.rows_counted != s.rows)
    return fail(SS_EINVAL, "target rank metrics: %lld rows counted, %lld collected", (long long)s.rows_counted,
                (long long)s.rows);
  if (L < 1) return fail(SS_EINVAL, "Please use a list length greater than 0 (L > 0)");
  if ((int64_t)L >= s.rows) return fail(SS_EINVAL, "Number of labels is less than length (L > y)");
  if (!(alpha > 0.0)) return fail(SS_EINVAL, "target rank metrics: alpha must be positive");
  if (!out) return fail(SS_EINVAL, "output buffer is NULL");
  timing_begin_call();
  hipStream_t st = ctx().stream;
  hipEvent_t e_begin, e_end;
  SS_TRY(timing_mark(&e_begin));
  double* dout = out;
  DevBuf<double> bout;
  if (mem == SS_MEM_HOST) {
    SS_TRY(bout.alloc((size_t)s.nt * 6));
    dout = bout.p;
  }
  SS_TRY(tr_metrics(s, alpha, L, dout));
  SS_TRY(timing_mark(&e_end));
  timing_span(ST_TOTAL, e_begin, e_end);
  if (mem == SS_MEM_HOST)
    SS_HIP(hipMemcpyAsync(out, bout.p, (size_t)s.nt * 6 * sizeof(double), hipMemcpyDeviceToHost, st));
  SS_HIP(hipStreamSynchronize(st));
  return SS_OK;
}

// ------------------------------------------------------------------ raw SpMM
template <class T>
static int spmat_check(const void* h, SpMat<T>** out) {
  if (!h) return fail(SS_EINVAL, "matrix handle is NULL");
  SpMatBox<T>* b = const_cast<SpMatBox<T>*>(reinterpret_cast<const SpMatBox<T>*>(h));
  if (b->dtype != (int)sizeof(T)) return fail(SS_EINVAL, "matrix handle was created with the other precision");
  *out = &b->m;
  return SS_OK;
}

template <class T>
static int spmat_create_impl(int64_t rows, int64_t cols, const int64_t* ptr, const int32_t* idx, const T* val,
                             int index_base, int mem, ss_spmat** out) {
  SS_TRY(require_init());
  SS_TRY(check_mem(mem));
  if (!out) return fail(SS_EINVAL, "out handle pointer is NULL");
  *out = nullptr;
  SpMatBox<T>* box = new (std::nothrow) SpMatBox<T>();
  if (!box) return fail(SS_ENOMEM, "host allocation failed");
  box->dtype = (int)sizeof(T);
  int rc = csr_from_user<T>(rows, cols, ptr, idx, val, index_base, mem, box->m.csr);
  if (rc != SS_OK) { delete box; return rc; }
  *out = reinterpret_cast<ss_spmat*>(box);
  return SS_OK;
}

// Which kernel serves a W*R of width B, and on which lazily built operand of the matrix handle.
enum WrFamily { WR_CSELL, WR_COLGROUP, WR_NARROW, WR_SELL };
struct WrRoute {
  WrFamily family;
  int slot;           // m.csell[slot], m.col[slot] or m.narrow[slot]; unused for WR_SELL
  int cols;           // columns of R per tile row (the padded width the operand is cut for)
  WrFamily fallback;  // WR_CSELL only: the family that serves B when the compact operand cannot hold the matrix
};

// the 2-D kernel (spmm_colgroup.hip): tile rows of 64 / 128 / 256 bytes in m.col[0..2]
template <class T>
static WrRoute colgroup_route(int64_t B) {
  const int64_t bytes = B * (int64_t)sizeof(T);
  const int rowb = bytes <= 64 ? 64 : (bytes <= 128 ? 128 : 256);
  return {WR_COLGROUP, rowb == 64 ? 0 : (rowb == 128 ? 1 : 2), rowb / (int)sizeof(T), WR_COLGROUP};
}
// the narrow kernel: B <= 1, 2, 4 in m.narrow[0..2]
template <class T>
static WrRoute narrow_route(int64_t B) {
  int slot = 0, bv = 1;
  while (bv < B) { bv <<= 1; ++slot; }
  return {WR_NARROW, slot, bv, WR_NARROW};
}

// Routing by width, row-major operands (measured at 100k x 100k / 1 %):
//   B <= 4                          narrow kernel: W streamed once, the chunk of R in LDS, lanes of a row folded -- the
//                                   HBM-bound regime (B = 1 0.13 ms = 4.6 TB/s of the 6 B/nnz operand).  B = 3, 4: the
//                                   lane-per-row kernel (spmm_csell.hip) with four columns per tile row (16 bytes in fp32:
//                                   0.136 vs 0.150 ms at B = 4; 32 bytes in fp64), m.csell[4].  fp64 B = 2: the same on
//                                   16-byte tile rows, m.csell[5]: 0.199 vs 0.234 ms (measured also: fp64 B = 1 0.204 vs
//                                   0.200, fp32 B = 1 / 2 0.138 / 0.139 vs 0.112 / 0.116 -- those stay narrow)
//   5 <= B, B*sizeof(T) <= 256 B    the lane-per-row kernel on the compact sliced-ELL operand, m.csell[0..2] by tile row of
//                                   64 / 128 / 256 bytes, fp32 B <= 8 on 32-byte tile rows (two pieces) in m.csell[3]
//                                   instead of half-empty 64-byte ones (fp32 B = 8 / 16 / 32 / 64 0.19 / 0.18 / 0.35 /
//                                   0.70 ms); SS_CSELL=0 or an operand that does not fit: the 2-D kernel
//                                   (spmm_colgroup.hip); fp32 B = 5..16 0.22-0.24 ms, 32 0.44, 64 0.9
//   wider, and pattern-only W (every value 1) above 128-byte tile rows: the SELL kernel of stage 2, which re-streams only
//                                   the 2-byte indices (B = 64: 0.61 vs 0.82 ms); column-major operands always
// SS_COL=0: no 2-D kernel (SELL instead); SS_COL_FROM: its first B, pattern-only wide cases included (comparisons, tests);
// SS_CSELL_ROW32 / SS_CSELL_ROW16 / SS_CSELL_B12 = 0: without the 32-byte / four-column / fp64 B = 2 operands
template <class T>
static WrRoute wr_route(int64_t B, bool rowmajor, bool binary) {
  const int64_t bytes = B * (int64_t)sizeof(T);
  if (rowmajor && B >= env_int("SS_COL_FROM", 5) && bytes <= 256 && (!(binary && bytes > 128) || env_set("SS_COL_FROM")) &&
      !env_off("SS_COL")) {
    const WrRoute col = colgroup_route<T>(B);
    if (env_off("SS_CSELL")) return col;
    if (sizeof(T) == 4 && B <= 8 && !env_off("SS_CSELL_ROW32")) return {WR_CSELL, 3, 32 / (int)sizeof(T), WR_COLGROUP};
    return {WR_CSELL, col.slot, col.cols, WR_COLGROUP};
  }
  if (rowmajor && B <= 4) {
    if (sizeof(T) == 8 && B == 2 && !env_off("SS_CSELL_B12") && !env_off("SS_CSELL"))
      return {WR_CSELL, 5, 16 / (int)sizeof(T), WR_NARROW};
    if (B >= 3 && !env_off("SS_CSELL_ROW16") && !env_off("SS_CSELL")) return {WR_CSELL, 4, 4, WR_NARROW};
    return narrow_route<T>(B);
  }
  return {WR_SELL, 0, 0, WR_SELL};
}

// SS_NARROW_CHUNK lowers the column chunk of a W*R operand (comparisons, tests)
static int wr_chunk_cols(int kc) { return (int)env_int_in("SS_NARROW_CHUNK", 16, kc, kc); }

// The lazily built operands of a route; *op is NULL when the slot cannot serve (csell only: take the fallback).
// soft (the csell operands of B <= 4): a failed build is no error and is tried again by the next call, and the chunk
// does not follow SS_NARROW_CHUNK; otherwise a failed build is the call's error.  A slot that built but cannot hold the
// matrix (!ok) is remembered and never serves.
template <class T>
static int csell_operand(SpMat<T>& m, const WrRoute& r, bool soft, DevCsell<T>** op) {
  DevCsell<T>& cs = m.csell[r.slot];
  *op = nullptr;
  if (!m.csell_tried[r.slot]) {
    const int kc = csell_chunk_cols(r.cols * (int)sizeof(T));
    const int rc = csell_build<T>(m.csr, soft ? kc : wr_chunk_cols(kc), r.cols, cs);
    if (rc != SS_OK) return soft ? SS_OK : rc;
    m.csell_tried[r.slot] = true;
  }
  if (cs.ok) *op = &cs;
  return SS_OK;
}
template <class T>
static int chunked_operand(SpMat<T>& m, const WrRoute& r, DevChunked<T>** op) {
  DevChunked<T>& c = r.family == WR_COLGROUP ? m.col[r.slot] : m.narrow[r.slot];
  if (c.SC == 0) {
    const int kc = r.family == WR_COLGROUP ? colgroup_chunk_cols<T>(r.cols) : narrow_chunk_cols<T>(r.cols);
    SS_TRY(chunked_build<T>(m.csr, wr_chunk_cols(kc), 4, c));
  }
  *op = &c;
  return SS_OK;
}

template <class T>
static int spmm_impl(ss_spmat* h, const T* R, int64_t B, int64_t ldr, int r_layout, T* F, int64_t ldf, int f_layout,
                     int mem) {
  SS_TRY(require_init());
  SS_TRY(check_mem(mem));
  SS_TRY(check_layout(r_layout));
  SS_TRY(check_layout(f_layout));
  SpMat<T>* mp = nullptr;
  SS_TRY(spmat_check<T>(h, &mp));
  SpMat<T>& m = *mp;
  const int64_t M = m.csr.rows, K = m.csr.cols;
  if (B < 0) return fail(SS_EINVAL, "B < 0");
  if (B == 0 || M == 0) return SS_OK;
  if (!F || (K > 0 && !R)) return fail(SS_EINVAL, "NULL operand");
  if (ldr < (r_layout == SS_LAYOUT_ROWMAJOR ? B : K)) return fail(SS_EINVAL, "ldr too small");
  if (ldf < (f_layout == SS_LAYOUT_ROWMAJOR ? B : M)) return fail(SS_EINVAL, "ldf too small");
  hipStream_t st = ctx().stream;
  timing_begin_call();

  // stage caller operands on the device in their own layout
  DevBuf<T> dR, dF;
  const T* Rd = R;
  T* Fd = F;
  int64_t ldr_d = ldr, ldf_d = ldf;
  if (mem == SS_MEM_HOST) {
    StageTimer t4(ST_H2D);
    const int64_t r_outer = (r_layout == SS_LAYOUT_ROWMAJOR) ? K : B, r_inner = (r_layout == SS_LAYOUT_ROWMAJOR) ? B : K;
    SS_TRY(dR.alloc((size_t)(r_outer > 0 ? r_outer : 1) * r_inner));
    if (r_outer > 0)
      SS_HIP(hipMemcpy2DAsync(dR.p, r_inner * sizeof(T), R, ldr * sizeof(T), r_inner * sizeof(T), r_outer,
                              hipMemcpyHostToDevice, st));
    Rd = dR.p;
    ldr_d = r_inner;
    const int64_t f_outer = (f_layout == SS_LAYOUT_ROWMAJOR) ? M : B, f_inner = (f_layout == SS_LAYOUT_ROWMAJOR) ? B : M;
    SS_TRY(dF.alloc((size_t)f_outer * f_inner));
    Fd = dF.p;
    ldf_d = f_inner;
  }
  hipEvent_t e_begin, e_end;
  SS_TRY(timing_mark(&e_begin));
  const bool rowmajor = r_layout == SS_LAYOUT_ROWMAJOR && f_layout == SS_LAYOUT_ROWMAJOR;
  WrRoute route = wr_route<T>(B, rowmajor, m.csr.binary);
  DevCsell<T>* cs = nullptr;
  if (route.family == WR_CSELL) {
    SS_TRY(csell_operand<T>(m, route, route.fallback == WR_NARROW, &cs));
    if (!cs) route = route.fallback == WR_NARROW ? narrow_route<T>(B) : colgroup_route<T>(B);
  }
  DevChunked<T>* op = nullptr;
  if (route.family == WR_COLGROUP || route.family == WR_NARROW) SS_TRY(chunked_operand<T>(m, route, &op));
  DevBuf<T> Rt, Ft;
  switch (route.family) {
  case WR_CSELL: {
    StageTimer t2(ST_SPMM);
    SS_TRY(launch_spmm_csell<T>(*cs, Rd, ldr_d, (int)B, Fd, ldf_d, m.partial));
    timing_count(ST_NSPMM, 1);
    break;
  }
  case WR_COLGROUP: {
    StageTimer t2(ST_SPMM);
    SS_TRY(launch_spmm_colgroup<T>(*op, route.cols, Rd, ldr_d, (int)B, Fd, ldf_d, m.partial));
    timing_count(ST_NSPMM, 1);
    break;
  }
  case WR_NARROW: {
    StageTimer t2(ST_SPMM);
    SS_TRY(launch_spmm_chunked_narrow<T>(*op, route.cols, Rd, ldr_d, (int)B, Fd, ldf_d, m.partial));
    timing_count(ST_NSPMM, 1);
    break;
  }
  case WR_SELL: {
    const int qt = sell_tile_width<T>();
    if (m.sell_qt != qt) {
      SS_TRY(sell_build<T>(m.csr, sell_chunk<T>(qt), m.sell));
      m.sell_qt = qt;
    }
    const T* Rc = Rd;   // column-major view: R(k,b) at Rc[b*ldrc + k]
    int64_t ldrc = ldr_d;
    if (r_layout == SS_LAYOUT_ROWMAJOR) {
      StageTimer t3(ST_EPILOGUE);
      SS_TRY(Rt.alloc((size_t)B * (K > 0 ? K : 1)));
      SS_TRY(launch_transpose<T>(Rd, K, B, ldr_d, Rt.p, K));
      Rc = Rt.p;
      ldrc = K;
    }
    T* Fc = Fd;
    int64_t ldfc = ldf_d;
    if (f_layout == SS_LAYOUT_ROWMAJOR) {
      SS_TRY(Ft.alloc((size_t)B * M));
      Fc = Ft.p;
      ldfc = M;
    }
    DevBuf<T> Fs;  // length-sorted operand: the sorted-order result
    SS_TRY(sell_rows<T>(m.sell, Rc, ldrc, M, Fs, B, B, nullptr, ScoreDest<T>{Fc, ldfc, 0, nullptr, nullptr}));
    if (f_layout == SS_LAYOUT_ROWMAJOR) {
      StageTimer t3(ST_EPILOGUE);
      SS_TRY(launch_transpose<T>(Fc, B, M, ldfc, Fd, ldf_d));
    }
    break;
  }
  }
  SS_TRY(timing_mark(&e_end));
  timing_span(ST_TOTAL, e_begin, e_end);
  if (mem == SS_MEM_HOST) {
    StageTimer t5(ST_D2H);
    const int64_t f_outer = (f_layout == SS_LAYOUT_ROWMAJOR) ? M : B, f_inner = (f_layout == SS_LAYOUT_ROWMAJOR) ? B : M;
    SS_HIP(hipMemcpy2DAsync(F, ldf * sizeof(T), dF.p, f_inner * sizeof(T), f_inner * sizeof(T), f_outer,
                            hipMemcpyDeviceToHost, st));
    t5.stop();
  }
  SS_HIP(hipStreamSynchronize(st));
  return SS_OK;
}

// ------------------------------------------------------------------ query sets
// the common head of the query-set constructors: the library and `mem` are usable, *out is cleared, the path note is
// emptied, gh is a graph of this precision that holds CSR blocks
template <class T>
static int queries_begin(const ss_graph* gh, int64_t nq, int mem, ss_queries** out, Graph<T>** gp) {
  SS_TRY(require_init());
  SS_TRY(check_mem(mem));
  if (!out) return fail(SS_EINVAL, "out handle pointer is NULL");
  *out = nullptr;
  path_note().clear();
  SS_TRY(graph_check<T>(gh, gp));
  if ((*gp)->general) return fail(SS_EUNSUPPORTED, "query sets: a general graph takes its rows when it is created");
  if ((*gp)->dense.on)
    return fail(SS_EUNSUPPORTED, "query sets: a dense-similarity graph holds no CSR query block");
  if (nq < 0) return fail(SS_EINVAL, "query sets: negative query count");
  return SS_OK;
}

// a new query set bound to gh whose block fill(Xq) produces
template <class T, class Fill>
static int queries_finish(const ss_graph* gh, Fill fill, ss_queries** out) {
  QueriesBox<T>* box = new (std::nothrow) QueriesBox<T>();
  if (!box) return fail(SS_ENOMEM, "host allocation failed");
  box->dtype = (int)sizeof(T);
  box->graph_id = reinterpret_cast<const GraphBox<T>*>(gh)->id;
  const int rc = fill(box->Xq);
  if (rc != SS_OK) { delete box; return rc; }
  *out = reinterpret_cast<ss_queries*>(box);
  return SS_OK;
}

template <class T>
static int queries_create_csr_impl(const ss_graph* gh, int64_t nq, const int64_t* ptr, const int32_t* idx, const T* val,
                                   int index_base, int mem, ss_queries** out) {
  Graph<T>* g = nullptr;
  SS_TRY(queries_begin<T>(gh, nq, mem, out, &g));
  return queries_finish<T>(
      gh, [&](DevCsr<T>& Xq) { return csr_from_user<T>(nq, g->nf, ptr, idx, val, index_base, mem, Xq); }, out);
}

// the sources a cross block is cut against are the graph's: features named after the sources, ns of them
template <class T>
static int queries_check_sources(const Graph<T>& g, int64_t ns) {
  if (g.nf != g.ns)
    return fail(SS_EINVAL, "query sets from raw data need a graph with nf == ns (features named after the sources)");
  if (ns != g.ns)
    return fail(SS_EINVAL, "query sets: Fs has %lld rows, the graph has %lld sources", (long long)ns, (long long)g.ns);
  return SS_OK;
}

// the cross block of producer Prod, counted by count(p), into a new query set; tag: its ss_path_last tag
template <class T, class Prod, class Count>
static int queries_from_producer(const ss_graph* gh, int64_t nq, int64_t ns, Count count, const char* tag,
                                 ss_queries** out) {
  return queries_finish<T>(
      gh,
      [&](DevCsr<T>& Xq) -> int {
        if (ns == 0) {  // no sources: an nq x 0 block (a producer given no second side would pair the queries with themselves)
          const std::vector<int64_t> zeros((size_t)nq + 1, 0);
          return csr_from_user<T>(nq, 0, zeros.data(), nullptr, nullptr, 0, SS_MEM_HOST, Xq);
        }
        Prod p;
        int rc = count(p);
        if (rc == SS_OK) rc = p.to_dev_csr(Xq);
        if (nq > 0) path_add(tag);
        return rc;
      },
      out);
}

template <class T>
static int queries_create_fingerprint_impl(const ss_graph* gh, int64_t nq, int64_t ns, int64_t nwords,
                                           const uint64_t* Fq, const uint64_t* Fs, T alpha, int weighted, int mem,
                                           ss_queries** out, int k = 0) {
  Graph<T>* g = nullptr;
  SS_TRY(queries_begin<T>(gh, nq, mem, out, &g));
  SS_TRY(queries_check_sources(*g, ns));
  SS_TRY(check_nwords(nwords));
  SS_TRY(check_fingerprints("Fq", Fq, nq, nwords));
  SS_TRY(check_fingerprints("Fs", Fs, ns, nwords));
  DevBuf<uint64_t> bq, bs;
  const uint64_t *dq = nullptr, *ds = nullptr;
  SS_TRY(stage_fingerprints(Fs, ns, nwords, mem, bs, &ds));
  SS_TRY(stage_fingerprints(Fq, nq, nwords, mem, bq, &dq));
  return queries_from_producer<T, TanimotoCsr<T>>(
      gh, nq, ns, [&](TanimotoCsr<T>& p) { return p.count(dq, nq, ds, ns, nwords, alpha, weighted != 0, k); },
      tanimoto_tag(false, k), out);
}

template <class T, class Prod, class Check, class Count>
static int features_queries_impl(const FeatureNames& nm, Check check, Count count, const ss_graph* gh, int64_t nq,
                                 int64_t ns, int64_t d, const T* Fq, int64_t ldq, const T* Fs, int64_t lds_, T alpha,
                                 int mem, ss_queries** out, int k = 0) {
  Graph<T>* g = nullptr;
  SS_TRY(queries_begin<T>(gh, nq, mem, out, &g));
  SS_TRY(queries_check_sources(*g, ns));
  SS_TRY(check_feature_args(nm, check, d, alpha));
  SS_TRY(check_features("Fq", Fq, nq, ldq, d));
  SS_TRY(check_features("Fs", Fs, ns, lds_, d));
  DevBuf<T> bq, bs;
  const T *dq = nullptr, *ds = nullptr;
  int64_t lq = 0, ls = 0;
  SS_TRY(stage_features(Fs, ns, lds_, d, mem, bs, &ds, &ls));
  SS_TRY(stage_features(Fq, nq, ldq, d, mem, bq, &dq, &lq));
  return queries_from_producer<T, Prod>(
      gh, nq, ns, [&](Prod& p) { return count(p, dq, nq, lq, ds, ns, ls); }, nm.tag(false, k), out);
}

template <class T>
static int queries_degrees_impl(const ss_queries* qh, int64_t* kq, int mem) {
  SS_TRY(require_init());
  SS_TRY(check_mem(mem));
  const QueriesBox<T>* q = reinterpret_cast<const QueriesBox<T>*>(qh);
  const int64_t nq = q->Xq.rows;
  if (nq == 0) return SS_OK;
  if (!kq) return fail(SS_EINVAL, "ss_queries_degrees: kq is NULL");
  hipStream_t st = ctx().stream;
  std::vector<int> hp((size_t)nq + 1);
  SS_HIP(hipMemcpyAsync(hp.data(), q->Xq.ptr.p, hp.size() * sizeof(int), hipMemcpyDeviceToHost, st));
  SS_HIP(hipStreamSynchronize(st));
  if (mem == SS_MEM_HOST) {
    for (int64_t r = 0; r < nq; ++r) kq[r] = hp[r + 1] - hp[r];
    return SS_OK;
  }
  std::vector<int64_t> k((size_t)nq);
  for (int64_t r = 0; r < nq; ++r) k[r] = hp[r + 1] - hp[r];
  SS_HIP(hipMemcpyAsync(kq, k.data(), (size_t)nq * sizeof(int64_t), hipMemcpyHostToDevice, st));
  SS_HIP(hipStreamSynchronize(st));
  return SS_OK;
}

// ------------------------------------------------------------------ support lists (support.hip)
template <class T>
static int support_impl(ss_graph* h, const ss_queries* qh, int kind, int64_t npairs, const int64_t* rows,
                        const int32_t* targets, int M, int32_t* src, T* contrib, int32_t* nsupp, int mem) {
  SS_TRY(require_init());
  SS_TRY(check_mem(mem));
  Graph<T>* gp = nullptr;
  SS_TRY(graph_check<T>(h, &gp));
  Graph<T>& g = *gp;
  if (g.general || g.dense.on)
    return fail(SS_EUNSUPPORTED, "support: only a graph that holds CSR blocks has a sparse transfer row");
  if (kind == SS_ROWS_SOURCE)
    return fail(SS_EUNSUPPORTED, "support: the transfer row of a source row mixes the feature and the target path");
  if (kind != SS_ROWS_QUERY && kind != SS_ROWS_LOO)
    return fail(SS_EINVAL, "support: rows_kind must be SS_ROWS_QUERY or SS_ROWS_LOO");
  const DevCsr<T>* xq = &g.Xq;
  int64_t limit = g.nq;
  if (kind == SS_ROWS_LOO) {
    if (qh) return fail(SS_EINVAL, "support: SS_ROWS_LOO takes the graph's own sources, q must be NULL");
    SS_TRY(loo_graph_check(g));
    limit = g.ns;
  } else if (qh) {
    SS_TRY(queries_check<T>(qh, h, &xq));
    limit = xq->rows;
  }
  if (npairs < 0) return fail(SS_EINVAL, "support: negative pair count");
  if (M < 1 || M > 64) return fail(SS_EINVAL, "support: M = %d outside 1..64", M);
  if (npairs == 0) return SS_OK;
  if (npairs >= (1LL << 31)) return fail(SS_EUNSUPPORTED, "support: %lld pairs (>= 2^31)", (long long)npairs);
  if (!rows || !targets || !src || !contrib || !nsupp) return fail(SS_EINVAL, "support: NULL buffer");
  hipStream_t st = ctx().stream;
  // the pair list on the host (it is small), checked whole before anything is written
  std::vector<int64_t> hr((size_t)npairs);
  std::vector<int32_t> ht((size_t)npairs);
  if (mem == SS_MEM_HOST) {
    memcpy(hr.data(), rows, hr.size() * sizeof(int64_t));
    memcpy(ht.data(), targets, ht.size() * sizeof(int32_t));
  } else {
    SS_HIP(hipMemcpyAsync(hr.data(), rows, hr.size() * sizeof(int64_t), hipMemcpyDeviceToHost, st));
    SS_HIP(hipMemcpyAsync(ht.data(), targets, ht.size() * sizeof(int32_t), hipMemcpyDeviceToHost, st));
    SS_HIP(hipStreamSynchronize(st));
  }
  for (int64_t p = 0; p < npairs; ++p) {
    if (hr[p] < 0 || hr[p] >= limit)
      return fail(SS_EINVAL, "support: rows[%lld] = %lld outside 0..%lld", (long long)p, (long long)hr[p],
                  (long long)limit - 1);
    if (ht[p] < 0 || (int64_t)ht[p] >= g.nt)
      return fail(SS_EINVAL, "support: targets[%lld] = %d outside 0..%lld", (long long)p, ht[p], (long long)g.nt - 1);
  }
  timing_begin_call();
  path_add("support");
  // pairs grouped by row: the distinct rows in ascending order take one slot of the transfer block each, batch by batch
  std::vector<int> order((size_t)npairs);
  for (int64_t p = 0; p < npairs; ++p) order[p] = (int)p;
  std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return hr[a] < hr[b]; });
  const int64_t ns = g.ns;
  std::vector<int> drow;                                   // distinct rows
  std::vector<int> hs((size_t)npairs * 3);                 // slot, target, position of every pair in row order
  std::vector<int64_t> first;                              // first pair (in row order) of every distinct row
  for (int64_t k = 0; k < npairs; ++k) {
    const int p = order[k];
    if (k == 0 || hr[p] != hr[order[k - 1]]) {
      drow.push_back((int)hr[p]);
      first.push_back(k);
    }
    hs[(size_t)npairs + k] = ht[p];
    hs[(size_t)npairs * 2 + k] = p;
  }
  const int64_t nd = (int64_t)drow.size();
  first.push_back(npairs);
  const int64_t rb = transfer_batch_rows(nd, ns, sizeof(T));
  for (int64_t d = 0; d < nd; ++d)
    for (int64_t k = first[d]; k < first[d + 1]; ++k) hs[k] = (int)(d % rb);
  SS_TRY(graph_chunked(g, false));
  const size_t need = (size_t)rb * (size_t)(ns > 0 ? ns : 1);
  if (g.Tws.n < need) SS_TRY(g.Tws.alloc(need));
  DevBuf<int> d_rows, d_pairs, d_src, d_nsupp;
  DevBuf<T> d_contrib;
  SS_TRY(d_rows.alloc((size_t)nd));
  SS_TRY(d_pairs.alloc(hs.size()));
  int* osrc = src;
  T* ocon = contrib;
  int* ons = nsupp;
  if (mem == SS_MEM_HOST) {
    SS_TRY(d_src.alloc((size_t)npairs * M));
    SS_TRY(d_contrib.alloc((size_t)npairs * M));
    SS_TRY(d_nsupp.alloc((size_t)npairs));
    osrc = d_src.p;
    ocon = d_contrib.p;
    ons = d_nsupp.p;
  }
  SS_TRY(upload<int>(d_rows.p, drow.data(), (size_t)nd, SS_MEM_HOST));
  SS_TRY(upload<int>(d_pairs.p, hs.data(), hs.size(), SS_MEM_HOST));
  hipEvent_t e_begin, e_end;
  SS_TRY(timing_mark(&e_begin));
  for (int64_t d0 = 0; d0 < nd; d0 += rb) {
    const int64_t nb = nd - d0 < rb ? nd - d0 : rb;
    {
      StageTimer t1(ST_TRANSFER);
      if (kind == SS_ROWS_LOO) {
        // one launch per run of consecutive folds
        for (int64_t a = d0; a < d0 + nb;) {
          int64_t b = a + 1;
          while (b < d0 + nb && drow[b] == drow[b - 1] + 1) ++b;
          SS_TRY(launch_transfer_loo<T>(g.Xs, g.XsTc, g.kf.p, g.ks.p, drow[a], b - a, g.Tws.p + (a - d0) * ns, ns));
          a = b;
        }
      } else {
        const DevCsr<T>* L[2] = {xq, nullptr};
        const DevChunked<T>* Mt[2] = {&g.XsTc, nullptr};
        const T* inv1[2] = {g.inv_kf.p, nullptr};
        SS_TRY(launch_transfer<T>(1, L, inv1, Mt, g.inv_ks.p, d0, nb, ns, g.Tws.p, ns, d_rows.p));
      }
      timing_count(ST_NTRANSFER, 1);
    }
    StageTimer t3(ST_EPILOGUE);
    const int64_t k0 = first[d0], k1 = first[d0 + nb];
    SS_TRY(launch_support<T>(g.YsT, g.Tws.p, ns, d_pairs.p + k0, d_pairs.p + npairs + k0, d_pairs.p + 2 * npairs + k0,
                             k1 - k0, M, osrc, ocon, ons));
  }
  SS_TRY(timing_mark(&e_end));
  timing_span(ST_TOTAL, e_begin, e_end);
  if (mem == SS_MEM_HOST) {
    StageTimer t5(ST_D2H);
    SS_HIP(hipMemcpyAsync(src, d_src.p, (size_t)npairs * M * sizeof(int), hipMemcpyDeviceToHost, st));
    SS_HIP(hipMemcpyAsync(contrib, d_contrib.p, (size_t)npairs * M * sizeof(T), hipMemcpyDeviceToHost, st));
    SS_HIP(hipMemcpyAsync(nsupp, d_nsupp.p, (size_t)npairs * sizeof(int), hipMemcpyDeviceToHost, st));
  }
  SS_HIP(hipStreamSynchronize(st));  // the pair list and the staging buffers are released on return
  return SS_OK;
}

}  // namespace ss

// ==================================================================== extern "C"
using namespace ss;

// Locking.  The process-wide context (device, stream) is read by every entry point and changed only by ss_init /
// ss_shutdown / ss_set_stream / ss_reset_stream: those take the context lock exclusively, everything else shares it.
// Work on a handle additionally holds that handle's own lock (HandleHead::mu).  Timings, the kernel-path note and
// the error message are per host thread.  So calls from several host threads / Julia tasks on different handles
// run concurrently (their kernels interleave on the library stream), calls on one handle are serialised.
static std::shared_mutex& ctx_mutex() {
  static std::shared_mutex m;
  return m;
}
// HIP's current device is per host thread: a thread that never called ss_init still has to launch on the library's
static inline void bind_device() {
  if (ctx().inited) {
    int cur = -1;
    if (hipGetDevice(&cur) != hipSuccess || cur != ctx().device) (void)hipSetDevice(ctx().device);
  }
}
#define SS_API_EXCLUSIVE() std::unique_lock<std::shared_mutex> _ss_ctx_guard(ctx_mutex())
#define SS_API_LOCK()                                             \
  std::shared_lock<std::shared_mutex> _ss_ctx_guard(ctx_mutex()); \
  bind_device()
#define SS_HANDLE_LOCK(h) \
  std::unique_lock<std::mutex> _ss_handle_guard(reinterpret_cast<HandleHead*>(const_cast<void*>(static_cast<const void*>(h)))->mu)

template <class T>
static int jaccard_impl(const T* F, int64_t n, int64_t d, int64_t ld, T* S, int64_t lds_, int mem) {
  SS_TRY(require_init());
  SS_TRY(check_mem(mem));
  if (n < 0 || d < 0 || ld < n || lds_ < n) return fail(SS_EINVAL, "similarity: bad shape / leading dimension");
  if (n == 0) return SS_OK;
  if ((d > 0 && !F) || !S) return fail(SS_EINVAL, "similarity: NULL buffer");
  hipStream_t st = ctx().stream;
  if (mem == SS_MEM_DEVICE) return launch_jaccard<T>(F, n, d, ld, S, lds_);
  DevBuf<T> dF, dS;
  SS_TRY(dF.alloc((size_t)n * (d > 0 ? d : 1)));
  SS_TRY(dS.alloc((size_t)n * n));
  if (d > 0)
    SS_HIP(hipMemcpy2DAsync(dF.p, n * sizeof(T), F, ld * sizeof(T), n * sizeof(T), d, hipMemcpyHostToDevice, st));
  SS_TRY(launch_jaccard<T>(dF.p, n, d, n, dS.p, n));
  SS_HIP(hipMemcpy2DAsync(S, lds_ * sizeof(T), dS.p, n * sizeof(T), n * sizeof(T), n, hipMemcpyDeviceToHost, st));
  SS_HIP(hipStreamSynchronize(st));
  return SS_OK;
}

extern "C" {

static int shutdown_locked();

int ss_version(void) { return SS_VERSION; }

const char* ss_last_error(void) { return last_error().c_str(); }

int ss_device_count(void) {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess) return 0;
  return n;
}

int ss_init(int device) {
  SS_API_EXCLUSIVE();
  Ctx& c = ctx();
  int n = 0;
  hipError_t e = hipGetDeviceCount(&n);
  if (e != hipSuccess || n <= 0) return fail(SS_ENODEV, "no HIP device visible (%s)", hipGetErrorString(e));
  if (device < 0 || device >= n) return fail(SS_EINVAL, "device %d outside 0..%d", device, n - 1);
  if (c.inited && c.device == device) return SS_OK;
  if (c.inited) shutdown_locked();
  SS_HIP(hipSetDevice(device));
  hipDeviceProp_t prop;
  SS_HIP(hipGetDeviceProperties(&prop, device));
  if (strncmp(prop.gcnArchName, "gfx950", 6) != 0)
    return fail(SS_ENODEV, "device %d is %s; this library carries gfx950 code objects only", device, prop.gcnArchName);
  c.num_cu = prop.multiProcessorCount;
  // binary_rows.hip's LDS-path row limit, lowered only (tests drive both paths over the same rows with it)
  c.binary_lds_cols = -1;
  if (env_set("SS_BINARY_LDS_COLS")) c.binary_lds_cols = (int)std::max<int64_t>(0, env_int("SS_BINARY_LDS_COLS", 0));
  c.target_rank_lds = -1;
  if (env_set("SS_TARGET_RANK_LDS")) c.target_rank_lds = (int)std::max<int64_t>(0, env_int("SS_TARGET_RANK_LDS", 0));
  SS_HIP(hipStreamCreateWithFlags(&c.own_stream, hipStreamNonBlocking));
  c.stream = c.own_stream;
  c.device = device;
  c.inited = true;
  return SS_OK;
}

static int shutdown_locked() {
  Ctx& c = ctx();
  if (!c.inited) return SS_OK;
  (void)hipStreamSynchronize(c.stream);
  {
    // the exclusive context lock is held: no other thread is inside an entry point, so every thread's pool is quiescent
    std::lock_guard<std::mutex> lk(timing_reg_mu());
    for (Timing* t : timing_reg()) {
      if (t->generation == c.generation)
        for (hipEvent_t e : t->pool) (void)hipEventDestroy(e);
      t->pool.clear();
      t->spans.clear();
      t->used = 0;
    }
  }
  ++c.generation;  // other threads notice at their next call (their lists are already empty)
  (void)hipStreamDestroy(c.own_stream);
  c.own_stream = nullptr;
  c.stream = nullptr;
  c.inited = false;
  c.device = -1;
  return SS_OK;
}

int ss_shutdown(void) {
  SS_API_EXCLUSIVE();
  return shutdown_locked();
}

int ss_set_stream(void* hip_stream) {
  SS_API_EXCLUSIVE();
  SS_TRY(require_init());
  Ctx& c = ctx();
  SS_HIP(hipStreamSynchronize(c.stream));
  c.stream = reinterpret_cast<hipStream_t>(hip_stream);  // NULL = the null stream
  return SS_OK;
}

int ss_reset_stream(void) {
  SS_API_EXCLUSIVE();
  SS_TRY(require_init());
  Ctx& c = ctx();
  SS_HIP(hipStreamSynchronize(c.stream));
  c.stream = c.own_stream;
  return SS_OK;
}

int ss_synchronize(void) {
  SS_API_LOCK();
  SS_TRY(require_init());
  SS_HIP(hipStreamSynchronize(ctx().stream));
  return SS_OK;
}

int ss_comm_unique_id(char id[128]) {
  SS_API_LOCK();
  return comm_unique_id(id);
}
int ss_comm_init(const char id[128], int rank, int nranks) {
  SS_API_LOCK();
  return comm_init(id, rank, nranks);
}
int ss_comm_destroy(void) {
  SS_API_LOCK();
  return comm_destroy();
}
int ss_comm_info(int* rank, int* nranks) { return comm_info(rank, nranks); }
int ss_gather_rows_f32(const float* local, int64_t ncols, const int64_t* counts, float* full, int root) {
  SS_API_LOCK();
  return gather_rows(local, ncols, counts, full, root, 4);
}
int ss_gather_rows_f64(const double* local, int64_t ncols, const int64_t* counts, double* full, int root) {
  SS_API_LOCK();
  return gather_rows(local, ncols, counts, full, root, 8);
}

int ss_path_last(char* buf, int n) {
  if (!buf || n <= 0) return fail(SS_EINVAL, "ss_path_last: no buffer");
  const std::string& s = path_note();
  const size_t m = s.size() < (size_t)(n - 1) ? s.size() : (size_t)(n - 1);
  memcpy(buf, s.data(), m);
  buf[m] = 0;
  return SS_OK;
}

int ss_timing_hold(int enable) {
  SS_API_LOCK();
  SS_TRY(require_init());
  Timing& t = timing();
  t.hold = false;
  if (enable) {
    timing_begin_call();  // start from zero
    t.hold = true;
  }
  return SS_OK;
}

int ss_timing_last(double* ms, int n) {
  SS_API_LOCK();
  SS_TRY(require_init());
  if (!ms || n <= 0) return fail(SS_EINVAL, "ss_timing_last: bad buffer");
  Timing& t = timing();
  if (t.dirty) {
    SS_HIP(hipStreamSynchronize(ctx().stream));
    for (double& r : t.resolved) r = 0;
    for (const Timing::Span& s : t.spans) {
      float f = 0;
      SS_HIP(hipEventElapsedTime(&f, s.a, s.b));
      t.resolved[s.stage] += f;
    }
    t.resolved[ST_NSPMM] = t.extra[ST_NSPMM];
    t.resolved[ST_NTRANSFER] = t.extra[ST_NTRANSFER];
    t.dirty = false;
  }
  for (int i = 0; i < n && i < 8; ++i) ms[i] = t.resolved[i];
  return SS_OK;
}

int ss_similarity_jaccard_f32(const float* F, int64_t n, int64_t d, int64_t ld, float* S, int64_t lds_, int mem) {
  SS_API_LOCK();
  return jaccard_impl<float>(F, n, d, ld, S, lds_, mem);
}
int ss_similarity_jaccard_f64(const double* F, int64_t n, int64_t d, int64_t ld, double* S, int64_t lds_, int mem) {
  SS_API_LOCK();
  return jaccard_impl<double>(F, n, d, ld, S, lds_, mem);
}

int ss_cutoff_f32(const float* X, int64_t rows, int64_t cols, int64_t ld, float alpha, int weighted, float* out,
                  int64_t ldo, int mem) {
  SS_API_LOCK();
  return cutoff_impl<float>(X, rows, cols, ld, alpha, weighted, out, ldo, mem);
}
int ss_cutoff_f64(const double* X, int64_t rows, int64_t cols, int64_t ld, double alpha, int weighted, double* out,
                  int64_t ldo, int mem) {
  SS_API_LOCK();
  return cutoff_impl<double>(X, rows, cols, ld, alpha, weighted, out, ldo, mem);
}
int ss_row_degree_f32(const float* G, int64_t rows, int64_t cols, int64_t ld, int64_t* deg, int mem) {
  SS_API_LOCK();
  return row_degree_impl<float>(G, rows, cols, ld, deg, mem);
}
int ss_row_degree_f64(const double* G, int64_t rows, int64_t cols, int64_t ld, int64_t* deg, int mem) {
  SS_API_LOCK();
  return row_degree_impl<double>(G, rows, cols, ld, deg, mem);
}
int ss_spread_f32(const float* G, int64_t rows, int64_t cols, int64_t ld, float* W, int64_t ldw, int mem) {
  SS_API_LOCK();
  return spread_impl<float>(G, rows, cols, ld, W, ldw, mem);
}
int ss_spread_f64(const double* G, int64_t rows, int64_t cols, int64_t ld, double* W, int64_t ldw, int mem) {
  SS_API_LOCK();
  return spread_impl<double>(G, rows, cols, ld, W, ldw, mem);
}

int ss_graph_create_csr_f32(int64_t nq, int64_t ns, int64_t nf, int64_t nt, const int64_t* xq_ptr,
                            const int32_t* xq_idx, const float* xq_val, const int64_t* xs_ptr, const int32_t* xs_idx,
                            const float* xs_val, const int64_t* ys_ptr, const int32_t* ys_idx, const float* ys_val,
                            int index_base, int mem, ss_graph** out) {
  SS_API_LOCK();
  return graph_create_csr_impl<float>(nq, ns, nf, nt, xq_ptr, xq_idx, xq_val, xs_ptr, xs_idx, xs_val, ys_ptr, ys_idx,
                                      ys_val, index_base, mem, out);
}
int ss_graph_create_csr_f64(int64_t nq, int64_t ns, int64_t nf, int64_t nt, const int64_t* xq_ptr,
                            const int32_t* xq_idx, const double* xq_val, const int64_t* xs_ptr, const int32_t* xs_idx,
                            const double* xs_val, const int64_t* ys_ptr, const int32_t* ys_idx, const double* ys_val,
                            int index_base, int mem, ss_graph** out) {
  SS_API_LOCK();
  return graph_create_csr_impl<double>(nq, ns, nf, nt, xq_ptr, xq_idx, xq_val, xs_ptr, xs_idx, xs_val, ys_ptr, ys_idx,
                                       ys_val, index_base, mem, out);
}
int ss_graph_create_dense_f32(int64_t nq, int64_t ns, int64_t nf, int64_t nt, const float* Sq, int64_t ldq,
                              const float* Ss, int64_t lds, const float* Y, int64_t ldy, int apply_cutoff, float alpha,
                              int weighted, int mem, ss_graph** out) {
  SS_API_LOCK();
  return graph_create_dense_impl<float>(nq, ns, nf, nt, Sq, ldq, Ss, lds, Y, ldy, apply_cutoff, alpha, weighted, mem,
                                        out);
}
int ss_graph_create_dense_f64(int64_t nq, int64_t ns, int64_t nf, int64_t nt, const double* Sq, int64_t ldq,
                              const double* Ss, int64_t lds, const double* Y, int64_t ldy, int apply_cutoff,
                              double alpha, int weighted, int mem, ss_graph** out) {
  SS_API_LOCK();
  return graph_create_dense_impl<double>(nq, ns, nf, nt, Sq, ldq, Ss, lds, Y, ldy, apply_cutoff, alpha, weighted, mem,
                                         out);
}

int ss_graph_create_general_f32(int64_t n, int64_t nr, int64_t nc, const int64_t* l_ptr, const int32_t* l_idx,
                                const float* l_val, const int64_t* b_ptr, const int32_t* b_idx, const float* b_val,
                                const int64_t* w_ptr, const int32_t* w_idx, const float* w_val, int index_base, int mem,
                                ss_graph** out) {
  SS_API_LOCK();
  return graph_create_general_impl<float>(n, nr, nc, l_ptr, l_idx, l_val, b_ptr, b_idx, b_val, w_ptr, w_idx, w_val,
                                          index_base, mem, out);
}
int ss_graph_create_general_f64(int64_t n, int64_t nr, int64_t nc, const int64_t* l_ptr, const int32_t* l_idx,
                                const double* l_val, const int64_t* b_ptr, const int32_t* b_idx, const double* b_val,
                                const int64_t* w_ptr, const int32_t* w_idx, const double* w_val, int index_base,
                                int mem, ss_graph** out) {
  SS_API_LOCK();
  return graph_create_general_impl<double>(n, nr, nc, l_ptr, l_idx, l_val, b_ptr, b_idx, b_val, w_ptr, w_idx, w_val,
                                           index_base, mem, out);
}

int ss_graph_create_similarity_f32(int64_t nq, int64_t ns, int64_t nt, const float* Sq, int64_t ldq, const float* Ss,
                                   int64_t lds, const int64_t* y_ptr, const int32_t* y_idx, const float* y_val,
                                   int index_base, float alpha, int weighted, int mem, ss_graph** out) {
  SS_API_LOCK();
  return graph_create_similarity_impl<float>(nq, ns, nt, Sq, ldq, Ss, lds, y_ptr, y_idx, y_val, index_base, alpha,
                                             weighted, mem, out);
}
int ss_graph_create_similarity_f64(int64_t nq, int64_t ns, int64_t nt, const double* Sq, int64_t ldq, const double* Ss,
                                   int64_t lds, const int64_t* y_ptr, const int32_t* y_idx, const double* y_val,
                                   int index_base, double alpha, int weighted, int mem, ss_graph** out) {
  SS_API_LOCK();
  return graph_create_similarity_impl<double>(nq, ns, nt, Sq, ldq, Ss, lds, y_ptr, y_idx, y_val, index_base, alpha,
                                              weighted, mem, out);
}

int ss_similarity_tanimoto_csr_f32(const uint64_t* Fa, int64_t na, const uint64_t* Fb, int64_t nb, int64_t nwords,
                                   float alpha, int weighted, int64_t* ptr, int32_t* idx, float* val, int64_t capacity,
                                   int64_t* nnz, int mem) {
  SS_API_LOCK();
  return tanimoto_csr_impl<float>(Fa, na, Fb, nb, nwords, alpha, weighted, ptr, idx, val, capacity, nnz, mem);
}
int ss_similarity_tanimoto_csr_f64(const uint64_t* Fa, int64_t na, const uint64_t* Fb, int64_t nb, int64_t nwords,
                                   double alpha, int weighted, int64_t* ptr, int32_t* idx, double* val, int64_t capacity,
                                   int64_t* nnz, int mem) {
  SS_API_LOCK();
  return tanimoto_csr_impl<double>(Fa, na, Fb, nb, nwords, alpha, weighted, ptr, idx, val, capacity, nnz, mem);
}
int ss_graph_create_fingerprint_f32(int64_t nq, int64_t ns, int64_t nt, int64_t nwords, const uint64_t* Fq,
                                    const uint64_t* Fs, const int64_t* y_ptr, const int32_t* y_idx, const float* y_val,
                                    int index_base, float alpha, int weighted, int mem, ss_graph** out) {
  SS_API_LOCK();
  return graph_create_fingerprint_impl<float>(nq, ns, nt, nwords, Fq, Fs, y_ptr, y_idx, y_val, index_base, alpha,
                                              weighted, mem, out);
}
int ss_graph_create_fingerprint_f64(int64_t nq, int64_t ns, int64_t nt, int64_t nwords, const uint64_t* Fq,
                                    const uint64_t* Fs, const int64_t* y_ptr, const int32_t* y_idx, const double* y_val,
                                    int index_base, double alpha, int weighted, int mem, ss_graph** out) {
  SS_API_LOCK();
  return graph_create_fingerprint_impl<double>(nq, ns, nt, nwords, Fq, Fs, y_ptr, y_idx, y_val, index_base, alpha,
                                               weighted, mem, out);
}

int ss_similarity_jaccard_csr_f32(const float* Fa, int64_t na, int64_t lda, const float* Fb, int64_t nb, int64_t ldb,
                                  int64_t d, float alpha, int weighted, int64_t* ptr, int32_t* idx, float* val,
                                  int64_t capacity, int64_t* nnz, int mem) {
  SS_API_LOCK();
  return jaccard_csr_impl<float>(Fa, na, lda, Fb, nb, ldb, d, alpha, weighted, ptr, idx, val, capacity, nnz, mem);
}
int ss_similarity_jaccard_csr_f64(const double* Fa, int64_t na, int64_t lda, const double* Fb, int64_t nb, int64_t ldb,
                                  int64_t d, double alpha, int weighted, int64_t* ptr, int32_t* idx, double* val,
                                  int64_t capacity, int64_t* nnz, int mem) {
  SS_API_LOCK();
  return jaccard_csr_impl<double>(Fa, na, lda, Fb, nb, ldb, d, alpha, weighted, ptr, idx, val, capacity, nnz, mem);
}
int ss_graph_create_features_f32(int64_t nq, int64_t ns, int64_t nt, int64_t d, const float* Fq, int64_t ldq,
                                 const float* Fs, int64_t lds, const int64_t* y_ptr, const int32_t* y_idx,
                                 const float* y_val, int index_base, float alpha, int weighted, int mem, ss_graph** out) {
  SS_API_LOCK();
  return graph_create_features_impl<float>(nq, ns, nt, d, Fq, ldq, Fs, lds, y_ptr, y_idx, y_val, index_base, alpha,
                                           weighted, mem, out);
}
int ss_graph_create_features_f64(int64_t nq, int64_t ns, int64_t nt, int64_t d, const double* Fq, int64_t ldq,
                                 const double* Fs, int64_t lds, const int64_t* y_ptr, const int32_t* y_idx,
                                 const double* y_val, int index_base, double alpha, int weighted, int mem,
                                 ss_graph** out) {
  SS_API_LOCK();
  return graph_create_features_impl<double>(nq, ns, nt, d, Fq, ldq, Fs, lds, y_ptr, y_idx, y_val, index_base, alpha,
                                            weighted, mem, out);
}

int ss_similarity_dot_csr_f32(const float* Fa, int64_t na, int64_t lda, const float* Fb, int64_t nb, int64_t ldb,
                              int64_t d, int metric, float alpha, int weighted, int64_t* ptr, int32_t* idx, float* val,
                              int64_t capacity, int64_t* nnz, int mem) {
  SS_API_LOCK();
  return dot_csr_impl<float>(Fa, na, lda, Fb, nb, ldb, d, metric, alpha, weighted, ptr, idx, val, capacity, nnz, mem);
}
int ss_similarity_dot_csr_f64(const double* Fa, int64_t na, int64_t lda, const double* Fb, int64_t nb, int64_t ldb,
                              int64_t d, int metric, double alpha, int weighted, int64_t* ptr, int32_t* idx,
                              double* val, int64_t capacity, int64_t* nnz, int mem) {
  SS_API_LOCK();
  return dot_csr_impl<double>(Fa, na, lda, Fb, nb, ldb, d, metric, alpha, weighted, ptr, idx, val, capacity, nnz, mem);
}
int ss_graph_create_vectors_f32(int64_t nq, int64_t ns, int64_t nt, int64_t d, int metric, const float* Fq, int64_t ldq,
                                const float* Fs, int64_t lds, const int64_t* y_ptr, const int32_t* y_idx,
                                const float* y_val, int index_base, float alpha, int weighted, int mem, ss_graph** out) {
  SS_API_LOCK();
  return graph_create_vectors_impl<float>(nq, ns, nt, d, metric, Fq, ldq, Fs, lds, y_ptr, y_idx, y_val, index_base,
                                          alpha, weighted, mem, out);
}
int ss_graph_create_vectors_f64(int64_t nq, int64_t ns, int64_t nt, int64_t d, int metric, const double* Fq,
                                int64_t ldq, const double* Fs, int64_t lds, const int64_t* y_ptr, const int32_t* y_idx,
                                const double* y_val, int index_base, double alpha, int weighted, int mem,
                                ss_graph** out) {
  SS_API_LOCK();
  return graph_create_vectors_impl<double>(nq, ns, nt, d, metric, Fq, ldq, Fs, lds, y_ptr, y_idx, y_val, index_base,
                                           alpha, weighted, mem, out);
}

int ss_cutoff_csr_f32(int64_t rows, int64_t cols, const int64_t* ptr, const int32_t* idx, const float* val,
                      int index_base, float alpha, int weighted, int64_t* optr, int32_t* oidx, float* oval,
                      int64_t capacity, int64_t* nnz, int mem) {
  SS_API_LOCK();
  return cutoff_csr_impl<float>(rows, cols, ptr, idx, val, index_base, alpha, weighted, optr, oidx, oval, capacity, nnz,
                                mem);
}
int ss_cutoff_csr_f64(int64_t rows, int64_t cols, const int64_t* ptr, const int32_t* idx, const double* val,
                      int index_base, double alpha, int weighted, int64_t* optr, int32_t* oidx, double* oval,
                      int64_t capacity, int64_t* nnz, int mem) {
  SS_API_LOCK();
  return cutoff_csr_impl<double>(rows, cols, ptr, idx, val, index_base, alpha, weighted, optr, oidx, oval, capacity, nnz,
                                 mem);
}
int ss_graph_recut_f32(const ss_graph* parent, float alpha, int weighted, ss_graph** out) {
  SS_API_LOCK();
  SS_TRY(require_init());
  if (!parent) return fail(SS_EINVAL, "handle is NULL");
  SS_HANDLE_LOCK(parent);
  return graph_recut_impl<float>(parent, alpha, weighted, out);
}
int ss_graph_recut_f64(const ss_graph* parent, double alpha, int weighted, ss_graph** out) {
  SS_API_LOCK();
  SS_TRY(require_init());
  if (!parent) return fail(SS_EINVAL, "handle is NULL");
  SS_HANDLE_LOCK(parent);
  return graph_recut_impl<double>(parent, alpha, weighted, out);
}
int ss_graph_set_cutoff_f32(ss_graph* g, float alpha, int weighted) {
  SS_API_LOCK();
  SS_TRY(require_init());
  if (!g) return fail(SS_EINVAL, "handle is NULL");
  SS_HANDLE_LOCK(g);
  return graph_set_cutoff_impl<float>(g, alpha, weighted);
}
int ss_graph_set_cutoff_f64(ss_graph* g, double alpha, int weighted) {
  SS_API_LOCK();
  SS_TRY(require_init());
  if (!g) return fail(SS_EINVAL, "handle is NULL");
  SS_HANDLE_LOCK(g);
  return graph_set_cutoff_impl<double>(g, alpha, weighted);
}

int ss_graph_destroy(ss_graph* h) {
  SS_API_LOCK();
  if (!h) return SS_OK;
  const int dtype = *reinterpret_cast<int*>(h);
  if (dtype != 4 && dtype != 8) return fail(SS_EINVAL, "not a graph handle");
  {  // wait for a call that still works on the handle (the caller must not start new ones), then for the device
    SS_HANDLE_LOCK(h);
    if (ctx().inited) (void)hipStreamSynchronize(ctx().stream);
  }
  if (dtype == 4) delete reinterpret_cast<GraphBox<float>*>(h);
  else if (dtype == 8) delete reinterpret_cast<GraphBox<double>*>(h);
  else return fail(SS_EINVAL, "not a graph handle");
  return SS_OK;
}

int ss_graph_info(const ss_graph* h, int64_t sizes[7]) {
  SS_API_LOCK();
  if (!h) return fail(SS_EINVAL, "handle is NULL");
  SS_HANDLE_LOCK(h);
  if (!h || !sizes) return fail(SS_EINVAL, "NULL argument");
  const int dtype = *reinterpret_cast<const int*>(h);
  auto fill = [&](auto* b) {
    sizes[0] = b->g.nq; sizes[1] = b->g.ns; sizes[2] = b->g.nf; sizes[3] = b->g.nt;
    // a general graph holds B and the asked-for columns only as the transposed operands XsT and YsT
    sizes[4] = b->g.Xq.nnz;
    sizes[5] = b->g.general ? b->g.XsT.nnz : b->g.Xs.nnz;
    sizes[6] = b->g.general ? b->g.YsT.nnz : b->g.Ys.nnz;
  };
  if (dtype == 4) fill(reinterpret_cast<const GraphBox<float>*>(h));
  else if (dtype == 8) fill(reinterpret_cast<const GraphBox<double>*>(h));
  else return fail(SS_EINVAL, "not a graph handle");
  return SS_OK;
}

int ss_graph_degrees(const ss_graph* h, int64_t* kf, int64_t* ks, int64_t* kt) {
  SS_API_LOCK();
  if (!h) return fail(SS_EINVAL, "handle is NULL");
  SS_HANDLE_LOCK(h);
  SS_TRY(require_init());
  if (!h) return fail(SS_EINVAL, "graph handle is NULL");
  const int dtype = *reinterpret_cast<const int*>(h);
  auto pull = [&](const DevBuf<int>& d, int64_t n, int64_t* out) -> int {
    if (!out || n == 0) return SS_OK;
    std::vector<int> tmp(n);
    SS_HIP(hipMemcpyAsync(tmp.data(), d.p, n * sizeof(int), hipMemcpyDeviceToHost, ctx().stream));
    SS_HIP(hipStreamSynchronize(ctx().stream));
    for (int64_t i = 0; i < n; ++i) out[i] = tmp[i];
    return SS_OK;
  };
  auto run = [&](auto* b) -> int {
    SS_TRY(pull(b->g.kf, b->g.nf, kf));
    SS_TRY(pull(b->g.ks, b->g.ns, ks));
    SS_TRY(pull(b->g.kt, b->g.nt, kt));
    return SS_OK;
  };
  if (dtype == 4) return run(reinterpret_cast<const GraphBox<float>*>(h));
  if (dtype == 8) return run(reinterpret_cast<const GraphBox<double>*>(h));
  return fail(SS_EINVAL, "not a graph handle");
}

int ss_predict_f32(ss_graph* g, int rows_kind, int64_t row_begin, int64_t row_end, int clean, float* out, int64_t ld,
                   int layout, int mem) {
  SS_API_LOCK();
  if (!g) return fail(SS_EINVAL, "handle is NULL");
  SS_HANDLE_LOCK(g);
  if (rows_kind != SS_ROWS_QUERY && rows_kind != SS_ROWS_SOURCE) return fail(SS_EINVAL, "bad rows_kind");
  return predict_impl<float>(g, rows_kind, row_begin, row_end, clean, out, ld, layout, mem);
}
int ss_predict_f64(ss_graph* g, int rows_kind, int64_t row_begin, int64_t row_end, int clean, double* out, int64_t ld,
                   int layout, int mem) {
  SS_API_LOCK();
  if (!g) return fail(SS_EINVAL, "handle is NULL");
  SS_HANDLE_LOCK(g);
  if (rows_kind != SS_ROWS_QUERY && rows_kind != SS_ROWS_SOURCE) return fail(SS_EINVAL, "bad rows_kind");
  return predict_impl<double>(g, rows_kind, row_begin, row_end, clean, out, ld, layout, mem);
}
int ss_predict_loo_f32(ss_graph* g, int64_t i_begin, int64_t i_end, int clean, float* out, int64_t ld, int layout,
                       int mem) {
  SS_API_LOCK();
  if (!g) return fail(SS_EINVAL, "handle is NULL");
  SS_HANDLE_LOCK(g);
  return predict_impl<float>(g, 2, i_begin, i_end, clean, out, ld, layout, mem);
}
int ss_predict_loo_f64(ss_graph* g, int64_t i_begin, int64_t i_end, int clean, double* out, int64_t ld, int layout,
                       int mem) {
  SS_API_LOCK();
  if (!g) return fail(SS_EINVAL, "handle is NULL");
  SS_HANDLE_LOCK(g);
  return predict_impl<double>(g, 2, i_begin, i_end, clean, out, ld, layout, mem);
}

// a graph and a query set: the graph's lock first, always
#define SS_QUERIES_LOCK(q) \
  std::unique_lock<std::mutex> _ss_queries_guard(reinterpret_cast<HandleHead*>(const_cast<ss_queries*>(q))->mu)

int ss_queries_create_csr_f32(const ss_graph* g, int64_t nq, const int64_t* ptr, const int32_t* idx, const float* val,
                              int index_base, int mem, ss_queries** out) {
  SS_API_LOCK();
  if (!g) return fail(SS_EINVAL, "handle is NULL");
  SS_HANDLE_LOCK(g);
  return queries_create_csr_impl<float>(g, nq, ptr, idx, val, index_base, mem, out);
}
int ss_queries_create_csr_f64(const ss_graph* g, int64_t nq, const int64_t* ptr, const int32_t* idx, const double* val,
                              int index_base, int mem, ss_queries** out) {
  SS_API_LOCK();
  if (!g) return fail(SS_EINVAL, "handle is NULL");
  SS_HANDLE_LOCK(g);
  return queries_create_csr_impl<double>(g, nq, ptr, idx, val, index_base, mem, out);
}
int ss_similarity_tanimoto_kth_f32(const uint64_t* Fa, int64_t na, const uint64_t* Fb, int64_t nb, int64_t nwords, int k,
                                   float* tau, int mem) {
  SS_API_LOCK();
  return tanimoto_kth_impl<float>(Fa, na, Fb, nb, nwords, k, tau, mem);
}
int ss_similarity_tanimoto_floor_csr_f32(const uint64_t* Fa, int64_t na, const uint64_t* Fb, int64_t nb, int64_t nwords,
                                         float alpha, int k, int weighted, int64_t* ptr, int32_t* idx, float* val,
                                         int64_t capacity, int64_t* nnz, int mem) {
  SS_API_LOCK();
  SS_TRY(check_floor<float>(k, alpha));
  return tanimoto_csr_impl<float>(Fa, na, Fb, nb, nwords, alpha, weighted, ptr, idx, val, capacity, nnz, mem, k);
}
int ss_graph_create_fingerprint_floor_f32(int64_t nq, int64_t ns, int64_t nt, int64_t nwords, const uint64_t* Fq,
                                          const uint64_t* Fs, const int64_t* y_ptr, const int32_t* y_idx,
                                          const float* y_val, int index_base, float alpha, int k, int weighted, int mem,
                                          ss_graph** out) {
  SS_API_LOCK();
  if (out) *out = nullptr;
  SS_TRY(check_floor<float>(k, alpha));
  return graph_create_fingerprint_impl<float>(nq, ns, nt, nwords, Fq, Fs, y_ptr, y_idx, y_val, index_base, alpha,
                                            weighted, mem, out, k);
}
int ss_queries_create_fingerprint_floor_f32(const ss_graph* g, int64_t nq, int64_t ns, int64_t nwords,
                                            const uint64_t* Fq, const uint64_t* Fs, float alpha, int k, int weighted,
                                            int mem, ss_queries** out) {
  SS_API_LOCK();
  if (out) *out = nullptr;
  if (!g) return fail(SS_EINVAL, "handle is NULL");
  SS_HANDLE_LOCK(g);
  SS_TRY(check_floor<float>(k, alpha));
  return queries_create_fingerprint_impl<float>(g, nq, ns, nwords, Fq, Fs, alpha, weighted, mem, out, k);
}
int ss_similarity_tanimoto_kth_f64(const uint64_t* Fa, int64_t na, const uint64_t* Fb, int64_t nb, int64_t nwords, int k,
                                   double* tau, int mem) {
  SS_API_LOCK();
  return tanimoto_kth_impl<double>(Fa, na, Fb, nb, nwords, k, tau, mem);
}
int ss_similarity_tanimoto_floor_csr_f64(const uint64_t* Fa, int64_t na, const uint64_t* Fb, int64_t nb, int64_t nwords,
                                         double alpha, int k, int weighted, int64_t* ptr, int32_t* idx, double* val,
                                         int64_t capacity, int64_t* nnz, int mem) {
  SS_API_LOCK();
  SS_TRY(check_floor<double>(k, alpha));
  return tanimoto_csr_impl<double>(Fa, na, Fb, nb, nwords, alpha, weighted, ptr, idx, val, capacity, nnz, mem, k);
}
int ss_graph_create_fingerprint_floor_f64(int64_t nq, int64_t ns, int64_t nt, int64_t nwords, const uint64_t* Fq,
                                          const uint64_t* Fs, const int64_t* y_ptr, const int32_t* y_idx,
                                          const double* y_val, int index_base, double alpha, int k, int weighted, int mem,
                                          ss_graph** out) {
  SS_API_LOCK();
  if (out) *out = nullptr;
  SS_TRY(check_floor<double>(k, alpha));
  return graph_create_fingerprint_impl<double>(nq, ns, nt, nwords, Fq, Fs, y_ptr, y_idx, y_val, index_base, alpha,
                                            weighted, mem, out, k);
}
int ss_queries_create_fingerprint_floor_f64(const ss_graph* g, int64_t nq, int64_t ns, int64_t nwords,
                                            const uint64_t* Fq, const uint64_t* Fs, double alpha, int k, int weighted,
                                            int mem, ss_queries** out) {
  SS_API_LOCK();
  if (out) *out = nullptr;
  if (!g) return fail(SS_EINVAL, "handle is NULL");
  SS_HANDLE_LOCK(g);
  SS_TRY(check_floor<double>(k, alpha));
  return queries_create_fingerprint_impl<double>(g, nq, ns, nwords, Fq, Fs, alpha, weighted, mem, out, k);
}
int ss_queries_create_fingerprint_f32(const ss_graph* g, int64_t nq, int64_t ns, int64_t nwords, const uint64_t* Fq,
                                      const uint64_t* Fs, float alpha, int weighted, int mem, ss_queries** out) {
  SS_API_LOCK();
  if (!g) return fail(SS_EINVAL, "handle is NULL");
  SS_HANDLE_LOCK(g);
  return queries_create_fingerprint_impl<float>(g, nq, ns, nwords, Fq, Fs, alpha, weighted, mem, out);
}
int ss_queries_create_fingerprint_f64(const ss_graph* g, int64_t nq, int64_t ns, int64_t nwords, const uint64_t* Fq,
                                      const uint64_t* Fs, double alpha, int weighted, int mem, ss_queries** out) {
  SS_API_LOCK();
  if (!g) return fail(SS_EINVAL, "handle is NULL");
  SS_HANDLE_LOCK(g);
  return queries_create_fingerprint_impl<double>(g, nq, ns, nwords, Fq, Fs, alpha, weighted, mem, out);
}
int ss_queries_create_features_f32(const ss_graph* g, int64_t nq, int64_t ns, int64_t d, const float* Fq, int64_t ldq,
                                   const float* Fs, int64_t lds, float alpha, int weighted, int mem, ss_queries** out) {
  SS_API_LOCK();
  if (!g) return fail(SS_EINVAL, "handle is NULL");
  SS_HANDLE_LOCK(g);
  return features_queries_impl<float, JaccardCsr<float>>(jaccard_names, no_check, jaccard_count<float>(d, alpha, weighted),
                                                         g, nq, ns, d, Fq, ldq, Fs, lds, alpha, mem, out);
}
int ss_queries_create_features_f64(const ss_graph* g, int64_t nq, int64_t ns, int64_t d, const double* Fq, int64_t ldq,
                                   const double* Fs, int64_t lds, double alpha, int weighted, int mem,
                                   ss_queries** out) {
  SS_API_LOCK();
  if (!g) return fail(SS_EINVAL, "handle is NULL");
  SS_HANDLE_LOCK(g);
  return features_queries_impl<double, JaccardCsr<double>>(jaccard_names, no_check,
                                                           jaccard_count<double>(d, alpha, weighted), g, nq, ns, d, Fq,
                                                           ldq, Fs, lds, alpha, mem, out);
}
int ss_queries_create_vectors_f32(const ss_graph* g, int64_t nq, int64_t ns, int64_t d, int metric, const float* Fq,
                                  int64_t ldq, const float* Fs, int64_t lds, float alpha, int weighted, int mem,
                                  ss_queries** out) {
  SS_API_LOCK();
  if (!g) return fail(SS_EINVAL, "handle is NULL");
  SS_HANDLE_LOCK(g);
  return features_queries_impl<float, DotCsr<float>>(
      dot_names, [=] { return check_sim_metric(metric); }, dot_count<float>(d, metric, alpha, weighted), g, nq, ns, d, Fq,
      ldq, Fs, lds, alpha, mem, out);
}
int ss_queries_create_vectors_f64(const ss_graph* g, int64_t nq, int64_t ns, int64_t d, int metric, const double* Fq,
                                  int64_t ldq, const double* Fs, int64_t lds, double alpha, int weighted, int mem,
                                  ss_queries** out) {
  SS_API_LOCK();
  if (!g) return fail(SS_EINVAL, "handle is NULL");
  SS_HANDLE_LOCK(g);
  return features_queries_impl<double, DotCsr<double>>(
      dot_names, [=] { return check_sim_metric(metric); }, dot_count<double>(d, metric, alpha, weighted), g, nq, ns, d,
      Fq, ldq, Fs, lds, alpha, mem, out);
}

// ---- include/simspread_hip_neighbours_real.h: the neighbour floor of the weighted-Jaccard and inner-product producers
int ss_similarity_jaccard_kth_f32(const float* Fa, int64_t na, int64_t lda, const float* Fb, int64_t nb, int64_t ldb,
                                  int64_t d, int k, float* tau, int mem) {
  SS_API_LOCK();
  return jaccard_kth_impl<float>(Fa, na, lda, Fb, nb, ldb, d, k, tau, mem);
}
int ss_similarity_jaccard_floor_csr_f32(const float* Fa, int64_t na, int64_t lda, const float* Fb, int64_t nb, int64_t ldb,
                                        int64_t d, float alpha, int k, int weighted, int64_t* ptr, int32_t* idx, float* val,
                                        int64_t capacity, int64_t* nnz, int mem) {
  SS_API_LOCK();
  SS_TRY(check_floor<float>(k, alpha));
  return jaccard_csr_impl<float>(Fa, na, lda, Fb, nb, ldb, d, alpha, weighted, ptr, idx, val, capacity, nnz, mem, k);
}
int ss_similarity_dot_kth_f32(const float* Fa, int64_t na, int64_t lda, const float* Fb, int64_t nb, int64_t ldb, int64_t d,
                              int metric, int k, float* tau, int mem) {
  SS_API_LOCK();
  return dot_kth_impl<float>(Fa, na, lda, Fb, nb, ldb, d, metric, k, tau, mem);
}
int ss_similarity_dot_floor_csr_f32(const float* Fa, int64_t na, int64_t lda, const float* Fb, int64_t nb, int64_t ldb,
                                    int64_t d, int metric, float alpha, int k, int weighted, int64_t* ptr, int32_t* idx,
                                    float* val, int64_t capacity, int64_t* nnz, int mem) {
  SS_API_LOCK();
  SS_TRY(check_floor<float>(k, alpha));
  return dot_csr_impl<float>(Fa, na, lda, Fb, nb, ldb, d, metric, alpha, weighted, ptr, idx, val, capacity, nnz, mem, k);
}
int ss_graph_create_features_floor_f32(int64_t nq, int64_t ns, int64_t nt, int64_t d, const float* Fq, int64_t ldq,
                                       const float* Fs, int64_t lds, const int64_t* y_ptr, const int32_t* y_idx,
                                       const float* y_val, int index_base, float alpha, int k, int weighted, int mem,
                                       ss_graph** out) {
  SS_API_LOCK();
  if (out) *out = nullptr;
  SS_TRY(check_floor<float>(k, alpha));
  return graph_create_features_impl<float>(nq, ns, nt, d, Fq, ldq, Fs, lds, y_ptr, y_idx, y_val, index_base, alpha, weighted,
                                       mem, out, k);
}
int ss_graph_create_vectors_floor_f32(int64_t nq, int64_t ns, int64_t nt, int64_t d, int metric, const float* Fq,
                                      int64_t ldq, const float* Fs, int64_t lds, const int64_t* y_ptr, const int32_t* y_idx,
                                      const float* y_val, int index_base, float alpha, int k, int weighted, int mem,
                                      ss_graph** out) {
  SS_API_LOCK();
  if (out) *out = nullptr;
  SS_TRY(check_floor<float>(k, alpha));
  return graph_create_vectors_impl<float>(nq, ns, nt, d, metric, Fq, ldq, Fs, lds, y_ptr, y_idx, y_val, index_base, alpha,
                                      weighted, mem, out, k);
}
int ss_queries_create_features_floor_f32(const ss_graph* g, int64_t nq, int64_t ns, int64_t d, const float* Fq,
                                         int64_t ldq, const float* Fs, int64_t lds, float alpha, int k, int weighted, int mem,
                                         ss_queries** out) {
  SS_API_LOCK();
  if (out) *out = nullptr;
  if (!g) return fail(SS_EINVAL, "handle is NULL");
  SS_HANDLE_LOCK(g);
  SS_TRY(check_floor<float>(k, alpha));
  return features_queries_impl<float, JaccardCsr<float>>(jaccard_names, no_check, jaccard_count<float>(d, alpha, weighted, k), g,
                                                   nq, ns, d, Fq, ldq, Fs, lds, alpha, mem, out, k);
}
int ss_queries_create_vectors_floor_f32(const ss_graph* g, int64_t nq, int64_t ns, int64_t d, int metric,
                                        const float* Fq, int64_t ldq, const float* Fs, int64_t lds, float alpha, int k,
                                        int weighted, int mem, ss_queries** out) {
  SS_API_LOCK();
  if (out) *out = nullptr;
  if (!g) return fail(SS_EINVAL, "handle is NULL");
  SS_HANDLE_LOCK(g);
  SS_TRY(check_floor<float>(k, alpha));
  return features_queries_impl<float, DotCsr<float>>(
      dot_names, [=] { return check_sim_metric(metric); }, dot_count<float>(d, metric, alpha, weighted, k), g, nq, ns, d, Fq,
      ldq, Fs, lds, alpha, mem, out, k);
}
// ---- include/simspread_hip_neighbours_real.h: the neighbour floor of the weighted-Jaccard and inner-product producers
int ss_similarity_jaccard_kth_f64(const double* Fa, int64_t na, int64_t lda, const double* Fb, int64_t nb, int64_t ldb,
                                  int64_t d, int k, double* tau, int mem) {
  SS_API_LOCK();
  return jaccard_kth_impl<double>(Fa, na, lda, Fb, nb, ldb, d, k, tau, mem);
}
int ss_similarity_jaccard_floor_csr_f64(const double* Fa, int64_t na, int64_t lda, const double* Fb, int64_t nb, int64_t ldb,
                                        int64_t d, double alpha, int k, int weighted, int64_t* ptr, int32_t* idx, double* val,
                                        int64_t capacity, int64_t* nnz, int mem) {
  SS_API_LOCK();
  SS_TRY(check_floor<double>(k, alpha));
  return jaccard_csr_impl<double>(Fa, na, lda, Fb, nb, ldb, d, alpha, weighted, ptr, idx, val, capacity, nnz, mem, k);
}
int ss_similarity_dot_kth_f64(const double* Fa, int64_t na, int64_t lda, const double* Fb, int64_t nb, int64_t ldb, int64_t d,
                              int metric, int k, double* tau, int mem) {
  SS_API_LOCK();
  return dot_kth_impl<double>(Fa, na, lda, Fb, nb, ldb, d, metric, k, tau, mem);
}
int ss_similarity_dot_floor_csr_f64(const double* Fa, int64_t na, int64_t lda, const double* Fb, int64_t nb, int64_t ldb,
                                    int64_t d, int metric, double alpha, int k, int weighted, int64_t* ptr, int32_t* idx,
                                    double* val, int64_t capacity, int64_t* nnz, int mem) {
  SS_API_LOCK();
  SS_TRY(check_floor<double>(k, alpha));
  return dot_csr_impl<double>(Fa, na, lda, Fb, nb, ldb, d, metric, alpha, weighted, ptr, idx, val, capacity, nnz, mem, k);
}
int ss_graph_create_features_floor_f64(int64_t nq, int64_t ns, int64_t nt, int64_t d, const double* Fq, int64_t ldq,
                                       const double* Fs, int64_t lds, const int64_t* y_ptr, const int32_t* y_idx,
                                       const double* y_val, int index_base, double alpha, int k, int weighted, int mem,
                                       ss_graph** out) {
  SS_API_LOCK();
  if (out) *out = nullptr;
  SS_TRY(check_floor<double>(k, alpha));
  return graph_create_features_impl<double>(nq, ns, nt, d, Fq, ldq, Fs, lds, y_ptr, y_idx, y_val, index_base, alpha, weighted,
                                       mem, out, k);
}
int ss_graph_create_vectors_floor_f64(int64_t nq, int64_t ns, int64_t nt, int64_t d, int metric, const double* Fq,
                                      int64_t ldq, const double* Fs, int64_t lds, const int64_t* y_ptr, const int32_t* y_idx,
                                      const double* y_val, int index_base, double alpha, int k, int weighted, int mem,
                                      ss_graph** out) {
  SS_API_LOCK();
  if (out) *out = nullptr;
  SS_TRY(check_floor<double>(k, alpha));
  return graph_create_vectors_impl<double>(nq, ns, nt, d, metric, Fq, ldq, Fs, lds, y_ptr, y_idx, y_val, index_base, alpha,
                                      weighted, mem, out, k);
}
int ss_queries_create_features_floor_f64(const ss_graph* g, int64_t nq, int64_t ns, int64_t d, const double* Fq,
                                         int64_t ldq, const double* Fs, int64_t lds, double alpha, int k, int weighted, int mem,
                                         ss_queries** out) {
  SS_API_LOCK();
  if (out) *out = nullptr;
  if (!g) return fail(SS_EINVAL, "handle is NULL");
  SS_HANDLE_LOCK(g);
  SS_TRY(check_floor<double>(k, alpha));
  return features_queries_impl<double, JaccardCsr<double>>(jaccard_names, no_check, jaccard_count<double>(d, alpha, weighted, k), g,
                                                   nq, ns, d, Fq, ldq, Fs, lds, alpha, mem, out, k);
}
int ss_queries_create_vectors_floor_f64(const ss_graph* g, int64_t nq, int64_t ns, int64_t d, int metric,
                                        const double* Fq, int64_t ldq, const double* Fs, int64_t lds, double alpha, int k,
                                        int weighted, int mem, ss_queries** out) {
  SS_API_LOCK();
  if (out) *out = nullptr;
  if (!g) return fail(SS_EINVAL, "handle is NULL");
  SS_HANDLE_LOCK(g);
  SS_TRY(check_floor<double>(k, alpha));
  return features_queries_impl<double, DotCsr<double>>(
      dot_names, [=] { return check_sim_metric(metric); }, dot_count<double>(d, metric, alpha, weighted, k), g, nq, ns, d, Fq,
      ldq, Fs, lds, alpha, mem, out, k);
}

int ss_queries_destroy(ss_queries* q) {
  SS_API_LOCK();
  if (!q) return SS_OK;
  const int dtype = *reinterpret_cast<int*>(q);
  if (dtype != 4 && dtype != 8) return fail(SS_EINVAL, "not a query-set handle");
  {  // wait for a call that still works on the handle, then for the device (a prediction may still read the block)
    SS_QUERIES_LOCK(q);
    if (ctx().inited) (void)hipStreamSynchronize(ctx().stream);
  }
  if (dtype == 4) delete reinterpret_cast<QueriesBox<float>*>(q);
  else delete reinterpret_cast<QueriesBox<double>*>(q);
  return SS_OK;
}

int ss_queries_info(const ss_queries* q, int64_t sizes[3]) {
  SS_API_LOCK();
  if (!q || !sizes) return fail(SS_EINVAL, "NULL argument");
  SS_QUERIES_LOCK(q);
  const int dtype = *reinterpret_cast<const int*>(q);
  auto fill = [&](auto* b) { sizes[0] = b->Xq.rows; sizes[1] = b->Xq.cols; sizes[2] = b->Xq.nnz; };
  if (dtype == 4) fill(reinterpret_cast<const QueriesBox<float>*>(q));
  else if (dtype == 8) fill(reinterpret_cast<const QueriesBox<double>*>(q));
  else return fail(SS_EINVAL, "not a query-set handle");
  return SS_OK;
}

int ss_queries_degrees(const ss_queries* q, int64_t* kq, int mem) {
  SS_API_LOCK();
  if (!q) return fail(SS_EINVAL, "handle is NULL");
  SS_QUERIES_LOCK(q);
  const int dtype = *reinterpret_cast<const int*>(q);
  if (dtype == 4) return queries_degrees_impl<float>(q, kq, mem);
  if (dtype == 8) return queries_degrees_impl<double>(q, kq, mem);
  return fail(SS_EINVAL, "not a query-set handle");
}

int ss_predict_queries_f32(ss_graph* g, const ss_queries* q, int64_t row_begin, int64_t row_end, int clean, float* out,
                           int64_t ld, int layout, int mem) {
  SS_API_LOCK();
  if (!g || !q) return fail(SS_EINVAL, "handle is NULL");
  SS_HANDLE_LOCK(g);
  SS_QUERIES_LOCK(q);
  return predict_impl<float>(g, SS_ROWS_QUERY, row_begin, row_end, clean, out, ld, layout, mem, q);
}
int ss_predict_queries_f64(ss_graph* g, const ss_queries* q, int64_t row_begin, int64_t row_end, int clean, double* out,
                           int64_t ld, int layout, int mem) {
  SS_API_LOCK();
  if (!g || !q) return fail(SS_EINVAL, "handle is NULL");
  SS_HANDLE_LOCK(g);
  SS_QUERIES_LOCK(q);
  return predict_impl<double>(g, SS_ROWS_QUERY, row_begin, row_end, clean, out, ld, layout, mem, q);
}

int ss_support_f32(ss_graph* g, const ss_queries* q, int rows_kind, int64_t npairs, const int64_t* rows,
                   const int32_t* targets, int M, int32_t* src, float* contrib, int32_t* nsupp, int mem) {
  SS_API_LOCK();
  if (!g) return fail(SS_EINVAL, "handle is NULL");
  SS_HANDLE_LOCK(g);
  std::unique_lock<std::mutex> _ss_queries_guard;
  if (q) _ss_queries_guard = std::unique_lock<std::mutex>(reinterpret_cast<HandleHead*>(const_cast<ss_queries*>(q))->mu);
  return support_impl<float>(g, q, rows_kind, npairs, rows, targets, M, src, contrib, nsupp, mem);
}
int ss_support_f64(ss_graph* g, const ss_queries* q, int rows_kind, int64_t npairs, const int64_t* rows,
                   const int32_t* targets, int M, int32_t* src, double* contrib, int32_t* nsupp, int mem) {
  SS_API_LOCK();
  if (!g) return fail(SS_EINVAL, "handle is NULL");
  SS_HANDLE_LOCK(g);
  std::unique_lock<std::mutex> _ss_queries_guard;
  if (q) _ss_queries_guard = std::unique_lock<std::mutex>(reinterpret_cast<HandleHead*>(const_cast<ss_queries*>(q))->mu);
  return support_impl<double>(g, q, rows_kind, npairs, rows, targets, M, src, contrib, nsupp, mem);
}

int ss_predict_kfold_f32(ss_graph* g, const int32_t* fold_of_source, int nfolds, int clean, float* out, int64_t ld,
                         int layout, int mem) {
  SS_API_LOCK();
  if (!g) return fail(SS_EINVAL, "handle is NULL");
  SS_HANDLE_LOCK(g);
  return predict_kfold_impl<float>(g, fold_of_source, nfolds, clean, out, ld, layout, mem);
}
int ss_predict_kfold_f64(ss_graph* g, const int32_t* fold_of_source, int nfolds, int clean, double* out, int64_t ld,
                         int layout, int mem) {
  SS_API_LOCK();
  if (!g) return fail(SS_EINVAL, "handle is NULL");
  SS_HANDLE_LOCK(g);
  return predict_kfold_impl<double>(g, fold_of_source, nfolds, clean, out, ld, layout, mem);
}

int ss_predict_kfold_rows_f32(ss_graph* g, const int32_t* fold_of_source, int nfolds, int64_t i_begin, int64_t i_end,
                              int clean, float* out, int64_t ld, int layout, int mem) {
  SS_API_LOCK();
  if (!g) return fail(SS_EINVAL, "handle is NULL");
  SS_HANDLE_LOCK(g);
  return predict_kfold_rows_impl<float>(g, fold_of_source, nfolds, i_begin, i_end, clean, out, ld, layout, mem);
}
int ss_predict_kfold_rows_f64(ss_graph* g, const int32_t* fold_of_source, int nfolds, int64_t i_begin, int64_t i_end,
                              int clean, double* out, int64_t ld, int layout, int mem) {
  SS_API_LOCK();
  if (!g) return fail(SS_EINVAL, "handle is NULL");
  SS_HANDLE_LOCK(g);
  return predict_kfold_rows_impl<double>(g, fold_of_source, nfolds, i_begin, i_end, clean, out, ld, layout, mem);
}
int ss_evaluate_kfold_f32(ss_graph* g, const int32_t* fold_of_source, int nfolds, int64_t i_begin, int64_t i_end,
                          int clean, double alpha, int L, int64_t block_rows, double* out, int mem) {
  SS_API_LOCK();
  if (!g) return fail(SS_EINVAL, "handle is NULL");
  SS_HANDLE_LOCK(g);
  return evaluate_kfold_impl<float>(g, fold_of_source, nfolds, i_begin, i_end, clean, false, alpha, L, block_rows, out, mem);
}
int ss_evaluate_kfold_f64(ss_graph* g, const int32_t* fold_of_source, int nfolds, int64_t i_begin, int64_t i_end,
                          int clean, double alpha, int L, int64_t block_rows, double* out, int mem) {
  SS_API_LOCK();
  if (!g) return fail(SS_EINVAL, "handle is NULL");
  SS_HANDLE_LOCK(g);
  return evaluate_kfold_impl<double>(g, fold_of_source, nfolds, i_begin, i_end, clean, false, alpha, L, block_rows, out, mem);
}
int ss_evaluate_kfold_binary_f32(ss_graph* g, const int32_t* fold_of_source, int nfolds, int64_t i_begin,
                                 int64_t i_end, int clean, int64_t block_rows, double* out, int mem) {
  SS_API_LOCK();
  if (!g) return fail(SS_EINVAL, "handle is NULL");
  SS_HANDLE_LOCK(g);
  return evaluate_kfold_impl<float>(g, fold_of_source, nfolds, i_begin, i_end, clean, true, 0.0, 0, block_rows, out, mem);
}
int ss_evaluate_kfold_binary_f64(ss_graph* g, const int32_t* fold_of_source, int nfolds, int64_t i_begin,
                                 int64_t i_end, int clean, int64_t block_rows, double* out, int mem) {
  SS_API_LOCK();
  if (!g) return fail(SS_EINVAL, "handle is NULL");
  SS_HANDLE_LOCK(g);
  return evaluate_kfold_impl<double>(g, fold_of_source, nfolds, i_begin, i_end, clean, true, 0.0, 0, block_rows, out, mem);
}

int ss_topl_f32(const float* scores, int64_t nrows, int64_t ncols, int64_t ld, int L, int32_t* idx, float* val,
                int mem) {
  SS_API_LOCK();
  SS_TRY(require_init());
  SS_TRY(check_mem(mem));
  if (nrows < 0 || ncols < 0 || ld < ncols) return fail(SS_EINVAL, "top-L: bad shape / leading dimension");
  if (nrows == 0) return SS_OK;
  if (!scores || !idx || !val) return fail(SS_EINVAL, "top-L: NULL buffer");
  hipStream_t st = ctx().stream;
  if (mem == SS_MEM_DEVICE) return launch_topl(scores, nrows, ncols, ld, L, idx, val);
  DevBuf<float> ds, dv;
  DevBuf<int> di;
  SS_TRY(ds.alloc((size_t)nrows * ncols));
  SS_TRY(dv.alloc((size_t)nrows * L));
  SS_TRY(di.alloc((size_t)nrows * L));
  SS_HIP(hipMemcpy2DAsync(ds.p, ncols * sizeof(float), scores, ld * sizeof(float), ncols * sizeof(float), nrows,
                          hipMemcpyHostToDevice, st));
  SS_TRY(launch_topl(ds.p, nrows, ncols, ncols, L, di.p, dv.p));
  SS_HIP(hipMemcpyAsync(idx, di.p, (size_t)nrows * L * sizeof(int), hipMemcpyDeviceToHost, st));
  SS_HIP(hipMemcpyAsync(val, dv.p, (size_t)nrows * L * sizeof(float), hipMemcpyDeviceToHost, st));
  SS_HIP(hipStreamSynchronize(st));
  return SS_OK;
}

int ss_rank_metrics_f32(const uint8_t* y, const float* yhat, int64_t n, double alpha, double out[4], int mem) {
  SS_API_LOCK();
  SS_TRY(require_init());
  SS_TRY(check_mem(mem));
  if (n <= 0) return fail(SS_EINVAL, "rank metrics: n must be positive");
  if (!y || !yhat || !out) return fail(SS_EINVAL, "rank metrics: NULL buffer");
  if (!(alpha > 0.0)) return fail(SS_EINVAL, "rank metrics: alpha must be positive");
  if (mem == SS_MEM_DEVICE) return launch_rank_metrics(y, yhat, n, alpha, out);
  hipStream_t st = ctx().stream;
  DevBuf<unsigned char> dy;
  DevBuf<float> ds;
  SS_TRY(dy.alloc((size_t)n));
  SS_TRY(ds.alloc((size_t)n));
  SS_HIP(hipMemcpyAsync(dy.p, y, (size_t)n, hipMemcpyHostToDevice, st));
  SS_HIP(hipMemcpyAsync(ds.p, yhat, (size_t)n * sizeof(float), hipMemcpyHostToDevice, st));
  return launch_rank_metrics(dy.p, ds.p, n, alpha, out);
}

int ss_rank_metrics_rows_f32(const int64_t* yptr, const int32_t* yidx, int index_base, const float* yhat, int64_t nrows,
                             int64_t ncols, int64_t ld, double alpha, int L, double* out, int mem) {
  SS_API_LOCK();
  return rank_rows_impl<float>(yptr, yidx, index_base, yhat, nrows, ncols, ld, alpha, L, out, mem);
}
int ss_rank_metrics_rows_f64(const int64_t* yptr, const int32_t* yidx, int index_base, const double* yhat, int64_t nrows,
                             int64_t ncols, int64_t ld, double alpha, int L, double* out, int mem) {
  SS_API_LOCK();
  return rank_rows_impl<double>(yptr, yidx, index_base, yhat, nrows, ncols, ld, alpha, L, out, mem);
}
int ss_evaluate_loo_f32(ss_graph* g, int64_t i_begin, int64_t i_end, int clean, double alpha, int L, int64_t block_rows,
                        double* out, int mem) {
  SS_API_LOCK();
  if (!g) return fail(SS_EINVAL, "handle is NULL");
  SS_HANDLE_LOCK(g);
  return evaluate_loo_impl<float>(g, i_begin, i_end, clean, alpha, L, block_rows, out, mem);
}
int ss_evaluate_loo_f64(ss_graph* g, int64_t i_begin, int64_t i_end, int clean, double alpha, int L, int64_t block_rows,
                        double* out, int mem) {
  SS_API_LOCK();
  if (!g) return fail(SS_EINVAL, "handle is NULL");
  SS_HANDLE_LOCK(g);
  return evaluate_loo_impl<double>(g, i_begin, i_end, clean, alpha, L, block_rows, out, mem);
}

int ss_binary_metrics_rows_f32(const int64_t* yptr, const int32_t* yidx, int index_base, const float* yhat,
                               int64_t nrows, int64_t ncols, int64_t ld, double* out, int mem) {
  SS_API_LOCK();
  return binary_rows_impl<float>(yptr, yidx, index_base, yhat, nrows, ncols, ld, out, mem);
}
int ss_binary_metrics_rows_f64(const int64_t* yptr, const int32_t* yidx, int index_base, const double* yhat,
                               int64_t nrows, int64_t ncols, int64_t ld, double* out, int mem) {
  SS_API_LOCK();
  return binary_rows_impl<double>(yptr, yidx, index_base, yhat, nrows, ncols, ld, out, mem);
}
int ss_evaluate_loo_binary_f32(ss_graph* g, int64_t i_begin, int64_t i_end, int clean, int64_t block_rows, double* out,
                               int mem) {
  SS_API_LOCK();
  if (!g) return fail(SS_EINVAL, "handle is NULL");
  SS_HANDLE_LOCK(g);
  return evaluate_loo_binary_impl<float>(g, i_begin, i_end, clean, block_rows, out, mem);
}
int ss_evaluate_loo_binary_f64(ss_graph* g, int64_t i_begin, int64_t i_end, int clean, int64_t block_rows, double* out,
                               int mem) {
  SS_API_LOCK();
  if (!g) return fail(SS_EINVAL, "handle is NULL");
  SS_HANDLE_LOCK(g);
  return evaluate_loo_binary_impl<double>(g, i_begin, i_end, clean, block_rows, out, mem);
}

int ss_spmat_create_csr_f32(int64_t rows, int64_t cols, const int64_t* ptr, const int32_t* idx, const float* val,
                            int index_base, int mem, ss_spmat** out) {
  SS_API_LOCK();
  return spmat_create_impl<float>(rows, cols, ptr, idx, val, index_base, mem, out);
}
int ss_spmat_create_csr_f64(int64_t rows, int64_t cols, const int64_t* ptr, const int32_t* idx, const double* val,
                            int index_base, int mem, ss_spmat** out) {
  SS_API_LOCK();
  return spmat_create_impl<double>(rows, cols, ptr, idx, val, index_base, mem, out);
}
int ss_spmat_destroy(ss_spmat* h) {
  SS_API_LOCK();
  if (!h) return SS_OK;
  const int dtype = *reinterpret_cast<int*>(h);
  if (dtype != 4 && dtype != 8) return fail(SS_EINVAL, "not a matrix handle");
  {  // wait for a call that still works on the handle (the caller must not start new ones), then for the device
    SS_HANDLE_LOCK(h);
    if (ctx().inited) (void)hipStreamSynchronize(ctx().stream);
  }
  if (dtype == 4) delete reinterpret_cast<SpMatBox<float>*>(h);
  else if (dtype == 8) delete reinterpret_cast<SpMatBox<double>*>(h);
  else return fail(SS_EINVAL, "not a matrix handle");
  return SS_OK;
}
int ss_spmm_f32(ss_spmat* w, const float* R, int64_t B, int64_t ldr, int r_layout, float* F, int64_t ldf, int f_layout,
                int mem) {
  SS_API_LOCK();
  if (!w) return fail(SS_EINVAL, "handle is NULL");
  SS_HANDLE_LOCK(w);
  return spmm_impl<float>(w, R, B, ldr, r_layout, F, ldf, f_layout, mem);
}
int ss_spmm_f64(ss_spmat* w, const double* R, int64_t B, int64_t ldr, int r_layout, double* F, int64_t ldf,
                int f_layout, int mem) {
  SS_API_LOCK();
  if (!w) return fail(SS_EINVAL, "handle is NULL");
  SS_HANDLE_LOCK(w);
  return spmm_impl<double>(w, R, B, ldr, r_layout, F, ldf, f_layout, mem);
}
int ss_spmat_cost(const ss_spmat* h, int64_t B, double* bytes, double* flops) {
  SS_API_LOCK();
  if (!h) return fail(SS_EINVAL, "handle is NULL");
  SS_HANDLE_LOCK(h);
  if (!h) return fail(SS_EINVAL, "matrix handle is NULL");
  const int dtype = *reinterpret_cast<const int*>(h);
  int64_t rows, cols, nnz;
  if (dtype == 4) { auto* b = reinterpret_cast<const SpMatBox<float>*>(h); rows = b->m.csr.rows; cols = b->m.csr.cols; nnz = b->m.csr.nnz; }
  else if (dtype == 8) { auto* b = reinterpret_cast<const SpMatBox<double>*>(h); rows = b->m.csr.rows; cols = b->m.csr.cols; nnz = b->m.csr.nnz; }
  else return fail(SS_EINVAL, "not a matrix handle");
  const double vb = dtype;
  if (bytes) *bytes = (double)nnz * (vb + 4) + (double)(rows + 1) * 4 + (double)cols * B * vb + (double)rows * B * vb;
  if (flops) *flops = 2.0 * (double)nnz * (double)B;
  return SS_OK;
}

// ------------------------------------------------------------------ pooled tables
int ss_pool_create_f32(int64_t max_entries, ss_pool** out) {
  SS_API_LOCK();
  return pool_create_impl<float>(max_entries, out);
}
int ss_pool_create_f64(int64_t max_entries, ss_pool** out) {
  SS_API_LOCK();
  return pool_create_impl<double>(max_entries, out);
}
int ss_pool_destroy(ss_pool* h) {
  SS_API_LOCK();
  if (!h) return SS_OK;
  int dt = 0;
  SS_TRY(pool_dtype(h, &dt));
  {  // wait for a call that still works on the handle (the caller must not start new ones), then for the device
    SS_HANDLE_LOCK(h);
    if (ctx().inited) (void)hipStreamSynchronize(ctx().stream);
  }
  if (dt == 4) delete reinterpret_cast<PoolBox<float>*>(h);
  else delete reinterpret_cast<PoolBox<double>*>(h);
  return SS_OK;
}
int ss_pool_reset(ss_pool* h) {
  SS_API_LOCK();
  int dt = 0;
  SS_TRY(pool_dtype(h, &dt));
  SS_HANDLE_LOCK(h);
  if (ctx().inited) (void)hipStreamSynchronize(ctx().stream);
  auto clear = [](auto* b) {
    b->lv.clear();
    b->w = decltype(b->w)();
    b->n = b->npos = 0;
  };
  if (dt == 4) clear(reinterpret_cast<PoolBox<float>*>(h));
  else clear(reinterpret_cast<PoolBox<double>*>(h));
  return SS_OK;
}
int ss_pool_info(const ss_pool* h, int64_t info[4]) {
  SS_API_LOCK();
  int dt = 0;
  SS_TRY(pool_dtype(h, &dt));
  if (!info) return fail(SS_EINVAL, "NULL argument");
  SS_HANDLE_LOCK(h);
  auto fill = [&](const auto* b) {
    info[0] = b->n;
    info[1] = b->npos;
    info[2] = pool_stored(b->lv);
    info[3] = b->max_entries;
  };
  if (dt == 4) fill(reinterpret_cast<const PoolBox<float>*>(h));
  else fill(reinterpret_cast<const PoolBox<double>*>(h));
  return SS_OK;
}
int ss_pool_add_rows_f32(ss_pool* pool, const int64_t* yptr, const int32_t* yidx, int index_base, const float* yhat,
                         int64_t nrows, int64_t ncols, int64_t ld, int mem) {
  SS_API_LOCK();
  if (!pool) return fail(SS_EINVAL, "handle is NULL");
  SS_HANDLE_LOCK(pool);
  return pool_add_rows_impl<float>(pool, yptr, yidx, index_base, yhat, nrows, ncols, ld, mem);
}
int ss_pool_add_rows_f64(ss_pool* pool, const int64_t* yptr, const int32_t* yidx, int index_base, const double* yhat,
                         int64_t nrows, int64_t ncols, int64_t ld, int mem) {
  SS_API_LOCK();
  if (!pool) return fail(SS_EINVAL, "handle is NULL");
  SS_HANDLE_LOCK(pool);
  return pool_add_rows_impl<double>(pool, yptr, yidx, index_base, yhat, nrows, ncols, ld, mem);
}
// a pool and a graph: the pool's lock first, always
int ss_pool_add_loo_f32(ss_pool* pool, ss_graph* g, int64_t i_begin, int64_t i_end, int clean, int64_t block_rows) {
  SS_API_LOCK();
  if (!pool || !g) return fail(SS_EINVAL, "handle is NULL");
  SS_HANDLE_LOCK(pool);
  std::unique_lock<std::mutex> _graph_guard(reinterpret_cast<HandleHead*>(g)->mu);
  return pool_add_loo_impl<float>(pool, g, i_begin, i_end, clean, block_rows);
}
int ss_pool_add_loo_f64(ss_pool* pool, ss_graph* g, int64_t i_begin, int64_t i_end, int clean, int64_t block_rows) {
  SS_API_LOCK();
  if (!pool || !g) return fail(SS_EINVAL, "handle is NULL");
  SS_HANDLE_LOCK(pool);
  std::unique_lock<std::mutex> _graph_guard(reinterpret_cast<HandleHead*>(g)->mu);
  return pool_add_loo_impl<double>(pool, g, i_begin, i_end, clean, block_rows);
}
int ss_pool_add_kfold_f32(ss_pool* pool, ss_graph* g, const int32_t* fold_of_source, int nfolds, int64_t i_begin,
                          int64_t i_end, int clean, int64_t block_rows, int mem) {
  SS_API_LOCK();
  if (!pool || !g) return fail(SS_EINVAL, "handle is NULL");
  SS_HANDLE_LOCK(pool);
  std::unique_lock<std::mutex> _graph_guard(reinterpret_cast<HandleHead*>(g)->mu);
  return pool_add_kfold_impl<float>(pool, g, fold_of_source, nfolds, i_begin, i_end, clean, block_rows, mem);
}
int ss_pool_add_kfold_f64(ss_pool* pool, ss_graph* g, const int32_t* fold_of_source, int nfolds, int64_t i_begin,
                          int64_t i_end, int clean, int64_t block_rows, int mem) {
  SS_API_LOCK();
  if (!pool || !g) return fail(SS_EINVAL, "handle is NULL");
  SS_HANDLE_LOCK(pool);
  std::unique_lock<std::mutex> _graph_guard(reinterpret_cast<HandleHead*>(g)->mu);
  return pool_add_kfold_impl<double>(pool, g, fold_of_source, nfolds, i_begin, i_end, clean, block_rows, mem);
}
int ss_pool_merge(ss_pool* dst, const ss_pool* src) {
  SS_API_LOCK();
  int dd = 0, ds = 0;
  SS_TRY(pool_dtype(dst, &dd));
  SS_TRY(pool_dtype(src, &ds));
  if (dd != ds) return fail(SS_EINVAL, "pool merge: the pools have different precisions");
  // two different pools: their locks in address order, so that merge(a, b) and merge(b, a) cannot deadlock
  HandleHead* a = reinterpret_cast<HandleHead*>(dst);
  HandleHead* b = reinterpret_cast<HandleHead*>(const_cast<ss_pool*>(src));
  if (b < a) std::swap(a, b);
  std::unique_lock<std::mutex> la(a->mu);
  std::unique_lock<std::mutex> lb;
  if (b != a) lb = std::unique_lock<std::mutex>(b->mu);
  return dd == 4 ? pool_merge_impl<float>(dst, src) : pool_merge_impl<double>(dst, src);
}
int ss_pool_export_f32(ss_pool* pool, float* keys, int64_t* npos, int64_t* nneg, int64_t cap, int64_t* count, int mem) {
  SS_API_LOCK();
  if (!pool) return fail(SS_EINVAL, "handle is NULL");
  SS_HANDLE_LOCK(pool);
  return pool_export_impl<float>(pool, keys, npos, nneg, cap, count, mem);
}
int ss_pool_export_f64(ss_pool* pool, double* keys, int64_t* npos, int64_t* nneg, int64_t cap, int64_t* count,
                       int mem) {
  SS_API_LOCK();
  if (!pool) return fail(SS_EINVAL, "handle is NULL");
  SS_HANDLE_LOCK(pool);
  return pool_export_impl<double>(pool, keys, npos, nneg, cap, count, mem);
}
int ss_pool_import_f32(ss_pool* pool, const float* keys, const int64_t* npos, const int64_t* nneg, int64_t n, int mem) {
  SS_API_LOCK();
  if (!pool) return fail(SS_EINVAL, "handle is NULL");
  SS_HANDLE_LOCK(pool);
  return pool_import_impl<float>(pool, keys, npos, nneg, n, mem);
}
int ss_pool_import_f64(ss_pool* pool, const double* keys, const int64_t* npos, const int64_t* nneg, int64_t n,
                       int mem) {
  SS_API_LOCK();
  if (!pool) return fail(SS_EINVAL, "handle is NULL");
  SS_HANDLE_LOCK(pool);
  return pool_import_impl<double>(pool, keys, npos, nneg, n, mem);
}
int ss_pool_metrics(ss_pool* pool, double out[21]) {
  SS_API_LOCK();
  SS_TRY(require_init());
  int dt = 0;
  SS_TRY(pool_dtype(pool, &dt));
  if (!out) return fail(SS_EINVAL, "NULL argument");
  SS_HANDLE_LOCK(pool);
  return dt == 4 ? pool_metrics_impl(*reinterpret_cast<PoolBox<float>*>(pool), out)
                 : pool_metrics_impl(*reinterpret_cast<PoolBox<double>*>(pool), out);
}

// ------------------------------------------------------------------ per-target top-L tables
int ss_target_topl_create_f32(int64_t nt, int L, ss_target_topl** out) {
  SS_API_LOCK();
  return tl_create_impl<float>(nt, L, out);
}
int ss_target_topl_create_f64(int64_t nt, int L, ss_target_topl** out) {
  SS_API_LOCK();
  return tl_create_impl<double>(nt, L, out);
}
int ss_target_topl_destroy(ss_target_topl* h) {
  SS_API_LOCK();
  if (!h) return SS_OK;
  int dt = 0;
  SS_TRY(tl_dtype(h, &dt));
  {  // wait for a call that still works on the handle (the caller must not start new ones), then for the device
    SS_HANDLE_LOCK(h);
    if (ctx().inited) (void)hipStreamSynchronize(ctx().stream);
  }
  if (dt == 4) delete reinterpret_cast<TlBox<float>*>(h);
  else delete reinterpret_cast<TlBox<double>*>(h);
  return SS_OK;
}
int ss_target_topl_reset(ss_target_topl* h) {
  SS_API_LOCK();
  int dt = 0;
  SS_TRY(tl_dtype(h, &dt));
  SS_HANDLE_LOCK(h);
  SS_TRY(require_init());
  auto clear = [](auto* b) -> int {
    SS_HIP(hipStreamSynchronize(ctx().stream));
    SS_HIP(hipMemsetAsync(b->t.npos.p, 0, (size_t)b->nt * sizeof(int64_t), ctx().stream));
    SS_HIP(hipStreamSynchronize(ctx().stream));
    b->rows = b->npos = 0;
    return SS_OK;
  };
  return dt == 4 ? clear(reinterpret_cast<TlBox<float>*>(h)) : clear(reinterpret_cast<TlBox<double>*>(h));
}
int ss_target_topl_info(const ss_target_topl* h, int64_t info[4]) {
  SS_API_LOCK();
  int dt = 0;
  SS_TRY(tl_dtype(h, &dt));
  if (!info) return fail(SS_EINVAL, "NULL argument");
  SS_HANDLE_LOCK(h);
  auto fill = [&](const auto* b) {
    info[0] = b->nt;
    info[1] = b->L;
    info[2] = b->rows;
    info[3] = b->npos;
  };
  if (dt == 4) fill(reinterpret_cast<const TlBox<float>*>(h));
  else fill(reinterpret_cast<const TlBox<double>*>(h));
  return SS_OK;
}
int ss_target_topl_add_rows_f32(ss_target_topl* h, const int64_t* yptr, const int32_t* yidx, int index_base,
                                const float* yhat, int64_t nrows, int64_t ncols, int64_t ld, int64_t row_begin,
                                int mem) {
  SS_API_LOCK();
  if (!h) return fail(SS_EINVAL, "handle is NULL");
  SS_HANDLE_LOCK(h);
  return tl_add_rows_impl<float>(h, yptr, yidx, index_base, yhat, nrows, ncols, ld, row_begin, mem);
}
int ss_target_topl_add_rows_f64(ss_target_topl* h, const int64_t* yptr, const int32_t* yidx, int index_base,
                                const double* yhat, int64_t nrows, int64_t ncols, int64_t ld, int64_t row_begin,
                                int mem) {
  SS_API_LOCK();
  if (!h) return fail(SS_EINVAL, "handle is NULL");
  SS_HANDLE_LOCK(h);
  return tl_add_rows_impl<double>(h, yptr, yidx, index_base, yhat, nrows, ncols, ld, row_begin, mem);
}
// a table and a graph: the table's lock first, always
int ss_target_topl_add_loo_f32(ss_target_topl* h, ss_graph* g, int64_t i_begin, int64_t i_end, int clean,
                               int64_t block_rows) {
  SS_API_LOCK();
  if (!h || !g) return fail(SS_EINVAL, "handle is NULL");
  SS_HANDLE_LOCK(h);
  std::unique_lock<std::mutex> _graph_guard(reinterpret_cast<HandleHead*>(g)->mu);
  return tl_add_loo_impl<float>(h, g, i_begin, i_end, clean, block_rows);
}
int ss_target_topl_add_loo_f64(ss_target_topl* h, ss_graph* g, int64_t i_begin, int64_t i_end, int clean,
                               int64_t block_rows) {
  SS_API_LOCK();
  if (!h || !g) return fail(SS_EINVAL, "handle is NULL");
  SS_HANDLE_LOCK(h);
  std::unique_lock<std::mutex> _graph_guard(reinterpret_cast<HandleHead*>(g)->mu);
  return tl_add_loo_impl<double>(h, g, i_begin, i_end, clean, block_rows);
}
int ss_target_topl_add_kfold_f32(ss_target_topl* h, ss_graph* g, const int32_t* fold_of_source, int nfolds,
                                 int64_t i_begin, int64_t i_end, int clean, int64_t block_rows, int mem) {
  SS_API_LOCK();
  if (!h || !g) return fail(SS_EINVAL, "handle is NULL");
  SS_HANDLE_LOCK(h);
  std::unique_lock<std::mutex> _graph_guard(reinterpret_cast<HandleHead*>(g)->mu);
  return tl_add_kfold_impl<float>(h, g, fold_of_source, nfolds, i_begin, i_end, clean, block_rows, mem);
}
int ss_target_topl_add_kfold_f64(ss_target_topl* h, ss_graph* g, const int32_t* fold_of_source, int nfolds,
                                 int64_t i_begin, int64_t i_end, int clean, int64_t block_rows, int mem) {
  SS_API_LOCK();
  if (!h || !g) return fail(SS_EINVAL, "handle is NULL");
  SS_HANDLE_LOCK(h);
  std::unique_lock<std::mutex> _graph_guard(reinterpret_cast<HandleHead*>(g)->mu);
  return tl_add_kfold_impl<double>(h, g, fold_of_source, nfolds, i_begin, i_end, clean, block_rows, mem);
}
int ss_target_topl_merge(ss_target_topl* dst, const ss_target_topl* src) {
  SS_API_LOCK();
  int dd = 0, ds = 0;
  SS_TRY(tl_dtype(dst, &dd));
  SS_TRY(tl_dtype(src, &ds));
  if (dd != ds) return fail(SS_EINVAL, "target top-L merge: the handles have different precisions");
  // two different handles: their locks in address order, so that merge(a, b) and merge(b, a) cannot deadlock
  HandleHead* a = reinterpret_cast<HandleHead*>(dst);
  HandleHead* b = reinterpret_cast<HandleHead*>(const_cast<ss_target_topl*>(src));
  if (b < a) std::swap(a, b);
  std::unique_lock<std::mutex> la(a->mu);
  std::unique_lock<std::mutex> lb;
  if (b != a) lb = std::unique_lock<std::mutex>(b->mu);
  return dd == 4 ? tl_merge_impl<float>(dst, src) : tl_merge_impl<double>(dst, src);
}
int ss_target_topl_export_f32(ss_target_topl* h, float* vals, int64_t* rows, uint8_t* labels, int64_t* npos,
                              int64_t* rows_added, int mem) {
  SS_API_LOCK();
  if (!h) return fail(SS_EINVAL, "handle is NULL");
  SS_HANDLE_LOCK(h);
  return tl_export_impl<float>(h, vals, rows, labels, npos, rows_added, mem);
}
int ss_target_topl_export_f64(ss_target_topl* h, double* vals, int64_t* rows, uint8_t* labels, int64_t* npos,
                              int64_t* rows_added, int mem) {
  SS_API_LOCK();
  if (!h) return fail(SS_EINVAL, "handle is NULL");
  SS_HANDLE_LOCK(h);
  return tl_export_impl<double>(h, vals, rows, labels, npos, rows_added, mem);
}
int ss_target_topl_import_f32(ss_target_topl* h, const float* vals, const int64_t* rows, const uint8_t* labels,
                              const int64_t* npos, int64_t rows_added, int mem) {
  SS_API_LOCK();
  if (!h) return fail(SS_EINVAL, "handle is NULL");
  SS_HANDLE_LOCK(h);
  return tl_import_impl<float>(h, vals, rows, labels, npos, rows_added, mem);
}
int ss_target_topl_import_f64(ss_target_topl* h, const double* vals, const int64_t* rows, const uint8_t* labels,
                              const int64_t* npos, int64_t rows_added, int mem) {
  SS_API_LOCK();
  if (!h) return fail(SS_EINVAL, "handle is NULL");
  SS_HANDLE_LOCK(h);
  return tl_import_impl<double>(h, vals, rows, labels, npos, rows_added, mem);
}
int ss_target_topl_metrics(ss_target_topl* h, int64_t* hits, int64_t* npos, double out[4], int mem) {
  SS_API_LOCK();
  SS_TRY(require_init());
  int dt = 0;
  SS_TRY(tl_dtype(h, &dt));
  if (!out) return fail(SS_EINVAL, "NULL argument");
  SS_HANDLE_LOCK(h);
  return dt == 4 ? tl_metrics_impl(*reinterpret_cast<TlBox<float>*>(h), hits, npos, out, mem)
                 : tl_metrics_impl(*reinterpret_cast<TlBox<double>*>(h), hits, npos, out, mem);
}

/* ---- include/simspread_hip_target_rank.h */
int ss_target_rank_create_f32(int64_t nt, ss_target_rank** out) {
  SS_API_LOCK();
  return tr_create_impl<float>(nt, out);
}
int ss_target_rank_create_f64(int64_t nt, ss_target_rank** out) {
  SS_API_LOCK();
  return tr_create_impl<double>(nt, out);
}
int ss_target_rank_destroy(ss_target_rank* h) {
  SS_API_LOCK();
  if (!h) return SS_OK;
  int dt = 0;
  SS_TRY(tr_dtype(h, &dt));
  {  // wait for a call that still works on the handle, then for the device
    SS_HANDLE_LOCK(h);
    if (ctx().inited) (void)hipStreamSynchronize(ctx().stream);
  }
  if (dt == 4) delete reinterpret_cast<TrBox<float>*>(h);
  else delete reinterpret_cast<TrBox<double>*>(h);
  return SS_OK;
}
int ss_target_rank_reset(ss_target_rank* h) {
  SS_API_LOCK();
  int dt = 0;
  SS_TRY(tr_dtype(h, &dt));
  SS_HANDLE_LOCK(h);
  SS_TRY(require_init());
  auto clear = [](auto* b) -> int {
    SS_HIP(hipStreamSynchronize(ctx().stream));
    b->s.phase = 0;
    b->s.rows = b->s.npos = b->s.rows_counted = 0;
    b->s.tiles_lds = b->s.tiles_large = 0;
    return SS_OK;
  };
  return dt == 4 ? clear(reinterpret_cast<TrBox<float>*>(h)) : clear(reinterpret_cast<TrBox<double>*>(h));
}
int ss_target_rank_info(const ss_target_rank* h, int64_t info[6]) {
  SS_API_LOCK();
  int dt = 0;
  SS_TRY(tr_dtype(h, &dt));
  if (!info) return fail(SS_EINVAL, "NULL argument");
  SS_HANDLE_LOCK(h);
  auto fill = [&](const auto* b) {
    info[0] = b->s.nt;
    info[1] = b->s.phase;
    info[2] = b->s.rows;
    info[3] = b->s.npos;
    info[4] = b->s.rows_counted;
    info[5] = 0;
  };
  if (dt == 4) fill(reinterpret_cast<const TrBox<float>*>(h));
  else fill(reinterpret_cast<const TrBox<double>*>(h));
  return SS_OK;
}
int ss_target_rank_add_rows_f32(ss_target_rank* h, const int64_t* yptr, const int32_t* yidx, int index_base,
                                const float* yhat, int64_t nrows, int64_t ncols, int64_t ld, int64_t row_begin,
                                int mem) {
  SS_API_LOCK();
  if (!h) return fail(SS_EINVAL, "handle is NULL");
  SS_HANDLE_LOCK(h);
  return tr_add_rows_impl<float>(h, yptr, yidx, index_base, yhat, nrows, ncols, ld, row_begin, mem);
}
int ss_target_rank_add_rows_f64(ss_target_rank* h, const int64_t* yptr, const int32_t* yidx, int index_base,
                                const double* yhat, int64_t nrows, int64_t ncols, int64_t ld, int64_t row_begin,
                                int mem) {
  SS_API_LOCK();
  if (!h) return fail(SS_EINVAL, "handle is NULL");
  SS_HANDLE_LOCK(h);
  return tr_add_rows_impl<double>(h, yptr, yidx, index_base, yhat, nrows, ncols, ld, row_begin, mem);
}
// a handle and a graph: the handle's lock first, always
int ss_target_rank_add_loo_f32(ss_target_rank* h, ss_graph* g, int64_t i_begin, int64_t i_end, int clean,
                               int64_t block_rows) {
  SS_API_LOCK();
  if (!h || !g) return fail(SS_EINVAL, "handle is NULL");
  SS_HANDLE_LOCK(h);
  std::unique_lock<std::mutex> _graph_guard(reinterpret_cast<HandleHead*>(g)->mu);
  return tr_add_loo_impl<float>(h, g, i_begin, i_end, clean, block_rows);
}
int ss_target_rank_add_loo_f64(ss_target_rank* h, ss_graph* g, int64_t i_begin, int64_t i_end, int clean,
                               int64_t block_rows) {
  SS_API_LOCK();
  if (!h || !g) return fail(SS_EINVAL, "handle is NULL");
  SS_HANDLE_LOCK(h);
  std::unique_lock<std::mutex> _graph_guard(reinterpret_cast<HandleHead*>(g)->mu);
  return tr_add_loo_impl<double>(h, g, i_begin, i_end, clean, block_rows);
}
int ss_target_rank_add_kfold_f32(ss_target_rank* h, ss_graph* g, const int32_t* fold_of_source, int nfolds,
                                 int64_t i_begin, int64_t i_end, int clean, int64_t block_rows, int mem) {
  SS_API_LOCK();
  if (!h || !g) return fail(SS_EINVAL, "handle is NULL");
  SS_HANDLE_LOCK(h);
  std::unique_lock<std::mutex> _graph_guard(reinterpret_cast<HandleHead*>(g)->mu);
  return tr_add_kfold_impl<float>(h, g, fold_of_source, nfolds, i_begin, i_end, clean, block_rows, mem);
}
int ss_target_rank_add_kfold_f64(ss_target_rank* h, ss_graph* g, const int32_t* fold_of_source, int nfolds,
                                 int64_t i_begin, int64_t i_end, int clean, int64_t block_rows, int mem) {
  SS_API_LOCK();
  if (!h || !g) return fail(SS_EINVAL, "handle is NULL");
  SS_HANDLE_LOCK(h);
  std::unique_lock<std::mutex> _graph_guard(reinterpret_cast<HandleHead*>(g)->mu);
  return tr_add_kfold_impl<double>(h, g, fold_of_source, nfolds, i_begin, i_end, clean, block_rows, mem);
}
int ss_target_rank_seal(ss_target_rank* h) {
  SS_API_LOCK();
  int dt = 0;
  SS_TRY(tr_dtype(h, &dt));
  SS_HANDLE_LOCK(h);
  return dt == 4 ? tr_seal_impl(*reinterpret_cast<TrBox<float>*>(h)) : tr_seal_impl(*reinterpret_cast<TrBox<double>*>(h));
}
int ss_target_rank_merge(ss_target_rank* dst, const ss_target_rank* src) {
  SS_API_LOCK();
  int dd = 0, ds = 0;
  SS_TRY(tr_dtype(dst, &dd));
  SS_TRY(tr_dtype(src, &ds));
  if (dd != ds) return fail(SS_EINVAL, "target rank merge: the handles have different precisions");
  // two different handles: their locks in address order, so that merge(a, b) and merge(b, a) cannot deadlock
  HandleHead* a = reinterpret_cast<HandleHead*>(dst);
  HandleHead* b = reinterpret_cast<HandleHead*>(const_cast<ss_target_rank*>(src));
  if (b < a) std::swap(a, b);
  std::unique_lock<std::mutex> la(a->mu);
  std::unique_lock<std::mutex> lb;
  if (b != a) lb = std::unique_lock<std::mutex>(b->mu);
  return dd == 4 ? tr_merge_impl<float>(dst, src) : tr_merge_impl<double>(dst, src);
}
int ss_target_rank_export_positives_f32(ss_target_rank* h, int32_t* targets, int64_t* rows, float* scores,
                                        int64_t* rows_added, int mem) {
  SS_API_LOCK();
  if (!h) return fail(SS_EINVAL, "handle is NULL");
  SS_HANDLE_LOCK(h);
  return tr_export_positives_impl<float>(h, targets, rows, scores, rows_added, mem);
}
int ss_target_rank_export_positives_f64(ss_target_rank* h, int32_t* targets, int64_t* rows, double* scores,
                                        int64_t* rows_added, int mem) {
  SS_API_LOCK();
  if (!h) return fail(SS_EINVAL, "handle is NULL");
  SS_HANDLE_LOCK(h);
  return tr_export_positives_impl<double>(h, targets, rows, scores, rows_added, mem);
}
int ss_target_rank_import_positives_f32(ss_target_rank* h, const int32_t* targets, const int64_t* rows,
                                        const float* scores, int64_t npos, int64_t rows_added, int mem) {
  SS_API_LOCK();
  if (!h) return fail(SS_EINVAL, "handle is NULL");
  SS_HANDLE_LOCK(h);
  return tr_import_positives_impl<float>(h, targets, rows, scores, npos, rows_added, mem);
}
int ss_target_rank_import_positives_f64(ss_target_rank* h, const int32_t* targets, const int64_t* rows,
                                        const double* scores, int64_t npos, int64_t rows_added, int mem) {
  SS_API_LOCK();
  if (!h) return fail(SS_EINVAL, "handle is NULL");
  SS_HANDLE_LOCK(h);
  return tr_import_positives_impl<double>(h, targets, rows, scores, npos, rows_added, mem);
}
int ss_target_rank_export_counts(ss_target_rank* h, int64_t* counts, int64_t* rows_counted, int mem) {
  SS_API_LOCK();
  int dt = 0;
  SS_TRY(tr_dtype(h, &dt));
  SS_HANDLE_LOCK(h);
  return dt == 4 ? tr_export_counts_impl(*reinterpret_cast<TrBox<float>*>(h), counts, rows_counted, mem)
                 : tr_export_counts_impl(*reinterpret_cast<TrBox<double>*>(h), counts, rows_counted, mem);
}
int ss_target_rank_import_counts(ss_target_rank* h, const int64_t* counts, int64_t ncounts, int64_t rows_counted,
                                 int mem) {
  SS_API_LOCK();
  int dt = 0;
  SS_TRY(tr_dtype(h, &dt));
  SS_HANDLE_LOCK(h);
  return dt == 4 ? tr_import_counts_impl(*reinterpret_cast<TrBox<float>*>(h), counts, ncounts, rows_counted, mem)
                 : tr_import_counts_impl(*reinterpret_cast<TrBox<double>*>(h), counts, ncounts, rows_counted, mem);
}
int ss_target_rank_metrics(ss_target_rank* h, double alpha, int L, double* out, int mem) {
  SS_API_LOCK();
  int dt = 0;
  SS_TRY(tr_dtype(h, &dt));
  SS_HANDLE_LOCK(h);
  return dt == 4 ? tr_metrics_impl(*reinterpret_cast<TrBox<float>*>(h), alpha, L, out, mem)
                 : tr_metrics_impl(*reinterpret_cast<TrBox<double>*>(h), alpha, L, out, mem);
}

/* ---- include/simspread_hip_clusters.h */
int ss_cluster_butina_csr(int64_t n, const int64_t* ptr, const int32_t* idx, int index_base, int32_t* centre,
                          int32_t* label, int32_t* size, int64_t* nclusters, int64_t* rounds, int mem) {
  SS_API_LOCK();
  return cluster_butina_csr_impl(n, ptr, idx, index_base, ClusterOut{centre, label, size, nclusters, rounds}, mem);
}
int ss_cluster_butina_fingerprint_f32(const uint64_t* F, int64_t n, int64_t nwords, float cutoff, int32_t* centre,
                                      int32_t* label, int32_t* size, int64_t* nclusters, int64_t* rounds, int mem) {
  SS_API_LOCK();
  return cluster_butina_fingerprint_impl<float>(F, n, nwords, cutoff, ClusterOut{centre, label, size, nclusters, rounds},
                                                mem);
}
int ss_cluster_butina_fingerprint_f64(const uint64_t* F, int64_t n, int64_t nwords, double cutoff, int32_t* centre,
                                      int32_t* label, int32_t* size, int64_t* nclusters, int64_t* rounds, int mem) {
  SS_API_LOCK();
  return cluster_butina_fingerprint_impl<double>(F, n, nwords, cutoff,
                                                 ClusterOut{centre, label, size, nclusters, rounds}, mem);
}
int ss_cluster_butina_features_f32(const float* F, int64_t n, int64_t d, int64_t ld, float cutoff, int32_t* centre,
                                   int32_t* label, int32_t* size, int64_t* nclusters, int64_t* rounds, int mem) {
  SS_API_LOCK();
  return cluster_butina_features_impl<float>(F, n, d, ld, cutoff, ClusterOut{centre, label, size, nclusters, rounds},
                                             mem);
}
int ss_cluster_butina_features_f64(const double* F, int64_t n, int64_t d, int64_t ld, double cutoff, int32_t* centre,
                                   int32_t* label, int32_t* size, int64_t* nclusters, int64_t* rounds, int mem) {
  SS_API_LOCK();
  return cluster_butina_features_impl<double>(F, n, d, ld, cutoff, ClusterOut{centre, label, size, nclusters, rounds},
                                              mem);
}
int ss_cluster_butina_vectors_f32(int metric, const float* F, int64_t n, int64_t d, int64_t ld, float cutoff,
                                  int32_t* centre, int32_t* label, int32_t* size, int64_t* nclusters, int64_t* rounds,
                                  int mem) {
  SS_API_LOCK();
  return cluster_butina_vectors_impl<float>(metric, F, n, d, ld, cutoff,
                                            ClusterOut{centre, label, size, nclusters, rounds}, mem);
}
int ss_cluster_butina_vectors_f64(int metric, const double* F, int64_t n, int64_t d, int64_t ld, double cutoff,
                                  int32_t* centre, int32_t* label, int32_t* size, int64_t* nclusters, int64_t* rounds,
                                  int mem) {
  SS_API_LOCK();
  return cluster_butina_vectors_impl<double>(metric, F, n, d, ld, cutoff,
                                             ClusterOut{centre, label, size, nclusters, rounds}, mem);
}
int ss_cluster_folds(const int32_t* label, int64_t n, int64_t nclusters, int nfolds, int32_t* fold_of_source, int mem) {
  SS_API_LOCK();
  return cluster_folds_impl(label, n, nclusters, nfolds, fold_of_source, mem);
}
int ss_cluster_cross_edges(int64_t n, const int64_t* ptr, const int32_t* idx, int index_base,
                           const int32_t* fold_of_source, int nfolds, int64_t* count, int mem) {
  SS_API_LOCK();
  return cluster_cross_edges_impl(n, ptr, idx, index_base, fold_of_source, nfolds, count, mem);
}

// ---- include/simspread_hip_half.h: the inner-product producer on 16-bit rows
int ss_similarity_dot_csr_h16(const uint16_t* Fa, int64_t na, int64_t lda, const uint16_t* Fb, int64_t nb, int64_t ldb,
                              int64_t d, int storage, int metric, float alpha, int weighted, int64_t* ptr, int32_t* idx,
                              float* val, int64_t capacity, int64_t* nnz, int mem) {
  SS_API_LOCK();
  return dot_csr_h16_impl(Fa, na, lda, Fb, nb, ldb, d, storage, metric, alpha, weighted, ptr, idx, val, capacity, nnz,
                          mem);
}
int ss_graph_create_vectors_h16(int64_t nq, int64_t ns, int64_t nt, int64_t d, int storage, int metric,
                                const uint16_t* Fq, int64_t ldq, const uint16_t* Fs, int64_t lds, const int64_t* y_ptr,
                                const int32_t* y_idx, const float* y_val, int index_base, float alpha, int weighted,
                                int mem, ss_graph** out) {
  SS_API_LOCK();
  return graph_create_vectors_h16_impl(nq, ns, nt, d, storage, metric, Fq, ldq, Fs, lds, y_ptr, y_idx, y_val, index_base,
                                       alpha, weighted, mem, out);
}
int ss_queries_create_vectors_h16(const ss_graph* g, int64_t nq, int64_t ns, int64_t d, int storage, int metric,
                                  const uint16_t* Fq, int64_t ldq, const uint16_t* Fs, int64_t lds, float alpha,
                                  int weighted, int mem, ss_queries** out) {
  SS_API_LOCK();
  if (!g) return fail(SS_EINVAL, "handle is NULL");
  SS_HANDLE_LOCK(g);
  Graph<float>* gp = nullptr;
  SS_TRY(queries_begin<float>(g, nq, mem, out, &gp));
  SS_TRY(queries_check_sources(*gp, ns));
  SS_TRY(check_h16_args(storage, metric, d, alpha));
  SS_TRY(check_rows_h16("Fq", Fq, nq, ldq, d));
  SS_TRY(check_rows_h16("Fs", Fs, ns, lds, d));
  DevBuf<uint16_t> bq, bs;
  const uint16_t *dq = nullptr, *ds = nullptr;
  int64_t lq = 0, ls = 0;
  SS_TRY(stage_rows_h16(Fs, ns, lds, d, mem, bs, &ds, &ls));
  SS_TRY(stage_rows_h16(Fq, nq, ldq, d, mem, bq, &dq, &lq));
  return queries_from_producer<float, DotCsrH16>(
      g, nq, ns,
      [&](DotCsrH16& p) { return p.count(dq, nq, lq, ds, ns, ls, d, storage, metric, alpha, weighted != 0); },
      h16_tag(false), out);
}

// ---- include/simspread_hip_int8.h: the inner-product producer and its neighbour floor on int8 rows
int ss_similarity_dot_csr_i8(const int8_t* Fa, int64_t na, int64_t lda, const int8_t* Fb, int64_t nb, int64_t ldb,
                             int64_t d, int metric, float alpha, int k, int weighted, int64_t* ptr, int32_t* idx,
                             float* val, int64_t capacity, int64_t* nnz, int mem) {
  SS_API_LOCK();
  return dot_csr_i8_impl(Fa, na, lda, Fb, nb, ldb, d, metric, alpha, k, weighted, ptr, idx, val, capacity, nnz, mem);
}
int ss_similarity_dot_kth_i8(const int8_t* Fa, int64_t na, int64_t lda, const int8_t* Fb, int64_t nb, int64_t ldb,
                             int64_t d, int metric, int k, float* tau, int mem) {
  SS_API_LOCK();
  return dot_kth_i8_impl(Fa, na, lda, Fb, nb, ldb, d, metric, k, tau, mem);
}
int ss_graph_create_vectors_i8(int64_t nq, int64_t ns, int64_t nt, int64_t d, int metric, const int8_t* Fq, int64_t ldq,
                               const int8_t* Fs, int64_t lds, const int64_t* y_ptr, const int32_t* y_idx,
                               const float* y_val, int index_base, float alpha, int k, int weighted, int mem,
                               ss_graph** out) {
  SS_API_LOCK();
  return graph_create_vectors_i8_impl(nq, ns, nt, d, metric, Fq, ldq, Fs, lds, y_ptr, y_idx, y_val, index_base, alpha, k,
                                      weighted, mem, out);
}
int ss_queries_create_vectors_i8(const ss_graph* g, int64_t nq, int64_t ns, int64_t d, int metric, const int8_t* Fq,
                                 int64_t ldq, const int8_t* Fs, int64_t lds, float alpha, int k, int weighted, int mem,
                                 ss_queries** out) {
  SS_API_LOCK();
  if (!g) return fail(SS_EINVAL, "handle is NULL");
  SS_HANDLE_LOCK(g);
  Graph<float>* gp = nullptr;
  SS_TRY(queries_begin<float>(g, nq, mem, out, &gp));
  SS_TRY(queries_check_sources(*gp, ns));
  SS_TRY(check_i8_args(metric, d, alpha, k, 0));
  SS_TRY(check_rows_i8("Fq", Fq, nq, ldq, d));
  SS_TRY(check_rows_i8("Fs", Fs, ns, lds, d));
  DevBuf<int8_t> bq, bs;
  const int8_t *dq = nullptr, *ds = nullptr;
  int64_t lq = 0, ls = 0;
  SS_TRY(stage_rows_i8(Fs, ns, lds, d, mem, bs, &ds, &ls));
  SS_TRY(stage_rows_i8(Fq, nq, ldq, d, mem, bq, &dq, &lq));
  return queries_from_producer<float, DotCsrI8>(
      g, nq, ns, [&](DotCsrI8& p) { return p.count(dq, nq, lq, ds, ns, ls, d, metric, alpha, weighted != 0, k); },
      i8_names.tag(false, k), out);
}

// ---- include/simspread_hip_profile.h: cutoff profiles of the fused producers
int ss_similarity_tanimoto_profile_f32(const uint64_t* Fa, int64_t na, const uint64_t* Fb, int64_t nb, int64_t nwords,
                                       const float* cuts, int ncuts, int weighted, int64_t* total, int32_t* rows,
                                       int mem) {
  SS_API_LOCK();
  return tanimoto_profile_impl<float>(Fa, na, Fb, nb, nwords, cuts, ncuts, weighted, total, rows, mem);
}
int ss_similarity_tanimoto_profile_f64(const uint64_t* Fa, int64_t na, const uint64_t* Fb, int64_t nb, int64_t nwords,
                                       const double* cuts, int ncuts, int weighted, int64_t* total, int32_t* rows,
                                       int mem) {
  SS_API_LOCK();
  return tanimoto_profile_impl<double>(Fa, na, Fb, nb, nwords, cuts, ncuts, weighted, total, rows, mem);
}
int ss_similarity_jaccard_profile_f32(const float* Fa, int64_t na, int64_t lda, const float* Fb, int64_t nb, int64_t ldb,
                                      int64_t d, const float* cuts, int ncuts, int weighted, int64_t* total,
                                      int32_t* rows, int mem) {
  SS_API_LOCK();
  return jaccard_profile_impl<float>(Fa, na, lda, Fb, nb, ldb, d, cuts, ncuts, weighted, total, rows, mem);
}
int ss_similarity_jaccard_profile_f64(const double* Fa, int64_t na, int64_t lda, const double* Fb, int64_t nb,
                                      int64_t ldb, int64_t d, const double* cuts, int ncuts, int weighted,
                                      int64_t* total, int32_t* rows, int mem) {
  SS_API_LOCK();
  return jaccard_profile_impl<double>(Fa, na, lda, Fb, nb, ldb, d, cuts, ncuts, weighted, total, rows, mem);
}
int ss_similarity_dot_profile_f32(const float* Fa, int64_t na, int64_t lda, const float* Fb, int64_t nb, int64_t ldb,
                                  int64_t d, int metric, const float* cuts, int ncuts, int weighted, int64_t* total,
                                  int32_t* rows, int mem) {
  SS_API_LOCK();
  return dot_profile_impl<float>(Fa, na, lda, Fb, nb, ldb, d, metric, cuts, ncuts, weighted, total, rows, mem);
}
int ss_similarity_dot_profile_f64(const double* Fa, int64_t na, int64_t lda, const double* Fb, int64_t nb, int64_t ldb,
                                  int64_t d, int metric, const double* cuts, int ncuts, int weighted, int64_t* total,
                                  int32_t* rows, int mem) {
  SS_API_LOCK();
  return dot_profile_impl<double>(Fa, na, lda, Fb, nb, ldb, d, metric, cuts, ncuts, weighted, total, rows, mem);
}
int ss_similarity_dot_profile_h16(const uint16_t* Fa, int64_t na, int64_t lda, const uint16_t* Fb, int64_t nb,
                                  int64_t ldb, int64_t d, int storage, int metric, const float* cuts, int ncuts,
                                  int weighted, int64_t* total, int32_t* rows, int mem) {
  SS_API_LOCK();
  return dot_profile_h16_impl(Fa, na, lda, Fb, nb, ldb, d, storage, metric, cuts, ncuts, weighted, total, rows, mem);
}

}  // extern "C"
