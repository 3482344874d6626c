// Device-resident sparse operands of the resource-spreading pass.
//
//   DevCsr   plain CSR, 4-byte row pointers and column indices (SURVEY.md 8d byte model)
//   DevSell  the same matrix re-cut for the wide W*R kernel: rows in slices of 64 (one
//            lane per row), columns in chunks of KC (one LDS tile of R per chunk),
//            chunk-local 16-bit column indices, four entries per lane per load
//   Graph    the blocks Xq, Xs, Ys of construct's adjacency (src/core.jl:165-187), their
//            transposes, and the count degrees of B (src/core.jl:365-371)
#pragma once
#include "common.hpp"

#include <type_traits>

namespace ss {

template <class T>
struct DevCsr {
  int64_t rows = 0, cols = 0, nnz = 0;
  DevBuf<int> ptr;   // rows+1
  DevBuf<int> idx;   // nnz, sorted within a row
  DevBuf<T> val;     // nnz
  bool binary = false;  // every stored value == 1
};

constexpr int SELL_Q1_STEP = 8;   // = 2 * SELL_NB (kernels.hip): the quads of one turn of spmm_sell_kernel's gather loop
constexpr int SELL_LEND_R = 3;    // receivers per donor row: their lanes fit bytes 0-2 of a lane's record
constexpr unsigned SELL_REC_NONE = 0x00ffffffu;

template <class T>
struct DevSell {
  int64_t rows = 0, cols = 0;
  int KC = 0;          // columns per chunk; local indices KC .. KC+15 are zero rows (padding targets)
  int qt = 0;          // columns per tile row the entry order was scheduled for (slot classes = 256 / (qt * sizeof(T)))
  int nchunks = 0;
  int nslices = 0;     // ceil(rows / 64)
  int64_t nquads = 0;  // total storage in units of 64 lanes x 4 entries
  bool binary = false;
  DevBuf<int> off;              // [nchunks*nslices + 1] quad offsets, chunk-major
  DevBuf<unsigned short> idx;   // [nquads][64][4]
  DevBuf<T> val;                // [nquads][64][4] unless binary
  // Slot lending (16-byte tile rows, not sorted; SS_SELL_LEND=0: off).  A slice is as long as its longest row, so short
  // rows pad it.  Slice (chunk, slice) = w is cut at Q2 = off[w+1] - off[w] quads, below its longest row, when the rows
  // longer than 4*Q2 ("donors") can park their excess in the quads q1[w] .. Q2-1 of rows with at most 4*q1[w] entries
  // ("receivers": one donor each, at most SELL_LEND_R receivers per donor).  q1[w] is a multiple of SELL_Q1_STEP, the
  // unit in which the kernel consumes quads; q1[w] == Q2: nothing is lent in the slice.  rec[w*64 + lane]: bytes 0-2 =
  // the lanes whose partial sums this lane adds to its own, in that order (0xFF: none); bit 24: this lane is a receiver
  // (its own sum ends at quad q1[w], what follows belongs to its donor).  Every row stays on its lane: the store and the
  // row order are those of the plain layout, and the entries a lane keeps sit where the plain layout puts them.
  DevBuf<int> q1;               // [nchunks*nslices] (16-byte tile rows only)
  DevBuf<unsigned> rec;         // [nchunks*nslices][64]
  bool lends = false;           // at least one slice lends
  // skewed row lengths (power-law graphs): rows are sorted by length before they are cut into slices so
  // that the 64 rows of a slice are equally long; results then come out in sorted order and are put back
  // by unpermute_kernel.  perm[sorted position] = row, inv[row] = sorted position.
  // Rows longer than a wave's fair share are first split into "virtual rows" of bounded length (their
  // partial scores are summed, in order, by the same epilogue), so a hot target cannot serialise a slice.
  bool sorted = false;
  int64_t vrows = 0;         // virtual rows (= slices * 64 rounded down); rows when not sorted
  DevBuf<int> vs, ve;        // [vrows] CSR entry range of the virtual row at each sorted position
  DevBuf<int> vfirst;        // [rows + 1] virtual ids of each real row
  DevBuf<int> inv;           // [vrows] sorted position of each virtual id
};

// CSR cut into column chunks of SC columns, stored chunk-major with chunk-local 16-bit indices:
// sub-row (c, r) = entries off[c*rows + r] .. off[c*rows + r + 1].  Stage 1 gives chunk c of every
// transfer row to workgroups with blockIdx % nchunks == c, so one XCD's L2 only ever sees the
// sub-rows of "its" chunks (nchunks is a multiple of 8).
template <class T>
struct DevChunked {
  int64_t rows = 0, cols = 0, nnz = 0;
  int64_t stored = 0;          // entries incl. padding
  bool binary = false;         // every stored value == 1 (unweighted features): kernels may skip the value stream
  int SC = 0, nchunks = 0;
  int align = 1;               // sub-rows padded to whole units of `align` entries; off[] counts units.
                               // Padding entries carry local index SC (a zero operand row) and value 0; so do
                               // the sentinels in the class-pure tails of the stage-1 operands (align 1, 32:
                               // a sub-row's stored length can exceed its entry count, see chunk_tail).
  DevBuf<int> off;             // [nchunks*rows + 1]
  DevBuf<unsigned short> idx;  // [stored + 64]
  DevBuf<T> val;               // [stored + 64]
  DevBuf<unsigned short> len;  // align 32 only: exact stored length of every sub-row [nchunks*rows]
  bool len_ok = false;         //   ... all of them < 65536
  float vmax = 0.f, vmin = 0.f;  // largest / smallest non-zero |value|
};

// Mid-width W*R operand of round 3 (spmm_csell.hip): "compact sliced ELL".  Rows in slices of 64 (one lane per row),
// columns in chunks of KC (one LDS tile of R); block (chunk c, slice s) = c*nslices + s stores its entries pair by pair:
// step u holds entries 2u, 2u+1 of every lane whose sub-row has them, lanes in ascending order, nothing for the others,
// so a wave step is one coalesced 4-byte (two 16-bit local indices) and one 8-byte (two values) load per lane and memory
// holds no padding except the odd last entry of a sub-row (index KC = the zero row of the tile, value 0).  The order of
// the entries inside a sub-row is chosen when the operand is built so that lanes which read the same 16-byte slot of an
// LDS line in the same cycle hold tile rows of different bank classes (tile rows narrower than 256 bytes).
template <class T>
struct DevCsell {
  int64_t rows = 0, cols = 0, nnz = 0;
  int KC = 0, nchunks = 0, nslices = 0;
  int QT = 0;                     // tile width (columns of R per tile row) the entry order was scheduled for: QT * sizeof(T) = 64, 128 or 256 bytes
  bool binary = false;            // every value 1: no value stream
  bool ok = false;                // built (false: not yet, or the matrix does not fit the format -> the 2-D kernel serves it)
  int64_t npairs = 0;
  DevBuf<int> desc;               // [nblocks + 1][2] {first pair, steps}; the last block is empty
  DevBuf<unsigned short> np;      // [(nblocks + 1) * 64] pairs per lane
  DevBuf<unsigned> pidx;          // [npairs + 64]
  DevBuf<T> pval;                 // [2 * (npairs + 64)] unless binary
};

// Dense-similarity regime: the raw similarities stay dense on the device (column-major), the cutoff is
// applied inside the stage-1 GEMM (dense.hip).
template <class T>
struct DenseSim {
  bool on = false;
  int64_t nq = 0, ns = 0, nf = 0;
  T alpha = T(0);
  bool weighted = true;
  DevBuf<T> Sq, Ss;       // nq x nf and ns x nf, column-major, ld = rows
  DevBuf<T> inv_kf_m1;    // 1/(kf-1): leave-one-out coefficient
  // bf16 planes of the thresholded operands (dense_bf16.hip): source side once per graph, query side per row block
  DevBuf<unsigned short> Bpl, Apl;
  int Bpl_np = 0;
  int64_t Bpl_Np = 0, Bpl_Kp = 0;
};

// Stage-1 coefficients of a left operand L, entry by entry: c[q] = L.val[q] * inv1[L.idx[q]] (query and source rows), or
// the leave-one-out coefficient of entry q of Xs.  They depend only on L and the degrees of the graph L is used with, so
// the handle that owns L keeps them from its first prediction on; `epoch` is the Graph::coef_epoch they were built at
// (0: not built).  The single-wave kernel then reads c[q] next to L.idx[q] instead of gathering inv1[a] (transfer.hip).
template <class T>
struct CoefTable {
  DevBuf<T> c;
  uint64_t epoch = 0;
  void drop() { c.release(); epoch = 0; }
};

template <class T>
struct Graph {
  int64_t nq = 0, ns = 0, nf = 0, nt = 0;
  bool general = false;
  DenseSim<T> dense;  // built by ss_graph_create_general: only Xq, XsT, YsT and kf == ks are set
  DevCsr<T> Xq;    // nq x nf
  DevCsr<T> Xs;    // ns x nf
  DevCsr<T> XsT;   // nf x ns
  DevCsr<T> Ys;    // ns x nt
  DevCsr<T> YsT;   // nt x ns   (the W of F = W*R)
  DevBuf<int> kf, ks, kt;           // count degrees in B
  DevBuf<T> inv_kf, inv_ks, inv_kt; // 1/k, 0 where k == 0   (the Inf/NaN -> 0 rule)
  // stage-2 operand, built lazily per tile width
  DevSell<T> W;
  int W_qt = 0;
  DevChunked<T> XsTc, YsTc;  // stage-1 operands (YsTc only for source rows), built lazily
  DevChunked<T> XsTb;        // stage-1 operand of the query-block kernel (sub-rows padded to L2 sectors), built lazily
  DevBuf<T> Cq;              // workspace of that kernel: Xq[r,a] * inv_kf[a], entry by entry
  // coefficient tables of the graph's own left operands: Xq * inv_kf, Xs * inv_kf, Ys * inv_kt, Xs * 1/(kf-1) (LOO).
  // Whatever writes kf / kt or their reciprocals, or replaces Xq / Xs / Ys, calls coef_drop(): the tables go and every
  // table a query set holds for this graph is out of date (its epoch no longer matches).
  CoefTable<T> coef_q, coef_s, coef_y, coef_loo;
  uint64_t coef_epoch = 1;
  void coef_drop() {
    coef_q.drop(); coef_s.drop(); coef_y.drop(); coef_loo.drop();
    ++coef_epoch;
  }
  DevBuf<T> Tws;  // workspace: rows of the transfer block T between stage 1 and stage 2
  DevBuf<T> Sws;  // workspace: sorted-order scores of a skew-sorted stage-2 operand
};

template <class T>
struct SpMat {
  DevCsr<T> csr;
  DevSell<T> sell;
  int sell_qt = 0;
  DevChunked<T> narrow[3];  // quad-aligned chunked operands of the narrow kernel for B <= 1, 2, 4 (built lazily)
  DevChunked<T> col[3];     // operands of the 2-D kernel: 64-, 128- and 256-byte tile rows (built lazily)
  DevCsell<T> csell[6];     // operands of the lane-per-row kernel for 64-, 128-, 256- and (fp32, B <= 8) 32-byte tile rows (built lazily)
  bool csell_tried[6] = {false, false, false, false, false, false};
  DevBuf<T> partial;        // partial sums of the narrow / 2-D kernels (and the padded copy of R, spmm_colgroup.hip)
};

// ---- assemble.hip
template <class T>
int csr_from_user(int64_t rows, int64_t cols, const int64_t* ptr, const int32_t* idx, const T* val,
                  int index_base, int mem, DevCsr<T>& out);
template <class T>
int csr_from_dense(const T* S, int64_t rows, int64_t cols, int64_t ld, bool apply_cutoff, T alpha,
                   bool weighted, int mem, DevCsr<T>& out);
template <class T>
int csr_transpose(const DevCsr<T>& in, DevCsr<T>& out);
template <class T>
int sell_build(const DevCsr<T>& in, int KCmax, DevSell<T>& out, int qt = 0);   // qt = 0: sell_tile_width<T>()
template <class T>
int chunked_build(const DevCsr<T>& in, int SC, int align, DevChunked<T>& out);
template <class T>
int csell_build(const DevCsr<T>& in, int KC, int QT, DevCsell<T>& out);   // out.ok == false: not representable (no error)
template <class T>
int graph_finalize(Graph<T>& g);  // transposes + degrees
template <class T>
int graph_degrees(Graph<T>& g);   // kf, ks, kt and their reciprocals from the row pointers of XsT, Xs + Ys, YsT (synchronises)
template <class T>
int graph_finalize_general(Graph<T>& g);  // degrees = row counts of B (held in XsT)
template <class T>
int graph_finalize_general_targets(Graph<T>& g);  // kt / inv_kt from YsT only

// ---- kernels.hip, transfer.hip (launch wrappers; everything is enqueued on ctx().stream)
template <class T>
struct CsrView {
  const int* ptr;
  const int* idx;
  const T* val;
};
template <class T>
inline CsrView<T> view(const DevCsr<T>& m) { return CsrView<T>{m.ptr.p, m.idx.p, m.val.p}; }

template <class T>
int launch_cutoff(const T* X, int64_t rows, int64_t cols, int64_t ld, T alpha, bool weighted, T* out, int64_t ldo);
template <class T>
int launch_row_degree(const T* G, int64_t rows, int64_t cols, int64_t ld, int* deg);
template <class T>
int launch_spread_dense(const T* G, int64_t rows, int64_t cols, int64_t ld, const int* deg, T* W, int64_t ldw);

// stage 1: T[r][j] = inv2[j] * sum_terms sum_a L[r,a] * inv1[a] * Mt[a][j]   (rows row_begin..+nrows)
// all Mt operands must share SC / nchunks.  coef: per term the coefficient table of L (transfer_coef_build) or NULL;
// with a table for every term the default kernels read it instead of gathering inv1 (SS_TRANSFER_COEF=0: never).
template <class T>
int launch_transfer(int nterms, const DevCsr<T>* L[2], const T* inv1[2], const DevChunked<T>* Mt[2],
                    const T* inv2, int64_t row_begin, int64_t nrows, int64_t nj, T* out, int64_t ld,
                    const int* row_ids = nullptr, bool accumulate = false, const T* const* coef = nullptr);
// coef[q] of every entry q of L, by the expression the kernel uses when it gathers: L.val[q] * inv1[L.idx[q]], or with
// kf_loo the leave-one-out coefficient (row != feature and kf - 1 > 0) ? L.val[q] * (1 / (kf - 1)) : 0
template <class T>
int transfer_coef_build(const DevCsr<T>& L, const T* inv1, const int* kf_loo, T* coef);
// stage 1 for plain query rows, query-block workgroups: sub-row offsets in LDS, coefficients precomputed into `coef`
// (L.nnz values of workspace).  transfer_block_fits: whether offsets + >= 8 waves of accumulators fit in LDS.
template <class T>
int launch_transfer_block(const DevCsr<T>& L, const T* inv1, const DevChunked<T>& Mt, const T* inv2, int64_t row_begin,
                          int64_t nrows, int64_t nj, T* out, int64_t ld, T* coef, float xmax, bool fixed);
template <class T>
bool transfer_block_fits(int64_t mrows, int SC);
// k-fold: degrees / reciprocal degrees of the graph without the members of one fold
template <class T>
int launch_fold_degrees(const DevCsr<T>& X, const DevCsr<T>& XT, const DevCsr<T>& Y, const int* members,
                        int64_t nmembers, int* kf, int* ks, int* kt);
template <class T>
int launch_fold_inverse(const int* kf, const int* ks, const int* fold, int phi, int64_t nf, int64_t ns, T* inv_kf,
                        T* inv_ks);
// leave-one-out flavour: row i of X against X' with the rank-1 degree corrections
template <class T>
int launch_transfer_loo(const DevCsr<T>& X, const DevChunked<T>& XT, const int* kf, const int* ks,
                        int64_t i_begin, int64_t nrows, T* out, int64_t ld, const T* coef = nullptr);

// stage 2, wide: F[b][m] = sum_k W[m][k] * R[b][k]   (R, F "column-major": one row of length K / M per b)
template <class T>
int sell_tile_width();  // QT for this T
template <class T>
int sell_max_chunk(int qt);
template <class T>
int launch_spmm_sell(const DevSell<T>& W, const T* R, int64_t ldr, int64_t B, T* F, int64_t ldf,
                     const int* clean_deg, const int* out_rows = nullptr);
// stage 2, narrow (serves B <= 7 by default, built for B <= 16): R chunk in LDS, W streamed once in chunk-major order
template <class T>
int narrow_chunk_cols(int bv);  // KC for a padded width bv
template <class T>
int launch_spmm_chunked_narrow(const DevChunked<T>& W, int bv, const T* R, int64_t ldr, int B, T* F, int64_t ldf,
                               DevBuf<T>& partial);
// stage 2, mid width (5 <= B, B*sizeof(T) <= 256 bytes): 2-D cut (row blocks x chunk groups) with conflict-free gathers
// (spmm_colgroup.hip): tile rows of 64, 128 or 256 bytes (fp32: B <= 16, 32, 64; fp64: B <= 8, 16, 32); same chunked
// operand format as the narrow kernel
// ---- spmm_csell.hip (5 <= B, B * sizeof(T) <= 256 bytes, row-major R and F)
int csell_chunk_cols(int rowb);   // tile rows (of rowb bytes) that fit in LDS next to the zero row
template <class T>
int launch_spmm_csell(const DevCsell<T>& W, const T* R, int64_t ldr, int B, T* F, int64_t ldf, DevBuf<T>& partial);
template <class T>
int colgroup_chunk_cols(int bv);
template <class T>
int launch_spmm_colgroup(const DevChunked<T>& W, int bv, const T* R, int64_t ldr, int B, T* F, int64_t ldf,
                         DevBuf<T>& partial);

// similarity producer of the reference's tutorial: weighted Jaccard between the rows of a feature matrix
template <class T>
int launch_jaccard(const T* F, int64_t n, int64_t d, int64_t ld, T* S, int64_t lds);

int launch_topl(const float* scores, int64_t nrows, int64_t ncols, int64_t ld, int L, int* oidx, float* oval);
// metrics.hip: AuROC, AuPRC, BEDROC(alpha), validity ratio of one score vector (device inputs, host outputs)
int launch_rank_metrics(const unsigned char* y, const float* yhat, int64_t n, double alpha, double* out4);

// rank_rows.hip: the six per-row ranking metrics of a row-major score block against CSR positives (device inputs and
// out, enqueued on the stream).  Row r's positives are yidx[yptr[r] - shift .. yptr[r+1] - shift), values - base;
// host_ptr is a host copy of yptr[0..nrows].  validate: sorted, unique, in range (syncs; SS_EINVAL otherwise).
template <class PtrT>
int launch_rank_rows_validate(const PtrT* yptr, int64_t shift, const int* yidx, int base, int64_t nrows, int64_t ncols);
template <class T, class PtrT>
int launch_rank_rows(const PtrT* yptr, int64_t shift, const int* yidx, int base, const PtrT* host_ptr, const T* yhat,
                     int64_t nrows, int64_t ncols, int64_t ld, double alpha, int L, double* out);
// binary_rows.hip: max / mean / std over every threshold of the six binary prediction metrics, per row of a row-major
// score block against CSR positives (device inputs and out, enqueued on the stream; out[r*18 + 3*m + s]).  Labels as
// for launch_rank_rows, checked beforehand by launch_rank_rows_validate.
template <class T, class PtrT>
int launch_binary_rows(const PtrT* yptr, int64_t shift, const int* yidx, int base, const T* yhat, int64_t nrows,
                       int64_t ncols, int64_t ld, double* out);
// ---- pooled.hip: (score, label) pairs pooled into a table of distinct scores with int64 counts of positives and
// negatives.  Scores are order-preserving unsigned keys (u32 for fp32, u64 for fp64, -0.0 -> +0.0's key); a table's keys
// are unique and descending.  A pool is a list of tables ("levels") whose union is its table.
template <class T>
using pool_key_t = typename std::conditional<sizeof(T) == 4, uint32_t, uint64_t>::type;
template <class K>
struct PoolTable {
  DevBuf<K> key;
  DevBuf<int64_t> npos, nneg;
  int64_t n = 0;  // entries
};
template <class K>
struct PoolWork {  // scratch reused across blocks
  DevBuf<K> s, s2, q, q2, qkey;
  DevBuf<int64_t> cnt, inc, rstart, qcnt;
  DevBuf<unsigned char> tmp;
  DevBuf<int> flag;
};
// the table of a row-major score block against CSR positives (labels as for launch_rank_rows, checked beforehand);
// SS_EINVAL when a score is NaN.  nnz = number of label entries of the block.
template <class T, class PtrT>
int pool_block_table(const PtrT* yptr, int64_t shift, const int* yidx, int base, int64_t nnz, const T* yhat,
                     int64_t nrows, int64_t ncols, int64_t ld, PoolWork<pool_key_t<T>>& w, PoolTable<pool_key_t<T>>& out);
// push a table onto the levels (merging levels of at most twice its size); SS_ENOMEM and the levels untouched when
// other + the entries stored afterwards exceed max_entries
template <class K>
int pool_push(std::vector<PoolTable<K>>& lv, PoolTable<K>&& t, int64_t other, int64_t max_entries, PoolWork<K>& w);
template <class K>
int pool_union(const std::vector<PoolTable<K>>& lv, PoolWork<K>& w, PoolTable<K>& out);
template <class K>
int pool_consolidate(std::vector<PoolTable<K>>& lv, PoolWork<K>& w);
template <class K>
int64_t pool_stored(const std::vector<PoolTable<K>>& lv);
// a caller's table (device arrays: scores, npos, nneg) checked and keyed; P / N: its pair counts
template <class T>
int pool_import_table(const T* v, const int64_t* np, const int64_t* nn, int64_t n, PoolWork<pool_key_t<T>>& w,
                      PoolTable<pool_key_t<T>>& out, int64_t* P, int64_t* N);
template <class T>
int pool_export_table(const PoolTable<pool_key_t<T>>& t, T* v);
// the 21 pooled numbers of one table (host out)
template <class K>
int pool_table_metrics(const PoolTable<K>& t, int64_t P, int64_t N, PoolWork<K>& w, double* out);
// ---- target_topl.hip: per target the L best rows under (score desc by isless, row asc).  Entry j of target t lies at
// t*L + j of key / row / lab; the first `fill` entries of every target are valid and sorted.  Keys are order-preserving
// unsigned images of the scores WITHOUT -0.0 -> +0.0 (isless ranks +0.0 before -0.0).
template <class K>
struct TlTable {
  DevBuf<K> key;
  DevBuf<int64_t> row;
  DevBuf<uint8_t> lab;
  DevBuf<int64_t> npos;  // nt positives seen per target
};
template <class K>
struct TlWork {  // scratch reused across blocks
  int64_t cap = 0;  // candidates kept per target per block (more: the long-list route)
  DevBuf<K> ck, thk;
  DevBuf<int64_t> cr, thr;
  DevBuf<uint8_t> cl;
  DevBuf<int> cnt, act, ovf, ctr, flag;
};
template <class K>
int tl_alloc(TlTable<K>& t, int64_t nt, int L);
// b = a (the first `fill` entries of every target and npos)
template <class K>
int tl_copy(const TlTable<K>& a, TlTable<K>& b, int64_t nt, int L, int64_t fill);
// scratch for one add; clears the add's flags
template <class K>
int tl_begin(TlWork<K>& w, int64_t nt, int L);
// One row-major score block (nb x nt, ld) into t, enqueued only: its rows are row_begin + r (rowmap == NULL) or
// rowmap[r]; labels as for launch_rank_rows (checked beforehand).  fill: entries per target before the block.
template <class T, class PtrT>
int tl_add_block(TlTable<pool_key_t<T>>& t, int64_t nt, int L, int64_t fill, const PtrT* yptr, int64_t shift,
                 const int* yidx, int base, int64_t nnz, const T* yhat, int64_t nb, int64_t ld, int64_t row_begin,
                 const int* rowmap, TlWork<pool_key_t<T>>& w);
// the add's verdict (syncs): SS_EINVAL when a score was NaN; names the long-list route when it ran
template <class K>
int tl_finish(TlWork<K>& w);
// out = top L of a (fa entries per target) and b (fb), npos added
template <class K>
int tl_merge_tables(const TlTable<K>& a, int64_t fa, const TlTable<K>& b, int64_t fb, int64_t nt, int L,
                    TlTable<K>& out);
// a caller's table (device arrays, nt x fill row-major) checked and keyed into out (fill <= L)
template <class T>
int tl_import_table(const T* vals, const int64_t* rows, const uint8_t* labels, const int64_t* npos, int64_t nt, int L,
                    int64_t fill, TlTable<pool_key_t<T>>& out, int64_t* P);
// the table as nt x fill row-major device arrays (any of them may be NULL)
template <class T>
int tl_export_table(const TlTable<pool_key_t<T>>& t, int64_t nt, int L, int64_t fill, T* vals, int64_t* rows,
                    uint8_t* labels);
// hits[t] = positives among target t's entries (device)
template <class K>
int tl_hits(const TlTable<K>& t, int64_t nt, int L, int64_t fill, int64_t* hits);
// ---- target_rank.hip: per-target ranking metrics from the positives and integer counts of negatives
// (include/simspread_hip_target_rank.h holds the contract and the count layout).  Collect phase: ct / cr / cv hold npos
// appended triples.  Count phase: st / sr / sv the same triples sorted by (target, score desc, row asc), off[nt + 1] the
// per-target offsets, counts the 3 npos + 6 nt int64 of the export format.  An add in the count phase accumulates into
// delta (hist | nz, 32-bit) and dmm (min keys | max keys) and only tr_count_commit adds them to counts.
template <class T>
struct TrState {
  int64_t nt = 0, rows = 0, npos = 0, rows_counted = 0;
  int phase = 0;
  DevBuf<int> ct, st, off;
  DevBuf<int64_t> cr, sr, counts;
  DevBuf<T> cv, sv;
  DevBuf<unsigned char> route;  // per tile of 64 targets: 1 = sealed positives and histograms in LDS
  int64_t tiles_lds = 0, tiles_large = 0;
  DevBuf<unsigned> delta;
  DevBuf<unsigned long long> dmm, flag;  // flag[0]: a NaN score; flag[1]: smallest (row << 32 | target) of a mismatch
  int64_t hist_len() const { return 3 * (npos + nt); }
  int64_t counts_len() const { return 3 * npos + 6 * nt; }
};
// clears the add's flags (and, in the count phase, its delta)
template <class T>
int tr_begin(TrState<T>& s);
// one row-major score block (nb x nt, ld), enqueued only; rows are row_begin + r (rowmap == NULL) or rowmap[r]; labels
// as for launch_rank_rows (checked beforehand).  collect: its positives are appended at entry `at` (capacity grows,
// contents kept); count: into delta
template <class T, class PtrT>
int tr_collect_block(TrState<T>& s, int64_t at, const PtrT* yptr, int64_t shift, const int* yidx, int base, int64_t nnz,
                     const T* yhat, int64_t nb, int64_t ld, int64_t row_begin, const int* rowmap);
template <class T, class PtrT>
int tr_count_block(TrState<T>& s, const PtrT* yptr, int64_t shift, const int* yidx, int base, int64_t nnz, const T* yhat,
                   int64_t nb, int64_t ld, int64_t row_begin, const int* rowmap);
// the add's verdict (syncs): SS_EINVAL for a NaN score or a positive that is not the sealed one
template <class T>
int tr_finish(TrState<T>& s);
// counts += delta (after tr_finish passed)
template <class T>
int tr_count_commit(TrState<T>& s);
template <class T>
int tr_seal(TrState<T>& s);
// device triples checked (targets in range, 0 <= rows < 2^31, no NaN) and appended at entry s.npos (npos unchanged)
template <class T>
int tr_append(TrState<T>& s, const int* targets, const int64_t* rows, const T* scores, int64_t n, bool check);
// do both hold the same sealed table, bit for bit (syncs)
template <class T>
int tr_same_table(const TrState<T>& a, const TrState<T>& b, bool* same);
// s.counts += a device table of the export layout; check: hist and nz entries must be >= 0 (SS_EINVAL, nothing added)
template <class T>
int tr_add_counts(TrState<T>& s, const int64_t* counts, bool check);
// out: nt x 6 doubles on the device
template <class T>
int tr_metrics(const TrState<T>& s, double alpha, int L, double* out);
// ---- support.hip: support lists.  Pair p reads transfer row slot[p] of Trows (row-major, leading dimension ldt) and row
// tgt[p] of Ys' and writes entry pos[p] of src / contrib (M slots each) and nsupp: the sources s with
// Trows[slot][s] * Ys'[t][s] != 0 under (product descending by isless, s ascending), the first M of them and their count.
// All arrays on the device, enqueued on the stream; 1 <= M <= 64.
template <class T>
int launch_support(const DevCsr<T>& YsT, const T* Trows, int64_t ldt, const int* slot, const int* tgt, const int* pos,
                   int64_t npairs, int M, int* src, T* contrib, int* nsupp);
// ---- dense.hip (fp32 only: fp32-input MFMA)
int launch_transfer_dense(const DenseSim<float>& d, bool loo, const float* inv_k, const float* inv_n, const int* ks,
                          int64_t row_begin, int64_t nrows, float* out, int64_t ldo, bool source_rows = false);
template <class T>
int dense_degrees(Graph<T>& g);
// dense_bf16.hip: the same product on the bf16 matrix cores with the operands split into exact bf16 planes
int launch_transfer_dense_bf16(DenseSim<float>& d, bool loo, const float* inv_k, const float* inv_n, const int* ks,
                               int64_t row_begin, int64_t nrows, float* out, int64_t ldo, bool source_rows = false,
                               const int* row_ids = nullptr);
template <class T>
int dense_fold_degrees(const Graph<T>& g, const int* members, int64_t nm, int* kf, int* ks, int* kt);
// dense_f64.hip: the dense-similarity stage 1 in fp64 (fp64 MFMA; the reference's default precision)
int launch_transfer_dense_f64(const DenseSim<double>& d, bool loo, const double* inv_k, const double* inv_n, const int* ks,
                              int64_t row_begin, int64_t nrows, double* out, int64_t ldo, bool source_rows = false,
                              const int* row_ids = nullptr);

template <class T>
int launch_transpose(const T* in, int64_t rows, int64_t cols, int64_t ldin, T* out, int64_t ldout);
// out[r][t] = clean(sum_{v in vfirst[t]..vfirst[t+1]} in[r][inv[v]]): undo the row split + sort of a
// skew-sorted SELL operand (+ fused clean!)
template <class T>
int launch_unpermute(const T* in, int64_t ldin, int64_t nrows, int64_t nt, const int* vfirst, const int* inv,
                     const int* clean_deg, T* out, int64_t ldout);
// clean! for leave-one-out rows: target t whose only edge belongs to query i
template <class T>
int launch_loo_clean_fix(const DevCsr<T>& YsT, const int* kt, int64_t i_begin, int64_t nrows, T* out, int64_t ld);
// ---- kfold_rows.hip: k-fold row blocks come out in fold order.  scatter: row q of src -> row dst_rows[q] of dst;
// gather_labels: the Ys rows of members[0..nrows) into out, row q at out[pptr[q] - shift ..] (pptr: int64 row pointers
// of the gathered CSR, built on the host)
template <class T>
int launch_scatter_rows(const T* src, int64_t lds, int64_t nrows, int64_t ncols, const int* dst_rows, T* dst,
                        int64_t ldd);
int launch_gather_labels(const int* ys_ptr, const int* ys_idx, const int* members, int64_t nrows, const int64_t* pptr,
                         int64_t shift, int* out);

// ---- pair_csr.hip: the host skeleton shared by the fused thresholded-similarity producers (fingerprint.hip,
// jaccard_csr.hip, dot_csr.hip; their device skeleton is pair_tile.hpp) and by the streaming cutoff (recut.hip).  A
// producer's count pass writes the kept entries of every (column tile, row) slot into counts; scan() turns them into
// in-row offsets and a 64-bit scan of the row totals into ptr and nnz; the producer's fill pass writes every slot at
// ptr[i] + its offset in column order.  A producer's count() sets the members its kernel reads, sizes the output with
// begin() or begin_tiles() and ends in count_pass(); launch() is its one hook.
template <class T>
struct PairCsr {
  const char* what = "";  // producer name for messages
  int64_t na = 0, nb = 0;
  int64_t nti = 0, ntj = 0;  // row tiles (tiled producers), column tiles
  int64_t nnz = 0;      // set by count(), summed in 64 bits (may be >= 2^31: the caller refuses it)
  T alpha = T(0);
  bool weighted = true, sym = false;
  DevBuf<int> counts;   // [ntj][na] in-row offset of every (column tile, row) slot
  DevBuf<int> tile_nz;  // per launched tile, producers that ask for it: 1 when the count pass kept a pair in it (their
                        // fill pass skips the others)
  DevBuf<int64_t> ptr;  // [na + 1] row pointers
  virtual ~PairCsr() = default;
  int fill(int* idx, T* val, bool* binary);  // device idx[nnz], val[nnz] (val may be null); binary: every value == 1
  int to_dev_csr(DevCsr<T>& out);            // fill a DevCsr (SS_EUNSUPPORTED when nnz >= 2^31)

 protected:
  int begin(int64_t na, int64_t nb, int64_t tile);  // sizes, ptr (zeroed and synchronised when na or nb is 0)
  // begin() for tile x tile blocks of pairs, then (unless na or nb is 0) counts and, with_tile_nz, tile_nz; refuses
  // more tiles than one launch holds
  int begin_tiles(int64_t na, int64_t nb, int64_t tile, bool with_tile_nz);
  dim3 tile_grid() const;  // sym: the upper triangle of nti x nti tiles as a 1-D grid; else (ntj, nti)
  // SS_EINVAL when Fa (na x d, column-major, lda >= na; padding rows are not read) or, unless sym, Fb holds a NaN
  // (synchronises); called before begin(), so that nothing, the row pointers included, is written
  int refuse_nan_features(const T* Fa, int64_t na, int64_t lda, const T* Fb, int64_t nb, int64_t ldb, int64_t d);
  int count_pass() { SS_TRY(launch(false, nullptr, nullptr, nullptr)); return scan(); }
  int scan();  // counts -> offsets, row totals -> ptr, nnz (synchronises)
  // enqueue the producer's kernel: the count pass (fill == false: counts, tile_nz) or the fill pass (idx, val, which
  // may be null, and *flag = 1 when a value is not 1), over tile_grid() when it is tiled
  virtual int launch(bool fill, int* idx, T* val, int* flag) = 0;
};
// SS_EINVAL when Fa (na x d, column-major, lda >= na; padding rows are not read) or Fb (nullptr: no second side) holds
// a NaN (synchronises)
template <class T>
int refuse_nan_rows(const char* what, const T* Fa, int64_t na, int64_t lda, const T* Fb, int64_t nb, int64_t ldb,
                    int64_t d);
// the tile grid of na x nb pairs in tile x tile blocks: nti, ntj, and the blocks of one launch (sym: the upper triangle
// of nti x nti tiles); SS_EUNSUPPORTED when one launch does not hold them.  pair_tile_grid: that launch's grid.
int pair_tile_blocks(const char* what, int64_t na, int64_t nb, int64_t tile, bool sym, int64_t& nti, int64_t& ntj,
                     int64_t& nblocks);
dim3 pair_tile_grid(bool sym, int64_t nti, int64_t ntj);
// the members a producer names unqualified
#define SS_PAIR_CSR_MEMBERS(T)                                                                                       \
  using PairCsr<T>::what, PairCsr<T>::na, PairCsr<T>::nb, PairCsr<T>::nti, PairCsr<T>::ntj, PairCsr<T>::nnz,          \
      PairCsr<T>::alpha, PairCsr<T>::weighted, PairCsr<T>::sym, PairCsr<T>::counts, PairCsr<T>::tile_nz,              \
      PairCsr<T>::ptr

// ---- fingerprint.hip: thresholded Tanimoto similarity of packed binary fingerprints as CSR (two passes: count, fill).
// Fa (na x nwords) against Fb (nb x nwords), both device-resident uint64 rows; Fb == nullptr: Fb = Fa (symmetric).
template <class T>
struct TanimotoCsr : PairCsr<T> {
  SS_PAIR_CSR_MEMBERS(T);
  const uint64_t* Fa = nullptr;
  const uint64_t* Fb = nullptr;
  int64_t nwords = 0;
  DevBuf<int> pop_a, pop_b;  // popcount of every row (pop_b unused when Fb == Fa)
  bool self = false;         // Fb == Fa (sym says whether the triangle grid runs: not with a per-row cut)
  const T* tau = nullptr;    // per-row cut of the neighbour floor: entry (i, j) is also kept when 0 < s and s >= tau[i]
  DevBuf<T> tau_buf;
  // k > 0: the neighbour floor -- tau = tanimoto_kth(k) first, then the count pass over the full (ntj, nti) grid
  int count(const uint64_t* Fa, int64_t na, const uint64_t* Fb, int64_t nb, int64_t nwords, T alpha, bool weighted,
            int k = 0);

 protected:
  int launch(bool fill, int* idx, T* val, int* flag) override;
};

// ---- neighbour_floor.hip: tau[i] = the k-th largest of the positive Tanimoto similarities of row i of Fa against the
// rows of Fb (multiplicity counted), +0 when there are fewer than k; 1 <= k <= NEIGHBOUR_K_MAX.  Device pointers,
// Fb == nullptr: Fb = Fa; pop_a / pop_b: the row popcounts (pop_a == nullptr: computed here).  Enqueued on the stream;
// the scratch (na * k * column groups values) is freed after a synchronisation.  Bitwise repeatable.
constexpr int NEIGHBOUR_K_MAX = 64;
template <class T>
int tanimoto_kth(const uint64_t* Fa, int64_t na, const uint64_t* Fb, int64_t nb, int64_t nwords, const int* pop_a,
                 const int* pop_b, int k, T* tau);

// ---- jaccard_csr.hip: thresholded weighted Jaccard (Ruzicka) similarity of real-valued feature rows as CSR, bitwise
// what jaccard_kernel followed by the dense cutoff assembly gives.  Fa (na x d, column-major, lda >= na) against Fb
// (nb x d, ldb >= nb), both device-resident; Fb == nullptr: Fb = Fa (symmetric).  count() refuses NaN features with
// SS_EINVAL before anything is written.
template <class T>
struct JaccardCsr : PairCsr<T> {
  SS_PAIR_CSR_MEMBERS(T);
  const T* Fa = nullptr;
  const T* Fb = nullptr;
  int64_t lda = 0, ldb = 0, d = 0;
  bool self = false;       // Fb == Fa (sym says whether the triangle grid runs: not with a per-row cut)
  const T* tau = nullptr;  // per-row cut of the neighbour floor: entry (i, j) is also kept when 0 < s and s >= tau[i]
  DevBuf<T> tau_buf;
  // k > 0: the neighbour floor -- tau = jaccard_kth(k) first, then the count pass over the full (ntj, nti) grid
  int count(const T* Fa, int64_t na, int64_t lda, const T* Fb, int64_t nb, int64_t ldb, int64_t d, T alpha,
            bool weighted, int k = 0);

 protected:
  int launch(bool fill, int* idx, T* val, int* flag) override;
};

// ---- dot_csr.hip: thresholded inner-product similarity (metric: SS_SIM_COSINE, SS_SIM_TANIMOTO, SS_SIM_DICE) of
// real-valued rows as CSR; the Gram block of every 128 x 128 tile runs on the matrix cores in T (fp32 / fp64 MFMA).
// Layout, symmetric mode and the NaN refusal as for JaccardCsr; the rule is the header comment of dot_csr.hip.
template <class T>
struct DotCsr : PairCsr<T> {
  SS_PAIR_CSR_MEMBERS(T);
  const T* Fa = nullptr;
  const T* Fb = nullptr;
  int64_t lda = 0, ldb = 0, d = 0;
  int metric = 0;
  DevBuf<T> norm_a, norm_b;  // squared row norms of each side (norm_b unused when Fb == Fa)
  bool self = false;         // Fb == Fa (sym says whether the triangle grid runs: not with a per-row cut)
  const T* tau = nullptr;    // per-row cut of the neighbour floor, as JaccardCsr::tau
  DevBuf<T> tau_buf;
  // k > 0: the neighbour floor -- tau = dot_kth(k) first, then the count pass over the full (ntj, nti) grid
  int count(const T* Fa, int64_t na, int64_t lda, const T* Fb, int64_t nb, int64_t ldb, int64_t d, int metric, T alpha,
            bool weighted, int k = 0);

 protected:
  int launch(bool fill, int* idx, T* val, int* flag) override;
};
// norm[i] = sum_k F[i, k]^2 in T (enqueued on the stream): the squared row norms the producer and dot_kth share
template <class T>
int dot_row_norms(const T* F, int64_t n, int64_t ld, int64_t d, T* norm);

// ---- dot_csr.hip, 16-bit operands (include/simspread_hip_half.h): DotCsr<float> on rows stored as raw bf16 / fp16 bit
// patterns (storage: SS_H16_BF16 / SS_H16_F16), ROW-MAJOR -- element (i, k) at F[i * ld + k], ld >= d -- on the 16-bit
// matrix instructions with fp32 accumulation; the same tile kernel and epilogue.  Device pointers; Fb == nullptr: Fb = Fa
// (symmetric).  count() refuses a NaN pattern, an unknown storage or metric and a NaN alpha before anything is written.
// No neighbour floor: its selection pass (dot_kth) would have to run the same 16-bit Gram tile.
struct DotCsrH16 : PairCsr<float> {
  const uint16_t* Fa = nullptr;
  const uint16_t* Fb = nullptr;
  int64_t lda = 0, ldb = 0, d = 0;
  int storage = 0, metric = 0;
  DevBuf<float> norm_a, norm_b;  // squared row norms of each side (norm_b unused when Fb == Fa)
  int count(const uint16_t* Fa, int64_t na, int64_t lda, const uint16_t* Fb, int64_t nb, int64_t ldb, int64_t d,
            int storage, int metric, float alpha, bool weighted);

 protected:
  int launch(bool fill, int* idx, float* val, int* flag) override;
};

// what DotCsrH16::count does before its tile pass, for the other passes over 16-bit rows (cut_profile.hip):
// a side may use 16-byte loads; norm[i] = sum_k w(F[i, k])^2 in fp32 (enqueued); SS_EINVAL when an element k < d of Fa
// or (not nullptr) Fb is a NaN pattern (synchronises)
bool h16_fast(const uint16_t* F, int64_t ld);
int h16_row_norms(int storage, const uint16_t* F, int64_t n, int64_t ld, int64_t d, float* norm);
int h16_refuse_nan_rows(int storage, const uint16_t* Fa, int64_t na, int64_t lda, const uint16_t* Fb, int64_t nb,
                        int64_t ldb, int64_t d);

// ---- dot_csr.hip, int8 operands (include/simspread_hip_int8.h): DotCsr<float> on rows of signed 8-bit integers,
// ROW-MAJOR -- element (i, k) at F[i * ld + k], ld >= d -- on v_mfma_i32_32x32x32_i8 with exact int32 sums; the same tile
// kernel and epilogue.  Device pointers; Fb == nullptr: Fb = Fa.  d <= 131071, the metric, alpha and k are the caller's
// to check before anything is staged.  There is no NaN to refuse.
struct DotCsrI8 : PairCsr<float> {
  const int8_t* Fa = nullptr;
  const int8_t* Fb = nullptr;
  int64_t lda = 0, ldb = 0, d = 0;
  int metric = 0;
  DevBuf<float> norm_a, norm_b;  // (float) of the exact squared row norms (norm_b unused when Fb == Fa)
  bool self = false;             // Fb == Fa (sym says whether the triangle grid runs: not with a per-row cut)
  const float* tau = nullptr;    // per-row cut of the neighbour floor, as DotCsr::tau
  DevBuf<float> tau_buf;
  // k > 0: the neighbour floor -- tau = dot_kth_i8(k) first, then the count pass over the full (ntj, nti) grid
  int count(const int8_t* Fa, int64_t na, int64_t lda, const int8_t* Fb, int64_t nb, int64_t ldb, int64_t d, int metric,
            float alpha, bool weighted, int k = 0);

 protected:
  int launch(bool fill, int* idx, float* val, int* flag) override;
};
// a side may use 16-byte loads (16-byte-aligned base, ld % 16 == 0); norm[i] = (float) sum_k F[i, k]^2 (enqueued)
bool i8_fast(const int8_t* F, int64_t ld);
int i8_row_norms(const int8_t* F, int64_t n, int64_t ld, int64_t d, float* norm);
// real_floor.hip: dot_kth on int8 rows, s bit for bit the producer's (dot_tile_i8.hpp); norm_a / norm_b as there
int dot_kth_i8(const int8_t* Fa, int64_t na, int64_t lda, const int8_t* Fb, int64_t nb, int64_t ldb, int64_t d,
               int metric, const float* norm_a, const float* norm_b, int k, float* tau);

// ---- cut_profile.hip: cutoff profiles (include/simspread_hip_profile.h holds the rule).  For each of the ncuts
// nondecreasing, NaN-free cuts (host array, 1 <= ncuts <= 32: checked by the caller) total[b] = the nnz and
// rows[i * ncuts + b] (rows may be nullptr) = the row degrees of the CSR the plain producer builds at alpha = cuts[b],
// from ONE run of the producer's own tile pass over the producer's own grid.  Operands, total and rows on the device,
// operands as for the producers (Fb == nullptr: symmetric).  NaN features are refused (SS_EINVAL) before total or rows
// are written; both are complete on return (synchronises).  Bitwise repeatable.
template <class T>
int tanimoto_profile(const uint64_t* Fa, int64_t na, const uint64_t* Fb, int64_t nb, int64_t nwords, const T* cuts,
                     int ncuts, bool weighted, int64_t* total, int* rows);
template <class T>
int jaccard_profile(const T* Fa, int64_t na, int64_t lda, const T* Fb, int64_t nb, int64_t ldb, int64_t d,
                    const T* cuts, int ncuts, bool weighted, int64_t* total, int* rows);
template <class T>
int dot_profile(const T* Fa, int64_t na, int64_t lda, const T* Fb, int64_t nb, int64_t ldb, int64_t d, int metric,
                const T* cuts, int ncuts, bool weighted, int64_t* total, int* rows);
int dot_profile_h16(const uint16_t* Fa, int64_t na, int64_t lda, const uint16_t* Fb, int64_t nb, int64_t ldb, int64_t d,
                    int storage, int metric, const float* cuts, int ncuts, bool weighted, int64_t* total, int* rows);

// ---- real_floor.hip: the neighbour floor of the two producers above.  tau[i] = the k-th largest of the positive
// similarities s(i, j) of row i of Fa against the rows of Fb (multiplicity counted), +0 when there are fewer than k;
// 1 <= k <= NEIGHBOUR_K_MAX; s is bit for bit the producer's (jaccard_tile.hpp, dot_tile.hpp).  Device pointers, layout
// as for the producers, Fb == nullptr: Fb = Fa (dot: s(i, i) = 1).  norm_a / norm_b: the squared row norms (norm_a ==
// nullptr: computed here).  Enqueued on the stream; the scratch is freed after a synchronisation.  Bitwise repeatable.
// NaN features are the caller's to refuse.
template <class T>
int jaccard_kth(const T* Fa, int64_t na, int64_t lda, const T* Fb, int64_t nb, int64_t ldb, int64_t d, int k, T* tau);
template <class T>
int dot_kth(const T* Fa, int64_t na, int64_t lda, const T* Fb, int64_t nb, int64_t ldb, int64_t d, int metric,
            const T* norm_a, const T* norm_b, int k, T* tau);

// ---- recut.hip: featurize on a device CSR matrix (entry kept iff v >= alpha, alpha > 0; as v when weighted, else 1),
// two streaming passes over `in`, which must outlive the producer.  graph_recut: g = p with Xq, Xs, XsT cut, the labels
// copied and the degrees recounted; lazily built operands of g stay empty.
template <class T>
struct CutCsr : PairCsr<T> {
  SS_PAIR_CSR_MEMBERS(T);
  const DevCsr<T>* in = nullptr;
  int gshift = 6;  // log2 of the lanes that share a row
  int count(const DevCsr<T>& in, T alpha, bool weighted);

 protected:
  int launch(bool fill, int* idx, T* val, int* flag) override;
};
template <class T>
int graph_recut(const Graph<T>& p, T alpha, bool weighted, Graph<T>& g);

// ---- cluster.hip: Taylor-Butina clustering of an n x n neighbour pattern (include/simspread_hip_clusters.h).  ptr
// (n + 1 row pointers, the first == base), idx and the outputs are device arrays; row i holds idx[ptr[i] - base ..
// ptr[i + 1] - base), each entry shifted by base; nnz_in = ptr[n] - base, read by the caller.  validate: check the pointers and the indices on the device first
// (SS_EINVAL, nothing written); a pattern a producer of this library made needs no check.  centre[n], label[n], size
// (nullable, capacity n, the first *nclusters written); *nclusters and *rounds on the host.  Synchronises.  The stages
// are timed as ST_TRANSFER (symmetrise), ST_SPMM (rounds) and ST_EPILOGUE (assign and label).
int butina_csr(int64_t n, const int64_t* ptr, const int32_t* idx, int base, int64_t nnz_in, bool validate, int* centre,
               int* label, int* size, int64_t* nclusters, int64_t* rounds);
// SS_EINVAL unless the pointers are monotone within [0, nnz_in], every index is in 0..n-1 and (fold != nullptr) every
// fold id in 0..nfolds-1 (synchronises)
int pattern_check(int64_t n, const int64_t* ptr, const int32_t* idx, int base, int64_t nnz_in, const int32_t* fold,
                  int nfolds);
// count[f] (device, nfolds entries) = stored off-diagonal entries (i, j) with fold[i] == f != fold[j]; checks first
int cross_edges(int64_t n, const int64_t* ptr, const int32_t* idx, int base, int64_t nnz_in, const int32_t* fold,
                int nfolds, int64_t* count);
// host arrays: the largest-first fold assignment that keeps clusters whole
int cluster_folds(const int32_t* label, int64_t n, int64_t nclusters, int nfolds, int32_t* fold);

// ---- comm.hip: in-library score gather over RCCL (dlopen'ed), one process per GPU
int comm_unique_id(char* id128);
int comm_init(const char* id128, int rank, int nranks);
int comm_destroy();
int comm_info(int* rank, int* nranks);
int gather_rows(const void* local, int64_t ncols, const int64_t* counts, void* full, int root, int elem);

}  // namespace ss
