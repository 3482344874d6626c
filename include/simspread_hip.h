/*
 * simspread_hip.h -- C ABI of libsimspread_hip.so (MI355X / gfx950).
 *
 * Drop-in boundary for the SimSpread.jl hot path
 *     featurize -> construct -> spread -> predict -> clean!
 * The reference (cvigilv/SimSpread.jl, pure Julia) has no FFI of its own; its
 * boundary is the method table exported at src/SimSpread.jl:21-56.  Each entry
 * point below names the reference method it stands behind (file:line under the
 * reference tree).  Julia binds these with `ccall` (see INTEGRATION.md and
 * julia/SimSpreadHIP.jl), this repository's Python mirror binds them with ctypes.
 *
 * Conventions
 *   - plain C types only; no C++/torch types cross this boundary;
 *   - every function returns SS_OK (0) or a negative SS_E* code and never throws or
 *     aborts; ss_last_error() returns a thread-local message for the last failure;
 *   - one process drives one GPU (ss_init(device)); multi-GPU = one process per GPU,
 *     rows/folds sharded by the host layer, RCCL only for the final score gather
 *     (ss_comm_init / ss_gather_rows_*);
 *   - thread safety: state is handle-scoped.  Calls on DIFFERENT handles may come from several host threads /
 *     Julia tasks at once and overlap; calls on the same handle queue up on that handle's lock; ss_init /
 *     ss_shutdown / ss_set_stream / ss_reset_stream exclude everything else while they run.  ss_last_error,
 *     ss_timing_last and ss_path_last are per host thread;
 *   - `mem` says where caller buffers live: SS_MEM_HOST (copied during the call) or
 *     SS_MEM_DEVICE (used in place, e.g. a torch tensor's data_ptr()); the caller
 *     keeps ownership of every buffer it passes; the library owns what is behind
 *     the opaque handles;
 *   - CSR inputs: int64 row pointers, int32 column indices, `index_base` 0 or 1
 *     (Julia's SparseMatrixCSC is the 1-based CSR of the transpose), column
 *     indices sorted within each row; a NULL value pointer means "all ones";
 *     explicitly stored zeros are dropped (degree = number of NON-ZEROS,
 *     src/graphs.jl:9-11);
 *   - dense inputs are column-major with a leading dimension, like Julia arrays;
 *   - score blocks are written in the layout the caller asks for:
 *       SS_LAYOUT_ROWMAJOR  (r,t) at out[r*ld + t]   (numpy C order; native, no extra pass)
 *       SS_LAYOUT_COLMAJOR  (r,t) at out[r + t*ld]   (Julia Matrix; one device transpose).
 */
#ifndef SIMSPREAD_HIP_H
#define SIMSPREAD_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SS_VERSION 100 /* 0.1.0 */

enum {
  SS_OK = 0,
  SS_EINVAL = -1,       /* bad argument / shape / unsorted or out-of-range indices */
  SS_ENOMEM = -2,       /* device or host allocation failed */
  SS_EHIP = -3,         /* a HIP runtime call failed (message has the HIP error string) */
  SS_ENODEV = -4,       /* no usable gfx950 device / ss_init not called */
  SS_EUNSUPPORTED = -5, /* valid request this build cannot serve (e.g. nnz >= 2^31) */
  SS_EINTERNAL = -6     /* a bound the library sets for itself was exceeded: a defect, reported instead of looping on */
};

enum { SS_MEM_HOST = 0, SS_MEM_DEVICE = 1 };
enum { SS_ROWS_QUERY = 0, SS_ROWS_SOURCE = 1, SS_ROWS_LOO = 2 /* leave-one-out folds: ss_support_* only */ };
enum { SS_LAYOUT_ROWMAJOR = 0, SS_LAYOUT_COLMAJOR = 1 };
enum { SS_SIM_COSINE = 0, SS_SIM_TANIMOTO = 1, SS_SIM_DICE = 2 }; /* `metric` of ss_similarity_dot_csr_* */

typedef struct ss_graph ss_graph; /* tri-partite query/source/feature/target graph, device resident */
typedef struct ss_spmat ss_spmat; /* one sparse operand W of F = W*R, device resident            */
typedef struct ss_queries ss_queries; /* a block of query rows bound to one graph, device resident */

/* ---------------------------------------------------------------- runtime ---- */
int ss_version(void);
/* Hash of the kernel sources (the .hip and .hpp files of csrc/) this library was built from -- what profiles/ records next to its
 * counters; a loader that sees the sources can tell a stale library from a current one. */
const char* ss_source_hash(void);
const char* ss_last_error(void);
int ss_device_count(void);
/* Select the GPU this process drives and create the library's stream.  Replaces the
 * reference's `GPU::Bool` switch (src/core.jl:402,404,446,448). */
int ss_init(int device);
int ss_shutdown(void);
/* Run on the caller's HIP stream (e.g. torch's current stream) so that kernels that produced
 * SS_MEM_DEVICE inputs are ordered before the library's.  NULL is HIP's null (default) stream.
 * The caller keeps ownership of the stream.  ss_reset_stream() returns to the library's own
 * (non-blocking) stream. */
int ss_set_stream(void* hip_stream);
int ss_reset_stream(void);
int ss_synchronize(void);
/* Timings of the last predict/spmm call, milliseconds, measured with hipEvents on the
 * library stream: ms[0] whole call on device, [1] transfer stage (stage 1), [2] W*R SpMM
 * (stage 2), [3] epilogues/transposes, [4] host->device, [5] device->host,
 * [6] number of SpMM launches, [7] number of stage-1 launches.  Writes min(n,8) values. */
int ss_timing_last(double* ms, int n);
/* Which kernels the last predict / spmm / fingerprint call of this host thread went through: a comma-separated list of tags
 * ("tanimoto_csr_sym", "tanimoto_csr_cross", "jaccard_csr_sym", "jaccard_csr_cross", "dot_csr_sym", "dot_csr_cross", "cutoff_csr", "recut", "support", "transfer", "transfer_loo", "transfer_dense_bf16_ring", "transfer_dense_bf16_128", "transfer_dense_f32_mfma", "transfer_dense_f32_mfma_256",
 * "spmm_sell", "spmm_sell_sorted", "spmm_csell", "spmm_colgroup", "spmm_chunked_narrow", ...), NUL-terminated, truncated
 * to n - 1 characters.  Lets a caller (and the parity tests) assert that a size-dependent routing decision was the one
 * expected.  Has no counterpart in the reference (its only switch is GPU::Bool, src/core.jl:402,404). */
int ss_path_last(char* buf, int n);
/* enable != 0: from now on the timings of successive calls add up (ss_timing_last returns the sums and launch
 * counts since the hold began) instead of replacing one another, so that a benchmark loop need not stop after
 * every call to read them; enable == 0: back to per-call timings. */
int ss_timing_hold(int enable);

/* ------------------------------------------------------------ final score gather ---- */
/* The one exchange of the multi-GPU path (north star: "RCCL over xGMI only for the final score gather"; the reference has
 * no counterpart -- no NCCL/MPI anywhere).  One process per GPU.  Rank 0 fills `id` (128 bytes) with ss_comm_unique_id,
 * the host framework hands those bytes to the other processes (MPI, Distributed.jl, torch.distributed: any channel), every
 * process calls ss_comm_init(id, rank, nranks) after ss_init(device).  RCCL is dlopen'ed at that point; a process that
 * never calls these functions never touches it.
 * ss_gather_rows_*: rank r holds counts[r] finished rows of the score matrix (`local`, counts[r] x ncols, row-major,
 * DEVICE memory); the ranks exchange them directly -- one receive per peer straight into its slice of `full`
 * (sum(counts) x ncols, row-major, DEVICE memory), one send per peer, one ncclGroup on the library stream -- so all
 * point-to-point xGMI links carry traffic at once.  root < 0: every rank receives the full matrix; root = r: only rank r
 * does (`full` may be NULL elsewhere).  Stream-ordered like a kernel launch: ss_synchronize() waits for it. */
int ss_comm_unique_id(char id[128]);
int ss_comm_init(const char id[128], int rank, int nranks);
int ss_comm_destroy(void);
int ss_comm_info(int* rank, int* nranks); /* nranks = 0 when no communicator exists */
int ss_gather_rows_f32(const float* local, int64_t ncols, const int64_t* counts, float* full, int root);
int ss_gather_rows_f64(const double* local, int64_t ncols, const int64_t* counts, double* full, int root);

/* ------------------------------------------------------ similarity producer -- */
/* The step before featurize in the reference's tutorial (docs/src/tutorial/fishers-flowers.jl:66,
 * `1 .- pairwise(Jaccard(), X, dims=1)`): S[i][j] = sum_k min(F[i,k],F[j,k]) / sum_k max(F[i,k],F[j,k]) between the
 * rows of the n x d feature matrix F (column-major, ld >= n); S is n x n column-major (lds >= n), symmetric with
 * unit diagonal; two all-zero rows have similarity 1 (Distances.jl: distance 0). */
int ss_similarity_jaccard_f32(const float* F, int64_t n, int64_t d, int64_t ld, float* S, int64_t lds, int mem);
int ss_similarity_jaccard_f64(const double* F, int64_t n, int64_t d, int64_t ld, double* S, int64_t lds, int mem);

/* featurize(1 .- pairwise(Jaccard(), F, dims=1), alpha, weighted) for binary fingerprints, as CSR
 * (src/core.jl:106-112; docs/src/tutorial/fishers-flowers.jl:66).  On 0/1 rows that similarity is Tanimoto:
 *     c = popcount(a & b), u = popcount(a) + popcount(b) - c, s = u == 0 ? 1 : T(c) / T(u)   (T = float / double)
 *     entry (i, j) is kept iff s >= alpha and v != 0, v = weighted ? s : 1
 * which is bitwise what ss_similarity_jaccard_* on the unpacked 0/1 rows followed by the cutoff assembly gives; the
 * dense n x n similarity never exists.
 * Layout: a fingerprint of d bits is nwords = ceil(d/64) little-endian uint64 words, bit k = bit k % 64 of word k / 64;
 * bits past d MUST be zero (the caller's contract).  Rows are contiguous: Fa is na x nwords row-major.  This is Julia's
 * BitVector.chunks layout: pass an nwords x n Matrix{UInt64} whose column i is fps[i].chunks.
 * Output: ptr[na + 1] (int64), idx[nnz] (int32, ascending within each row), val[nnz] (s when weighted, 1 otherwise;
 * val == NULL: not written), all in `mem`; deterministic run to run.
 * Fb == NULL: Fb = Fa, nb = na (symmetric; the Xs block, diagonal included).  idx == NULL: size query -- writes ptr and
 * *nnz only.  capacity < nnz: SS_EINVAL with *nnz set.  nnz >= 2^31: SS_EUNSUPPORTED with *nnz set, nothing else
 * written (use the dense-similarity graph). */
int ss_similarity_tanimoto_csr_f32(const uint64_t* Fa, int64_t na, const uint64_t* Fb, int64_t nb, int64_t nwords,
                                   float alpha, int weighted, int64_t* ptr, int32_t* idx, float* val,
                                   int64_t capacity, int64_t* nnz, int mem);
int ss_similarity_tanimoto_csr_f64(const uint64_t* Fa, int64_t na, const uint64_t* Fb, int64_t nb, int64_t nwords,
                                   double alpha, int weighted, int64_t* ptr, int32_t* idx, double* val,
                                   int64_t capacity, int64_t* nnz, int mem);

/* featurize(1 .- pairwise(Jaccard(), X, dims=1), alpha, weighted) for real-valued feature rows, as CSR
 * (src/core.jl:106-112; docs/src/tutorial/fishers-flowers.jl:66,95-96).  On non-negative rows that similarity is the
 * weighted Jaccard (Ruzicka) Σmin / Σmax:
 *     smin = smax = +0; for k = 0 .. d-1 in order, in T: smin += min(a_k, b_k), smax += max(a_k, b_k)
 *     s = smax == 0 ? 1 : smin / smax                    (T = float / double, one correctly rounded division)
 *     entry (i, j) is kept iff s >= alpha and v != 0, v = weighted ? s : 1
 * which is bitwise what ss_similarity_jaccard_* on the stacked rows followed by the cutoff assembly gives; the dense
 * n x n similarity never exists.  Negative and infinite features give what that route gives; a NaN feature or a NaN
 * alpha is SS_EINVAL, checked before anything is written.  d = 0: every pair has s = 1.
 * Layout: as ss_similarity_jaccard_*: Fa is na x d column-major with lda >= na (Fb likewise), i.e. a Julia Matrix with
 * one sample per row, or X.t().contiguous() of a torch (n, d) tensor.
 * Output and size protocol as ss_similarity_tanimoto_csr_*: ptr[na + 1] (int64), idx[nnz] (int32, ascending within each
 * row), val[nnz] (val == NULL: not written), all in `mem`; deterministic run to run.  Fb == NULL: Fb = Fa, nb = na
 * (symmetric).  idx == NULL: size query -- writes ptr and *nnz only.  capacity < nnz: SS_EINVAL with *nnz set.
 * nnz >= 2^31: SS_EUNSUPPORTED with *nnz set, nothing else written. */
int ss_similarity_jaccard_csr_f32(const float* Fa, int64_t na, int64_t lda, const float* Fb, int64_t nb, int64_t ldb,
                                  int64_t d, float alpha, int weighted, int64_t* ptr, int32_t* idx, float* val,
                                  int64_t capacity, int64_t* nnz, int mem);
int ss_similarity_jaccard_csr_f64(const double* Fa, int64_t na, int64_t lda, const double* Fb, int64_t nb, int64_t ldb,
                                  int64_t d, double alpha, int weighted, int64_t* ptr, int32_t* idx, double* val,
                                  int64_t capacity, int64_t* nnz, int mem);

/* featurize(S, alpha, weighted) with S an inner-product similarity of real-valued rows (learned embeddings, continuous
 * descriptors), as CSR; the dense n x n similarity never exists and the Gram blocks run on the matrix cores in full
 * T = float / double precision.  For row i of Fa and row j of Fb:
 *     g = sum_k a_k b_k, A = sum_k a_k^2, B = sum_k b_k^2, accumulated in T in an order the implementation chooses;
 *     everything after the three sums is fixed, in T, with correctly rounded sqrt, *, /:
 *       metric SS_SIM_COSINE    den = sqrt(A) * sqrt(B)   s = clamp(g / den, -1, 1)
 *       metric SS_SIM_TANIMOTO  den = (A + B) - g         s = g / den
 *       metric SS_SIM_DICE      den = A + B               s = (g + g) / den
 *       den == 0:               s = (A == 0 && B == 0) ? 1 : 0    (two all-zero rows are identical; d = 0: s = 1)
 *     Fb == NULL (symmetric): entry (i, i) has s = 1 exactly and entry (j, i) carries the bits of (i, j);
 *     entry (i, j) is kept iff s >= alpha and v != 0, v = weighted ? s : 1  (a NaN s, from infinite features, is dropped).
 * s of a pair does not depend on alpha, weighted or the run.  When every product and partial sum is exactly
 * representable in T (small-integer features), g, A and B are exact in any order and the CSR is bitwise defined by the
 * rule; otherwise g differs from the exact sum by at most the usual bound of a d-term sum in T.
 * A NaN feature or a NaN alpha is SS_EINVAL, checked before anything is written; so is a metric outside 0..2.  Any
 * other alpha is accepted.  Layout, output and size protocol exactly as ss_similarity_jaccard_csr_*. */
int ss_similarity_dot_csr_f32(const float* Fa, int64_t na, int64_t lda, const float* Fb, int64_t nb, int64_t ldb,
                              int64_t d, int metric, float alpha, int weighted, int64_t* ptr, int32_t* idx,
                              float* val, int64_t capacity, int64_t* nnz, int mem);
int ss_similarity_dot_csr_f64(const double* Fa, int64_t na, int64_t lda, const double* Fb, int64_t nb, int64_t ldb,
                              int64_t d, int metric, double alpha, int weighted, int64_t* ptr, int32_t* idx,
                              double* val, int64_t capacity, int64_t* nnz, int mem);

/* ------------------------------------------------------- cutoff / k / spread -- */
/* cutoff(X, alpha, weighted): out = x >= alpha ? (weighted ? x : 1) : 0, element-wise
 * (src/core.jl:37-43,55-60; `>=` inclusive per test/runtests.jl:46-47).  Also the value
 * part of featurize (src/core.jl:106-112).  rows x cols, column-major, ld >= rows. */
int ss_cutoff_f32(const float* X, int64_t rows, int64_t cols, int64_t ld, float alpha,
                  int weighted, float* out, int64_t ldo, int mem);
int ss_cutoff_f64(const double* X, int64_t rows, int64_t cols, int64_t ld, double alpha,
                  int weighted, double* out, int64_t ldo, int mem);
/* featurize(X, alpha, weighted) (src/core.jl:106-112) on a matrix that is already CSR: the reference's featurize takes
 * any X, so it also cuts an already-featurized one.  Output entry (i, j) exists iff the input stores v at (i, j),
 * v >= alpha (inclusive) and w = weighted ? v : 1 is non-zero; for alpha > 0 these are exactly the non-zeros of
 * ss_cutoff_* on the densified matrix.  alpha <= 0 or NaN: SS_EINVAL (an unstored zero would pass an unweighted cutoff
 * at alpha <= 0, which CSR cannot represent).  Input: rows x cols CSR as for ss_graph_create_csr_* (ptr[rows + 1] int64,
 * idx int32 strictly ascending within a row, index_base 0 or 1, val == NULL: every stored value is 1), checked the same
 * way.  Output and size protocol as ss_similarity_tanimoto_csr_*: optr[rows + 1] (int64), oidx[nnz] (int32, 0-BASED
 * whatever index_base is, ascending within each row), oval[nnz] (oval == NULL: not written), all in `mem`; deterministic
 * run to run.  oidx == NULL: size query -- writes optr and *nnz only.  capacity < nnz: SS_EINVAL with *nnz set.
 * Cost: the caller's CSR is first staged and checked like a graph block (ss_graph_create_csr_*: upload when `mem` is
 * host, one validating pass, one compaction into a device copy of idx and val -- also when `mem` is device), then cut
 * by two streaming passes over that copy (ss_path_last: "cutoff_csr"); about twice the traffic of the cut alone and a
 * temporary of the input's size.  ss_graph_recut_* cuts resident blocks directly and pays the two passes only. */
int ss_cutoff_csr_f32(int64_t rows, int64_t cols, const int64_t* ptr, const int32_t* idx, const float* val,
                      int index_base, float alpha, int weighted, int64_t* optr, int32_t* oidx, float* oval,
                      int64_t capacity, int64_t* nnz, int mem);
int ss_cutoff_csr_f64(int64_t rows, int64_t cols, const int64_t* ptr, const int32_t* idx, const double* val,
                      int index_base, double alpha, int weighted, int64_t* optr, int32_t* oidx, double* oval,
                      int64_t capacity, int64_t* nnz, int mem);
/* k(G): number of non-zeros in every row (src/graphs.jl:9-11). */
int ss_row_degree_f32(const float* G, int64_t rows, int64_t cols, int64_t ld, int64_t* deg, int mem);
int ss_row_degree_f64(const double* G, int64_t rows, int64_t cols, int64_t ld, int64_t* deg, int mem);
/* spread(G): W[i,j] = G[i,j] / k(i), rows of degree 0 give 0 (src/core.jl:365-371). */
int ss_spread_f32(const float* G, int64_t rows, int64_t cols, int64_t ld, float* W, int64_t ldw, int mem);
int ss_spread_f64(const double* G, int64_t rows, int64_t cols, int64_t ld, double* W, int64_t ldw, int mem);

/* ------------------------------------------------------------ graph handles --- */
/* construct(...) (src/core.jl:148-201,217-276,294-296,308-337): instead of the dense
 * N x N block matrices A and B the handle keeps the three non-zero blocks
 *     Xq = A[queries, features]  (nq x nf)    Xs = A[sources, features]  (ns x nf)
 *     Ys = A[sources, targets]   (ns x nt)
 * as CSR on the device together with their transposes and the count degrees kf, ks, kt
 * of B (spread, src/core.jl:365-371).  nq may be 0 (3-layer graph of src/core.jl:308-337). */
int ss_graph_create_csr_f32(int64_t nq, int64_t ns, int64_t nf, int64_t nt,
                            const int64_t* xq_ptr, const int32_t* xq_idx, const float* xq_val,
                            const int64_t* xs_ptr, const int32_t* xs_idx, const float* xs_val,
                            const int64_t* ys_ptr, const int32_t* ys_idx, const float* ys_val,
                            int index_base, int mem, ss_graph** out);
int ss_graph_create_csr_f64(int64_t nq, int64_t ns, int64_t nf, int64_t nt,
                            const int64_t* xq_ptr, const int32_t* xq_idx, const double* xq_val,
                            const int64_t* xs_ptr, const int32_t* xs_idx, const double* xs_val,
                            const int64_t* ys_ptr, const int32_t* ys_idx, const double* ys_val,
                            int index_base, int mem, ss_graph** out);
/* Same graph from dense column-major blocks; the similarity cutoff of featurize
 * (src/core.jl:106-112) is applied on the device while the CSR is assembled when
 * apply_cutoff != 0 (Sq, Ss raw similarities), otherwise non-zeros are kept as they are.
 * Y (ns x nt) keeps its non-zero values. */
int ss_graph_create_dense_f32(int64_t nq, int64_t ns, int64_t nf, int64_t nt,
                              const float* Sq, int64_t ldq, const float* Ss, int64_t lds,
                              const float* Y, int64_t ldy, int apply_cutoff, float alpha,
                              int weighted, int mem, ss_graph** out);
int ss_graph_create_dense_f64(int64_t nq, int64_t ns, int64_t nf, int64_t nt,
                              const double* Sq, int64_t ldq, const double* Ss, int64_t lds,
                              const double* Y, int64_t ldy, int apply_cutoff, double alpha,
                              int weighted, int mem, ss_graph** out);
/* Dense-similarity regime (thresholded similarity too full for CSR, e.g. 90 % of 50k x 50k): the raw
 * similarities stay dense on the device and featurize's cutoff (src/core.jl:106-112) is applied inside
 * the stage-1 product, which runs on the matrix cores (bf16 MFMA over exact bf16 planes of the fp32 operands;
 * SS_DENSE_BF16=0: fp32-input MFMA); the labels Y stay sparse (CSR, ns x nt).
 * Sq (nq x ns) and Ss (ns x ns) are column-major raw similarities whose columns are the features named
 * after the sources; nq may be 0.  Ss need not be symmetric: element (s, f), at Ss[s + f * lds], is source s (row)
 * against feature f (column), so kf counts a column and ks a row.  Serves ss_predict_f32 (query and source rows),
 * ss_predict_loo_f32 and ss_predict_kfold_f32.
 * _f32: bf16 matrix cores on exact bf16 planes (the reference's GPU=true precision, src/core.jl:404); _f64: the fp64
 * matrix instruction (the reference's default precision, src/core.jl:402 GPU=false).
 * Input domain, the same in every engine and in ss_graph_set_cutoff_*: the rule is featurize's
 * x >= alpha ? (weighted ? x : 1) : 0, and an edge is a non-zero result.  Any finite alpha is accepted, zero and negative
 * included: unweighted, alpha <= 0 makes every finite entry an edge (zeros and negatives too); weighted, a zero of either
 * sign is no edge and a negative weight is kept with its sign.  A NaN similarity is no edge anywhere.  Not supported:
 * +-Inf and, in _f32, magnitudes from 2^127 * (2 - 2^-8) up (they overflow the bf16 split of the operands); results
 * are then undefined, nothing is checked. */
int ss_graph_create_similarity_f32(int64_t nq, int64_t ns, int64_t nt,
                                   const float* Sq, int64_t ldq, const float* Ss, int64_t lds,
                                   const int64_t* y_ptr, const int32_t* y_idx, const float* y_val,
                                   int index_base, float alpha, int weighted, int mem, ss_graph** out);
int ss_graph_create_similarity_f64(int64_t nq, int64_t ns, int64_t nt,
                                   const double* Sq, int64_t ldq, const double* Ss, int64_t lds,
                                   const int64_t* y_ptr, const int32_t* y_idx, const double* y_val,
                                   int index_base, double alpha, int weighted, int mem, ss_graph** out);
/* construct(y, X, ...) with X = featurize(Tanimoto(F), alpha, weighted) for binary fingerprints (layout as in
 * ss_similarity_tanimoto_csr_*): Xq = cut(T(Fq, Fs)) (nq x ns), Xs = cut(T(Fs, Fs)) (ns x ns), the features named after
 * the sources (nf = ns); Y (ns x nt CSR) as in ss_graph_create_similarity_*.  The CSR blocks are produced on the device
 * (ss_path_last: "tanimoto_csr_sym", "tanimoto_csr_cross").  nq may be 0 (Fq may then be NULL).  Serves ss_predict_* (query
 * and source rows), ss_predict_loo_* and ss_predict_kfold_*. */
int ss_graph_create_fingerprint_f32(int64_t nq, int64_t ns, int64_t nt, int64_t nwords,
                                    const uint64_t* Fq, const uint64_t* Fs,
                                    const int64_t* y_ptr, const int32_t* y_idx, const float* y_val,
                                    int index_base, float alpha, int weighted, int mem, ss_graph** out);
int ss_graph_create_fingerprint_f64(int64_t nq, int64_t ns, int64_t nt, int64_t nwords,
                                    const uint64_t* Fq, const uint64_t* Fs,
                                    const int64_t* y_ptr, const int32_t* y_idx, const double* y_val,
                                    int index_base, double alpha, int weighted, int mem, ss_graph** out);
/* construct(y, X, ...) with X = featurize(J(F), alpha, weighted), J the weighted Jaccard similarity of real-valued
 * feature rows (layout and rule as in ss_similarity_jaccard_csr_*; src/core.jl:106-112,148-201;
 * docs/src/tutorial/fishers-flowers.jl:66,95-96): Xq = cut(J(Fq, Fs)) (nq x ns), Xs = cut(J(Fs, Fs)) (ns x ns), the
 * features named after the sources (nf = ns); Y (ns x nt CSR) as in ss_graph_create_similarity_*.  The CSR blocks are
 * produced on the device (ss_path_last: "jaccard_csr_sym", "jaccard_csr_cross").  nq may be 0 (Fq may then be NULL).
 * Serves ss_predict_* (query and source rows), ss_predict_loo_*, ss_predict_kfold_* and ss_evaluate_loo_*. */
int ss_graph_create_features_f32(int64_t nq, int64_t ns, int64_t nt, int64_t d,
                                 const float* Fq, int64_t ldq, const float* Fs, int64_t lds,
                                 const int64_t* y_ptr, const int32_t* y_idx, const float* y_val,
                                 int index_base, float alpha, int weighted, int mem, ss_graph** out);
int ss_graph_create_features_f64(int64_t nq, int64_t ns, int64_t nt, int64_t d,
                                 const double* Fq, int64_t ldq, const double* Fs, int64_t lds,
                                 const int64_t* y_ptr, const int32_t* y_idx, const double* y_val,
                                 int index_base, double alpha, int weighted, int mem, ss_graph** out);
/* construct(y, X, ...) with X = featurize(S(F), alpha, weighted), S the inner-product similarity `metric` of real-valued
 * rows (layout and rule as in ss_similarity_dot_csr_*): Xq = cut(S(Fq, Fs)) (nq x ns), Xs = cut(S(Fs, Fs)) (ns x ns), the
 * features named after the sources (nf = ns); Y (ns x nt CSR) as in ss_graph_create_similarity_*.  The CSR blocks are
 * produced on the device (ss_path_last: "dot_csr_sym", "dot_csr_cross").  nq may be 0 (Fq may then be NULL).
 * Serves ss_predict_* (query and source rows), ss_predict_loo_*, ss_predict_kfold_* and ss_evaluate_loo_*. */
int ss_graph_create_vectors_f32(int64_t nq, int64_t ns, int64_t nt, int64_t d, int metric,
                                const float* Fq, int64_t ldq, const float* Fs, int64_t lds,
                                const int64_t* y_ptr, const int32_t* y_idx, const float* y_val,
                                int index_base, float alpha, int weighted, int mem, ss_graph** out);
int ss_graph_create_vectors_f64(int64_t nq, int64_t ns, int64_t nt, int64_t d, int metric,
                                const double* Fq, int64_t ldq, const double* Fs, int64_t lds,
                                const int64_t* y_ptr, const int32_t* y_idx, const double* y_val,
                                int index_base, double alpha, int weighted, int mem, ss_graph** out);
/* General form for caller-built adjacency matrices: predict accepts ANY named A, B
 * (src/core.jl:402-425; the reference's own test passes hand-written 9 x 9 matrices,
 * test/runtests.jl:120-158).  With n nodes, the caller passes
 *     L  = A[rows of y, :]        (nr x n)   the rows of A that are asked for
 *     Bm = B                      (n  x n)   the graph spread() normalises
 *     Wt = (B[:, cols of y])'     (nc x n)   the columns of B that are asked for, transposed
 * and ss_predict_*(g, SS_ROWS_QUERY, 0, nr, ...) returns the nr x nc block of A * spread(B)^2.
 * Degrees are the row non-zero counts of B.  SS_ROWS_SOURCE / leave-one-out do not apply. */
int ss_graph_create_general_f32(int64_t n, int64_t nr, int64_t nc,
                                const int64_t* l_ptr, const int32_t* l_idx, const float* l_val,
                                const int64_t* b_ptr, const int32_t* b_idx, const float* b_val,
                                const int64_t* w_ptr, const int32_t* w_idx, const float* w_val,
                                int index_base, int mem, ss_graph** out);
int ss_graph_create_general_f64(int64_t n, int64_t nr, int64_t nc,
                                const int64_t* l_ptr, const int32_t* l_idx, const double* l_val,
                                const int64_t* b_ptr, const int32_t* b_idx, const double* b_val,
                                const int64_t* w_ptr, const int32_t* w_idx, const double* w_val,
                                int index_base, int mem, ss_graph** out);
/* Cutoff sweeps.  ss_graph_recut_*: a new, independent handle equal to `parent` with Xq and Xs (and the transpose of Xs)
 * replaced by their cutoff under the rule of ss_cutoff_csr_*; the labels are copied on the device, the degrees are
 * recounted, lazily built operands start empty.  The parent is untouched, stays usable and may be destroyed before the
 * child.  Nothing is re-read from the caller and no all-pairs producer or sort runs: the cost is two streaming passes
 * over the parent's three similarity blocks (ss_path_last: "recut").
 * Contract: for a parent built WEIGHTED at a cutoff a0 > 0 by ss_graph_create_fingerprint_*, _features_*, _vectors_*, _dense_* (with
 * apply_cutoff) and a child at alpha >= a0, the child is the graph the parent's own constructor builds at (alpha,
 * weighted): ss_graph_info, ss_graph_degrees and every score of ss_predict_*, ss_predict_loo_* and
 * ss_predict_kfold_rows_* match bit for bit, hence every evaluator too (the edges with s >= alpha are a subset of those
 * with s >= a0, and a weighted graph stores s itself).  For any other parent (ss_graph_create_csr_*, an unweighted
 * parent, alpha < a0) it is featurize applied to the stored X.  A child can be cut again.
 * alpha <= 0 or NaN: SS_EINVAL.  A general graph: SS_EUNSUPPORTED.  A dense-similarity graph: SS_EUNSUPPORTED (use
 * ss_graph_set_cutoff_*).  A handle of the other precision: SS_EINVAL.  On any error *out is NULL. */
int ss_graph_recut_f32(const ss_graph* parent, float alpha, int weighted, ss_graph** out);
int ss_graph_recut_f64(const ss_graph* parent, double alpha, int weighted, ss_graph** out);
/* The same for a dense-similarity graph (ss_graph_create_similarity_*), IN PLACE: the raw similarities are resident and
 * the cutoff is applied inside the stage-1 product, so a new cutoff only replaces (alpha, weighted) in the handle,
 * recounts the degrees and drops the cached bf16 planes of the thresholded source side; nothing is copied or re-staged,
 * and alpha may go down as well as up.  Afterwards every serving call gives, bit for bit, what a fresh
 * ss_graph_create_similarity_* at (alpha, weighted) gives.  Any alpha the constructor accepts is accepted.  A graph of
 * another kind: SS_EUNSUPPORTED (use ss_graph_recut_*), handle untouched.  SS_ENOMEM / SS_EHIP from the degree recount
 * (it re-allocates the degree buffers) leave the handle with the new cutoff and without valid degrees: call
 * ss_graph_set_cutoff_* again until it succeeds, or destroy the handle, before any serving call. */
int ss_graph_set_cutoff_f32(ss_graph* g, float alpha, int weighted);
int ss_graph_set_cutoff_f64(ss_graph* g, double alpha, int weighted);
int ss_graph_destroy(ss_graph* g);
/* sizes[0..6] = nq, ns, nf, nt, nnz(Xq), nnz(Xs), nnz(Ys) after dropping stored zeros.  A general graph reports
 * nr, n, n, nc, nnz(L), nnz(Bm), nnz(Wt). */
int ss_graph_info(const ss_graph* g, int64_t sizes[7]);
/* Count degrees of the query-free graph B: kf[nf], ks[ns], kt[nt] (host buffers; any may be NULL). */
int ss_graph_degrees(const ss_graph* g, int64_t* kf, int64_t* ks, int64_t* kt);

/* ------------------------------------------------------------------ predict --- */
/* predict((A,B), y) / predict(A,B,y) / predict(A, ytrain) (src/core.jl:402-425,446-466):
 * the block of F = A * spread(B)^2 for rows [row_begin,row_end) of the query nodes
 * (SS_ROWS_QUERY) or of the source nodes (SS_ROWS_SOURCE; feature path + target path,
 * which is also what the 3-layer predict(A, ytrain) returns) and all nt targets.
 * clean != 0 fuses clean! (src/core.jl:478-484): column t becomes -99 when target t
 * has no edge in A.  out holds (row_end-row_begin) x nt scores in `layout`.
 * With mem == SS_MEM_DEVICE and SS_LAYOUT_ROWMAJOR the kernels write straight into `out` and the call returns
 * once they are enqueued (stream order, like a kernel launch): work queued later on the same stream sees the
 * scores, anything else waits with ss_synchronize().  Every other combination returns with `out` complete. */
int ss_predict_f32(ss_graph* g, int rows_kind, int64_t row_begin, int64_t row_end, int clean,
                   float* out, int64_t ld, int layout, int mem);
int ss_predict_f64(ss_graph* g, int rows_kind, int64_t row_begin, int64_t row_end, int clean,
                   double* out, int64_t ld, int layout, int mem);
/* Leave-one-out cross-validation: row i of the result is
 *   predict(construct(y, X, [source_i]), y[[source_i], :])   (+ clean! when clean != 0)
 * for i in [i_begin, i_end), i.e. construct's fold form (src/core.jl:148-201) with
 * one query per fold, computed from the resident graph by rank-1 degree corrections
 * instead of rebuilding a graph per fold.  Needs a graph with nq == 0 and ns == nf whose
 * feature column j is the one named after source j (the column construct drops,
 * src/core.jl:152).  Folds are independent: shard [i_begin,i_end) across processes. */
int ss_predict_loo_f32(ss_graph* g, int64_t i_begin, int64_t i_end, int clean,
                       float* out, int64_t ld, int layout, int mem);
int ss_predict_loo_f64(ss_graph* g, int64_t i_begin, int64_t i_end, int clean,
                       double* out, int64_t ld, int layout, int mem);

/* k-fold cross-validation in one call: fold_of_source[i] in [0, nfolds) for every source i; row i of the
 * result is what the reference's fold loop computes for source i when its fold is the query set,
 *   predict(construct(y, X, fold_members), y[fold_members, :])  (+ clean!)   (src/core.jl:148-201,402-423),
 * i.e. the members of a fold are removed from the sources AND their feature columns are dropped
 * (src/core.jl:152-153), degrees recounted.  Needs a graph with nq == 0 and ns == nf whose feature column j
 * is the one named after source j.  out is ns x nt.  With one source per fold this equals leave-one-out. */
int ss_predict_kfold_f32(ss_graph* g, const int32_t* fold_of_source, int nfolds, int clean,
                         float* out, int64_t ld, int layout, int mem);
int ss_predict_kfold_f64(ss_graph* g, const int32_t* fold_of_source, int nfolds, int clean,
                         double* out, int64_t ld, int layout, int mem);
/* A row range of that sweep, so that k-fold shards across ranks like leave-one-out: row i - i_begin of out is bitwise
 * row i of ss_predict_kfold_*(g, fold_of_source, nfolds, clean), for every range and both layouts; out is
 * (i_end - i_begin) x nt in source order whatever the fold order.  A fold's degrees depend on all of its members, so the
 * whole fold_of_source (ns entries, in `mem` like out) is checked before anything is written: an id outside
 * 0..nfolds-1, nfolds < 1 or a bad range gives SS_EINVAL and out is untouched.  Only the folds with members in the
 * range are recounted and predicted; empty folds are allowed; nfolds == 1 holds every source out (all scores 0, -99
 * when cleaned).  i_begin == i_end: no-op after the argument checks.  Same graphs and preconditions as
 * ss_predict_kfold_* (CSR, dense-similarity, fingerprint and feature graphs). */
int ss_predict_kfold_rows_f32(ss_graph* g, const int32_t* fold_of_source, int nfolds, int64_t i_begin, int64_t i_end,
                              int clean, float* out, int64_t ld, int layout, int mem);
int ss_predict_kfold_rows_f64(ss_graph* g, const int32_t* fold_of_source, int nfolds, int64_t i_begin, int64_t i_end,
                              int clean, double* out, int64_t ld, int layout, int mem);

/* Ranked evaluation without moving the scores ("next" row of the scope table: recallatL / precisionatL,
 * src/performance.jl:308-385): for every row of a row-major score block the L best columns in the order
 * sortperm(yhat, rev=true) gives (score descending, ties by ascending column; as Julia's isless orders floats, +0.0 ranks
 * before -0.0 -- SimSpread scores are sums of non-negative products and clean!'s -99, so -0.0 does not occur in them).
 * idx and val are nrows x L,
 * row-major; L <= 1024 and L <= ncols.  With the labels of those columns recall@L and precision@L follow on
 * the host from nrows*L numbers instead of nrows*ncols scores. */
int ss_topl_f32(const float* scores, int64_t nrows, int64_t ncols, int64_t ld, int L,
                int32_t* idx, float* val, int mem);

/* Threshold-free evaluation of one score vector on the device ("next" row of the scope table):
 * out[0] = AuROC, out[1] = AuPRC (src/performance.jl:49-89: confusion matrix at every unique score, a sample is
 * predicted positive when score >= threshold, trapezoidal rule over exactly those points), out[2] =
 * BEDROC(alpha) (src/performance.jl:22-38; ranks in sortperm(yhat, rev=true) order), out[3] = validity ratio
 * (share of non-zero scores, src/performance.jl:558-560).  y: n labels (0 = negative, anything else =
 * positive), yhat: n scores; both host or both device (mem); out is always host memory.  n < 2^31.
 * AuROC/AuPRC are NaN when a class is missing, as in the reference. */
int ss_rank_metrics_f32(const uint8_t* y, const float* yhat, int64_t n, double alpha, double out[4], int mem);

/* Ranking metrics of every row of a score block, on the device (one vector per row, as src/performance.jl evaluates
 * one vector): out[r*6 + 0..5] = AuROC, AuPRC, BEDROC(alpha), validity ratio (src/performance.jl:22-89,558-560),
 * recall@L, precision@L (src/performance.jl:308-385).  Row r's scores are yhat[r*ld .. r*ld + ncols) (row-major,
 * ld >= ncols); its positives are the CSR column indices yidx[yptr[r] - index_base .. yptr[r+1] - index_base)
 * (pattern only: every stored entry is a positive; sorted, unique and in range, otherwise SS_EINVAL and nothing is
 * written; yptr[0] may exceed index_base, so a slice of a larger CSR can be passed as it is).  Each row follows
 * ss_rank_metrics_f32's conventions: order sortperm(yhat, rev=true) (score descending, ties by ascending column), a
 * confusion matrix at every unique score, trapezoid without a (0,0) point, AuROC/AuPRC NaN when a class is missing
 * and the row has two or more distinct scores, clean!'s -99 an ordinary score; recall@L / precision@L count the
 * positives of rank <= L, recall NaN without positives.  Scores must not be NaN.  out (nrows x 6 doubles, row-major)
 * lives in `mem` like the inputs and is complete on return.  nrows == 0: no-op.  ncols < 2, ncols >= 2^31, L < 1 or
 * L >= ncols ("Number of labels is less than length", src/performance.jl:311): SS_EINVAL.  Bitwise repeatable;
 * scratch O(nrows + nnz(labels)).  ss_path_last: "rank_rows_lds" (rows of at most 2048 positives) and/or
 * "rank_rows_large". */
int ss_rank_metrics_rows_f32(const int64_t* yptr, const int32_t* yidx, int index_base, const float* yhat, int64_t nrows,
                             int64_t ncols, int64_t ld, double alpha, int L, double* out, int mem);
int ss_rank_metrics_rows_f64(const int64_t* yptr, const int32_t* yidx, int index_base, const double* yhat, int64_t nrows,
                             int64_t ncols, int64_t ld, double alpha, int L, double* out, int mem);
/* A leave-one-out sweep evaluated in place: row i - i_begin of out (6 doubles as in ss_rank_metrics_rows_*) is fold i of
 * ss_predict_loo_*(g, i_begin, i_end, clean) ranked against the graph's own labels Ys[i, :] -- bitwise what
 * ss_predict_loo_* into a device buffer followed by ss_rank_metrics_rows_* gives, for every block_rows.  The library
 * streams blocks of block_rows folds through a score buffer of its own (0: its choice, about 1 GiB of scores); no
 * score leaves the device.  Same preconditions as ss_predict_loo_* (CSR, dense-similarity and fingerprint graphs).
 * out (n x 6 doubles) lives in `mem` and is complete on return. */
int ss_evaluate_loo_f32(ss_graph* g, int64_t i_begin, int64_t i_end, int clean, double alpha, int L, int64_t block_rows,
                        double* out, int mem);
int ss_evaluate_loo_f64(ss_graph* g, int64_t i_begin, int64_t i_end, int clean, double alpha, int L, int64_t block_rows,
                        double* out, int mem);

/* Binary prediction metrics of every row of a score block over all thresholds, on the device: for each of f1score, mcc,
 * accuracy, balancedaccuracy, recall, precision (m = 0..5, src/performance.jl:102-296) the max, mean and corrected std
 * (s = 0..2) of its value over the row's thresholds, as maxperformance / meanperformance / meanstdperformance
 * (src/performance.jl:420-520) give them: out[r*18 + 3*m + s].  Scores and labels are passed as for
 * ss_rank_metrics_rows_* (row-major yhat with ld >= ncols; CSR positives sorted, unique and in range, otherwise
 * SS_EINVAL and nothing is written; yptr[0] may exceed index_base).  Definition, row by row (n = ncols, P positives,
 * N = n - P):
 *   - the thresholds are the row's U distinct scores, sort(unique(yhat)); at threshold v a column is predicted positive
 *     iff score >= v, compared in the row's own type.  clean!'s -99 is an ordinary score; -0.0 equals +0.0; scores
 *     must not be NaN.
 *   - each metric is evaluated in double on the integer counts (tp, fp, tn, fn) exactly as the host mirror
 *     (simspread.jl_amd/metrics.py) writes it, mcc's four limit forms with eps = floatmin(Float64) included (they
 *     can reach +-Inf, as on the host).  mcc's numerator tp*tn - fp*fn and its denominator p_pred*n_pred*p_act*n_act
 *     are formed exactly (128-bit products) and each rounded to double once: bitwise the mirror's value.  The mirror
 *     (Python integers) is the definition here: Julia's own Int64 products overflow above about 110k balanced
 *     columns.
 *   - max; mean = sum / U; std = sqrt(sum((m - mean)^2) / (U - 1)) (StatsBase mean_and_std), NaN when U == 1.  A NaN
 *     at any threshold makes all three NaN (recall and balancedaccuracy when P == 0, balancedaccuracy when N == 0).
 * out (nrows x 18 doubles, row-major) lives in `mem` like the inputs and is complete on return.  nrows == 0: no-op.
 * ncols < 1 or ncols >= 2^31: SS_EINVAL.  Bitwise repeatable, and a row's values do not depend on the path that served
 * it.  ss_path_last: "binary_rows_lds" (ncols <= 16384: one workgroup sorts and reduces a row in LDS) or
 * "binary_rows_large" (segmented radix sort in device scratch of at most 2^25 elements per batch). */
int ss_binary_metrics_rows_f32(const int64_t* yptr, const int32_t* yidx, int index_base, const float* yhat,
                               int64_t nrows, int64_t ncols, int64_t ld, double* out, int mem);
int ss_binary_metrics_rows_f64(const int64_t* yptr, const int32_t* yidx, int index_base, const double* yhat,
                               int64_t nrows, int64_t ncols, int64_t ld, double* out, int mem);
/* A leave-one-out sweep judged by the binary metrics in place: row i - i_begin of out (18 doubles as in
 * ss_binary_metrics_rows_*) is fold i of ss_predict_loo_*(g, i_begin, i_end, clean) against the graph's own labels
 * Ys[i, :] -- bitwise what ss_predict_loo_* into a device buffer followed by ss_binary_metrics_rows_* gives, for every
 * block_rows (0: the library's choice, about 1 GiB of scores).  Same graphs and preconditions as ss_evaluate_loo_*.
 * out (n x 18 doubles) lives in `mem` and is complete on return. */
int ss_evaluate_loo_binary_f32(ss_graph* g, int64_t i_begin, int64_t i_end, int clean, int64_t block_rows, double* out,
                               int mem);
int ss_evaluate_loo_binary_f64(ss_graph* g, int64_t i_begin, int64_t i_end, int clean, int64_t block_rows, double* out,
                               int mem);
/* A k-fold sweep evaluated in place: row i - i_begin of out (6 doubles as in ss_rank_metrics_rows_*) is source i's row
 * of ss_predict_kfold_rows_*(g, fold_of_source, nfolds, i_begin, i_end, clean) ranked against the graph's own labels
 * Ys[i, :] -- bitwise what ss_predict_kfold_rows_* into a device buffer followed by ss_rank_metrics_rows_* gives, for
 * every block_rows.  The library streams blocks of block_rows members (fold order; 0: its choice, about 1 GiB of
 * scores) through a score buffer of its own, gathers the members' label rows in the same order and writes the metric
 * rows in source order; no score leaves the device.  fold_of_source, the range and the graphs as for
 * ss_predict_kfold_rows_* (checked whole before anything is written); alpha, L and nt as for ss_evaluate_loo_*.
 * i_begin == i_end: no-op after the argument checks.  out (n x 6 doubles) lives in `mem` and is complete on return.
 * ss_path_last names the metric paths used, as for ss_evaluate_loo_*. */
int ss_evaluate_kfold_f32(ss_graph* g, const int32_t* fold_of_source, int nfolds, int64_t i_begin, int64_t i_end,
                          int clean, double alpha, int L, int64_t block_rows, double* out, int mem);
int ss_evaluate_kfold_f64(ss_graph* g, const int32_t* fold_of_source, int nfolds, int64_t i_begin, int64_t i_end,
                          int clean, double alpha, int L, int64_t block_rows, double* out, int mem);
/* The same sweep judged by the binary metrics: row i - i_begin of out (18 doubles as in ss_binary_metrics_rows_*) --
 * bitwise ss_predict_kfold_rows_* followed by ss_binary_metrics_rows_* against Ys[i, :], for every block_rows.  Same
 * arguments, checks and limits as ss_evaluate_kfold_* and ss_evaluate_loo_binary_*. */
int ss_evaluate_kfold_binary_f32(ss_graph* g, const int32_t* fold_of_source, int nfolds, int64_t i_begin, int64_t i_end,
                                 int clean, int64_t block_rows, double* out, int mem);
int ss_evaluate_kfold_binary_f64(ss_graph* g, const int32_t* fold_of_source, int nfolds, int64_t i_begin, int64_t i_end,
                                 int clean, int64_t block_rows, double* out, int mem);

/* ------------------------------------------------------------- pooled evaluation ---- */
/* The reference judges a model on the whole score matrix, pooled: AuROC(Bool.(vec(ytest)), vec(yhat)), AuPRC(...)
 * (docs/src/tutorial/getting-started.jl, fishers-flowers.jl) and maxperformance(vec(y), vec(yhat), f1score) over a
 * cross-validation written out by `save`.  Those numbers depend only on the multiset of (score, label) pairs, so a pool
 * keeps a table of the DISTINCT scores, each with an int64 count of positives and of negatives: exact, mergeable in any
 * order (union of the scores, counts added), and built where the scores are produced.  A pool has one precision
 * (_f32 / _f64): scores are compared in it; -0.0 equals +0.0; clean!'s -99 is an ordinary score; NaN is refused.
 *
 * Out of scope: BEDROC depends on positions inside tie groups, which Julia breaks by the column-major vec order and
 * no sharded sweep reproduces; recall@L / precision@L are per group in the reference, not pooled: grouped by row they
 * are served by ss_rank_metrics_rows_* / ss_evaluate_*, grouped by target by ss_target_topl_* (below).
 *
 * Memory: the table holds one entry per distinct score (fp32: 4 + 16 bytes, fp64: 8 + 16).  An fp32 table is bounded
 * (at most about 2^31 distinct non-negative scores, plus -99 and the like); an fp64 sweep can have as many distinct
 * scores as scores.  While adds go on the table is kept as a few levels of decreasing size (an add's table absorbs the
 * top level while that holds at most twice its entries, so an entry is merged O(log adds) times, not once per block):
 * the entries stored can reach about twice the distinct scores until ss_pool_metrics / ss_pool_export merge them.
 * max_entries bounds the entries stored (0 at creation: the library's choice, half the device memory free at that
 * moment counted twice for a merge's double buffer).
 *
 * Every add (add_rows, add_loo, add_kfold, merge, import) is all or nothing: a NaN score, bad labels, a handle of the
 * other precision, bad arguments (SS_EINVAL) or more than max_entries entries stored afterwards (SS_ENOMEM) leave the
 * pool bitwise as it was.  ss_path_last names the sort ("pool_radix_u32" / "pool_radix_u64", rocPRIM radix sort of
 * the keys); ss_timing_last reports the call in ms[0] and the pooling's share of it in ms[3] (for add_loo / add_kfold
 * ms[1] and ms[2] are the prediction's stages). */
typedef struct ss_pool ss_pool; /* a pooled (score, label) table, device resident */
int ss_pool_create_f32(int64_t max_entries, ss_pool** out);
int ss_pool_create_f64(int64_t max_entries, ss_pool** out);
int ss_pool_destroy(ss_pool* pool);
/* empty the pool (max_entries stays) */
int ss_pool_reset(ss_pool* pool);
/* info[0] = pairs pooled, [1] = positives among them, [2] = table entries stored, [3] = max_entries */
int ss_pool_info(const ss_pool* pool, int64_t info[4]);
/* Pool every (score, label) pair of a row-major score block: scores and CSR positives exactly as for
 * ss_binary_metrics_rows_* (1 <= ncols < 2^31, ld >= ncols, labels sorted, unique, in range, yptr[0] may exceed
 * index_base; all in `mem`). */
int ss_pool_add_rows_f32(ss_pool* pool, const int64_t* yptr, const int32_t* yidx, int index_base, const float* yhat,
                         int64_t nrows, int64_t ncols, int64_t ld, int mem);
int ss_pool_add_rows_f64(ss_pool* pool, const int64_t* yptr, const int32_t* yidx, int index_base, const double* yhat,
                         int64_t nrows, int64_t ncols, int64_t ld, int mem);
/* Pool the leave-one-out folds [i_begin, i_end) against the graph's own labels Ys[i, :]: the pairs of
 * ss_predict_loo_*(g, i_begin, i_end, clean) -- the table is bitwise that of predict_loo into a device buffer followed
 * by ss_pool_add_rows_*, for every block_rows.  Blocks of block_rows folds stream through a score buffer of the
 * library's (0: its choice, about 1 GiB of scores), as in ss_evaluate_loo_*; same graphs and preconditions; no score
 * leaves the device.  The graph and the pool have the same precision. */
int ss_pool_add_loo_f32(ss_pool* pool, ss_graph* g, int64_t i_begin, int64_t i_end, int clean, int64_t block_rows);
int ss_pool_add_loo_f64(ss_pool* pool, ss_graph* g, int64_t i_begin, int64_t i_end, int clean, int64_t block_rows);
/* The same for the k-fold rows [i_begin, i_end) of ss_predict_kfold_rows_*(g, fold_of_source, nfolds, ...): arguments,
 * checks and blocks as for ss_evaluate_kfold_* (fold_of_source in `mem`). */
int ss_pool_add_kfold_f32(ss_pool* pool, ss_graph* g, const int32_t* fold_of_source, int nfolds, int64_t i_begin,
                          int64_t i_end, int clean, int64_t block_rows, int mem);
int ss_pool_add_kfold_f64(ss_pool* pool, ss_graph* g, const int32_t* fold_of_source, int nfolds, int64_t i_begin,
                          int64_t i_end, int clean, int64_t block_rows, int mem);
/* dst gains every pair of src (same precision; src is unchanged, dst == src doubles every count) */
int ss_pool_merge(ss_pool* dst, const ss_pool* src);
/* The table, scores descending: *count = its entries; keys == NULL: size query (count only).  Otherwise keys[k] (the
 * score), npos[k], nneg[k] for k < *count, all in `mem`; cap < *count: SS_EINVAL.  (Merges the levels first.) */
int ss_pool_export_f32(ss_pool* pool, float* keys, int64_t* npos, int64_t* nneg, int64_t cap, int64_t* count, int mem);
int ss_pool_export_f64(ss_pool* pool, double* keys, int64_t* npos, int64_t* nneg, int64_t cap, int64_t* count, int mem);
/* Add a table such as export writes (n entries in `mem`): scores strictly descending (after -0.0 -> +0.0) and not NaN,
 * counts >= 0, every entry with at least one pair; otherwise SS_EINVAL.  Tables of several ranks meet this way. */
int ss_pool_import_f32(ss_pool* pool, const float* keys, const int64_t* npos, const int64_t* nneg, int64_t n, int mem);
int ss_pool_import_f64(ss_pool* pool, const double* keys, const int64_t* npos, const int64_t* nneg, int64_t n, int mem);
/* The pooled numbers (host out): out[0] = AuROC, out[1] = AuPRC (the conventions of ss_rank_metrics_f32: a confusion
 * matrix at every distinct score, trapezoid without a (0,0) point, NaN when a class is missing and there are two or
 * more distinct scores), out[2] = validity ratio (share of non-zero scores), out[3 + 3*m + s] = max / mean / std over
 * every threshold of f1score, mcc, accuracy, balancedaccuracy, recall, precision as ss_binary_metrics_rows_* defines
 * them for one row (counts may pass 2^31: mcc's products are the host mirror's Python integers, rounded once).
 * Reductions run in a fixed order on the merged table: the 21 doubles are bitwise a function of the multiset of pairs,
 * whatever the blocks, their order, the ranks or block_rows.  An empty pool: SS_EINVAL. */
int ss_pool_metrics(ss_pool* pool, double out[21]);

/* ------------------------------------------------------------- per-target top-L ---- */
/* recallatL(y, yhat, grouping, L) and precisionatL(y, yhat, grouping, L) (src/performance.jl:308-409) with grouping =
 * the TARGET of every entry of vec(yhat): "for each target, are its true sources among the L highest-scored rows?"
 * (ss_rank_metrics_rows_* / ss_evaluate_* serve the grouping by row).  Inside a target group Julia's stable
 * sortperm(yhat_g, rev=true) orders the rows by (score descending, row ascending), vec being column-major; scores are
 * compared as isless does: +0.0 ranks before -0.0, clean!'s -99 is an ordinary score, NaN is refused.  Under that total
 * order the top L of a union of row blocks is the top L of the blocks' own top-L lists, so a handle keeps, per target,
 * the L best (score, row, label) entries seen so far -- nt x L entries on the device, exact and mergeable in any order
 * -- plus npos[t], the positives of target t over every row added.  Its rows are the virtual-screening result: per
 * target the best L compounds of everything added.
 *
 * Rows are int64 ids >= 0 chosen by the caller (add_rows: row_begin + r; add_loo / add_kfold: the source index) and
 * must be distinct across everything a handle absorbs.  A repeated id is not detected: both copies then compete as
 * separate entries (a row can take two places), which is no longer the reference's list.  Every row adds one entry to
 * every target, so every target holds fill = min(L, rows added) entries.
 *
 * Every add (add_rows, add_loo, add_kfold, merge, import) is all or nothing: a NaN score, bad labels, a handle of the
 * other precision, ncols != nt or other bad arguments (SS_EINVAL) leave the handle bitwise as it was.  ss_path_last
 * names the kernels: "target_topl_seed" (while a target holds fewer than L entries: its top L of them and
 * of the block's first max(L - fill, 2L, 512) rows), "target_topl_filter" (one pass over the
 * block keeps the scores that beat their target's L-th entry), "target_topl_merge_lds" (per target, candidates sorted
 * and merged in LDS) and "target_topl_merge_large" (the long-list route: a target with more candidates than the LDS
 * path holds is served by a radix select over its whole column of the block).  ss_timing_last reports the call in
 * ms[0] and the top-L share of it in ms[3] (for add_loo / add_kfold ms[1] and ms[2] are the prediction's stages). */
typedef struct ss_target_topl ss_target_topl; /* a per-target top-L table, device resident */
/* nt targets (1 <= nt < 2^31), lists of L (1 <= L <= 1024) */
int ss_target_topl_create_f32(int64_t nt, int L, ss_target_topl** out);
int ss_target_topl_create_f64(int64_t nt, int L, ss_target_topl** out);
int ss_target_topl_destroy(ss_target_topl* h);
/* empty the table (nt and L stay) */
int ss_target_topl_reset(ss_target_topl* h);
/* info[0] = nt, [1] = L, [2] = rows added, [3] = positives among them */
int ss_target_topl_info(const ss_target_topl* h, int64_t info[4]);
/* Add the rows of a row-major score block (nrows x ncols, ld >= ncols, ncols == nt, 0 <= nrows < 2^31): row r is row id
 * row_begin + r (row_begin >= 0); labels exactly as for ss_pool_add_rows_* (CSR positives sorted, unique, in range,
 * yptr[0] may exceed index_base); all in `mem`. */
int ss_target_topl_add_rows_f32(ss_target_topl* h, const int64_t* yptr, const int32_t* yidx, int index_base,
                                const float* yhat, int64_t nrows, int64_t ncols, int64_t ld, int64_t row_begin,
                                int mem);
int ss_target_topl_add_rows_f64(ss_target_topl* h, const int64_t* yptr, const int32_t* yidx, int index_base,
                                const double* yhat, int64_t nrows, int64_t ncols, int64_t ld, int64_t row_begin,
                                int mem);
/* Add the leave-one-out folds [i_begin, i_end) against the graph's own labels Ys[i, :], fold i as row id i: bitwise
 * ss_predict_loo_* into a device buffer followed by ss_target_topl_add_rows_*(..., row_begin = i_begin), for every
 * block_rows.  Blocks stream as in ss_pool_add_loo_* (0: about 1 GiB of scores); same graphs and preconditions; the
 * graph has the handle's nt and precision; no score leaves the device. */
int ss_target_topl_add_loo_f32(ss_target_topl* h, ss_graph* g, int64_t i_begin, int64_t i_end, int clean,
                               int64_t block_rows);
int ss_target_topl_add_loo_f64(ss_target_topl* h, ss_graph* g, int64_t i_begin, int64_t i_end, int clean,
                               int64_t block_rows);
/* The same for the k-fold rows [i_begin, i_end) of ss_predict_kfold_rows_*, source i as row id i (bitwise
 * predict_kfold_rows followed by add_rows with row_begin = i_begin); arguments, checks and blocks as for
 * ss_pool_add_kfold_* (fold_of_source in `mem`). */
int ss_target_topl_add_kfold_f32(ss_target_topl* h, ss_graph* g, const int32_t* fold_of_source, int nfolds,
                                 int64_t i_begin, int64_t i_end, int clean, int64_t block_rows, int mem);
int ss_target_topl_add_kfold_f64(ss_target_topl* h, ss_graph* g, const int32_t* fold_of_source, int nfolds,
                                 int64_t i_begin, int64_t i_end, int clean, int64_t block_rows, int mem);
/* dst gains every row of src (same precision, nt and L; src is unchanged; dst == src adds every row a second time) */
int ss_target_topl_merge(ss_target_topl* dst, const ss_target_topl* src);
/* The table: target t's fill entries in order at [t*fill, (t+1)*fill) of vals (the scores), rows (row ids) and labels
 * (0 / 1), npos[t] for every target (nt); all in `mem`, any of them may be NULL.  *rows_added (host, may be NULL) gives
 * fill = min(L, rows added). */
int ss_target_topl_export_f32(ss_target_topl* h, float* vals, int64_t* rows, uint8_t* labels, int64_t* npos,
                              int64_t* rows_added, int mem);
int ss_target_topl_export_f64(ss_target_topl* h, double* vals, int64_t* rows, uint8_t* labels, int64_t* npos,
                              int64_t* rows_added, int mem);
/* Add a table such as export writes (nt x min(L, rows_added) entries and nt npos, in `mem`), validated whole first:
 * scores not NaN, rows >= 0, labels 0 / 1, every target's entries strictly in (score desc, row asc) order, npos >= the
 * target's labelled entries; otherwise SS_EINVAL.  rows_added == 0: no-op.  Tables of several ranks meet this way. */
int ss_target_topl_import_f32(ss_target_topl* h, const float* vals, const int64_t* rows, const uint8_t* labels,
                              const int64_t* npos, int64_t rows_added, int mem);
int ss_target_topl_import_f64(ss_target_topl* h, const double* vals, const int64_t* rows, const uint8_t* labels,
                              const int64_t* npos, int64_t rows_added, int mem);
/* hits[t] = positives among target t's L entries and npos[t] (nt each, in `mem`, either may be NULL); out (host):
 * out[0] = mean recall@L over the targets in target order, exactly the reference's: a target without positives gives
 * NaN and skipmissing does not skip NaN, so the mean is NaN then; out[1] = mean precision@L (hits / L).  Beyond the
 * reference: out[2] = mean recall@L over the targets that have positives (NaN if none), out[3] = how many do.  The
 * means are sums in target order divided by the count (Julia's mean over an iterator).  Rows added <= L: SS_EINVAL
 * (the reference's `length(y) > L` assertion). */
int ss_target_topl_metrics(ss_target_topl* h, int64_t* hits, int64_t* npos, double out[4], int mem);

/* Query sets (ss_queries_*, ss_predict_queries_*) and support lists (ss_support_*) -- prospective screening on a resident
 * graph -- are declared in simspread_hip_screening.h, which this header includes at its end.  The neighbour floor of the
 * fingerprint producer (ss_similarity_tanimoto_kth_*, ss_similarity_tanimoto_floor_csr_*, ss_graph_create_fingerprint_floor_*,
 * ss_queries_create_fingerprint_floor_*: "at least the k nearest sources, whatever alpha says") is declared in
 * simspread_hip_neighbours.h, included there too. */

/* -------------------------------------------------------------- raw W*R SpMM --- */
/* The resource-spreading product F = W * R on its own (kernel unit tests and the
 * roofline benchmark; inside predict W = Ys' and R = the transfer block, src/core.jl:413).
 * W: rows x cols CSR.  R: cols x B dense, F: rows x B dense.
 *   *_layout == SS_LAYOUT_ROWMAJOR : R(k,b) at R[k*ldr + b], F(m,b) at F[m*ldf + b]
 *   *_layout == SS_LAYOUT_COLMAJOR : R(k,b) at R[k + b*ldr], F(m,b) at F[m + b*ldf]
 * B <= 64 with row-major operands takes the HBM-bound CSR kernel; wider B takes the
 * LDS-tiled kernel (natively column-major; other layouts pay one transpose). */
int ss_spmat_create_csr_f32(int64_t rows, int64_t cols, const int64_t* ptr, const int32_t* idx,
                            const float* val, int index_base, int mem, ss_spmat** out);
int ss_spmat_create_csr_f64(int64_t rows, int64_t cols, const int64_t* ptr, const int32_t* idx,
                            const double* val, int index_base, int mem, ss_spmat** out);
int ss_spmat_destroy(ss_spmat* w);
int ss_spmm_f32(ss_spmat* w, const float* R, int64_t B, int64_t ldr, int r_layout,
                float* F, int64_t ldf, int f_layout, int mem);
int ss_spmm_f64(ss_spmat* w, const double* R, int64_t B, int64_t ldr, int r_layout,
                double* F, int64_t ldf, int f_layout, int mem);
/* Algorithmic bytes of one ss_spmm call (SURVEY.md section 8d:
 * nnz*(vb+4) + (rows+1)*4 + cols*B*vb + rows*B*vb) and its flops 2*nnz*B. */
int ss_spmat_cost(const ss_spmat* w, int64_t B, double* bytes, double* flops);

#ifdef __cplusplus
}
#endif

#include "simspread_hip_screening.h"
#include "simspread_hip_neighbours.h"
#include "simspread_hip_neighbours_real.h"
#include "simspread_hip_clusters.h"
#include "simspread_hip_target_rank.h"
#include "simspread_hip_half.h"
#include "simspread_hip_int8.h"
#include "simspread_hip_profile.h"

#endif /* SIMSPREAD_HIP_H */
