/* libsimspread_hip -- prospective screening on a resident graph: query sets bound to a graph and support lists of
 * (row, target) hits.  Part of the C ABI of simspread_hip.h, which includes this file: include that header.  Types,
 * error codes, `mem`, layouts and SS_ROWS_* are declared there. */
#ifndef SIMSPREAD_HIP_SCREENING_H
#define SIMSPREAD_HIP_SCREENING_H

#include "simspread_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ------------------------------------------------- query sets and support lists --- */
/* Prospective screening on a resident graph.  A query set is an nq x nf block Xq of query rows on the device that
 * belongs to ONE graph g: what the graph's constructor would have stored as its query block had it been given these
 * queries, built without touching the graph -- no sort, transpose, degree pass or operand cut runs, and ss_graph_info,
 * ss_graph_degrees and every serving and evaluating call on g (leave-one-out and k-fold on a graph with nq == 0
 * included) give the same bits before, while and after query sets exist.  Any number of query sets may be bound to a
 * graph; a query set may be destroyed after its graph (it is then of no further use).  g must hold CSR blocks
 * (ss_graph_create_csr_*, _dense_*, _fingerprint_*, _features_*, _vectors_*, ss_graph_recut_*): a dense-similarity or a
 * general graph gives SS_EUNSUPPORTED.  A graph of the other precision: SS_EINVAL.  nq may be 0.  On any error *out is
 * NULL.  A query set has its own lock; a call that takes a graph and a query set holds the graph's lock, then the query
 * set's.
 *
 * ss_queries_create_csr_*: the nq x nf block as CSR, checked and stored exactly as the Xq block of
 * ss_graph_create_csr_* (nf is the graph's). */
int ss_queries_create_csr_f32(const ss_graph* g, int64_t nq, const int64_t* ptr, const int32_t* idx, const float* val,
                              int index_base, int mem, ss_queries** out);
int ss_queries_create_csr_f64(const ss_graph* g, int64_t nq, const int64_t* ptr, const int32_t* idx, const double* val,
                              int index_base, int mem, ss_queries** out);
/* From raw data: the cross block cut(S(Fq, Fs)) of the producer that built the graph -- ss_graph_create_fingerprint_*,
 * _features_*, _vectors_* -- with the same rules, layouts, NaN refusals and ss_path_last tags ("tanimoto_csr_cross",
 * "jaccard_csr_cross", "dot_csr_cross").  The graph records no origin: the caller passes the sources Fs (ns rows, in
 * `mem` like Fq), alpha, weighted and metric again, and the query set equals the constructor's block when they are the
 * constructor's.  The graph must have nf == ns and ns must be the graph's: otherwise SS_EINVAL.  Only the nq x ns cross
 * block is computed. */
int ss_queries_create_fingerprint_f32(const ss_graph* g, int64_t nq, int64_t ns, int64_t nwords, const uint64_t* Fq,
                                      const uint64_t* Fs, float alpha, int weighted, int mem, ss_queries** out);
int ss_queries_create_fingerprint_f64(const ss_graph* g, int64_t nq, int64_t ns, int64_t nwords, const uint64_t* Fq,
                                      const uint64_t* Fs, double alpha, int weighted, int mem, ss_queries** out);
int ss_queries_create_features_f32(const ss_graph* g, int64_t nq, int64_t ns, int64_t d, const float* Fq, int64_t ldq,
                                   const float* Fs, int64_t lds, float alpha, int weighted, int mem, ss_queries** out);
int ss_queries_create_features_f64(const ss_graph* g, int64_t nq, int64_t ns, int64_t d, const double* Fq, int64_t ldq,
                                   const double* Fs, int64_t lds, double alpha, int weighted, int mem,
                                   ss_queries** out);
int ss_queries_create_vectors_f32(const ss_graph* g, int64_t nq, int64_t ns, int64_t d, int metric, const float* Fq,
                                  int64_t ldq, const float* Fs, int64_t lds, float alpha, int weighted, int mem,
                                  ss_queries** out);
int ss_queries_create_vectors_f64(const ss_graph* g, int64_t nq, int64_t ns, int64_t d, int metric, const double* Fq,
                                  int64_t ldq, const double* Fs, int64_t lds, double alpha, int weighted, int mem,
                                  ss_queries** out);
int ss_queries_destroy(ss_queries* q);
/* sizes[0..2] = nq, nf, nnz(Xq) after dropping stored zeros */
int ss_queries_info(const ss_queries* q, int64_t sizes[3]);
/* kq[nq] (in `mem`): stored entries of every query row; 0 = the query has no neighbour among the sources at this
 * cutoff (outside the applicability domain: all its scores are 0). */
int ss_queries_degrees(const ss_queries* q, int64_t* kq, int mem);
/* Rows [row_begin, row_end) of the query set against all targets: bit for bit what
 * ss_predict_*(g', SS_ROWS_QUERY, row_begin, row_end, clean, ...) gives on g', the graph g's constructor builds from the
 * same sources and labels with these queries (for a recut child: at the child's cutoff) -- for every range, both layouts
 * and both `mem`.  It is the same code path with the query block exchanged; asynchrony, timings and ss_path_last as for
 * ss_predict_*.  The graph's lazily built operands and workspaces are shared with its own calls.  q must have been
 * created for g (the identity of the handle counts, not its shape): otherwise SS_EINVAL.  A bad range or a handle of the
 * other precision: SS_EINVAL; on any error nothing is written.  An empty range is a no-op after the checks. */
int ss_predict_queries_f32(ss_graph* g, const ss_queries* q, int64_t row_begin, int64_t row_end, int clean, float* out,
                           int64_t ld, int layout, int mem);
int ss_predict_queries_f64(ss_graph* g, const ss_queries* q, int64_t row_begin, int64_t row_end, int clean, double* out,
                           int64_t ld, int layout, int mem);
/* Support lists: which sources carry a score.  A score is Yhat[r,t] = sum_s T[r,s] * Ys[s,t], T[r,:] being the transfer
 * row (the stage-1 output, 1/ks included; for a leave-one-out fold the degree-corrected row) that prediction of that kind
 * hands to stage 2 -- it comes from the same stage-1 kernel, so it has the same bits.  For pair p = (rows[p],
 * targets[p]) and every stored Ys[s,t], c_s = T[r,s] * Ys[s,t] is one correctly rounded multiply in the graph's
 * precision (by 1 for pattern-only labels); the support of p is the set of s with c_s != 0, ordered by c_s descending as
 * ss_topl_f32 orders floats, ties by ascending s.  src[p*M + j] and contrib[p*M + j] hold its first M entries (unused
 * slots: src = -1, contrib = 0), nsupp[p] the size of the whole support, which may exceed M.  With M >= nsupp[p] the
 * contributions sum to the score up to the rounding of a sum of nsupp[p] terms.
 * rows_kind: SS_ROWS_QUERY -- rows of the query set q, or of the graph's own query block when q is NULL; SS_ROWS_LOO --
 * fold i of ss_predict_loo_* (q must be NULL; same graphs and preconditions as ss_predict_loo_*).  SS_ROWS_SOURCE gives
 * SS_EUNSUPPORTED (its transfer row mixes the feature and the target path), and so does a dense-similarity or a general
 * graph.  1 <= M <= 64.  Pairs may repeat rows and targets in any order; npairs == 0 is a no-op after the checks.  rows,
 * targets and the outputs are all in `mem`.  An index out of range, M outside 1..64, q bound to another graph or a
 * handle of the other precision: SS_EINVAL, and nothing is written.  The output is bitwise repeatable (no position comes
 * from an atomic).  ss_path_last: "support" next to the stage-1 tag; ss_timing_last: ms[1] stage 1, ms[3] the support
 * kernel.  Returns with the outputs complete. */
int ss_support_f32(ss_graph* g, const ss_queries* q, int rows_kind, int64_t npairs, const int64_t* rows,
                   const int32_t* targets, int M, int32_t* src, float* contrib, int32_t* nsupp, int mem);
int ss_support_f64(ss_graph* g, const ss_queries* q, int rows_kind, int64_t npairs, const int64_t* rows,
                   const int32_t* targets, int M, int32_t* src, double* contrib, int32_t* nsupp, int mem);

#ifdef __cplusplus
}
#endif
#endif /* SIMSPREAD_HIP_SCREENING_H */
