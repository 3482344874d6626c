/* libsimspread_hip -- the neighbour floor for graphs from real-valued rows: weighted Jaccard of descriptors and the
 * inner-product similarities (cosine, real-valued Tanimoto, Dice) of embeddings, with a per-row k-th-similarity cut next
 * to the cutoff alpha.  Part of the C ABI of simspread_hip.h, which includes this file: include that header.  Types,
 * error codes, `mem`, SS_SIM_* and the column-major feature layout are declared there. */
#ifndef SIMSPREAD_HIP_NEIGHBOURS_REAL_H
#define SIMSPREAD_HIP_NEIGHBOURS_REAL_H

#include "simspread_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ------------------------------------------------------------------ neighbour floor, real-valued rows --- */
/* The rule of simspread_hip_neighbours.h, word for word, with the producer's own similarity.  For rows i of Fa (na x d,
 * column-major, lda >= na) against rows j of Fb (Fb == NULL: Fb = Fa), in precision T:
 *
 *   s(i,j)  = the similarity the plain producer computes for the ordered pair (i, j):
 *             jaccard  smin / smax summed sequentially over k, as ss_similarity_jaccard_csr_*
 *             dot      g, A, B, then the formula of `metric`, as ss_similarity_dot_csr_*; Fb == NULL: s(i,i) = 1 exactly
 *                      (as the symmetric mode), and every other pair is what the cross producer computes for (i, j)
 *   P_i     = multiset { s(i,j) : 0 <= j < nb, s(i,j) > 0 }                             (a NaN s is not > 0)
 *   tau_i   = the k-th largest element of P_i (multiplicity counted) when |P_i| >= k, else +0      (k >= 1)
 *   v       = weighted ? s : 1
 *   entry (i,j) is kept iff v != 0 and ( s >= alpha  or  ( s > 0 and s >= tau_i ) )
 *
 *  - Ties at tau_i are all kept, so a row may get more than k entries; the result does not depend on column order or on
 *    any tie-break.
 *  - A row with fewer than k positive similarities keeps all of them.
 *  - Negative similarities (signed embeddings, negative features) never count among the k: they survive only through
 *    s >= alpha.
 *  - The output is in general NOT symmetric: (i,j) is decided by tau_i, (j,i) by tau_j.  The floor case therefore runs
 *    the full grid of tiles, not the triangle.  For the dot producer s(i,j) and s(j,i) are computed by different tiles
 *    there and are not promised to agree bit for bit.
 *  - alpha = +infinity gives the pure k-nearest-neighbour graph.
 *  - k == 0 is exactly the plain producer: the same kernels (triangle grid included), the same bits, the same
 *    ss_path_last tags.
 *  - 0 <= k <= 64; anything else, or a NaN alpha: SS_EINVAL, nothing is written and *out is NULL.  NaN features are
 *    refused as by the plain producers.
 *  - d == 0 gives s = 1 everywhere, so tau_i = 1 when nb >= k.
 * The selection and the emit pass run the same tile computation (for dot: the same matrix-core instructions in the same
 * k order), so they agree bit for bit on s, and tau and the CSR are bitwise repeatable (no float atomics; no position
 * comes from an atomic).  A configuration whose selection lists do not fit the workgroup's local memory is
 * SS_EUNSUPPORTED (none within 0 <= k <= 64).
 *
 * A floor graph is an ordinary CSR graph afterwards: leave-one-out, k-fold, the evaluators, pools, per-target top-L,
 * support lists, ss_graph_recut_* and query sets of either kind all apply, as said in simspread_hip_neighbours.h
 * (including: pass k + 1 for k neighbours in every leave-one-out fold).
 *
 * ss_similarity_jaccard_kth_* / ss_similarity_dot_kth_*: tau[na] (in `mem`), 1 <= k <= 64 (k == 0: SS_EINVAL).
 * na == 0: no-op; nb == 0: tau is all +0.  ss_path_last: "jaccard_kth" / "dot_kth". */
int ss_similarity_jaccard_kth_f32(const float* Fa, int64_t na, int64_t lda, const float* Fb, int64_t nb, int64_t ldb,
                                  int64_t d, int k, float* tau, int mem);
int ss_similarity_jaccard_kth_f64(const double* Fa, int64_t na, int64_t lda, const double* Fb, int64_t nb, int64_t ldb,
                                  int64_t d, int k, double* tau, int mem);
int ss_similarity_dot_kth_f32(const float* Fa, int64_t na, int64_t lda, const float* Fb, int64_t nb, int64_t ldb,
                              int64_t d, int metric, int k, float* tau, int mem);
int ss_similarity_dot_kth_f64(const double* Fa, int64_t na, int64_t lda, const double* Fb, int64_t nb, int64_t ldb,
                              int64_t d, int metric, int k, double* tau, int mem);
/* The CSR of the rule above; layouts, the size protocol (idx == NULL: *nnz and ptr only; capacity < nnz: SS_EINVAL with
 * *nnz set) and the nnz >= 2^31 refusal as for ss_similarity_jaccard_csr_* / ss_similarity_dot_csr_*.  ss_path_last:
 * "jaccard_csr_floor_sym" / "dot_csr_floor_sym" (Fb == NULL) or "jaccard_csr_floor_cross" / "dot_csr_floor_cross"; with
 * k == 0 the plain producer's tags. */
int ss_similarity_jaccard_floor_csr_f32(const float* Fa, int64_t na, int64_t lda, const float* Fb, int64_t nb,
                                        int64_t ldb, int64_t d, float alpha, int k, int weighted, int64_t* ptr,
                                        int32_t* idx, float* val, int64_t capacity, int64_t* nnz, int mem);
int ss_similarity_jaccard_floor_csr_f64(const double* Fa, int64_t na, int64_t lda, const double* Fb, int64_t nb,
                                        int64_t ldb, int64_t d, double alpha, int k, int weighted, int64_t* ptr,
                                        int32_t* idx, double* val, int64_t capacity, int64_t* nnz, int mem);
int ss_similarity_dot_floor_csr_f32(const float* Fa, int64_t na, int64_t lda, const float* Fb, int64_t nb, int64_t ldb,
                                    int64_t d, int metric, float alpha, int k, int weighted, int64_t* ptr, int32_t* idx,
                                    float* val, int64_t capacity, int64_t* nnz, int mem);
int ss_similarity_dot_floor_csr_f64(const double* Fa, int64_t na, int64_t lda, const double* Fb, int64_t nb, int64_t ldb,
                                    int64_t d, int metric, double alpha, int k, int weighted, int64_t* ptr, int32_t* idx,
                                    double* val, int64_t capacity, int64_t* nnz, int mem);
/* ss_graph_create_features_* / ss_graph_create_vectors_* with the floor (`int k` after alpha): Xs = floor(S(Fs, Fs))
 * with every source's k taken among the sources (itself included), Xq = floor(S(Fq, Fs)) with every query's k taken
 * among the sources.  Everything else as there. */
int ss_graph_create_features_floor_f32(int64_t nq, int64_t ns, int64_t nt, int64_t d, const float* Fq, int64_t ldq,
                                       const float* Fs, int64_t lds, const int64_t* y_ptr, const int32_t* y_idx,
                                       const float* y_val, int index_base, float alpha, int k, int weighted, int mem,
                                       ss_graph** out);
int ss_graph_create_features_floor_f64(int64_t nq, int64_t ns, int64_t nt, int64_t d, const double* Fq, int64_t ldq,
                                       const double* Fs, int64_t lds, const int64_t* y_ptr, const int32_t* y_idx,
                                       const double* y_val, int index_base, double alpha, int k, int weighted, int mem,
                                       ss_graph** out);
int ss_graph_create_vectors_floor_f32(int64_t nq, int64_t ns, int64_t nt, int64_t d, int metric, const float* Fq,
                                      int64_t ldq, const float* Fs, int64_t lds, const int64_t* y_ptr,
                                      const int32_t* y_idx, const float* y_val, int index_base, float alpha, int k,
                                      int weighted, int mem, ss_graph** out);
int ss_graph_create_vectors_floor_f64(int64_t nq, int64_t ns, int64_t nt, int64_t d, int metric, const double* Fq,
                                      int64_t ldq, const double* Fs, int64_t lds, const int64_t* y_ptr,
                                      const int32_t* y_idx, const double* y_val, int index_base, double alpha, int k,
                                      int weighted, int mem, ss_graph** out);
/* ss_queries_create_features_* / ss_queries_create_vectors_* with the floor (`int k` after alpha): the cross block
 * floor(S(Fq, Fs)), on any CSR graph with nf == ns (a plain or a floor graph).  ss_queries_degrees is then
 * >= min(k, |P_i|) for every query: no query with a positive similarity is left outside the applicability domain. */
int ss_queries_create_features_floor_f32(const ss_graph* g, int64_t nq, int64_t ns, int64_t d, const float* Fq,
                                         int64_t ldq, const float* Fs, int64_t lds, float alpha, int k, int weighted,
                                         int mem, ss_queries** out);
int ss_queries_create_features_floor_f64(const ss_graph* g, int64_t nq, int64_t ns, int64_t d, const double* Fq,
                                         int64_t ldq, const double* Fs, int64_t lds, double alpha, int k, int weighted,
                                         int mem, ss_queries** out);
int ss_queries_create_vectors_floor_f32(const ss_graph* g, int64_t nq, int64_t ns, int64_t d, int metric,
                                        const float* Fq, int64_t ldq, const float* Fs, int64_t lds, float alpha, int k,
                                        int weighted, int mem, ss_queries** out);
int ss_queries_create_vectors_floor_f64(const ss_graph* g, int64_t nq, int64_t ns, int64_t d, int metric,
                                        const double* Fq, int64_t ldq, const double* Fs, int64_t lds, double alpha, int k,
                                        int weighted, int mem, ss_queries** out);

#ifdef __cplusplus
}
#endif
#endif /* SIMSPREAD_HIP_NEIGHBOURS_REAL_H */
