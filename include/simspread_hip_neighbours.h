/* libsimspread_hip -- fingerprint graphs with a neighbour floor: a per-row k-th-similarity cut next to the cutoff alpha.
 * Part of the C ABI of simspread_hip.h, which includes this file: include that header.  Types, error codes, `mem` and
 * the fingerprint layout are declared there. */
#ifndef SIMSPREAD_HIP_NEIGHBOURS_H
#define SIMSPREAD_HIP_NEIGHBOURS_H

#include "simspread_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ------------------------------------------------------------------ neighbour floor --- */
/* One cutoff alpha for a whole fingerprint library is wrong in both directions: compounds in dense series get thousands
 * of neighbours, singletons and new chemotypes get none (ss_queries_degrees reports kq == 0: outside the applicability
 * domain).  The neighbour floor says "at least the k nearest sources, whatever alpha says".  For rows i of Fa against
 * rows j of Fb (Fb == NULL: Fb = Fa), packed as for ss_similarity_tanimoto_csr_*, in precision T:
 *
 *   c = popcount(a & b), u = popcount(a) + popcount(b) - c, s(i,j) = u == 0 ? 1 : T(c) / T(u)   (as the plain producer)
 *   P_i   = multiset { s(i,j) : 0 <= j < nb, s(i,j) > 0 }
 *   tau_i = the k-th largest element of P_i (multiplicity counted) when |P_i| >= k, else +0      (k >= 1)
 *   v     = weighted ? s : 1
 *   entry (i,j) is kept iff v != 0 and ( s >= alpha  or  ( s > 0 and s >= tau_i ) )
 *
 * i.e. a per-row cutoff min(alpha, tau_i) restricted to positive similarities.
 *  - Ties at tau_i are all kept, so a row may get more than k entries; the result does not depend on column order or on
 *    any tie-break.
 *  - A row with fewer than k positive similarities keeps all of them.  Two all-zero fingerprints have s = 1 and count.
 *  - Fb == NULL: the diagonal (s = 1) counts among the k.  The output is in general NOT symmetric: (i,j) is decided by
 *    tau_i, (j,i) by tau_j.  (The pass therefore runs the full grid of tiles, twice the pair work of the plain
 *    producer's triangle.)
 *  - alpha = +infinity (or any alpha above 1) gives the pure k-nearest-neighbour graph.
 *  - k == 0 is exactly the plain producer: the same kernels, the same bits, the same ss_path_last tags.
 *  - 0 <= k <= 64 (the bound of M in ss_support_*); anything else, or a NaN alpha: SS_EINVAL, nothing is written and
 *    *out is NULL.
 * The selection and the emit pass compute s by the same expression, so they agree bit for bit, and tau and the CSR are
 * bitwise repeatable (no float atomics; no position comes from an atomic).
 *
 * A floor graph is an ordinary CSR graph afterwards: leave-one-out, k-fold, the evaluators, pools, per-target top-L,
 * support lists and query sets of either kind all apply.  ss_graph_recut_* treats it as any other parent: featurize on
 * the stored X, so floor-only entries below the new alpha go.  In a leave-one-out fold the held-out source's own column
 * is dropped as always, so its row keeps at least min(k, |P_i|) - 1 entries: a caller who wants k neighbours in every
 * fold passes k + 1.
 *
 * ss_similarity_tanimoto_kth_*: tau[na] (in `mem`), 1 <= k <= 64 (k == 0: SS_EINVAL).  na == 0: no-op; nb == 0: tau is
 * all +0.  ss_path_last: "tanimoto_kth". */
int ss_similarity_tanimoto_kth_f32(const uint64_t* Fa, int64_t na, const uint64_t* Fb, int64_t nb, int64_t nwords, int k,
                                   float* tau, int mem);
int ss_similarity_tanimoto_kth_f64(const uint64_t* Fa, int64_t na, const uint64_t* Fb, int64_t nb, int64_t nwords, int k,
                                   double* tau, int mem);
/* The CSR of the rule above; the size protocol (idx == NULL: *nnz and ptr only; capacity < nnz: SS_EINVAL with *nnz set)
 * and the nnz >= 2^31 refusal as for ss_similarity_tanimoto_csr_*.  ss_path_last: "tanimoto_csr_floor_sym" (Fb == NULL)
 * or "tanimoto_csr_floor_cross"; with k == 0 the plain producer's tags. */
int ss_similarity_tanimoto_floor_csr_f32(const uint64_t* Fa, int64_t na, const uint64_t* Fb, int64_t nb, int64_t nwords,
                                         float alpha, int k, int weighted, int64_t* ptr, int32_t* idx, float* val,
                                         int64_t capacity, int64_t* nnz, int mem);
int ss_similarity_tanimoto_floor_csr_f64(const uint64_t* Fa, int64_t na, const uint64_t* Fb, int64_t nb, int64_t nwords,
                                         double alpha, int k, int weighted, int64_t* ptr, int32_t* idx, double* val,
                                         int64_t capacity, int64_t* nnz, int mem);
/* ss_graph_create_fingerprint_* with the floor: Xs = floor(T(Fs, Fs)) with every source's k taken among the sources
 * (itself included), Xq = floor(T(Fq, Fs)) with every query's k taken among the sources.  Everything else as there. */
int ss_graph_create_fingerprint_floor_f32(int64_t nq, int64_t ns, int64_t nt, int64_t nwords, const uint64_t* Fq,
                                          const uint64_t* Fs, const int64_t* y_ptr, const int32_t* y_idx,
                                          const float* y_val, int index_base, float alpha, int k, int weighted, int mem,
                                          ss_graph** out);
int ss_graph_create_fingerprint_floor_f64(int64_t nq, int64_t ns, int64_t nt, int64_t nwords, const uint64_t* Fq,
                                          const uint64_t* Fs, const int64_t* y_ptr, const int32_t* y_idx,
                                          const double* y_val, int index_base, double alpha, int k, int weighted,
                                          int mem, ss_graph** out);
/* ss_queries_create_fingerprint_* with the floor: the cross block floor(T(Fq, Fs)), on any CSR graph with nf == ns (a
 * plain or a floor graph).  ss_queries_degrees is then >= min(k, |P_i|) for every query: no query with a positive
 * similarity is left outside the applicability domain. */
int ss_queries_create_fingerprint_floor_f32(const ss_graph* g, int64_t nq, int64_t ns, int64_t nwords,
                                            const uint64_t* Fq, const uint64_t* Fs, float alpha, int k, int weighted,
                                            int mem, ss_queries** out);
int ss_queries_create_fingerprint_floor_f64(const ss_graph* g, int64_t nq, int64_t ns, int64_t nwords,
                                            const uint64_t* Fq, const uint64_t* Fs, double alpha, int k, int weighted,
                                            int mem, ss_queries** out);

#ifdef __cplusplus
}
#endif
#endif /* SIMSPREAD_HIP_NEIGHBOURS_H */
