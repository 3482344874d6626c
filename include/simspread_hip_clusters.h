/* libsimspread_hip -- Taylor-Butina clustering of a neighbour pattern on the device, folds that keep clusters whole, and
 * the count of what a split still leaks.  Part of the C ABI of simspread_hip.h, which includes this file: include that
 * header.  Types, error codes, `mem`, SS_SIM_* and the column-major feature layout are declared there. */
#ifndef SIMSPREAD_HIP_CLUSTERS_H
#define SIMSPREAD_HIP_CLUSTERS_H

#include "simspread_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ------------------------------------------------------------------ the rule --- */
/* The input is the pattern P of an n x n CSR matrix; values are never read.
 *
 *   N(i)      = { j != i : (i,j) in P or (j,i) in P }        diagonal and duplicate entries are ignored; a pattern
 *                                                            that is not symmetric (a neighbour-floor graph) is
 *                                                            symmetrised by union
 *   d_i       = |N(i)|                                       distinct neighbours
 *   priority  i precedes j  iff  d_i > d_j, or d_i == d_j and i < j
 *             a total order; as a 64-bit key (d_i << 32) | (0xFFFFFFFF - i), larger is earlier
 *
 * Taylor-Butina without re-counting: visit the sources in priority order; an unassigned source becomes a centre and all
 * its still-unassigned neighbours join its cluster.  Equivalently: the centres are the lexicographically-first maximal
 * independent set under the priority, every other source belongs to its earliest-priority centre neighbour, and an
 * isolated source is the centre of a cluster of one.  The result is unique, so it does not depend on scheduling, and it
 * is bitwise repeatable (no float atomics; no position comes from an atomic).  Ties between equal degrees go to the
 * LOWER index: this is not RDKit's Butina.ClusterData, which breaks them the other way round, so the clusters of
 * the two can differ wherever degrees tie.
 *
 * Outputs, always 0-based.  The arrays are in `mem`; *nclusters and *rounds are host integers, like *nnz of the
 * producers.
 *   centre[n]   the index of the source's centre; centre[c] == c for a centre
 *   label[n]    clusters numbered 0..nc-1 in priority order of their centres (cluster 0 has the earliest centre)
 *   size        NULL, or capacity n: size[l] = sources with label l for l < nc; entries from nc on are not written
 *   *nclusters  nc
 *   *rounds     NULL, or the number of rounds the device loop took (1 <= rounds <= n for n > 0)
 *
 * The device path: the off-diagonal entries and their transposes are sorted as 64-bit keys and the distinct ones kept,
 * which gives a symmetric CSR and the degrees; then rounds over one byte of state per source, in which an undecided row
 * that sees a centre neighbour becomes a member and one that sees no undecided neighbour of earlier priority becomes a
 * centre; the earliest undecided row decides in every round, so the loop ends within n rounds, and it is cut off there:
 * more would be a defect and returns SS_EINTERNAL.  ptr and idx are validated on the device before anything else reads
 * them: ptr[0] != index_base, pointers that decrease or an index outside the n columns give SS_EINVAL and no output is
 * written.  2^30 or more stored entries: SS_EUNSUPPORTED.  n >= 2^31: SS_EUNSUPPORTED.  index_base is 0 or 1 and
 * applies to ptr and idx.  n == 0: a no-op with *nclusters = 0.  ss_path_last: "butina_csr".
 * ss_timing_last after any of the clustering calls: transfer_ms = symmetrise, spmm_ms = rounds, epilogue_ms = assign
 * and label. */
int ss_cluster_butina_csr(int64_t n, const int64_t* ptr, const int32_t* idx, int index_base, int32_t* centre,
                          int32_t* label, int32_t* size, int64_t* nclusters, int64_t* rounds, int mem);

/* The fused forms: the pattern is the plain self-similarity producer's -- unweighted, s >= cutoff, Fb == NULL,
 * val == NULL -- made and consumed on the device.  The similarity bits are the producer's, so `cutoff` sits on exactly
 * the boundary ss_similarity_tanimoto_csr_* / ss_similarity_jaccard_csr_* / ss_similarity_dot_csr_* draw, and the
 * argument checks are theirs (a NaN cutoff or NaN features: SS_EINVAL, nothing written).  A pattern of 2^30 or more
 * entries: SS_EUNSUPPORTED.  Layouts as for the producers: F is n x nwords packed uint64 rows, or n x d column-major
 * with ld >= n.  ss_path_last: "butina_csr" and the producer's tag ("tanimoto_csr_sym", "jaccard_csr_sym",
 * "dot_csr_sym"). */
int ss_cluster_butina_fingerprint_f32(const uint64_t* F, int64_t n, int64_t nwords, float cutoff, int32_t* centre,
                                      int32_t* label, int32_t* size, int64_t* nclusters, int64_t* rounds, int mem);
int ss_cluster_butina_fingerprint_f64(const uint64_t* F, int64_t n, int64_t nwords, double cutoff, int32_t* centre,
                                      int32_t* label, int32_t* size, int64_t* nclusters, int64_t* rounds, int mem);
int ss_cluster_butina_features_f32(const float* F, int64_t n, int64_t d, int64_t ld, float cutoff, int32_t* centre,
                                   int32_t* label, int32_t* size, int64_t* nclusters, int64_t* rounds, int mem);
int ss_cluster_butina_features_f64(const double* F, int64_t n, int64_t d, int64_t ld, double cutoff, int32_t* centre,
                                   int32_t* label, int32_t* size, int64_t* nclusters, int64_t* rounds, int mem);
int ss_cluster_butina_vectors_f32(int metric, const float* F, int64_t n, int64_t d, int64_t ld, float cutoff,
                                  int32_t* centre, int32_t* label, int32_t* size, int64_t* nclusters, int64_t* rounds,
                                  int mem);
int ss_cluster_butina_vectors_f64(int metric, const double* F, int64_t n, int64_t d, int64_t ld, double cutoff,
                                  int32_t* centre, int32_t* label, int32_t* size, int64_t* nclusters, int64_t* rounds,
                                  int mem);

/* Folds that keep clusters whole.  This one is host code (label and fold_of_source in device memory are copied over and
 * back): deterministic, largest first.  Clusters are taken by size descending, ties by label ascending; each goes to
 * the fold with the fewest sources so far, ties to the lowest fold id.  fold_of_source[n] (int32, ids in [0, nfolds))
 * goes straight into ss_predict_kfold_* / ss_evaluate_kfold_* / ss_pool_add_kfold_*.  The folds differ in size by at
 * most the largest cluster.  nfolds < 1, nclusters < 0 or a label outside 0..nclusters-1: SS_EINVAL, nothing written.
 * n == 0: a no-op. */
int ss_cluster_folds(const int32_t* label, int64_t n, int64_t nclusters, int nfolds, int32_t* fold_of_source, int mem);

/* How much a split leaks: count[f] (int64, nfolds entries, in `mem`) = the number of stored off-diagonal entries (i,j)
 * of the pattern with fold[i] == f != fold[j].  One pass over the pattern as given: not symmetrised, duplicates counted
 * as often as they are stored.  The pattern is validated as above and the fold ids must lie in [0, nfolds): otherwise
 * SS_EINVAL.  nfolds < 1: SS_EINVAL.  n == 0: count is all zero.  ss_path_last: "cross_edges". */
int ss_cluster_cross_edges(int64_t n, const int64_t* ptr, const int32_t* idx, int index_base,
                           const int32_t* fold_of_source, int nfolds, int64_t* count, int mem);

#ifdef __cplusplus
}
#endif
#endif /* SIMSPREAD_HIP_CLUSTERS_H */
