/* libsimspread_hip -- cutoff profiles: the size and the row degrees of the graph a fused producer would build, at up to
 * 32 cutoffs, from ONE pass over the pairs and without building a graph.  Part of the C ABI of simspread_hip.h, which
 * includes this file: include that header.  Types, error codes, `mem`, SS_SIM_* and SS_H16_* are declared there and in
 * simspread_hip_half.h.
 *
 * `alpha` is the one hyperparameter, and s(i, j) does not depend on it.  A profile answers, before any graph exists,
 * what the idx == NULL size query of a producer answers for one alpha per all-pairs pass: which is the lowest alpha
 * whose graph fits a budget (also below the alpha at which the producers refuse, nnz >= 2^31), and how many rows still
 * have a neighbour at each alpha (coverage).
 *
 * THE RULE.  Inputs are the same operands as the matching plain producer (`Fa`, `Fb` or `NULL`, layouts, `metric`,
 * `storage`), plus:
 *
 *   - `weighted`
 *   - `cuts[ncuts]` of type T, nondecreasing, `1 <= ncuts <= 32`
 *
 * `s(i, j)` is the similarity the plain producer computes for the entry (i, j) of its CSR, same bits.  In symmetric mode
 * (`Fb == NULL`) that means:
 *
 *   - the value of the tile on or above the diagonal, mirrored, as the producers emit it;
 *   - for the inner-product similarities, `s(i, i) = 1` exactly.
 *
 * `v = weighted ? s : 1`.  Pair (i, j) counts for cut b iff `s >= cuts[b] and v != 0`.  A NaN `s` counts for none.
 *
 * Outputs:
 *
 *   - `rows[i * ncuts + b]` (int32, `na x ncuts` row-major, may be `NULL`): the number of j that count for cut b.
 *   - `total[b]` (int64): the sum of `rows[., b]`.
 *   - `total` is int64 so that a profile answers exactly where a producer refuses.  There is no 2^31 refusal here.  Only
 *     `nb < 2^31`, as everywhere.
 *
 * The contract, for every b, both modes, every producer:
 *
 *   - `total[b]` is bitwise the `*nnz`, and `rows[i, b]` is bitwise `ptr[i + 1] - ptr[i]`, of the matching
 *     `ss_similarity_*_csr_*` call.
 *   - That call uses `alpha = cuts[b]`, the same `weighted` and `idx == NULL`.
 *   - Only the plain producer is covered (`k == 0`, no neighbour floor).
 *
 * Refusals, all before anything is written:
 *
 *   - `SS_EINVAL`: `ncuts` outside 1..32; a NaN cut; decreasing cuts; a NaN feature where the producer refuses one; a
 *     metric outside 0..2; a storage outside 0..1.
 *   - Equal cuts and +-inf are legal.
 *
 * Empty cases:
 *
 *   - `na == 0`: `total` is all zero.
 *   - `nb == 0`: everything is zero.
 *   - `d == 0`: falls out of the producers' own rule (`s = 1`).
 *
 * Memory and repeatability:
 *
 *   - `cuts` is always host memory.  `rows` and `total` live in `mem` like the operands and are complete on return.
 *   - The result is bitwise repeatable.
 *   - `ss_path_last`: `"tanimoto_profile"`, `"jaccard_profile"`, `"dot_profile"`, `"dot_h16_profile"`.
 *
 * Layouts are exactly those of the matching producer: packed uint64 words, row-major (fingerprints); column-major
 * ld >= n (_f32 / _f64 rows); row-major ld >= d, any 2-byte-aligned base, padding never interpreted (_h16; the result is
 * independent of ld and alignment). */
#ifndef SIMSPREAD_HIP_PROFILE_H
#define SIMSPREAD_HIP_PROFILE_H

#include "simspread_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* the profile of ss_similarity_tanimoto_csr_*: packed binary fingerprints */
int ss_similarity_tanimoto_profile_f32(const uint64_t* Fa, int64_t na, const uint64_t* Fb, int64_t nb, int64_t nwords,
                                       const float* cuts, int ncuts, int weighted, int64_t* total, int32_t* rows,
                                       int mem);
int ss_similarity_tanimoto_profile_f64(const uint64_t* Fa, int64_t na, const uint64_t* Fb, int64_t nb, int64_t nwords,
                                       const double* cuts, int ncuts, int weighted, int64_t* total, int32_t* rows,
                                       int mem);
/* the profile of ss_similarity_jaccard_csr_*: weighted Jaccard of real-valued rows */
int ss_similarity_jaccard_profile_f32(const float* Fa, int64_t na, int64_t lda, const float* Fb, int64_t nb, int64_t ldb,
                                      int64_t d, const float* cuts, int ncuts, int weighted, int64_t* total,
                                      int32_t* rows, int mem);
int ss_similarity_jaccard_profile_f64(const double* Fa, int64_t na, int64_t lda, const double* Fb, int64_t nb,
                                      int64_t ldb, int64_t d, const double* cuts, int ncuts, int weighted,
                                      int64_t* total, int32_t* rows, int mem);
/* the profile of ss_similarity_dot_csr_*: cosine, real-valued Tanimoto, Dice (metric: SS_SIM_*) */
int ss_similarity_dot_profile_f32(const float* Fa, int64_t na, int64_t lda, const float* Fb, int64_t nb, int64_t ldb,
                                  int64_t d, int metric, const float* cuts, int ncuts, int weighted, int64_t* total,
                                  int32_t* rows, int mem);
int ss_similarity_dot_profile_f64(const double* Fa, int64_t na, int64_t lda, const double* Fb, int64_t nb, int64_t ldb,
                                  int64_t d, int metric, const double* cuts, int ncuts, int weighted, int64_t* total,
                                  int32_t* rows, int mem);
/* the profile of ss_similarity_dot_csr_h16: 16-bit rows (storage: SS_H16_*), ROW-MAJOR as there; float cuts */
int ss_similarity_dot_profile_h16(const uint16_t* Fa, int64_t na, int64_t lda, const uint16_t* Fb, int64_t nb,
                                  int64_t ldb, int64_t d, int storage, int metric, const float* cuts, int ncuts,
                                  int weighted, int64_t* total, int32_t* rows, int mem);

#ifdef __cplusplus
}
#endif
#endif /* SIMSPREAD_HIP_PROFILE_H */
