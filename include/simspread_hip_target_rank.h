/* libsimspread_hip -- per-target AuROC, AuPRC, BEDROC, validity ratio, recall@L and precision@L of whole score sweeps,
 * on the device and without the score matrix.  Part of the C ABI of simspread_hip.h, which includes this file: include
 * that header.  Types, error codes and `mem` are declared there. */
#ifndef SIMSPREAD_HIP_TARGET_RANK_H
#define SIMSPREAD_HIP_TARGET_RANK_H

#include "simspread_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ------------------------------------------------------------------ the contract --- */
/* Let S be the n x nt score matrix of every row added to a handle (row ids distinct, as for ss_target_topl_*) and Y its
 * 0/1 labels.  For every target t the handle yields the six numbers ss_rank_metrics_rows_* gives for the vector
 * (Y[:, t], S[:, t]) taken in row-id order: AuROC, AuPRC, BEDROC(alpha), validity ratio, recall@L, precision@L, under
 * every convention documented there (order: score descending, ties by ascending ROW ID; a confusion matrix at every
 * distinct score; trapezoid without a (0,0) point; NaN when a class is missing and the column holds two or more distinct
 * scores; clean!'s -99 an ordinary score; recall NaN without positives).  Scores compare as ss_rank_metrics_rows_*
 * compares them inside a row: by value, so -0.0 ties with +0.0.  NaN scores are refused.
 *
 * A per-target evaluation costs TWO sweeps.  None of the six numbers needs the negatives' scores themselves, only the
 * sorted positives of a target and, for each of them, integer counts of negatives; but a positive's score is known only
 * once its row has been produced, and the matrix is not kept (40 GB at 100k x 100k), so a handle has two phases:
 *   collect  every add records (target, row id, score) of the block's positives
 *   seal     sorts them by (target, score descending, row ascending), builds per-target offsets and zeroes the counts;
 *            positives can no longer be added
 *   count    the same rows are added again; every entry whose LABEL is 0 is located among its target's sealed positives
 *            and one integer count is incremented
 * The second pass re-runs the sweep; its scores are bitwise those of the first (the sweeps are bitwise repeatable), and
 * the count pass verifies that instead of trusting it: before anything is counted every positive of the block is looked
 * up in the sealed table by (target, row id, this block's score bits); one that is missing or carries other bits fails
 * the call with SS_EINVAL and a message naming the row and the target.
 *
 * The count layout (part of the export format).  P = positives of the handle, P_t those of target t, off[t] the number
 * of positives of targets < t, positives of t numbered 0..P_t-1 in sealed order.  counts holds 3 P + 6 nt int64:
 *   hist   3 (P + nt) entries; target t owns the 3 (P_t + 1) entries from 3 (off[t] + t):
 *            gap [j], j = 0..P_t   negatives that tie with no positive and have exactly j positives scoring higher
 *                                  (strictly between two distinct positive scores; j = P_t: below every positive)
 *            tieG[j]               negatives that tie with the positives whose first (in sealed order) is j
 *            tieK[k]               tied negatives with exactly k positives before them in (score desc, row asc) order
 *          so strict `>` counts are prefix sums of gap and tieG, `==` counts are tieG, and the row-order position of a
 *          tied negative inside its tie group is tieK
 *   nz     nt entries: scores != 0 of the column (every label)
 *   kmin   nt entries: the smallest score of the column as an order-preserving unsigned 64-bit key (-0.0 as +0.0; fp32
 *          keys zero-extended), stored bit for bit in the int64; 2^64 - 1 while the column is empty
 *   kmax   nt entries: the largest, 0 while empty (kmin != kmax: two or more distinct scores)
 * Everything is integer valued: exact, independent of block order, and merged across blocks and ranks by addition
 * (kmin / kmax by min / max).
 *
 * Limits: nt < 2^31, positives per handle < 2^31, row ids < 2^31.  All-or-nothing: an add, merge or import that fails
 * (NaN score, bad labels, the other precision, ncols != nt, a wrong phase, a count-phase mismatch) leaves the handle
 * bitwise as it was.  No float atomics; every result is bitwise repeatable.  No entry point throws or aborts. */
typedef struct ss_target_rank ss_target_rank;
int ss_target_rank_create_f32(int64_t nt, ss_target_rank** out);
int ss_target_rank_create_f64(int64_t nt, ss_target_rank** out);
int ss_target_rank_destroy(ss_target_rank* h);
/* back to an empty handle in the collect phase (nt stays) */
int ss_target_rank_reset(ss_target_rank* h);
/* info[0] = nt, [1] = phase (0 collect, 1 count), [2] = rows collected, [3] = positives collected, [4] = rows counted,
 * [5] = 0 */
int ss_target_rank_info(const ss_target_rank* h, int64_t info[6]);

/* Rows of a score block, acting according to the handle's phase.  Arguments, label format and checks are those of
 * ss_target_topl_add_rows_*: row-major yhat with ld >= ncols == nt; CSR positives sorted, unique and in range
 * (yptr[0] may exceed index_base); row r gets the id row_begin + r; everything in `mem`.
 * ss_path_last: "target_rank_collect", or "target_rank_count_lds" (tiles of 64 targets whose sealed positives fit the
 * LDS budget: at most 2048 together and at most SS_TARGET_RANK_LDS each) and / or "target_rank_count_large" (searched in
 * global memory).  ss_timing_last: ms[0] the call, ms[3] the collect or count work. */
int ss_target_rank_add_rows_f32(ss_target_rank* h, const int64_t* yptr, const int32_t* yidx, int index_base,
                                const float* yhat, int64_t nrows, int64_t ncols, int64_t ld, int64_t row_begin, int mem);
int ss_target_rank_add_rows_f64(ss_target_rank* h, const int64_t* yptr, const int32_t* yidx, int index_base,
                                const double* yhat, int64_t nrows, int64_t ncols, int64_t ld, int64_t row_begin,
                                int mem);
/* Sweeps against the graph's own labels: bitwise ss_predict_loo_* / ss_predict_kfold_rows_* into a device buffer
 * followed by add_rows(row_begin = i_begin), for every block_rows (0: about 1 GiB of scores).  ms[1] and ms[2] of
 * ss_timing_last are the prediction's stages. */
int ss_target_rank_add_loo_f32(ss_target_rank* h, ss_graph* g, int64_t i_begin, int64_t i_end, int clean,
                               int64_t block_rows);
int ss_target_rank_add_loo_f64(ss_target_rank* h, ss_graph* g, int64_t i_begin, int64_t i_end, int clean,
                               int64_t block_rows);
int ss_target_rank_add_kfold_f32(ss_target_rank* h, ss_graph* g, const int32_t* fold_of_source, int nfolds,
                                 int64_t i_begin, int64_t i_end, int clean, int64_t block_rows, int mem);
int ss_target_rank_add_kfold_f64(ss_target_rank* h, ss_graph* g, const int32_t* fold_of_source, int nfolds,
                                 int64_t i_begin, int64_t i_end, int clean, int64_t block_rows, int mem);

/* collect -> count.  A handle in the count phase: SS_EINVAL. */
int ss_target_rank_seal(ss_target_rank* h);

/* Collect phase: dst gains src's positives and rows (a union; src is unchanged).  Count phase: both handles must hold
 * the same sealed table, compared bit for bit on the device; the counts add.  A phase mismatch, different nt or
 * precision, a differing table, or dst == src (its row ids would repeat): SS_EINVAL. */
int ss_target_rank_merge(ss_target_rank* dst, const ss_target_rank* src);

/* The positives as (target, row, score) triples, info[3] of each, in `mem` (any array may be NULL): in collection order
 * while collecting, in sealed order (target, score descending, row ascending) afterwards.  *rows_added (host, may be
 * NULL) = rows collected. */
int ss_target_rank_export_positives_f32(ss_target_rank* h, int32_t* targets, int64_t* rows, float* scores,
                                        int64_t* rows_added, int mem);
int ss_target_rank_export_positives_f64(ss_target_rank* h, int32_t* targets, int64_t* rows, double* scores,
                                        int64_t* rows_added, int mem);
/* Collect phase only: add npos triples and rows_added rows (another rank's export).  The whole table is validated
 * first: targets in [0, nt), 0 <= rows < 2^31, no NaN. */
int ss_target_rank_import_positives_f32(ss_target_rank* h, const int32_t* targets, const int64_t* rows,
                                        const float* scores, int64_t npos, int64_t rows_added, int mem);
int ss_target_rank_import_positives_f64(ss_target_rank* h, const int32_t* targets, const int64_t* rows,
                                        const double* scores, int64_t npos, int64_t rows_added, int mem);
/* Count phase only.  counts: 3 * info[3] + 6 * nt int64 in the layout above, in `mem`; *rows_counted is a host integer
 * (may be NULL).  import adds a table of exactly that size (ncounts) counted over rows_counted rows against the same
 * sealed positives; hist and nz entries must be non-negative. */
int ss_target_rank_export_counts(ss_target_rank* h, int64_t* counts, int64_t* rows_counted, int mem);
int ss_target_rank_import_counts(ss_target_rank* h, const int64_t* counts, int64_t ncounts, int64_t rows_counted,
                                 int mem);

/* out[t*6 + 0..5] (nt x 6 doubles in `mem`) = AuROC, AuPRC, BEDROC(alpha), validity ratio, recall@L, precision@L of
 * target t.  Requires the count phase, rows counted == rows collected and 1 <= L < rows (the reference's
 * length(y) > L), alpha > 0: otherwise SS_EINVAL.  Can be called repeatedly with other alpha and L.
 * ss_path_last: "target_rank_metrics". */
int ss_target_rank_metrics(ss_target_rank* h, double alpha, int L, double* out, int mem);

#ifdef __cplusplus
}
#endif
#endif /* SIMSPREAD_HIP_TARGET_RANK_H */
