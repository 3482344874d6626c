/* libsimspread_hip -- exact graphs from rows stored as signed 8-bit integers (quantised embeddings, small-count or
 * signed-hash fingerprints): the inner-product producer (cosine, real-valued Tanimoto, Dice) on the integer matrix
 * instruction v_mfma_i32_32x32x32_i8, with the neighbour floor.  Part of the C ABI of simspread_hip.h, which includes
 * this file: include that header.  Types, error codes, `mem` and SS_SIM_* are declared there.
 *
 * LAYOUT -- READ THIS: the int8 feature blocks are ROW-MAJOR, as those of simspread_hip_half.h.  Element (i, k) is at
 * F[i * ld + k], ld >= d.  That is a contiguous or row-strided torch (n, d) int8 tensor (ld = stride(0)) and a Julia
 * d x n Matrix{Int8}.
 *
 *   - Any base and any ld >= d are accepted.
 *   - Bytes k >= d of a row (padding) are never interpreted.
 *   - No byte past (n - 1) * ld + d - 1 is read: the last row of a strided view may end its allocation.
 *   - The result does not depend on the base alignment or on ld: a block that allows 16-byte loads (16-byte-aligned
 *     base, ld % 16 == 0) and one that does not give bitwise the same CSR.
 *   - Every value -128 .. 127 is a valid element.  There is no NaN and no NaN scan.
 *
 * THE RULE.  For row a of Fa and row b of Fb:
 *
 *   g = sum_k a_k b_k,   A = sum_k a_k^2,   B = sum_k b_k^2
 *
 * are EXACT 32-bit integers, whatever the order of the sums.  That needs d <= 131071 (d * 2^14 <= 2^31 - 1); a larger d
 * is SS_EINVAL before anything is read or written.  Each of the three integers is converted to fp32 by one
 * round-to-nearest-even conversion.  From there on the rule is that of ss_similarity_dot_csr_f32, word for word, in fp32:
 * ra = sqrt((float)A) for the cosine and (float)A otherwise; the expression of `metric`; the zero-denominator rule (two
 * all-zero rows: s = 1; d == 0: s = 1 everywhere); the cosine clamp; s(i, i) = 1 exactly when a block runs against
 * itself.  The graph precision is float only.
 *
 * The similarity of a pair is therefore a pure function of the two rows, and the CSR is defined bit for bit for EVERY
 * input -- not only for inputs whose partial sums happen to be exact, as on the floating-point routes.  s(i, j) and
 * s(j, i) agree bit for bit: g(a, b) = g(b, a) exactly, and float addition and multiplication are commutative.
 *
 * KEEP RULE AND NEIGHBOUR FLOOR: exactly those of simspread_hip_neighbours_real.h, 0 <= k <= 64.
 *   k == 0   keep (i, j) iff s >= alpha and v != 0, v = weighted ? s : 1; Fb == NULL runs the triangle of tiles and
 *            entry (j, i) carries the bits of (i, j).
 *   k >  0   keep (i, j) iff v != 0 and (s >= alpha or (s > 0 and s >= tau_i)); tau_i is the k-th largest positive s
 *            of row i, multiplicity counted, +0 when the row has fewer than k; ties at tau_i are all kept.  The full
 *            grid runs.  Selection and emit run the same integer Gram tile, so they agree on s by construction.
 *
 *   - A NaN alpha, a metric outside 0..2, a k outside 0..64 (1..64 for ss_similarity_dot_kth_i8) or d > 131071:
 *     SS_EINVAL with nothing written.
 *   - Output, the size protocol (idx == NULL: *nnz and ptr only; capacity < nnz: SS_EINVAL with *nnz set), the memory
 *     kinds, the 2^31 refusals and index_base are those of the _h16 entry points.
 *   - Cutoff profiles and the Butina entry points have no int8 form. */
#ifndef SIMSPREAD_HIP_INT8_H
#define SIMSPREAD_HIP_INT8_H

#include "simspread_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ss_similarity_dot_floor_csr_f32 on int8 rows: Fa (na x d, row-major, lda >= d) against Fb (nb x d, ldb >= d; NULL: Fa
 * against itself).  ss_path_last: k == 0 "dot_i8_sym" (Fb == NULL) or "dot_i8_cross"; k > 0 "dot_i8_floor_sym" or
 * "dot_i8_floor_cross". */
int ss_similarity_dot_csr_i8(const int8_t* Fa, int64_t na, int64_t lda, const int8_t* Fb, int64_t nb, int64_t ldb,
                             int64_t d, int metric, float alpha, int k, int weighted, int64_t* ptr, int32_t* idx,
                             float* val, int64_t capacity, int64_t* nnz, int mem);
/* tau[na] (in `mem`): the k-th largest positive s of every row of Fa against Fb, 1 <= k <= 64, +0 where a row has fewer
 * than k.  Empty inputs as ss_similarity_dot_kth_f32: na == 0 writes nothing, nb == 0 gives tau = 0.  ss_path_last:
 * "dot_i8_kth". */
int ss_similarity_dot_kth_i8(const int8_t* Fa, int64_t na, int64_t lda, const int8_t* Fb, int64_t nb, int64_t ldb,
                             int64_t d, int metric, int k, float* tau, int mem);
/* ss_graph_create_vectors_floor_f32 with the two feature blocks int8 row-major (Fq: nq x d, ldq >= d; Fs: ns x d,
 * lds >= d): Xs = cut(S(Fs, Fs)), Xq = cut(S(Fq, Fs)).  Y and the handle are fp32; the graph is an ordinary fp32 CSR
 * graph afterwards.  ss_path_last: the symmetric tag, then (nq > 0) the cross tag. */
int ss_graph_create_vectors_i8(int64_t nq, int64_t ns, int64_t nt, int64_t d, int metric, const int8_t* Fq, int64_t ldq,
                               const int8_t* Fs, int64_t lds, const int64_t* y_ptr, const int32_t* y_idx,
                               const float* y_val, int index_base, float alpha, int k, int weighted, int mem,
                               ss_graph** out);
/* ss_queries_create_vectors_floor_f32 likewise: the cross block cut(S(Fq, Fs)) as a query set of the fp32 graph g, which
 * may have been built by any constructor (nf == ns). */
int ss_queries_create_vectors_i8(const ss_graph* g, int64_t nq, int64_t ns, int64_t d, int metric, const int8_t* Fq,
                                 int64_t ldq, const int8_t* Fs, int64_t lds, float alpha, int k, int weighted, int mem,
                                 ss_queries** out);

#ifdef __cplusplus
}
#endif
#endif /* SIMSPREAD_HIP_INT8_H */
