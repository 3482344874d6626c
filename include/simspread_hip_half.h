/* libsimspread_hip -- graphs from embeddings stored in 16 bits: the inner-product producer (cosine, real-valued
 * Tanimoto, Dice) on rows of bfloat16 or IEEE half values, computed on the 16-bit matrix instructions with fp32
 * accumulation.  Part of the C ABI of simspread_hip.h, which includes this file: include that header.  Types, error
 * codes, `mem` and SS_SIM_* are declared there.
 *
 * LAYOUT -- READ THIS: the 16-bit feature blocks are ROW-MAJOR.  Element (i, k) is at F[i * ld + k], ld >= d.  That is a
 * contiguous or row-strided torch (n, d) tensor (ld = stride(0)) and a Julia d x n matrix.  Every other feature entry
 * point of the library (ss_similarity_dot_csr_f32, ...) takes column-major blocks with ld >= n; these do not.
 *
 *   - Any 2-byte-aligned base and any ld >= d is accepted.
 *   - Elements k >= d of a row (padding) are never interpreted; they may hold NaN patterns.
 *   - No byte past element (n - 1) * ld + d - 1 is read: the last row of a strided view may end its allocation.
 *   - The result does not depend on the base alignment or on ld: a block that allows 16-byte loads (16-byte-aligned base,
 *     ld % 8 == 0) and one that does not give bitwise the same CSR.
 *
 * THE RULE.  Inputs are raw 16-bit patterns; `storage` says what they are.  The graph precision is float only.  With
 * w(x) the exact widening of a pattern to fp32, for row a of Fa and row b of Fb:
 *
 *   g = sum_k w(a_k) w(b_k),   A = sum_k w(a_k)^2,   B = sum_k w(b_k)^2
 *
 * Every product is exact in fp32 (16 significant bits for bf16, 22 for half); the three sums are accumulated in fp32 in
 * an order the implementation chooses.  Everything after the three sums is the rule of ss_similarity_dot_csr_f32, word for
 * word: the expression of `metric`, the zero-denominator rule (two all-zero rows: s = 1; d == 0: s = 1 everywhere), the
 * cosine clamp, s(i, i) = 1 exactly and mirrored bits in symmetric mode, keep (i, j) iff s >= alpha and v != 0 with
 * v = weighted ? s : 1.  The operands are not reduced in precision -- they are 16-bit to begin with -- so:
 *
 *   - when all partial sums are exactly representable in fp32 (small-integer features, say), the CSR is bitwise the one
 *     ss_similarity_dot_csr_f32 gives on the widened inputs;
 *   - in general it is a valid output of the fp32 rule on the widened inputs, up to the order of the sums.
 *
 *   - A NaN pattern among the elements k < d of either block, or a NaN alpha: SS_EINVAL before anything is written.
 *   - A metric outside 0..2 or a storage outside 0..1: SS_EINVAL likewise.
 *   - +-inf features behave as in the fp32 route: a NaN s is dropped.
 *   - How the matrix instructions treat subnormal 16-bit operands is NOT specified here (a subnormal may count as zero in
 *     g while the row norms widen it exactly).
 *   - The neighbour floor (simspread_hip_neighbours_real.h) and the Butina entry points have no 16-bit form. */
#ifndef SIMSPREAD_HIP_HALF_H
#define SIMSPREAD_HIP_HALF_H

#include "simspread_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

enum { SS_H16_BF16 = 0, SS_H16_F16 = 1 }; /* `storage`: bfloat16 (1-8-7) or IEEE binary16 (1-5-10) bit patterns */

/* ss_similarity_dot_csr_f32 on 16-bit rows: Fa (na x d, row-major, lda >= d) against Fb (nb x d, ldb >= d; NULL: Fa
 * against itself, symmetric mode).  Output, the size protocol (idx == NULL: *nnz and ptr only; capacity < nnz: SS_EINVAL
 * with *nnz set), the memory kinds and the 2^31 refusals are exactly those of ss_similarity_dot_csr_f32.  ss_path_last:
 * "dot_h16_sym" (Fb == NULL) or "dot_h16_cross". */
int ss_similarity_dot_csr_h16(const uint16_t* Fa, int64_t na, int64_t lda, const uint16_t* Fb, int64_t nb, int64_t ldb,
                              int64_t d, int storage, int metric, float alpha, int weighted, int64_t* ptr, int32_t* idx,
                              float* val, int64_t capacity, int64_t* nnz, int mem);
/* ss_graph_create_vectors_f32 with the two feature blocks 16-bit row-major (Fq: nq x d, ldq >= d; Fs: ns x d, lds >= d):
 * Xs = cut(S(Fs, Fs)), Xq = cut(S(Fq, Fs)).  Y and the handle are fp32; the graph is an ordinary fp32 CSR graph
 * afterwards.  ss_path_last: "dot_h16_sym", then (nq > 0) "dot_h16_cross". */
int ss_graph_create_vectors_h16(int64_t nq, int64_t ns, int64_t nt, int64_t d, int storage, int metric,
                                const uint16_t* Fq, int64_t ldq, const uint16_t* Fs, int64_t lds, const int64_t* y_ptr,
                                const int32_t* y_idx, const float* y_val, int index_base, float alpha, int weighted,
                                int mem, ss_graph** out);
/* ss_queries_create_vectors_f32 likewise: the cross block cut(S(Fq, Fs)) as a query set of the fp32 graph g, which may
 * have been built by any constructor (nf == ns). */
int ss_queries_create_vectors_h16(const ss_graph* g, int64_t nq, int64_t ns, int64_t d, int storage, int metric,
                                  const uint16_t* Fq, int64_t ldq, const uint16_t* Fs, int64_t lds, float alpha,
                                  int weighted, int mem, ss_queries** out);

#ifdef __cplusplus
}
#endif
#endif /* SIMSPREAD_HIP_HALF_H */
