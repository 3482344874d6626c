"""Host reference of the cutoff profiles (include/simspread_hip_profile.h), no GPU: the rule restated in numpy on a
dense similarity matrix S.  This is the definition the device tests compare against.

    v = weighted ? s : 1;  pair (i, j) counts for cut b iff s >= cuts[b] and v != 0;  a NaN s counts for none
    rows[i, b] = #{j : (i, j) counts for b};  total[b] = sum_i rows[i, b]
"""
import numpy as np


def profile_ref(S, cuts, weighted):
    """(total int64 (ncuts,), rows int32 (na, ncuts)) of the rule on S; S and cuts are compared as they are (give them
    in the graph's dtype)."""
    S = np.asarray(S)
    cuts = np.asarray(cuts)
    assert S.ndim == 2 and cuts.ndim == 1 and S.dtype == cuts.dtype
    rows = np.zeros((S.shape[0], cuts.size), np.int32)
    with np.errstate(invalid="ignore"):
        alive = (S != 0) if weighted else np.ones(S.shape, bool)
        for b, c in enumerate(cuts):
            rows[:, b] = ((S >= c) & alive).sum(axis=1)
    return rows.astype(np.int64).sum(axis=0), rows


def unpack_bits(F):
    """(n, 64 * nwords) 0/1 of packed fingerprints (pack_fingerprints' layout)."""
    F = np.ascontiguousarray(F, np.uint64)
    return np.unpackbits(F.view(np.uint8), axis=1, bitorder="little")


def tanimoto_dense(Fa, Fb, dtype):
    """The fingerprint producer's similarity on packed rows: c = popcount(a & b), u = popcount(a) + popcount(b) - c,
    s = u == 0 ? 1 : T(c) / T(u).  The counts are exact integers and the quotient is one correctly rounded division, so
    numpy gives the device's bits in both precisions."""
    A = unpack_bits(Fa).astype(np.float64)                 # 0 / 1: the products and sums below are exact integers
    B = A if Fb is None else unpack_bits(Fb).astype(np.float64)
    c = (A @ B.T).astype(np.int64)
    u = A.sum(1).astype(np.int64)[:, None] + B.sum(1).astype(np.int64)[None, :] - c
    T = np.dtype(dtype).type
    with np.errstate(invalid="ignore", divide="ignore"):
        s = c.astype(T) / u.astype(T)
    s[u == 0] = T(1)
    return s


# ---- the helpers of CutoffProfile by brute force (plain loops over a degree table)
def fill_ref(nnz, shape):
    return [n / (shape[0] * shape[1]) if shape[0] * shape[1] else 0.0 for n in nnz]


def coverage_ref(degrees, cuts, min_degree=1, exclude_self=False):
    degrees = np.asarray(degrees)
    out = []
    for b, c in enumerate(cuts):
        have = 0
        for i in range(degrees.shape[0]):
            deg = int(degrees[i, b])
            if exclude_self and c <= 1 and deg > 0:
                deg -= 1
            have += deg >= min_degree
        out.append(have / degrees.shape[0] if degrees.shape[0] else 0.0)
    return out


def alpha_for_nnz_ref(cuts, nnz, budget):
    for c, n in zip(cuts, nnz):
        if n <= budget:
            return c
    return None


def alpha_for_mean_degree_ref(cuts, nnz, na, k):
    for c, n in zip(cuts, nnz):
        if n <= k * na:
            return c
    return None
