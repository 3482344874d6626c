"""The tile skeleton the three fused producers share (csrc/pair_tile.hpp), on the one case their own case matrices do
not guarantee: a tile that keeps nothing between tiles that keep something.  Its counts must be zero slots in the rows'
offsets, the producers that skip such tiles in the fill pass must skip exactly these, and the mirror of the empty tile
must stay empty.

n = 300 is a 3 x 3 grid of 128 x 128 tiles with a partial last tile.  Rows 0..127 live on the first half of the
features and rows 128..255 on the second half, no row is zero, so every similarity between the two groups is 0 and tile
(0, 1) and its mirror keep nothing at alpha > 0; rows 256..299 are copies of rows of both groups, so tiles (0, 2) and
(1, 2) keep something.  The cross call against the first 140 rows has the empty tile at (1, 0).  The features are small
integers, so the inner-product producer is bitwise defined too (dot_ref.ref_exact); every CSR is compared bit for bit
with the host reference of the producer's own test file."""
import numpy as np
import pytest

import simspread_jl_amd as ss

import dot_ref
import test_gpu_fingerprint as fp_ref
import test_gpu_jaccard_csr as jac_ref

pytestmark = pytest.mark.gpu

N, NB, D, TILE = 300, 140, 16, 128
ALPHA = 0.5


def two_group_rows():
    rng = np.random.default_rng(300)
    X = np.zeros((N, D))
    for lo, rows in ((0, slice(0, TILE)), (D // 2, slice(TILE, 2 * TILE))):
        X[rows, lo:lo + D // 2] = rng.integers(0, 4, (TILE, D // 2))
        X[rows, lo] = rng.integers(1, 4, TILE)           # no zero row: two zero rows would be identical (s = 1)
    tail = np.arange(2 * TILE, N)
    X[tail] = X[np.where(tail % 2 == 0, tail - 2 * TILE, tail - TILE)]   # copies of rows 0, 129, 2, 131, ...
    return X


def producer(name, dt):
    """(device call, host reference) of one producer: (Fa, Fb or None, weighted) -> CSR at ALPHA."""
    if name == "tanimoto":
        def run(A, B, weighted):
            return ss.tanimoto_csr(ss.pack_fingerprints(A > 0), None if B is None else ss.pack_fingerprints(B > 0),
                                   alpha=ALPHA, weighted=weighted, dtype=dt)

        def ref(A, B, weighted):
            Pa, Pb = ss.pack_fingerprints(A > 0), ss.pack_fingerprints((A if B is None else B) > 0)
            return fp_ref.ref_cut(fp_ref.ref_similarity(*fp_ref.ref_counts(Pa, Pb), dt), ALPHA, weighted, dt)
        return [(run, ref)]
    if name == "jaccard":
        def run(A, B, weighted):
            return ss.jaccard_csr(A, B, alpha=ALPHA, weighted=weighted, dtype=dt)

        def ref(A, B, weighted):
            return jac_ref.ref_cut(jac_ref.ref_similarity(A, A if B is None else B, dt), ALPHA, weighted, dt)
        return [(run, ref)]
    out = []
    for metric in dot_ref.METRICS:
        def run(A, B, weighted, metric=metric):
            return ss.dot_csr(A, B, metric=metric, alpha=ALPHA, weighted=weighted, dtype=dt)

        def ref(A, B, weighted, metric=metric):
            e = dot_ref.ref_exact(A, A if B is None else B, metric, dt, sym=B is None)
            return dot_ref.ref_cut(e, ALPHA, weighted, dt)
        out.append((run, ref))
    return out


def block_nnz(M, it, jt):
    return M[it * TILE:(it + 1) * TILE, jt * TILE:(jt + 1) * TILE].nnz


@pytest.mark.parametrize("dt", [np.float32, np.float64])
@pytest.mark.parametrize("name", ["tanimoto", "jaccard", "dot"])
def test_an_empty_tile_between_kept_tiles(name, dt):
    ss.init(0)
    X = two_group_rows()
    for run, ref in producer(name, dt):
        for weighted in (True, False):
            want = ref(X, None, weighted)
            # the case is what it claims to be, by the host reference alone
            assert block_nnz(want, 0, 1) == 0 and block_nnz(want, 1, 0) == 0
            assert block_nnz(want, 0, 2) > 0 and block_nnz(want, 1, 2) > 0 and block_nnz(want, 2, 2) > 0
            assert 0 < block_nnz(want, 0, 0) < TILE * TILE       # the cutoff keeps some pairs and drops others
            fp_ref.assert_csr_equal(run(X, None, weighted), want)
            want_x = ref(X, X[:NB], weighted)
            assert block_nnz(want_x, 1, 0) == 0
            assert block_nnz(want_x, 0, 0) > 0 and block_nnz(want_x, 1, 1) > 0 and block_nnz(want_x, 2, 0) > 0
            fp_ref.assert_csr_equal(run(X, X[:NB], weighted), want_x)
