"""Host reference of featurize on a CSR matrix (ss_cutoff_csr_*, ss_graph_recut_*), shared by the CPU and GPU tests."""
import numpy as np
import scipy.sparse as sp


def ref_cutoff_csr(X, alpha, weighted, dt):
    """Entry (i, j) exists iff X stores v there, v >= alpha (in the precision dt) and w = v if weighted else 1 is
    non-zero; order inside a row is kept.  Returns a scipy CSR with int64 pointers, int32 indices, dt values."""
    X = sp.csr_matrix(X)
    X.sort_indices()
    v = X.data.astype(dt)
    w = v if weighted else np.ones_like(v)
    with np.errstate(invalid="ignore"):
        keep = (v >= dt(alpha)) & (w != 0)
    rows = np.repeat(np.arange(X.shape[0]), np.diff(X.indptr))
    counts = np.bincount(rows[keep], minlength=X.shape[0])
    ptr = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    out = sp.csr_matrix((w[keep].astype(dt), X.indices[keep].astype(np.int32), ptr), shape=X.shape)
    return out


def assert_csr_bitwise(got, want):
    got, want = sp.csr_matrix(got), sp.csr_matrix(want)
    assert got.shape == want.shape
    assert np.array_equal(got.indptr, want.indptr)
    assert np.array_equal(got.indices, want.indices)
    assert got.data.dtype == want.data.dtype
    assert np.array_equal(got.data.view(np.uint8), want.data.view(np.uint8))
