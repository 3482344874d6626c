"""Host reference of the neighbour floor of the real-valued producers (include/simspread_hip_neighbours_real.h): dense
similarities that are bitwise defined, and the inputs of the case matrix.  The rule itself (tau, the keep rule) is
tests/neighbour_ref.py: ref_kth, ref_floor, ref_cut, assert_csr_equal, positives.

    jaccard   smin, smax summed sequentially over k in dt, one division: bitwise what the device computes on any input
    dot       dot_ref.ref_exact: the rule in dt on exact integer sums; on integer-valued rows g, A and B are exact in any
              order, so the device (whatever order the matrix cores sum in) must equal it bit for bit
"""
import functools

import numpy as np

import dot_ref
from neighbour_ref import assert_csr_equal, positives, ref_cut, ref_floor, ref_kth  # noqa: F401  (re-exported)
from test_gpu_jaccard_csr import features, ref_similarity

N, NQ, D = 300, 130, 37          # three 128-tiles with a ragged last one; three staging steps of 16 with a ragged last one
KS = (1, 5, 33, 64)              # 33 crosses the fp64 rows-per-block switch
ALPHAS = (0.7, np.inf, -0.5)


def jaccard_s(A, B, dt):
    """Dense weighted Jaccard of the rows of A against those of B (None: A) in precision dt."""
    A = np.asarray(A, dt)
    s = ref_similarity(A, A if B is None else np.asarray(B, dt), dt)
    return np.ascontiguousarray(s, dtype=dt)


def dot_s(A, B, metric, dt):
    """Dense inner-product similarity of integer-valued rows; B None: A against itself with the diagonal exactly 1."""
    return np.ascontiguousarray(dot_ref.ref_exact(A, A if B is None else B, metric, dt, sym=B is None), dtype=dt)


@functools.lru_cache(maxsize=None)
def feature_rows():
    """The Jaccard source set: features(300, 37, 11) with zero rows {0, 5, 299} and rows 10..49 exact copies of row 7."""
    X = features(N, D, 11)
    X[[0, 5, N - 1]] = 0
    X[10:50] = X[7]
    X.setflags(write=False)
    return X


@functools.lru_cache(maxsize=None)
def feature_queries():
    """130 query rows: 60 near sources, one all-zero, one an exact copy of the duplicated source row."""
    X = features(NQ, D, 12)
    src = feature_rows()
    rng = np.random.default_rng(6)
    X[:60] = src[rng.integers(0, N, 60)] * np.exp(rng.normal(0, 0.05, (60, D)))
    X[3] = 0
    X[4] = src[7]
    X.setflags(write=False)
    return X


@functools.lru_cache(maxsize=None)
def integer_sources():
    X = dot_ref.integer_rows(N, D, 5)
    X.setflags(write=False)
    return X


@functools.lru_cache(maxsize=None)
def integer_queries():
    X = dot_ref.integer_rows(NQ, D, 6)
    X[20:40] = integer_sources()[100:120]          # exact copies of sources: similarity 1 off any diagonal
    X.setflags(write=False)
    return X


def tied_rows(s, k):
    """Rows with at least k positives whose k-th largest positive value occurs more than once."""
    tau = ref_kth(s, k)
    return np.nonzero((positives(s) >= k) & (((s == tau[:, None]) & (s > 0)).sum(axis=1) > 1))[0]


def gained_rows(s, alpha, k):
    """Rows to which the floor adds entries at this alpha."""
    return np.nonzero(np.diff(ref_floor(s, alpha, k, True).indptr) > np.diff(ref_cut(s, alpha, True).indptr))[0]
