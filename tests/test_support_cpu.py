"""support_ref.py, the host restatement of ss_support_*, pinned to the reference's predict: the contributions of a
(row, target) pair sum to its score (query rows and leave-one-out folds), and the list rules -- order, ties, padding,
nsupp beyond M -- hold on hand-made transfer rows."""
import numpy as np
import pytest
import scipy.sparse as sp

from oracle import simspread_oracle as O
from support_ref import support_lists, support_ref, transfer_rows


def _all_pairs(nrows, nt):
    r, t = np.meshgrid(np.arange(nrows), np.arange(nt), indexing="ij")
    return r.ravel(), t.ravel()


def _sums(contrib, nrows, nt):
    return contrib.sum(axis=1).reshape(nrows, nt)


def _weighted_graph(seed, ns=150, nq=40, nt=9):
    return O.synth_bipartite(nq, ns, ns, nt, 0.08, 0.2, seed=seed, weighted=True, dtype=np.float64)


def test_contributions_sum_to_the_score_on_the_kat(kats):
    p = kats["predict"]
    A = np.array(p["A"], dtype=np.float64)       # q1 | s1 s2 s3 | f1 f2 f3 | t1 t2
    Xq, Xs, Ys = A[0:1, 4:7], A[1:4, 4:7], A[1:4, 7:9]
    rows, targets = _all_pairs(1, 2)
    src, contrib, nsupp = support_ref(Xq, Xs, Ys, rows, targets, M=3)
    np.testing.assert_allclose(_sums(contrib, 1, 2), np.array(p["yhat"]), rtol=0, atol=1e-12)
    np.testing.assert_allclose(_sums(contrib, 1, 2), O.predict_factored(Xq, Xs, Ys, "query"), rtol=0, atol=1e-12)
    # t1 is held by s1 and s2, which q1 does not reach; t2 by s3 alone
    assert nsupp.tolist() == [0, 1]
    assert src.tolist() == [[-1, -1, -1], [2, -1, -1]]
    assert contrib[1, 0] == 0.5


@pytest.mark.parametrize("seed", [11, 12, 13])
def test_contributions_sum_to_the_score_query_rows(seed):
    Xq, Xs, Ys = _weighted_graph(seed)
    nq, nt = Xq.shape[0], Ys.shape[1]
    rows, targets = _all_pairs(nq, nt)
    src, contrib, nsupp = support_ref(Xq, Xs, Ys, rows, targets, M=Xs.shape[0])
    want = O.predict_factored(Xq, Xs, Ys, "query")
    assert np.abs(want).max() > 0
    np.testing.assert_allclose(_sums(contrib, nq, nt), want, rtol=0, atol=1e-12)
    assert (nsupp <= np.diff(sp.csc_matrix(Ys).indptr)[targets]).all()
    assert ((src >= 0).sum(axis=1) == nsupp).all()


@pytest.mark.parametrize("seed", [11, 12, 13])
def test_contributions_sum_to_the_score_loo_rows(seed):
    _, Xs, Ys = _weighted_graph(seed)
    ns, nt = Ys.shape
    rows, targets = _all_pairs(ns, nt)
    src, contrib, nsupp = support_ref(None, Xs, Ys, rows, targets, M=ns, loo=True)
    want = O.predict_loo_factored(Xs, Ys)
    assert np.abs(want).max() > 0
    np.testing.assert_allclose(_sums(contrib, ns, nt), want, rtol=0, atol=1e-12)
    # a fold never supports itself
    assert not (src == rows[:, None]).any()


def test_transfer_rows_match_the_reference_transfer_block():
    Xq, Xs, Ys = _weighted_graph(14)
    rows = [3, 0, 39]
    np.testing.assert_allclose(transfer_rows(Xq, Xs, Ys, rows), O.transfer_factored(Xq, Xs, Ys)[rows], rtol=1e-13,
                               atol=0)


def test_order_ties_padding_and_nsupp_beyond_m():
    # one transfer row, three targets over six sources
    T = np.array([[0.25, 0.5, 0.5, 0.0, 0.125, 0.5]])
    Ys = sp.csr_matrix(np.array([[1, 0, 1],
                                 [1, 0, 0],
                                 [1, 0, 2],
                                 [1, 0, 0],     # T == 0: stored label, no contribution
                                 [1, 0, 0],
                                 [1, 0, 0.5]], dtype=np.float64))
    slot = np.zeros(3, np.int64)
    src, contrib, nsupp = support_lists(T, slot, Ys, [0, 1, 2], M=4)
    # target 0: ties at 0.5 come in ascending source order; five contribute, four are listed
    assert nsupp.tolist() == [5, 0, 3]
    assert src[0].tolist() == [1, 2, 5, 0]
    assert contrib[0].tolist() == [0.5, 0.5, 0.5, 0.25]
    # target 1: nobody holds it
    assert src[1].tolist() == [-1] * 4 and contrib[1].tolist() == [0.0] * 4
    # target 2: the label value weighs in; ties between sources 0 and 5 at 0.25
    assert src[2].tolist() == [2, 0, 5, -1]
    assert contrib[2].tolist() == [1.0, 0.25, 0.25, 0.0]
    src1, contrib1, nsupp1 = support_lists(T, slot, Ys, [0, 1, 2], M=1)
    assert src1[:, 0].tolist() == [1, -1, 2] and nsupp1.tolist() == [5, 0, 3]


def test_products_are_rounded_in_the_dtype_of_the_transfer_row():
    T = np.array([[np.float32(1) / np.float32(3)]], dtype=np.float32)
    Ys = sp.csr_matrix(np.array([[0.1]]))
    _, contrib, _ = support_lists(T, [0], Ys, [0], M=1)
    assert contrib.dtype == np.float32
    assert contrib[0, 0] == T[0, 0] * np.float32(0.1)
