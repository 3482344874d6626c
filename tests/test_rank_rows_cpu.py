"""Per-row ranking metrics (ss_rank_metrics_rows_*, ss_evaluate_loo_*) without a GPU: the C / ctypes / Julia surface of
the four new entry points, the Python wrapper's argument checks (they must fire before the device is touched: on a
machine without a GPU any library call would raise SS_ENODEV instead), and the host reference of tests/rank_ref.py
against the literal oracle."""
import os
import re

import numpy as np
import pytest
import scipy.sparse as sp

import simspread_jl_amd as ss
from oracle import simspread_oracle as O
from simspread_jl_amd import _lib
from rank_ref import FIELDS, assert_rows_close, ref_row

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["ss_rank_metrics_rows_f32", "ss_rank_metrics_rows_f64", "ss_evaluate_loo_f32", "ss_evaluate_loo_f64"]


def test_new_symbols_are_declared_bound_and_exported():
    hdr = _lib.header_symbols()
    for name in NEW:
        assert name in hdr and name in _lib.SIGNATURES, name
    with open(os.path.join(ROOT, "julia", "SimSpreadHIP.jl")) as f:
        jl = f.read()
    for name in NEW:
        assert re.search(r"ccall\(\(:" + name + r"\b", jl), name
    for fn in ("rank_metrics_rows", "evaluate_loo"):
        assert re.search(r"^function " + fn + r"\(", jl, flags=re.M), fn
    lib = _lib.load()
    for name in NEW:
        assert hasattr(lib, name), name
    assert ss.RANK_ROWS_FIELDS == FIELDS
    assert callable(ss.rank_metrics_rows) and callable(ss.DeviceGraph.evaluate_loo)


def _case():
    S = np.array([[0.3, 0.1, 0.2, 0.0], [0.0, 0.5, 0.5, 0.1]], np.float32)
    Y = np.array([[1, 0, 0, 1], [0, 1, 0, 0]], np.uint8)
    return Y, S


def test_wrapper_rejects_shape_mismatch():
    Y, S = _case()
    with pytest.raises(ValueError):
        ss.rank_metrics_rows(Y[:, :3], S, L=1)
    with pytest.raises(ValueError):
        ss.rank_metrics_rows(sp.csr_matrix(Y[:1]), S, L=1)
    with pytest.raises(ValueError):
        ss.rank_metrics_rows((np.array([0, 1], np.int64), np.array([0], np.int32)), S, L=1)   # ptr of 1 row for 2
    with pytest.raises(ValueError):
        ss.rank_metrics_rows(Y[0], S[0], L=1)                                                 # 1-D scores
    with pytest.raises(TypeError):
        ss.rank_metrics_rows(Y, S.astype(np.float16), L=1)


def test_wrapper_rejects_L_as_the_reference_does():
    Y, S = _case()
    with pytest.raises(AssertionError, match=re.escape("Number of labels is less than length (L > y)")):
        ss.rank_metrics_rows(Y, S, L=4)
    with pytest.raises(AssertionError, match=re.escape("Number of labels is less than length (L > y)")):
        ss.rank_metrics_rows(Y, S, L=9)
    with pytest.raises(AssertionError, match="greater than 0"):
        ss.rank_metrics_rows(Y, S, L=0)


@pytest.mark.parametrize("idx, why", [([2, 1, 3], "unsorted"), ([1, 1, 3], "duplicate"), ([0, 4, 1], "range"),
                                      ([0, -1, 1], "range")])
def test_wrapper_rejects_bad_label_indices(idx, why):
    _, S = _case()
    ptr = np.array([0, 2, 3], np.int64)
    with pytest.raises(ValueError, match="sorted and unique" if why != "range" else "out of range"):
        ss.rank_metrics_rows((ptr, np.array(idx, np.int32)), S, L=1)


def test_wrapper_rejects_unsorted_scipy_labels():
    _, S = _case()
    m = sp.csr_matrix((np.ones(3), np.array([3, 0, 1], np.int32), np.array([0, 2, 3])), shape=(2, 4))
    assert not m.has_sorted_indices
    with pytest.raises(ValueError, match="sorted and unique"):
        ss.rank_metrics_rows(m, S, L=1)


def _oracle_row(y, s, alpha, L):
    with np.errstate(invalid="ignore", divide="ignore"):
        head = [O.auroc(y, s), O.auprc(y, s), O.bedroc(y, s, alpha=alpha), O.validity_ratio(s)]
    order = np.argsort(-np.asarray(s, np.float64), kind="stable")
    hits = int((np.asarray(y) != 0)[order][:L].sum())
    P = int(np.count_nonzero(y))
    return np.array(head + [hits / P if P else np.nan, hits / L])


def test_host_reference_matches_the_literal_oracle():
    rng = np.random.default_rng(11)
    for t in range(600):
        n = int(rng.integers(2, 40))
        vals = np.array([0.0, -99.0, 0.5, 1.0, 2.0, 0.25])
        s = rng.choice(vals[:int(rng.integers(1, 7))], n) if t % 3 else rng.random(n)
        y = (rng.random(n) < rng.random()).astype(np.uint8)
        if t % 17 == 0:
            y[:] = 0
        if t % 19 == 0:
            y[:] = 1
        L = int(rng.integers(1, n))
        assert_rows_close(ref_row(y, s, 20.0, L)[None], _oracle_row(y, s, 20.0, L)[None], 1e-12, 1e-14, f"case {t}")
