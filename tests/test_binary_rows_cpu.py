"""Per-row binary prediction metrics (ss_binary_metrics_rows_*, ss_evaluate_loo_binary_*) without a GPU: the C / ctypes
/ Julia surface of the four entry points, the Python wrapper's argument checks (they must fire before the device is
touched: on a machine without a GPU any library call would raise SS_ENODEV instead), and the host reference of
tests/binary_ref.py against the host mirror (simspread_jl_amd.metrics) and the definition's degenerate rows."""
import math
import os
import re

import numpy as np
import pytest
import scipy.sparse as sp

import simspread_jl_amd as ss
from binary_ref import FIELDS, METRICS, ref_row, threshold_values
from simspread_jl_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["ss_binary_metrics_rows_f32", "ss_binary_metrics_rows_f64", "ss_evaluate_loo_binary_f32",
       "ss_evaluate_loo_binary_f64"]


def _mcc_ieee(c):
    """ss.mcc with IEEE division: where a limit form's denominator underflows to 0, Python raises and Julia (the
    definition) divides, giving +-Inf."""
    try:
        return ss.mcc(c)
    except ZeroDivisionError:
        tn, fp, fn, tp = c.tn, c.fp, c.fn, c.tp
        if tp + fp == 0:
            a, b = tn, fn
        elif fn + tn == 0:
            a, b = tp, fp
        elif tp + fn == 0:
            a, b = tn, fp
        else:
            a, b = tp, fn
        num = float(a) * 2.2250738585072014e-308 - float(b) * 2.2250738585072014e-308
        return math.copysign(math.inf, num) if num != 0 else math.nan


MIRROR = [ss.f1score, _mcc_ieee, ss.accuracy, ss.balancedaccuracy, ss.recall, ss.precision]


def test_new_symbols_are_declared_bound_and_exported():
    hdr = _lib.header_symbols()
    for name in NEW:
        assert name in hdr and name in _lib.SIGNATURES, name
    with open(os.path.join(ROOT, "julia", "SimSpreadHIP.jl")) as f:
        jl = f.read()
    for name in NEW:
        assert re.search(r"ccall\(\(:" + name + r"\b", jl), name
    for fn in ("binary_metrics_rows", "evaluate_loo_binary"):
        assert re.search(r"^function " + fn + r"\(", jl, flags=re.M), fn
    lib = _lib.load()
    for name in NEW:
        assert hasattr(lib, name), name
    assert ss.BINARY_ROWS_FIELDS == FIELDS
    assert FIELDS[:3] == ("f1score_max", "f1score_mean", "f1score_std") and len(FIELDS) == 18
    assert callable(ss.binary_metrics_rows) and callable(ss.DeviceGraph.evaluate_loo_binary)


def _case():
    S = np.array([[0.3, 0.1, 0.2, 0.0], [0.0, 0.5, 0.5, 0.1]], np.float32)
    Y = np.array([[1, 0, 0, 1], [0, 1, 0, 0]], np.uint8)
    return Y, S


def test_wrapper_rejects_bad_shapes():
    Y, S = _case()
    with pytest.raises(ValueError):
        ss.binary_metrics_rows(Y[:, :3], S)
    with pytest.raises(ValueError):
        ss.binary_metrics_rows(sp.csr_matrix(Y[:1]), S)
    with pytest.raises(ValueError):
        ss.binary_metrics_rows((np.array([0, 1], np.int64), np.array([0], np.int32)), S)   # ptr of 1 row for 2
    with pytest.raises(ValueError):
        ss.binary_metrics_rows(Y[0], S[0][:3])                                              # 1-D, lengths differ
    with pytest.raises(ValueError):
        ss.binary_metrics_rows(Y, S[0])                                                     # 1-D scores, 2-D labels
    with pytest.raises(ValueError):
        ss.binary_metrics_rows(Y[None], S[None])                                            # 3-D
    with pytest.raises(ValueError):
        ss.binary_metrics_rows(np.zeros((2, 0), np.uint8), np.zeros((2, 0), np.float32))    # ncols = 0
    with pytest.raises(TypeError):
        ss.binary_metrics_rows(Y, S.astype(np.float16))


@pytest.mark.parametrize("idx, why", [([2, 1, 3], "unsorted"), ([1, 1, 3], "duplicate"), ([0, 4, 1], "range"),
                                      ([0, -1, 1], "range")])
def test_wrapper_rejects_bad_label_indices(idx, why):
    _, S = _case()
    ptr = np.array([0, 2, 3], np.int64)
    with pytest.raises(ValueError, match="sorted and unique" if why != "range" else "out of range"):
        ss.binary_metrics_rows((ptr, np.array(idx, np.int32)), S)


def test_wrapper_rejects_unsorted_scipy_labels():
    _, S = _case()
    m = sp.csr_matrix((np.ones(3), np.array([3, 0, 1], np.int32), np.array([0, 2, 3])), shape=(2, 4))
    assert not m.has_sorted_indices
    with pytest.raises(ValueError, match="sorted and unique"):
        ss.binary_metrics_rows(m, S)


def _mirror_row(y, s):
    """max via ss.maxperformance, mean and std via ss.meanstdperformance, per metric (the host mirror)."""
    out = []
    for f in MIRROR:
        with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
            mean, std = ss.meanstdperformance(y, s, f)
            out += [ss.maxperformance(y, s, f), mean, std]
    return np.array(out)


def test_host_reference_matches_the_mirror():
    rng = np.random.default_rng(17)
    for t in range(400):
        n = int(rng.integers(1, 40))
        vals = np.array([0.0, -99.0, 0.5, 1.0, 2.0, 0.25, -0.0])
        s = rng.choice(vals[:int(rng.integers(1, 8))], n) if t % 3 else rng.random(n)
        s = s.astype(np.float32 if t % 2 else np.float64)
        y = (rng.random(n) < rng.random()).astype(np.uint8)
        if t % 17 == 0:
            y[:] = 0
        if t % 19 == 0:
            y[:] = 1
        got, want = ref_row(y, s), _mirror_row(y, s)
        g3, w3 = got.reshape(6, 3), want.reshape(6, 3)
        for k, name in enumerate(METRICS):
            if np.isnan(threshold_values(y, s)[:, k]).any():
                # Python's max() does not propagate NaN; the definition (Julia's maximum) does
                assert np.isnan(g3[k]).all(), (t, name)
                continue
            assert g3[k, 0] == w3[k, 0] or (np.isinf(w3[k, 0]) and g3[k, 0] == w3[k, 0]), (t, name, g3[k], w3[k])
            for s_ in (1, 2):
                a, b = g3[k, s_], w3[k, s_]
                if np.isnan(b) or np.isinf(b):
                    assert (np.isnan(a) and np.isnan(b)) or a == b, (t, name, s_, a, b)
                else:
                    assert abs(a - b) <= 1e-12 * max(1.0, abs(b)), (t, name, s_, a, b)


def test_degenerate_rows_follow_the_definition():
    # n = 1: one threshold; std NaN everywhere
    r = ref_row([1], [0.5]).reshape(6, 3)
    assert np.isnan(r[:, 2]).all()
    assert r[0, 0] == r[0, 1] == 1.0                                    # f1 = 1
    assert math.isinf(r[1, 0]) and r[1, 0] > 0                          # mcc limit form (tp, fp) = (1, 0) -> +Inf
    assert np.isnan(r[3]).all()                                         # balancedaccuracy: N == 0
    assert r[4, 0] == 1.0 and r[5, 0] == 1.0
    # P = 0: recall and balancedaccuracy NaN, precision 0, f1 0
    r = ref_row(np.zeros(5), [0.1, 0.2, 0.2, 0.3, 0.0]).reshape(6, 3)
    assert np.isnan(r[4]).all() and np.isnan(r[3]).all()
    assert (r[5, :2] == 0).all() and (r[0, :2] == 0).all()
    assert r[1, 1] == -math.inf                                         # mcc's (tp, fp) = (0, N) form at the bottom
    # N = 0: balancedaccuracy NaN; accuracy, recall, precision at thresholds of all-positive rows
    r = ref_row(np.ones(4), [0.1, 0.2, 0.2, 0.3]).reshape(6, 3)
    assert np.isnan(r[3]).all()
    assert r[2, 0] == 1.0 and r[5, 0] == 1.0 and r[5, 2] == 0.0
    # U = 1: a single distinct score (ties everywhere, -0.0 == +0.0)
    r = ref_row([1, 0, 0], [0.0, -0.0, 0.0]).reshape(6, 3)
    assert np.isnan(r[:, 2]).all()
    assert r[2, 0] == r[2, 1] == 1 / 3                                  # accuracy: everything predicted positive
    assert r[5, 0] == 1 / 3 and r[4, 0] == 1.0
    assert r[0, 0] == 1 / (1 + 0.5 * 2)
    # the mcc numerator and denominator as the mirror forms them (Python integers)
    y = np.r_[np.ones(7), np.zeros(5)]
    s = np.arange(12.0)[::-1]
    v = threshold_values(y, s)
    for u, c in enumerate(ss.roc(y, s, np.unique(s)[::-1])):
        assert v[u, 1] == _mcc_ieee(c), u
