"""Per-target top-L tables without a GPU: the numpy reference (tests/target_topl_ref.py) against a literal
restatement of the reference's grouped recallatL / precisionatL with grouping = target on vec of random matrices,
the reference's own known-answer test, ties, +-0.0, -99, the NaN mean, rows <= L, and the ctypes / header tables."""
import math

import numpy as np
import pytest

import target_topl_ref as R
from simspread_jl_amd import _lib

EXPORTS = ["ss_target_topl_create_f32", "ss_target_topl_create_f64", "ss_target_topl_destroy", "ss_target_topl_reset",
           "ss_target_topl_info", "ss_target_topl_add_rows_f32", "ss_target_topl_add_rows_f64",
           "ss_target_topl_add_loo_f32", "ss_target_topl_add_loo_f64", "ss_target_topl_add_kfold_f32",
           "ss_target_topl_add_kfold_f64", "ss_target_topl_merge", "ss_target_topl_export_f32",
           "ss_target_topl_export_f64", "ss_target_topl_import_f32", "ss_target_topl_import_f64",
           "ss_target_topl_metrics"]


def _grouped_by_target(Y, S, L):
    n, nt = S.shape
    grouping = np.repeat(np.arange(nt), n)                  # target of every entry of vec (column-major)
    return R.julia_grouped(Y.ravel(order="F"), S.ravel(order="F"), grouping, L)


def _same(a, b):
    assert (math.isnan(a) and math.isnan(b)) or a == b, (a, b)


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_reference_is_the_grouped_recall_and_precision_by_target(dtype):
    rng = np.random.default_rng(11)
    for n, nt, L, levels in ((40, 7, 5, 6), (90, 13, 20, 30), (30, 4, 1, 3), (25, 5, 24, 1000)):
        S = (rng.integers(-3, levels, (n, nt)) / 4).astype(dtype)
        S[rng.random((n, nt)) < 0.1] = dtype(-99.0)
        S[rng.random((n, nt)) < 0.1] = dtype(-0.0)
        S[rng.random((n, nt)) < 0.1] = dtype(0.0)
        Y = (rng.random((n, nt)) < 0.2).astype(np.int64)
        Y[:, 0] = 0                                         # a target without positives: the mean is NaN
        vals, rid, lab, npos = R.table(Y, S, L)
        got, _ = R.metrics(lab, npos, L)
        want = _grouped_by_target(Y, S, L)
        _same(got[0], want[0])
        assert math.isnan(got[0])
        assert got[1] == want[1]
        # without the empty target the means are finite and still the reference's
        Y[:, 0] = 1
        vals, rid, lab, npos = R.table(Y, S, L)
        got, _ = R.metrics(lab, npos, L)
        want = _grouped_by_target(Y, S, L)
        assert got[0] == want[0] and got[1] == want[1] and got[2] == got[0] and got[3] == nt


def test_known_answers_of_the_reference():
    # test/runtests.jl:226-243: one group, scores 1..10, positives at rows 8..10
    y = np.array([0, 0, 0, 0, 0, 0, 0, 1, 1, 1])
    S = np.arange(1, 11, dtype=np.float64).reshape(10, 1)
    for L, rec, prec in ((5, 1.0, 3 / 5), (1, 1 / 3, 1.0)):
        _, _, lab, npos = R.table(y.reshape(10, 1), S, L)
        got, hits = R.metrics(lab, npos, L)
        assert got[0] == pytest.approx(rec) and got[1] == pytest.approx(prec)
        assert (got[0], got[1]) == R.julia_grouped(y, S.ravel(), np.ones(10), L)


def test_ties_zeros_and_clean_scores_order():
    # ties by ascending row, +0.0 before -0.0, -99 below every non-negative score
    S = np.array([[0.5], [-0.0], [0.0], [0.5], [-99.0], [0.0], [1.0]], dtype=np.float32)
    vals, rid, lab, _ = R.table(np.zeros_like(S), S, 7)
    assert rid[0].tolist() == [6, 0, 3, 2, 5, 1, 4]
    assert np.signbit(vals[0]).tolist() == [False, False, False, False, False, True, True]
    # row ids other than 0..n-1: the order is by id, not by position
    vals, rid, _, _ = R.table(np.zeros_like(S), S, 3, rows=[9, 8, 7, 6, 5, 4, 3])
    assert rid[0].tolist() == [3, 6, 9]


def test_rows_at_most_L_are_refused_by_the_reference():
    S = np.arange(5, dtype=np.float64).reshape(5, 1)
    with pytest.raises(AssertionError, match="less than length"):
        R.julia_grouped(np.ones(5), S.ravel(), np.ones(5), 5)


def test_ctypes_and_header_cover_every_new_export():
    declared = _lib.header_symbols()
    for name in EXPORTS:
        assert name in declared, name
        assert name in _lib.SIGNATURES, name
    assert len([s for s in declared if s.startswith("ss_target_topl_")]) == 17
    lib = _lib.load()
    assert all(hasattr(lib, s) for s in EXPORTS)
