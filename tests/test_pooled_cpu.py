"""The host reference of pooled evaluation (tests/pooled_ref.py) against the host mirror on plain vectors -- the
reference's AuROC(vec(y), vec(yhat)) / maxperformance(vec(y), vec(yhat), f) on a flattened matrix -- and the algebra
the device pools rest on: a table of distinct scores is exact, and tables merge in any split and order to one table.
Also the ABI of the pool (header, ctypes table, exported symbols).  No GPU needed."""
import math

import numpy as np
import pytest

import simspread_jl_amd as ss
from simspread_jl_amd import _lib
import pooled_ref as R

_FNS = (ss.f1score, ss.mcc, ss.accuracy, ss.balancedaccuracy, ss.recall, ss.precision)


def _cases():
    rng = np.random.default_rng(7)
    n = 3000
    heavy = rng.integers(0, 12, n).astype(np.float64) / 4.0     # heavy ties
    heavy[rng.random(n) < 0.1] = -0.0                          # -0.0 ties with +0.0
    heavy[rng.random(n) < 0.05] = -99.0                        # clean!'s -99
    y = (rng.random(n) < 0.2).astype(np.uint8)
    yield "ties_f64", y, heavy
    yield "ties_f32", y, heavy.astype(np.float32)
    yield "distinct", y, rng.random(n)
    yield "single", y, np.full(n, 0.5)
    yield "no_positive", np.zeros(n, np.uint8), heavy
    yield "no_negative", np.ones(n, np.uint8), heavy
    yield "few", np.array([1, 0, 0, 1, 0], np.uint8), np.array([0.3, 0.3, -0.0, 0.0, -99.0])


def _trapezoid(y, s):
    """A literal per-threshold trapezoid: confusion matrices of metrics.roc at the distinct scores, highest first."""
    ths = np.unique(np.where(s == 0, 0, s))[::-1]
    c = ss.roc(y, s, ths)
    P, N = c[0].p, c[0].n
    tpr = [x.tp / P if P else math.nan for x in c]
    fpr = [x.fp / N if N else math.nan for x in c]
    prec = [x.tp / (x.tp + x.fp) for x in c]
    roc = math.fsum((fpr[k] - fpr[k - 1]) * (tpr[k] + tpr[k - 1]) / 2 for k in range(1, len(c)))
    prc = math.fsum((tpr[k] - tpr[k - 1]) * (prec[k] + prec[k - 1]) / 2 for k in range(1, len(c)))
    return abs(roc), abs(prc)


@pytest.mark.parametrize("name,y,s", list(_cases()), ids=[c[0] for c in _cases()])
def test_reference_matches_the_mirror(name, y, s):
    got, _ = R.metrics(*R.table(y, s))
    roc, prc = _trapezoid(y, s)
    for i, want in ((0, roc), (1, prc)):
        if math.isnan(want):
            assert math.isnan(got[i]), (name, i)
        else:
            assert abs(got[i] - want) <= 1e-12 * max(want, 1e-300), (name, i, got[i], want)
    assert got[2] == np.count_nonzero(s) / s.size
    for m, f in enumerate(_FNS):
        try:
            mx = ss.maxperformance(y, s, f)
            mean, std = ss.meanstdperformance(y, s, f)
        except ZeroDivisionError:   # mcc's limit forms with a class missing: Python raises, IEEE gives +-Inf / NaN
            assert f is ss.mcc and name.startswith("no_")
            continue
        k = 3 + 3 * m
        if math.isnan(mean):
            assert all(math.isnan(v) for v in got[k:k + 3]), (name, f.__name__)
            continue
        assert got[k] == mx, (name, f.__name__, got[k], mx)
        assert abs(got[k + 1] - mean) <= 1e-12 * max(abs(mean), 1.0), (name, f.__name__)
        if math.isnan(std):
            assert math.isnan(got[k + 2])
        else:
            assert abs(got[k + 2] - std) <= 1e-12 * max(std, 1.0), (name, f.__name__)


def test_single_distinct_score_and_missing_class():
    y = np.array([1, 0, 1, 0], np.uint8)
    one, _ = R.metrics(*R.table(y, np.full(4, 2.0)))
    assert one[0] == 0.0 and one[1] == 0.0                 # one threshold: no trapezoid at all
    assert all(math.isnan(one[5 + 3 * m]) for m in range(6))   # std over one threshold
    nop, _ = R.metrics(*R.table(np.zeros(4), np.array([1.0, 2.0, 2.0, 3.0])))
    assert math.isnan(nop[0]) and math.isnan(nop[1])
    assert all(math.isnan(v) for v in nop[12:15])          # recall (and balancedaccuracy) undefined without positives


def test_tables_merge_in_any_split_and_order():
    rng = np.random.default_rng(11)
    n = 5000
    s = rng.integers(-3, 40, n).astype(np.float32) / 8
    s[rng.random(n) < 0.05] = -0.0
    y = rng.random(n) < 0.1
    whole = R.table(y, s)
    for trial in range(5):
        cuts = np.sort(rng.choice(np.arange(1, n), size=trial + 2, replace=False))
        parts = [R.table(yy, ss_) for yy, ss_ in zip(np.split(y, cuts), np.split(s, cuts))]
        order = rng.permutation(len(parts))
        merged = R.merge(*[parts[i] for i in order])
        # pairwise, in another order
        acc = parts[order[-1]]
        for i in order[:-1]:
            acc = R.merge(parts[i], acc)
        for t in (merged, acc):
            for a, b in zip(t, whole):
                np.testing.assert_array_equal(a, b)
    np.testing.assert_array_equal(R.metrics(*merged)[0], R.metrics(*whole)[0])


def test_counts_past_int64_products_use_python_integers():
    # ~1e10 pairs: tp*tn passes 2^63; the reference stays the mirror's Python-integer value
    keys = np.array([3.0, 2.0, 1.0, 0.0])
    npos = np.array([4_000_000_000, 3_000_000_000, 2_000_000_000, 1_000_000_000], np.int64)
    nneg = np.array([1_000_000_000, 5_000_000_000, 9_000_000_000, 13_000_000_000], np.int64)
    got, _ = R.metrics(keys, npos, nneg)
    P, N = int(npos.sum()), int(nneg.sum())
    tp, fp = 4_000_000_000, 1_000_000_000
    c = ss.ROCNums(P, N, tp, N - fp, fp, P - tp)
    assert got[6] >= ss.mcc(c)                              # mcc max over thresholds includes this one
    assert (tp * (N - fp)) > 2 ** 63


def test_pool_abi_is_declared_and_exported():
    names = ["ss_pool_create_f32", "ss_pool_create_f64", "ss_pool_destroy", "ss_pool_reset", "ss_pool_info",
             "ss_pool_add_rows_f32", "ss_pool_add_rows_f64", "ss_pool_add_loo_f32", "ss_pool_add_loo_f64",
             "ss_pool_add_kfold_f32", "ss_pool_add_kfold_f64", "ss_pool_merge", "ss_pool_export_f32",
             "ss_pool_export_f64", "ss_pool_import_f32", "ss_pool_import_f64", "ss_pool_metrics"]
    declared = set(_lib.header_symbols())
    lib = _lib.load()
    for nm in names:
        assert nm in declared and nm in _lib.SIGNATURES and hasattr(lib, nm), nm
    assert ss.POOLED_FIELDS == R.FIELDS
