"""k-fold row blocks (ss_predict_kfold_rows_*, ss_evaluate_kfold_*, ss_evaluate_kfold_binary_*) without a GPU: the C /
ctypes / Julia surface of the six entry points and the Python wrapper's argument checks, which must fire before the
library is touched."""
import os
import re

import numpy as np
import pytest

import simspread_jl_amd as ss
from simspread_jl_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = [f"{base}_{suf}" for base in ("ss_predict_kfold_rows", "ss_evaluate_kfold", "ss_evaluate_kfold_binary")
       for suf in ("f32", "f64")]


def test_new_symbols_are_declared_bound_and_exported():
    hdr = _lib.header_symbols()
    for name in NEW:
        assert name in hdr and name in _lib.SIGNATURES, name
    with open(os.path.join(ROOT, "julia", "SimSpreadHIP.jl")) as f:
        jl = f.read()
    for name in NEW:
        assert re.search(r"ccall\(\(:" + name + r"\b", jl), name
    for fn in ("predict_kfold_rows", "evaluate_kfold", "evaluate_kfold_binary"):
        assert re.search(r"^function " + fn + r"\(", jl, flags=re.M), fn
    lib = _lib.load()
    for name in NEW:
        assert hasattr(lib, name), name
    for fn in ("predict_kfold_rows", "evaluate_kfold", "evaluate_kfold_binary"):
        assert callable(getattr(ss.DeviceGraph, fn)), fn


def test_signatures_match_the_header_argument_counts():
    with open(os.path.join(ROOT, "include", "simspread_hip.h")) as f:
        hdr = f.read()
    for name in NEW:
        m = re.search(r"\b" + name + r"\(([^)]*)\)", hdr)
        assert m, name
        assert len(_lib.SIGNATURES[name][0]) == m.group(1).count(",") + 1, name


class _NoLib:
    def __getattr__(self, name):
        raise AssertionError(f"the library was touched ({name}) before the arguments were checked")


def _graph(monkeypatch, ns=10, nt=30):
    """A DeviceGraph shell (no handle, no device) whose library access fails the test."""
    g = object.__new__(ss.DeviceGraph)
    g._h = None
    g.dtype = np.dtype(np.float32)
    g._suf = "f32"
    g.general = False
    g.nq, g.ns, g.nf, g.nt = 0, ns, ns, nt
    monkeypatch.setattr(_lib, "lib", lambda: _NoLib())
    monkeypatch.setattr(_lib, "load", lambda: _NoLib())
    return g


@pytest.mark.parametrize("fold", [np.zeros(9, np.int32), np.zeros(11, np.int32), np.zeros((10, 1), np.int32),
                                  np.zeros((2, 5), np.int32), np.zeros(10, np.float64), np.full(10, 0.5),
                                  np.zeros(10, bool), np.array([1 << 40] * 10)])
def test_bad_fold_assignments_are_refused_in_python(monkeypatch, fold):
    g = _graph(monkeypatch)
    with pytest.raises(ValueError):
        g.predict_kfold_rows(fold, 2)
    with pytest.raises(ValueError):
        g.evaluate_kfold(fold, 2, L=5)
    with pytest.raises(ValueError):
        g.evaluate_kfold_binary(fold, 2)


def test_bad_L_is_refused_in_python(monkeypatch):
    g = _graph(monkeypatch, nt=30)
    fold = np.zeros(10, np.int32)
    for L in (0, -3, 30, 31):
        with pytest.raises(AssertionError, match="L > "):     # the reference's assertions, as evaluate_loo raises them
            g.evaluate_kfold(fold, 1, L=L)


def test_nfolds_defaults_to_the_largest_id_plus_one(monkeypatch):
    g = _graph(monkeypatch)
    fold, nfolds = g._folds(np.array([0, 3, 1, 1, 2, 0, 0, 3, 3, 1], np.int64), None)
    assert fold.dtype == np.int32 and fold.flags.c_contiguous and nfolds == 4
    assert g._folds(list(range(10)), 12)[1] == 12
