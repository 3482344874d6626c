"""CPU-side checks of the real-valued feature route (no GPU): the four weighted-Jaccard CSR entry points are declared,
exported and bound (ctypes and Julia), refuse to run without ss_init (no CPU fallback), and the Python mirror rejects
wrong dtypes and shapes on the host before it calls the library."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import simspread_jl_amd as ss
from simspread_jl_amd import _lib

NAMES = {"ss_similarity_jaccard_csr_f32", "ss_similarity_jaccard_csr_f64",
         "ss_graph_create_features_f32", "ss_graph_create_features_f64"}
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_jaccard_csr_symbols_are_declared_exported_and_bound():
    assert NAMES <= set(_lib.header_symbols())
    assert NAMES <= set(_lib.SIGNATURES)
    lib = _lib.load()
    assert all(hasattr(lib, n) for n in NAMES)
    with open(os.path.join(ROOT, "julia", "SimSpreadHIP.jl")) as f:
        jl = f.read()
    for n in NAMES:
        assert re.search(r"ccall\(\(:" + n + r"\b", jl), n
    assert "function jaccard_csr(" in jl and "function graph_features(" in jl
    assert "jaccard_csr" in ss.__all__ and ss.jaccard_csr is not None


def test_entry_points_need_ss_init():
    """Without ss_init every entry point returns SS_ENODEV and writes nothing."""
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    lib = _lib.load()
    X = np.asfortranarray(np.random.default_rng(0).random((4, 3)))
    ptr = np.full(5, -7, np.int64)
    nnz = C.c_int64(-7)
    for suf, ft, dt in (("f32", C.c_float, np.float32), ("f64", C.c_double, np.float64)):
        F = np.asfortranarray(X, dtype=dt)
        rc = getattr(lib, f"ss_similarity_jaccard_csr_{suf}")(F.ctypes.data, 4, 4, None, 4, 4, 3, ft(0.5), 1,
                                                              ptr.ctypes.data, None, None, 0, C.byref(nnz), 0)
        assert rc == -4, (suf, rc)
        assert "ss_init" in lib.ss_last_error().decode()
        h = C.c_void_p()
        yp, yi = np.array([0, 1, 1, 2, 2], np.int64), np.array([0, 1], np.int32)
        rc = getattr(lib, f"ss_graph_create_features_{suf}")(0, 4, 2, 3, None, 1, F.ctypes.data, 4, yp.ctypes.data,
                                                             yi.ctypes.data, None, 0, ft(0.5), 1, 0, C.byref(h))
        assert rc == -4, (suf, rc)
        assert h.value is None
    assert nnz.value == -7 and (ptr == -7).all()
    with pytest.raises(ss.SimSpreadError) as e:
        ss.jaccard_csr(X, alpha=0.5)
    assert e.value.code == -4
    with pytest.raises(ss.SimSpreadError) as e:
        ss.DeviceGraph.from_features(None, X, np.eye(4, 2), alpha=0.5)
    assert e.value.code == -4


def test_python_mirror_rejects_wrong_dtypes_and_shapes_on_the_host():
    X = np.random.default_rng(1).random((5, 3))
    Y = np.eye(5, 2)
    with pytest.raises(TypeError):
        ss.jaccard_csr(X)                                            # alpha is required
    with pytest.raises(TypeError):
        ss.jaccard_csr(X, alpha=0.5, dtype=np.float16)
    with pytest.raises(TypeError):
        ss.jaccard_csr(X.astype(np.complex128), alpha=0.5)
    with pytest.raises(TypeError):
        ss.jaccard_csr(X.astype(bool), alpha=0.5)
    with pytest.raises(ValueError):
        ss.jaccard_csr(X[0], alpha=0.5)                              # a vector, not an (n, d) matrix
    with pytest.raises(ValueError):
        ss.jaccard_csr(X, X[:, :2], alpha=0.5)                       # different numbers of features
    with pytest.raises(TypeError):
        ss.DeviceGraph.from_features(None, X, Y, alpha=0.5, dtype=np.int32)
    with pytest.raises(ValueError):
        ss.DeviceGraph.from_features(X[:, :2], X, Y, alpha=0.5)
    with pytest.raises(ValueError):
        ss.DeviceGraph.from_features(None, X[None], Y, alpha=0.5)
    with pytest.raises(AssertionError):
        ss.DeviceGraph.from_features(None, X, np.eye(4, 2), alpha=0.5)   # labels of another number of sources
