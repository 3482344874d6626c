"""CPU-side checks of the inner-product similarity route (no GPU): the four entry points are declared, exported and
bound (ctypes and Julia), the Python mirror exists, the inputs of the GPU case matrix keep almost every pair outside
the error band of the cutoff (a condition on the inputs, not a tolerance), and the two host references agree where both
are exact."""
import os
import re

import numpy as np
import pytest

import simspread_jl_amd as ss
from simspread_jl_amd import _lib

import dot_ref as R

NAMES = {"ss_similarity_dot_csr_f32", "ss_similarity_dot_csr_f64",
         "ss_graph_create_vectors_f32", "ss_graph_create_vectors_f64"}
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_dot_csr_symbols_are_declared_exported_and_bound():
    assert NAMES <= set(_lib.header_symbols())
    assert NAMES <= set(_lib.SIGNATURES)
    lib = _lib.load()
    assert all(hasattr(lib, n) for n in NAMES)
    with open(os.path.join(ROOT, "julia", "SimSpreadHIP.jl")) as f:
        jl = f.read()
    for n in NAMES:
        assert re.search(r"ccall\(\(:" + n + r"\b", jl), n
    assert "function dot_csr(" in jl and "function graph_vectors(" in jl
    with open(os.path.join(ROOT, "julia", "SimSpreadDevice.jl")) as f:
        assert "function featurize_vectors(" in f.read()
    assert "dot_csr" in ss.__all__ and callable(ss.dot_csr)
    assert callable(ss.DeviceGraph.from_vectors)
    with open(os.path.join(ROOT, "include", "simspread_hip.h")) as f:
        h = f.read()
    assert re.search(r"SS_SIM_COSINE = 0, SS_SIM_TANIMOTO = 1, SS_SIM_DICE = 2", h)
    assert len(_lib.header_symbols()) == 117


def test_python_mirror_rejects_bad_arguments_on_the_host():
    X = np.zeros((4, 3))
    with pytest.raises(TypeError):
        ss.dot_csr(X)                                   # alpha is required
    with pytest.raises(ValueError):
        ss.dot_csr(X, metric="euclid", alpha=0.5)
    with pytest.raises(TypeError):
        ss.dot_csr(X, alpha=0.5, dtype=np.float16)
    with pytest.raises(ValueError):
        ss.dot_csr(X, np.zeros((2, 5)), alpha=0.5)
    with pytest.raises(ValueError):
        ss.DeviceGraph.from_vectors(None, X, np.eye(4, 2), alpha=0.5, metric="l2")


@pytest.mark.parametrize("n,d", R.CASES)
def test_case_matrix_inputs_stay_out_of_the_band(n, d):
    """For every case, metric and alpha of the GPU test at most 1 % of the pairs lie within band of alpha."""
    worst = 0.0
    for signed in (False, True):
        F, G = R.case_inputs(n, d, signed)
        for dt in (np.float32, np.float64):
            sums = (R.sums64(F, F, dt), R.sums64(F, G, dt))
            for metric in R.METRICS:
                for sym, sm in zip((True, False), sums):
                    s = R.rule(*sm, metric, np.float64, sym)
                    alphas = R.ALPHAS + (R.EXTRA_ALPHAS if (n, d) == R.EXTRA_ALPHA_CASE else ())
                    for alpha in alphas:
                        share = R.in_band_share(s, alpha, dt, d)
                        worst = max(worst, share)
                        assert share <= 0.01, (signed, dt.__name__, metric, sym, alpha, share)
    print(f"n={n} d={d}: largest in-band share {worst:.4%}")


def test_numpy_fp32_gram_is_far_inside_the_band():
    """The first step of the band's derivation: an fp32 Gram block in whatever order (numpy's here) differs from fp64 by
    at most gamma_d * sqrt(A B), gamma_d ~ d eps / 2 <= band / 8."""
    F, _ = R.case_inputs(300, 300, True)
    A = F.astype(np.float32)
    g32 = (A @ A.T).astype(np.float64)
    g64, a, _ = R.sums64(F, F, np.float32)
    rel = np.abs(g32 - g64) / np.maximum(np.sqrt(a[:, None] * a[None, :]), 1e-300)
    assert rel.max() <= R.band(np.float32, 300) / 8


@pytest.mark.parametrize("dt", [np.float32, np.float64])
@pytest.mark.parametrize("n,d", [(200, 9), (129, 300)])
def test_ref_exact_equals_ref_s64_rounded_where_the_quotient_is_exact(n, d, dt):
    X = R.integer_rows(n, d, seed=n + d)
    for metric in ("tanimoto", "dice"):          # rational in the sums: fp64 evaluates them to within half an fp64 ulp
        e = R.ref_exact(X, X, metric, dt, sym=True)
        s = R.ref_s64(X, X, metric, dt, sym=True)
        exact = (s * 1024 == np.round(s * 1024))                 # dyadic quotients: exact in both precisions
        assert exact.sum() > n                                   # the diagonal, the duplicates, the 0.5 pairs, the zeros
        assert np.array_equal(e[exact].astype(np.float64), s[exact])
        assert np.abs(e.astype(np.float64) - s).max() <= np.finfo(dt).eps
        assert (e == dt(0.5)).any(), metric
    c = R.ref_exact(X, X, "cosine", dt, sym=True)
    assert c[10, 11] == dt(0.5) and c[11, 10] == dt(0.5)         # (2,0,0,0) x (1,1,1,1): sqrt(4) * sqrt(4) is exact
    assert np.abs(c.astype(np.float64) - R.ref_s64(X, X, "cosine", dt, sym=True)).max() <= 2 * np.finfo(dt).eps
    # duplicates are exactly 1 under Tanimoto and Dice, the zero row is 1 with itself and 0 with the others
    t = R.ref_exact(X, X, "tanimoto", dt, sym=True)
    assert t[n - 1, 3] == 1 and t[n - 2, n - 1] == 1 and t[n // 2, n // 3] == 1
    assert t[7, 7] == 1 and t[7, 8] == 0 and t[8, 7] == 0
