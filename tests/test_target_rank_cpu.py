"""The per-target ranking metrics (include/simspread_hip_target_rank.h) without a GPU: the counts-based two-pass
algorithm (tests/target_rank_ref.py, the numpy restatement of what the device does) equals rank_ref.ref_row of every
column for every block split and block order; the header declares exactly the twenty names, the library exports them,
and the three descriptions of each signature -- C header, ctypes table (_lib.TARGET_RANK_SIGNATURES), Julia `ccall`
(julia/SimSpreadTargetRank.jl, unexecuted like the other Julia files) -- agree type class by type class; without a
device every entry point raises SimSpreadError."""
import os
import re

import numpy as np
import pytest

import target_rank_ref as R
from rank_ref import assert_rows_close
from simspread_jl_amd import _lib
from test_julia_binding import _c_class, _ctypes_class, _julia_ccalls

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ({"ss_target_rank_" + n for n in ("destroy", "reset", "info", "seal", "merge", "export_counts", "import_counts",
                                          "metrics")}
         | {f"ss_target_rank_{n}_{suf}" for n in ("create", "add_rows", "add_loo", "add_kfold", "export_positives",
                                                  "import_positives") for suf in ("f32", "f64")})
NT = 40
RTOL, ATOL = 1e-9, 1e-12          # the band of the per-row metrics against the literal oracle


def _splits(n):
    """Row cuts: one block, three uneven blocks, seven uneven blocks (as many as n allows)."""
    three = sorted({0, n // 3, (2 * n) // 3 + (n > 3), n})
    seven = sorted({0, n} | {min(n, c) for c in (1, 3, n // 4 + 2, n // 2, n // 2 + 1, n - 2) if c > 0})
    return [[0, n], three, seven]


def _run(Y, S, cuts, dtype, reverse):
    h = R.RefTargetRank(Y.shape[1], dtype)
    blocks = list(zip(cuts[:-1], cuts[1:]))
    for a, b in blocks:
        h.add_rows(Y[a:b], S[a:b], a)
    h.seal()
    for a, b in (blocks[::-1] if reverse else blocks):
        h.add_rows(Y[a:b], S[a:b], a)
    return h


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("n, L", [(2, 1), (37, 1), (37, 5), (37, 20), (129, 5), (129, 64), (300, 20), (300, 64)])
def test_counts_algorithm_equals_the_definition_for_every_split_and_order(dtype, n, L):
    Y, S = R.case_matrix(n, NT, L, dtype)
    want = R.ref_targets(Y, S.astype(np.float64), 20.0, L)
    first = None
    for cuts in _splits(n):
        for reverse in (False, True):
            h = _run(Y, S, cuts, dtype, reverse)
            got = h.metrics(20.0, L)
            assert_rows_close(got, want, RTOL, ATOL, f"n={n} L={L} cuts={cuts} reverse={reverse}")
            np.testing.assert_array_equal(got[:, 4:], want[:, 4:])            # recall@L, precision@L: exact
            table = (h.export_positives(), h.export_counts())
            if first is None:
                first = table
            for a, b in zip(first[0] + first[1], table[0] + table[1]):        # one table whatever the blocks
                np.testing.assert_array_equal(np.asarray(a), np.asarray(b))


def test_fp64_scores_below_fp32_resolution_are_not_ties():
    n = 50
    rng = np.random.default_rng(5)
    S = 0.5 + np.arange(n, dtype=np.float64)[:, None] * 1e-12 * np.ones((1, 3))
    Y = (rng.random((n, 3)) < 0.4).astype(np.uint8)
    assert np.unique(S[:, 0].astype(np.float32)).size == 1
    h = _run(Y, S, [0, 17, n], np.float64, True)
    assert_rows_close(h.metrics(20.0, 5), R.ref_targets(Y, S, 20.0, 5), RTOL, ATOL, "fp64")
    counts, _ = h.export_counts()
    P = int(Y.sum())
    tie = sum(int(h._views(t)[3].sum()) for t in range(3))
    assert tie == 0 and counts[:3 * (P + 3)].sum() == (Y == 0).sum()


def test_a_second_pass_that_differs_is_noticed():
    Y, S = R.case_matrix(37, NT, 5, np.float64)
    h = R.RefTargetRank(NT, np.float64).add_rows(Y, S).seal()
    r, t = np.argwhere(Y)[3]
    S2 = S.copy()
    S2[r, t] = np.nextafter(S2[r, t], 2.0)
    with pytest.raises(AssertionError, match=f"row {r}, target {t}"):
        h.add_rows(Y, S2)


# ------------------------------------------------------------------------------------------ the three descriptions
def _header_signatures():
    with open(_lib.TARGET_RANK_HEADER_PATH) as f:
        text = re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)
    text = re.sub(r"^\s*#.*$", "", text, flags=re.M)       # preprocessor lines
    text = re.sub(r"typedef[^;]*;", "", text)
    sigs = {}
    for m in re.finditer(r"([A-Za-z_][\w\s\*]*?)\b(ss_[a-z0-9_]+)\s*\(([^;{]*?)\)\s*;", text):
        ret, name, args = m.group(1).strip(), m.group(2), m.group(3).strip()
        sigs[name] = (_c_class(ret, ret=True), [_c_class(a.strip()) for a in args.split(",")])
    return sigs


def test_every_target_rank_symbol_is_declared_exported_and_in_the_table():
    declared = _lib.target_rank_header_symbols()
    assert set(declared) == NAMES and len(declared) == 20
    assert sorted(_lib.TARGET_RANK_SIGNATURES) == declared
    lib = _lib.load()
    assert not [s for s in declared if not hasattr(lib, s)]
    with open(_lib.HEADER_PATH) as f:
        assert '#include "simspread_hip_target_rank.h"' in f.read()
    others = (set(_lib.SIGNATURES) | set(_lib.SCREENING_SIGNATURES) | set(_lib.NEIGHBOUR_SIGNATURES)
              | set(_lib.REAL_NEIGHBOUR_SIGNATURES) | set(_lib.CLUSTER_SIGNATURES))
    assert not others & NAMES and len(others) + len(NAMES) == 185
    assert sorted(_lib.SIGNATURES) == _lib.header_symbols()          # the main table stays the main header's


def test_the_three_descriptions_of_every_signature_agree():
    header = _header_signatures()
    assert set(header) == NAMES
    for name, (args, res) in _lib.TARGET_RANK_SIGNATURES.items():
        hret, hargs = header[name]
        assert _ctypes_class(res) == hret, name
        assert [_ctypes_class(a) for a in args] == hargs, name
    calls = _julia_ccalls(os.path.join(ROOT, "julia", "SimSpreadTargetRank.jl"))
    assert {c[0] for c in calls} == NAMES and len(calls) == 20
    for name, ret, args in calls:
        hret, hargs = header[name]
        assert ret == hret, (name, ret, hret)
        assert args == hargs, (name, args, hargs)


def test_the_python_surface_exists():
    import simspread_jl_amd as ss
    for name in ("TargetRank", "target_rank", "target_rank_positives"):
        assert name in ss.__all__ and callable(getattr(ss, name))
    assert ss.TARGET_RANK_FIELDS == ss.RANK_ROWS_FIELDS
    for m in ("add_rows", "add_loo", "add_kfold", "seal", "merge", "export_positives", "import_positives",
              "export_counts", "import_counts", "info", "metrics", "close"):
        assert callable(getattr(ss.TargetRank, m))
    for m in ("evaluate_loo_targets", "evaluate_kfold_targets"):
        assert callable(getattr(ss.DeviceGraph, m))


# ------------------------------------------------------------------------------------------ no device, no answer
def _has_gpu():
    try:
        import torch
        return torch.cuda.is_available()
    except Exception:
        return False


@pytest.mark.skipif(_has_gpu(), reason="the refusal without a device can only be seen without one")
def test_without_a_device_every_entry_point_raises():
    import simspread_jl_amd as ss
    with pytest.raises(ss.SimSpreadError):
        ss.TargetRank(4, np.float32)
    with pytest.raises(ss.SimSpreadError):
        ss.TargetRank(4, np.float64)
    lib = _lib.load()
    buf = np.zeros(64, np.int64)
    p, h = buf.ctypes.data, None                # no handle can exist without a device: NULL is refused, not followed
    calls = {"reset": (h,), "info": (h, p), "seal": (h,), "merge": (h, h), "export_counts": (h, p, p, 0),
             "import_counts": (h, p, 0, 0, 0), "metrics": (h, 20.0, 1, p, 0)}
    for suf in ("f32", "f64"):
        calls[f"create_{suf}"] = (4, p)
        calls[f"add_rows_{suf}"] = (h, p, p, 0, p, 1, 1, 1, 0, 0)
        calls[f"add_loo_{suf}"] = (h, h, 0, 1, 0, 0)
        calls[f"add_kfold_{suf}"] = (h, h, p, 1, 0, 1, 0, 0, 0)
        calls[f"export_positives_{suf}"] = (h, p, p, p, p, 0)
        calls[f"import_positives_{suf}"] = (h, p, p, p, 0, 0, 0)
    for name, args in calls.items():
        with pytest.raises(ss.SimSpreadError):
            _lib.check(getattr(lib, "ss_target_rank_" + name)(*args))
