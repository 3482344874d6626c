"""The neighbour-floor entry points (include/simspread_hip_neighbours.h) without a GPU: the header declares exactly the
eight names, the library exports them, the three descriptions of each signature -- C header, ctypes table
(_lib.NEIGHBOUR_SIGNATURES), Julia `ccall` (julia/SimSpreadNeighbours.jl) -- agree type class by type class, the Python
surface exists, and the host reference of the rule (tests/neighbour_ref.py) does what the rule says on the properties
the device tests rely on."""
import inspect
import os
import re

import numpy as np

import neighbour_ref as R
from simspread_jl_amd import _lib
from test_julia_binding import _c_class, _ctypes_class, _julia_ccalls

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = {f"{n}_{suf}" for suf in ("f32", "f64")
         for n in ("ss_similarity_tanimoto_kth", "ss_similarity_tanimoto_floor_csr", "ss_graph_create_fingerprint_floor",
                   "ss_queries_create_fingerprint_floor")}


def _header_signatures():
    with open(_lib.NEIGHBOURS_HEADER_PATH) as f:
        text = re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)
    text = re.sub(r"^\s*#.*$", "", text, flags=re.M)       # preprocessor lines
    sigs = {}
    for m in re.finditer(r"([A-Za-z_][\w\s\*]*?)\b(ss_[a-z0-9_]+)\s*\(([^;{]*?)\)\s*;", text):
        ret, name, args = m.group(1).strip(), m.group(2), m.group(3).strip()
        sigs[name] = (_c_class(ret, ret=True), [_c_class(a.strip()) for a in args.split(",")])
    return sigs


def test_every_neighbour_symbol_is_declared_exported_and_in_the_table():
    declared = _lib.neighbours_header_symbols()
    assert set(declared) == NAMES and len(declared) == 8
    assert sorted(_lib.NEIGHBOUR_SIGNATURES) == declared
    assert not set(declared) & set(_lib.SIGNATURES)
    assert not set(declared) & set(_lib.SCREENING_SIGNATURES)
    assert not set(declared) & set(_lib.header_symbols()) and not set(declared) & set(_lib.screening_header_symbols())
    lib = _lib.load()
    assert not [s for s in declared if not hasattr(lib, s)]
    assert len(_lib.header_symbols()) + len(_lib.screening_header_symbols()) + len(declared) == 140
    with open(_lib.HEADER_PATH) as f:
        main = f.read()
    assert '#include "simspread_hip_neighbours.h"' in main


def test_the_three_descriptions_of_every_signature_agree():
    header = _header_signatures()
    assert set(header) == NAMES
    for name, (args, res) in _lib.NEIGHBOUR_SIGNATURES.items():
        hret, hargs = header[name]
        assert _ctypes_class(res) == hret, name
        assert [_ctypes_class(a) for a in args] == hargs, name
    calls = _julia_ccalls(os.path.join(ROOT, "julia", "SimSpreadNeighbours.jl"))
    assert {c[0] for c in calls} == NAMES and len(calls) == 8
    for name, ret, args in calls:
        hret, hargs = header[name]
        assert ret == hret, (name, ret, hret)
        assert args == hargs, (name, args, hargs)


def test_the_python_mirror_exposes_the_floor():
    import simspread_jl_amd as ss
    assert "tanimoto_kth" in ss.__all__ and callable(ss.tanimoto_kth)
    assert inspect.signature(ss.tanimoto_kth).parameters["k"].default is None
    for fn in (ss.tanimoto_csr, ss.DeviceGraph.from_fingerprints, ss.DeviceQueries.from_fingerprints):
        assert inspect.signature(fn).parameters["min_neighbours"].default == 0, fn


# ------------------------------------------------------------------------------------------ the reference itself
def _case(dt):
    import simspread_jl_amd as ss
    return R.ref_similarity(ss.pack_fingerprints(R.case_bits()), None, dt)


def test_reference_k0_is_the_plain_cut():
    for dt in (np.float32, np.float64):
        s = _case(dt)
        for alpha in (0.0, 0.7, np.inf):
            for weighted in (True, False):
                want = (s >= dt(alpha)) & ((s if weighted else np.ones_like(s)) != 0)
                got = R.ref_floor(s, alpha, 0, weighted)
                assert np.array_equal(got.toarray() != 0, want)
                R.assert_csr_equal(got, R.ref_cut(s, alpha, weighted))


def test_reference_keeps_ties_and_short_rows_and_reaches_every_branch():
    """n = 300, d = 167, k = 5: the properties the device case matrix is chosen for."""
    k = 5
    for dt in (np.float32, np.float64):
        s = _case(dt)
        tau = R.ref_kth(s, k)
        npos = R.positives(s)
        knn = R.ref_floor(s, np.inf, k, True)
        deg = np.diff(knn.indptr)
        # fewer than k positives: the all-zero rows see one another only (s = 1 three times) and keep all of them
        short = np.nonzero(npos < k)[0]
        assert set(short) >= {0, 5, 299} and (tau[short] == 0).all()
        assert np.array_equal(deg[short], npos[short])
        # every other row keeps at least k, exactly the entries >= tau_i, ties included
        full = np.nonzero(npos >= k)[0]
        assert (deg[full] >= k).all()
        for i in full:
            assert deg[i] == (s[i] >= tau[i]).sum() and (s[i] > tau[i]).sum() < k
        tied = [i for i in full if (s[i] == tau[i]).sum() > 1]
        assert len(tied) > 10 and (deg > k).any()
        # not symmetric
        d = knn.toarray() != 0
        assert (d != d.T).any()
        # alpha = 0.7: rows the floor adds to and rows it leaves alone
        plain, floor = R.ref_cut(s, 0.7, True), R.ref_floor(s, 0.7, k, True)
        more = np.diff(floor.indptr) > np.diff(plain.indptr)
        assert more.any() and (~more).any()
        assert ((floor.toarray() != 0) >= (plain.toarray() != 0)).all()
        # a cutoff above every similarity is the pure k-nearest rule
        R.assert_csr_equal(R.ref_floor(s, 2.0, k, True), knn)
