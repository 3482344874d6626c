"""The neighbour-floor entry points of the real-valued producers (include/simspread_hip_neighbours_real.h) without a GPU:
the header declares exactly the sixteen names, the library exports them, the three descriptions of each signature -- C
header, ctypes table (_lib.REAL_NEIGHBOUR_SIGNATURES), Julia `ccall` (julia/SimSpreadNeighboursReal.jl, unexecuted like
the other Julia files) -- agree type class by type class, the four headers are disjoint and sum to 156, the Python
surface exists, and the host reference (tests/real_floor_ref.py) has the properties the device cases rely on."""
import inspect
import os
import re

import numpy as np

import dot_ref
import real_floor_ref as R
from simspread_jl_amd import _lib
from test_julia_binding import _c_class, _ctypes_class, _julia_ccalls

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = {f"{n}_{suf}" for suf in ("f32", "f64")
         for n in ("ss_similarity_jaccard_kth", "ss_similarity_jaccard_floor_csr", "ss_similarity_dot_kth",
                   "ss_similarity_dot_floor_csr", "ss_graph_create_features_floor", "ss_graph_create_vectors_floor",
                   "ss_queries_create_features_floor", "ss_queries_create_vectors_floor")}
DTYPES = (np.float32, np.float64)


def _header_signatures():
    with open(_lib.REAL_NEIGHBOURS_HEADER_PATH) as f:
        text = re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)
    text = re.sub(r"^\s*#.*$", "", text, flags=re.M)       # preprocessor lines
    sigs = {}
    for m in re.finditer(r"([A-Za-z_][\w\s\*]*?)\b(ss_[a-z0-9_]+)\s*\(([^;{]*?)\)\s*;", text):
        ret, name, args = m.group(1).strip(), m.group(2), m.group(3).strip()
        sigs[name] = (_c_class(ret, ret=True), [_c_class(a.strip()) for a in args.split(",")])
    return sigs


def test_every_real_neighbour_symbol_is_declared_exported_and_in_the_table():
    declared = _lib.real_neighbours_header_symbols()
    assert set(declared) == NAMES and len(declared) == 16
    assert sorted(_lib.REAL_NEIGHBOUR_SIGNATURES) == declared
    lib = _lib.load()
    assert not [s for s in declared if not hasattr(lib, s)]
    with open(_lib.HEADER_PATH) as f:
        main = f.read()
    assert '#include "simspread_hip_neighbours_real.h"' in main


def test_the_four_headers_are_disjoint_and_sum_to_156():
    headers = [_lib.header_symbols(), _lib.screening_header_symbols(), _lib.neighbours_header_symbols(),
               _lib.real_neighbours_header_symbols()]
    tables = [_lib.SIGNATURES, _lib.SCREENING_SIGNATURES, _lib.NEIGHBOUR_SIGNATURES, _lib.REAL_NEIGHBOUR_SIGNATURES]
    assert [len(h) for h in headers] == [117, 15, 8, 16]
    assert len(set().union(*headers)) == sum(len(h) for h in headers) == 156
    assert len(set().union(*tables)) == sum(len(t) for t in tables) == 156
    for h, t in zip(headers, tables):
        assert sorted(t) == h


def test_the_three_descriptions_of_every_signature_agree():
    header = _header_signatures()
    assert set(header) == NAMES
    for name, (args, res) in _lib.REAL_NEIGHBOUR_SIGNATURES.items():
        hret, hargs = header[name]
        assert _ctypes_class(res) == hret, name
        assert [_ctypes_class(a) for a in args] == hargs, name
    calls = _julia_ccalls(os.path.join(ROOT, "julia", "SimSpreadNeighboursReal.jl"))
    assert {c[0] for c in calls} == NAMES and len(calls) == 16
    for name, ret, args in calls:
        hret, hargs = header[name]
        assert ret == hret, (name, ret, hret)
        assert args == hargs, (name, args, hargs)


def test_floor_variants_differ_from_the_plain_entry_points_by_one_int_after_alpha():
    plain = {**_lib.SIGNATURES, **_lib.SCREENING_SIGNATURES}
    for stem in ("ss_similarity_jaccard{}_csr", "ss_similarity_dot{}_csr", "ss_graph_create_features{}",
                 "ss_graph_create_vectors{}", "ss_queries_create_features{}", "ss_queries_create_vectors{}"):
        for suf, ft in (("f32", "f32"), ("f64", "f64")):
            base, _ = plain[stem.format("") + "_" + suf]
            floor, _ = _lib.REAL_NEIGHBOUR_SIGNATURES[stem.format("_floor") + "_" + suf]
            at = [_ctypes_class(a) for a in base].index(ft) + 1          # alpha is the only float argument
            assert [_ctypes_class(a) for a in floor] == ([_ctypes_class(a) for a in base[:at]] + ["i32"]
                                                         + [_ctypes_class(a) for a in base[at:]])


def test_the_python_mirror_exposes_the_floor():
    import simspread_jl_amd as ss
    for name in ("jaccard_kth", "dot_kth"):
        assert name in ss.__all__ and callable(getattr(ss, name))
        assert inspect.signature(getattr(ss, name)).parameters["k"].default is None
    assert inspect.signature(ss.dot_kth).parameters["metric"].default == "cosine"
    assert list(inspect.signature(ss.jaccard_kth).parameters) == ["Fa", "Fb", "k", "dtype"]
    assert list(inspect.signature(ss.dot_kth).parameters) == ["Fa", "Fb", "metric", "k", "dtype"]
    for fn in (ss.jaccard_csr, ss.dot_csr, ss.DeviceGraph.from_features, ss.DeviceGraph.from_vectors,
               ss.DeviceQueries.from_features, ss.DeviceQueries.from_vectors):
        assert inspect.signature(fn).parameters["min_neighbours"].default == 0, fn


# ------------------------------------------------------------------------------------------ the reference itself
def _check_rule_properties(s, k, short_rows):
    """What the rule promises, on a dense s: short rows keep all their positives, every other row keeps exactly the
    positives >= tau_i with fewer than k above tau_i, and alpha above every similarity is the pure k-nearest rule."""
    tau, npos = R.ref_kth(s, k), R.positives(s)
    knn = R.ref_floor(s, np.inf, k, True)
    deg = np.diff(knn.indptr)
    short = np.nonzero(npos < k)[0]
    assert len(short) == short_rows and (tau[short] == 0).all() and np.array_equal(deg[short], npos[short])
    full = np.nonzero(npos >= k)[0]
    assert (tau[full] > 0).all() and (deg[full] >= k).all()
    for i in full:
        assert deg[i] == ((s[i] > 0) & (s[i] >= tau[i])).sum() and (s[i] > tau[i]).sum() < k
    R.assert_csr_equal(R.ref_floor(s, 2.0, k, True), knn)
    R.assert_csr_equal(R.ref_floor(s, 0.7, 0, True), R.ref_cut(s, 0.7, True))
    return knn


def test_integer_rows_have_the_properties_the_dot_cases_rely_on():
    X = R.integer_sources()
    for dt in DTYPES:
        for metric in dot_ref.METRICS:
            s = R.dot_s(X, None, metric, dt)
            assert (np.diag(s) == 1).all() and 0.45 < (s < 0).mean() < 0.52        # about half are negative
            knn = _check_rule_properties(s, 5, short_rows=1)                         # the zero row sees itself only
            assert len(R.tied_rows(s, 5)) == 6 and 17 <= len(R.tied_rows(s, 64)) <= 26
            d = knn.toarray() != 0
            assert (d != d.T).any()                                                   # not symmetric
            assert (knn.data > 0).all()                                               # negatives never count among the k
            assert len(R.gained_rows(s, 0.7, 5)) == 299                              # all but the zero row
            assert (R.ref_floor(s, -0.5, 5, True).toarray() < 0).any()               # they survive through alpha only
        gained = len(R.gained_rows(R.dot_s(X, None, "cosine", dt), 0.3, 5))
        assert 0 < gained < 299                                                       # both kinds of row at alpha = 0.3


def test_feature_rows_have_the_properties_the_jaccard_cases_rely_on():
    X = R.feature_rows()
    for dt in DTYPES:
        s = R.jaccard_s(X, None, dt)
        knn = _check_rule_properties(s, 5, short_rows=3)              # the three zero rows see one another only
        assert set(np.nonzero(R.positives(s) < 5)[0]) == {0, 5, 299}
        assert len(R.tied_rows(s, 5)) == 44 and len(R.tied_rows(s, 64)) == 91
        assert (np.diff(knn.indptr) > 5).any()
        _check_rule_properties(s, 64, short_rows=3)
        gained = R.gained_rows(s, 0.9, 5)
        assert len(gained) == 241 and s.shape[0] - len(gained) == 59
        # the queries: some have no source at alpha = 0.9, and the floor serves all of them but the all-zero one
        sx = R.jaccard_s(R.feature_queries(), X, dt)
        plain_deg = np.diff(R.ref_cut(sx, 0.9, True).indptr)
        floor_deg = np.diff(R.ref_floor(sx, 0.9, 5, True).indptr)
        assert ((plain_deg == 0) & (R.positives(sx) > 0)).any()
        assert (floor_deg >= np.minimum(5, R.positives(sx))).all()


def test_d_zero_and_k_at_the_row_count():
    """d == 0 gives s = 1 everywhere, so tau = 1 when nb >= k and +0 otherwise."""
    for dt in DTYPES:
        s = R.jaccard_s(np.zeros((4, 0)), np.zeros((7, 0)), dt)
        assert (s == 1).all()
        assert (R.ref_kth(s, 7) == 1).all() and (R.ref_kth(s, 8) == 0).all()
        assert (R.dot_s(np.zeros((4, 0)), np.zeros((7, 0)), "cosine", dt) == 1).all()
