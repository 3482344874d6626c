"""The clustering entry points (include/simspread_hip_clusters.h) without a GPU: the header declares exactly the nine
names, disjoint from the other four headers (165 in all), the library exports them, the three descriptions of each
signature -- C header, ctypes table (_lib.CLUSTER_SIGNATURES), Julia `ccall` (julia/SimSpreadClusters.jl, unexecuted like
the other Julia files) -- agree type class by type class, the Python surface exists, the host reference
(tests/cluster_ref.py) has the properties of the rule on the graphs the device cases use, and without a device every new
call raises SimSpreadError."""
import inspect
import os
import re

import numpy as np
import pytest
import scipy.sparse as sp

import cluster_ref as R
from simspread_jl_amd import _lib
from test_julia_binding import _c_class, _ctypes_class, _julia_ccalls

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ({"ss_cluster_butina_csr", "ss_cluster_folds", "ss_cluster_cross_edges"}
         | {f"ss_cluster_butina_{kind}_{suf}" for kind in ("fingerprint", "features", "vectors")
            for suf in ("f32", "f64")})


def _header_signatures():
    with open(_lib.CLUSTERS_HEADER_PATH) as f:
        text = re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)
    text = re.sub(r"^\s*#.*$", "", text, flags=re.M)       # preprocessor lines
    sigs = {}
    for m in re.finditer(r"([A-Za-z_][\w\s\*]*?)\b(ss_[a-z0-9_]+)\s*\(([^;{]*?)\)\s*;", text):
        ret, name, args = m.group(1).strip(), m.group(2), m.group(3).strip()
        sigs[name] = (_c_class(ret, ret=True), [_c_class(a.strip()) for a in args.split(",")])
    return sigs


def test_every_cluster_symbol_is_declared_exported_and_in_the_table():
    declared = _lib.clusters_header_symbols()
    assert set(declared) == NAMES and len(declared) == 9
    assert sorted(_lib.CLUSTER_SIGNATURES) == declared
    lib = _lib.load()
    assert not [s for s in declared if not hasattr(lib, s)]
    with open(_lib.HEADER_PATH) as f:
        main = f.read()
    assert '#include "simspread_hip_clusters.h"' in main
    assert re.search(r"SS_EINTERNAL\s*=\s*-6\b", main) and _lib._ERR_NAMES[-6] == "SS_EINTERNAL"


def test_the_five_headers_are_disjoint_and_sum_to_165():
    headers = [_lib.header_symbols(), _lib.screening_header_symbols(), _lib.neighbours_header_symbols(),
               _lib.real_neighbours_header_symbols(), _lib.clusters_header_symbols()]
    tables = [_lib.SIGNATURES, _lib.SCREENING_SIGNATURES, _lib.NEIGHBOUR_SIGNATURES, _lib.REAL_NEIGHBOUR_SIGNATURES,
              _lib.CLUSTER_SIGNATURES]
    assert [len(h) for h in headers] == [117, 15, 8, 16, 9]
    assert len(set().union(*headers)) == sum(len(h) for h in headers) == 165
    assert len(set().union(*tables)) == sum(len(t) for t in tables) == 165
    for h, t in zip(headers, tables):
        assert sorted(t) == h


def test_the_three_descriptions_of_every_signature_agree():
    header = _header_signatures()
    assert set(header) == NAMES
    for name, (args, res) in _lib.CLUSTER_SIGNATURES.items():
        hret, hargs = header[name]
        assert _ctypes_class(res) == hret, name
        assert [_ctypes_class(a) for a in args] == hargs, name
    calls = _julia_ccalls(os.path.join(ROOT, "julia", "SimSpreadClusters.jl"))
    assert {c[0] for c in calls} == NAMES and len(calls) == 9
    for name, ret, args in calls:
        hret, hargs = header[name]
        assert ret == hret, (name, ret, hret)
        assert args == hargs, (name, args, hargs)


def test_the_python_mirror_exposes_the_clustering():
    import simspread_jl_amd as ss
    for name in ("butina_clusters", "cluster_folds", "cross_fold_edges", "split_clusters", "ButinaClusters"):
        assert name in ss.__all__ and callable(getattr(ss, name))
    p = inspect.signature(ss.butina_clusters).parameters
    assert list(p) == ["X", "fingerprints", "features", "vectors", "metric", "cutoff", "dtype", "index_base"]
    assert p["X"].default is None and p["X"].kind is inspect.Parameter.POSITIONAL_OR_KEYWORD
    assert all(p[k].kind is inspect.Parameter.KEYWORD_ONLY for k in list(p)[1:])
    assert p["metric"].default == "cosine" and p["cutoff"].default is None and p["index_base"].default == 0
    assert p["dtype"].default is np.float32
    assert list(inspect.signature(ss.cluster_folds).parameters) == ["label", "nfolds"]
    assert list(inspect.signature(ss.cross_fold_edges).parameters)[:3] == ["X", "fold_of_source", "nfolds"]
    assert list(inspect.signature(ss.split_clusters).parameters) == ["y", "label", "k"]
    r = ss.ButinaClusters(np.zeros(3, np.int32), np.zeros(3, np.int32), np.array([3], np.int32), 1)
    assert (r.nclusters, r.rounds) == (1, 1) and r.centre.shape == r.label.shape == (3,)
    # bad requests are refused before the library is asked for anything
    with pytest.raises(TypeError):
        ss.butina_clusters()
    with pytest.raises(TypeError):
        ss.butina_clusters(sp.eye(3, format="csr"), fingerprints=np.zeros((3, 1), np.uint64), cutoff=0.5)


# ------------------------------------------------------------------------------------------ the reference itself
@pytest.mark.parametrize("name", sorted(R.graphs()))
def test_reference_has_the_properties_of_the_rule(name):
    A = R.neighbours(R.graphs()[name])
    centre, label, size = R.reference(name)
    R.check_properties(A, centre, label, size)


def test_reference_on_graphs_whose_answer_is_known():
    n = 300
    centre, label, size = R.reference("path")
    # interior nodes (degree 2) go first, in index order, and degrees are not re-counted: 1 takes 0 and 2, then 3 is the
    # next unassigned one and takes 4 only, 5 takes 6, ...: every decision waits for the one before it (the slow chain)
    assert np.array_equal(np.nonzero(centre == np.arange(n))[0], np.arange(1, 300, 2))
    assert np.array_equal(size, [3] + [2] * 148 + [1]) and label[299] == 149
    centre, label, size = R.reference("ring_lattice")          # all degrees equal: the index decides everything
    assert np.array_equal(np.nonzero(centre == np.arange(n))[0], np.arange(0, 300, 3))
    assert np.array_equal(size, [5] + [3] * 98 + [1]) and np.array_equal(centre[[298, 299, 1, 2, 297]], [0, 0, 0, 0, 297])
    assert np.array_equal(label, centre // 3)
    centre, label, size = R.reference("k70")
    assert (centre == 0).all() and (label == 0).all() and np.array_equal(size, [70])
    centre, label, size = R.reference("empty65")
    assert np.array_equal(centre, np.arange(65)) and np.array_equal(label, np.arange(65)) and (size == 1).all()
    centre, label, size = R.reference("hub")
    assert (centre == 17).all() and np.array_equal(size, [600])
    # the hub is far above a wave's width and the p = 0.3 graph has rows on both sides of it
    deg = R.neighbours(R.graphs()["random_p0.3"]).sum(axis=1)
    assert (deg > 64).any() and (deg <= 64).any()
    assert R.neighbours(R.graphs()["hub"]).sum(axis=1).max() == 599
    k = R.graphs()["directed_knn"]
    assert (k != k.T).any()


def test_the_noisy_parts_describe_the_same_graph():
    A = R.graphs()["random_p0.05"]
    ptr, idx = R.csr_parts(A, index_base=1, noise_seed=3)
    n = A.shape[0]
    assert ptr[0] == 1 and len(idx) == ptr[-1] - 1 > A.sum() + n
    B = np.zeros_like(A)
    rows = np.repeat(np.arange(n), np.diff(ptr))
    B[rows, idx - 1] = True
    assert B.diagonal().all() and np.array_equal(R.neighbours(B), R.neighbours(A))
    assert any(len(set(idx[ptr[i] - 1:ptr[i + 1] - 1])) < ptr[i + 1] - ptr[i] for i in range(n))     # duplicates


def test_fold_and_cross_edge_references():
    label = np.array([0, 0, 0, 1, 1, 2, 2, 3, 4], np.int32)               # sizes 3, 2, 2, 1, 1
    fold = R.ref_folds(label, 2)
    # 0 -> fold 0 (3); 1 -> fold 1 (2); 2 -> fold 1 (4); 3 -> fold 0 (4); 4 -> tie, fold 0
    assert np.array_equal(fold, [0, 0, 0, 1, 1, 1, 1, 0, 0])
    assert np.array_equal(R.ref_folds(label, 1), np.zeros(9))
    for name in ("random_p0.05", "hub", "path"):
        _, lab, size = R.reference(name)
        for nf in (2, 5, 7):
            f = R.ref_folds(lab, nf)
            assert all(len(set(f[lab == c])) == 1 for c in range(len(size)))
            load = np.bincount(f, minlength=nf)
            assert load.max() - load.min() <= size.max()
    A = R.graphs()["path"]
    ptr, idx = R.csr_parts(A)
    fold = (np.arange(300) // 100).astype(np.int32)
    assert np.array_equal(R.ref_cross_edges(ptr, idx, fold, 3), [1, 2, 1])
    assert np.array_equal(R.ref_cross_edges(ptr, idx, np.zeros(300, np.int32), 1), [0])


def test_split_clusters_groups_names_like_split():
    import simspread_jl_amd as ss
    assert inspect.signature(ss.split_clusters).return_annotation == inspect.signature(ss.split).return_annotation


# ------------------------------------------------------------------------------------------ no device, no answer
def _has_gpu():
    try:
        import torch
        return torch.cuda.is_available()
    except Exception:
        return False


@pytest.mark.skipif(_has_gpu(), reason="the refusal without a device can only be seen without one")
def test_without_a_device_every_new_call_raises():
    import simspread_jl_amd as ss
    X = sp.csr_matrix(R.graphs()["k70"])
    F = np.random.default_rng(0).random((8, 3))
    calls = [lambda: ss.butina_clusters(X),
             lambda: ss.butina_clusters(fingerprints=ss.pack_fingerprints(F > 0.5), cutoff=0.5),
             lambda: ss.butina_clusters(features=F, cutoff=0.5),
             lambda: ss.butina_clusters(vectors=F, metric="dice", cutoff=0.5),
             lambda: ss.cluster_folds(np.zeros(4, np.int32), 2),
             lambda: ss.cross_fold_edges(X, np.zeros(70, np.int32), 1),
             lambda: ss.split_clusters(ss.NamedMatrix(np.zeros((2, 2)), ["a", "b"], ["x", "y"]), [0, 1], 2)]
    for call in calls:
        with pytest.raises(ss.SimSpreadError):
            call()
