"""Butina clusters, cluster folds and cross-fold edges on the device (include/simspread_hip_clusters.h).  Everything is
integers, so every comparison with the host reference (tests/cluster_ref.py, the sequential rule) is exact equality.

The shapes are the smallest at which each piece can go wrong: n = 257 is no multiple of a wave, p = 0.3 puts rows on both
sides of the lane-per-row / wave-per-row switch (degree 64), the hub row of the n = 600 graph is far above it next to
short rows, the path is the slow chain (every decision waits for the one before it), the ring lattice has all degrees
equal so that the index tie-break decides everything.  tests/test_cluster_cpu.py checks that the reference has the
properties of the rule on these graphs."""
import ctypes as C
import functools
import os

import numpy as np
import pytest
import scipy.sparse as sp

import cluster_ref as R
import dot_ref
import neighbour_ref
import real_floor_ref
import simspread_jl_amd as ss
from simspread_jl_amd import _lib

pytestmark = pytest.mark.gpu

DTYPES = [np.float32, np.float64]
EINVAL = -1
NAMES = sorted(R.graphs())


def assert_result(res, want, n):
    centre, label, size = want
    for got, ref, what in ((res.centre, centre, "centre"), (res.label, label, "label"), (res.size, size, "size")):
        got = got.cpu().numpy() if type(got).__module__.startswith("torch") else got
        assert got.dtype == np.int32 and np.array_equal(got, ref), what
    assert res.nclusters == len(size)
    assert 1 <= res.rounds <= n


# ------------------------------------------------------------------------------------------------ 1. the CSR form
@pytest.mark.parametrize("name", NAMES)
def test_every_graph_matches_the_sequential_rule(name):
    ss.init(0)
    A = R.graphs()[name]
    res = ss.butina_clusters(sp.csr_matrix(A))
    assert_result(res, R.reference(name), A.shape[0])
    assert ss.path_last() == ["butina_csr"]
    again = ss.butina_clusters(sp.csr_matrix(A))                                 # bitwise repeatable
    assert np.array_equal(again.centre, res.centre) and np.array_equal(again.label, res.label)
    print(f"{name}: n = {A.shape[0]}, clusters = {res.nclusters}, rounds = {res.rounds}")


def test_both_row_mappings_are_exercised():
    """Rows on both sides of a wave's width in one graph, and the rule's answer for both kinds of row."""
    for name in ("random_p0.3", "hub"):
        deg = R.neighbours(R.graphs()[name]).sum(axis=1)
        assert (deg > 64).any() and (deg <= 64).any()
    deg = R.neighbours(R.graphs()["random_p0.3"]).sum(axis=1)
    centre = R.reference("random_p0.3")[0]
    members = centre != np.arange(len(centre))
    assert (members & (deg > 64)).any() and (members & (deg <= 64)).any()        # both assign kernels give members
    assert (~members & (deg > 64)).any()                                         # and a long row turns centre


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
@pytest.mark.parametrize("name", ["random_p0.05", "random_p0.3", "hub", "directed_knn"])
def test_diagonal_duplicates_and_index_base_one(name, device):
    """The same graphs with every row's diagonal entry and duplicates added, rows unsorted, 1-based, from host and from
    device memory: the clusters are the clean graph's."""
    ss.init(0)
    A = R.graphs()[name]
    ptr, idx = R.csr_parts(A, index_base=1, noise_seed=7)
    if device:
        import torch
        X = (torch.from_numpy(ptr).cuda(), torch.from_numpy(idx).cuda())
    else:
        X = (ptr, idx)
    res = ss.butina_clusters(X, index_base=1)
    if device:
        assert res.centre.is_cuda and res.label.is_cuda and res.size.is_cuda
    assert_result(res, R.reference(name), A.shape[0])


def test_the_path_is_slow_but_ends_within_n_rounds():
    ss.init(0)
    res = ss.butina_clusters(sp.csr_matrix(R.graphs()["path"]))
    assert_result(res, R.reference("path"), 300)
    assert 2 < res.rounds <= 300


def test_degenerate_sizes():
    ss.init(0)
    lib = _lib.lib()
    nc, rounds = C.c_int64(-7), C.c_int64(-7)
    rc = lib.ss_cluster_butina_csr(0, None, None, 0, None, None, None, C.byref(nc), C.byref(rounds), _lib.SS_MEM_HOST)
    assert rc == 0 and nc.value == 0 and rounds.value == 0
    res = ss.butina_clusters((np.zeros(1, np.int64), np.zeros(0, np.int32)))
    assert res.nclusters == 0 and res.centre.shape == (0,) and res.label.shape == (0,)
    res = ss.butina_clusters(sp.csr_matrix((1, 1)))
    assert_result(res, (np.zeros(1, np.int32), np.zeros(1, np.int32), np.ones(1, np.int32)), 1)
    res = ss.butina_clusters(sp.csr_matrix(np.ones((1, 1))))                     # a lone diagonal entry
    assert_result(res, (np.zeros(1, np.int32), np.zeros(1, np.int32), np.ones(1, np.int32)), 1)
    # size and rounds are optional
    ptr, idx = R.csr_parts(R.graphs()["k70"])
    centre, label = np.full(70, -7, np.int32), np.full(70, -7, np.int32)
    rc = lib.ss_cluster_butina_csr(70, ptr.ctypes.data, idx.ctypes.data, 0, centre.ctypes.data, label.ctypes.data, None,
                                   C.byref(nc), None, _lib.SS_MEM_HOST)
    assert rc == 0 and nc.value == 1 and (centre == 0).all() and (label == 0).all()


def _bad_patterns():
    A = R.graphs()["random_p0.05"]
    n = A.shape[0]
    ptr, idx = R.csr_parts(A)
    out = {}
    p, i = ptr.copy(), idx.copy()
    i[len(i) // 2] = n
    out["index == n"] = (p, i, 0)
    p, i = ptr.copy(), idx.copy()
    i[3] = -1
    out["index == -1"] = (p, i, 0)
    p, i = R.csr_parts(A, index_base=1)
    i[-1] = 0
    out["index 0 with base 1"] = (p, i, 1)
    p, i = ptr.copy(), idx.copy()
    p[100] = p[101] + 1                                                          # decreases to p[101]
    out["ptr not monotone"] = (p, i, 0)
    p, i = ptr.copy(), idx.copy()
    p[50] = p[-1] + 5                                                            # beyond the entry count
    out["ptr beyond nnz"] = (p, i, 0)
    p, i = ptr.copy(), idx.copy()
    p[0] = 1
    out["ptr[0] != base"] = (p, i, 0)
    return n, out


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
def test_bad_patterns_are_refused_and_nothing_is_written(device):
    """An index out of range or a row pointer that decreases is SS_EINVAL from the check on the device: the outputs keep
    their contents and nothing faults."""
    ss.init(0)
    lib = _lib.lib()
    n, cases = _bad_patterns()
    for what, (ptr, idx, base) in cases.items():
        nc, rounds = C.c_int64(-7), C.c_int64(-7)
        if device:
            import torch
            tp, ti = torch.from_numpy(ptr).cuda(), torch.from_numpy(idx).cuda()
            outs = [torch.full((n,), -7, dtype=torch.int32, device="cuda") for _ in range(3)]
            rc = lib.ss_cluster_butina_csr(n, tp.data_ptr(), ti.data_ptr(), base, *[o.data_ptr() for o in outs],
                                           C.byref(nc), C.byref(rounds), _lib.SS_MEM_DEVICE)
            outs = [o.cpu().numpy() for o in outs]
        else:
            outs = [np.full(n, -7, np.int32) for _ in range(3)]
            rc = lib.ss_cluster_butina_csr(n, ptr.ctypes.data, idx.ctypes.data, base, *[o.ctypes.data for o in outs],
                                           C.byref(nc), C.byref(rounds), _lib.SS_MEM_HOST)
        assert rc == EINVAL, what
        assert all((o == -7).all() for o in outs), what
        fold = np.zeros(n, np.int32)
        with pytest.raises(ss.SimSpreadError) as e:
            ss.cross_fold_edges((ptr, idx), fold, 1, index_base=base)
        assert e.value.code == EINVAL, what
    # index_base outside {0, 1}; no place for the cluster count
    ptr, outs, nc = np.full(4, 2, np.int64), [np.full(3, -7, np.int32) for _ in range(2)], C.c_int64(-7)
    assert lib.ss_cluster_butina_csr(3, ptr.ctypes.data, None, 2, outs[0].ctypes.data, outs[1].ctypes.data, None,
                                     C.byref(nc), None, _lib.SS_MEM_HOST) == EINVAL
    ptr[:] = 0
    assert lib.ss_cluster_butina_csr(3, ptr.ctypes.data, None, 0, outs[0].ctypes.data, outs[1].ctypes.data, None, None,
                                     None, _lib.SS_MEM_HOST) == EINVAL
    assert all((o == -7).all() for o in outs)


# ------------------------------------------------------------------------------------------------ 2. the fused forms
@functools.lru_cache(maxsize=None)
def _fingerprints():
    """300 fingerprints of 128 bits around prototypes, with pairs whose similarity is exactly 2/4."""
    bits = neighbour_ref.base_bits(300, 128, 23)
    bits[20], bits[21], bits[22] = False, False, False
    bits[20, [0, 1, 2]] = True
    bits[21, [0, 1, 3]] = True                                                   # c = 2, u = 4 against row 20
    bits[22, [0, 1]] = True                                                      # c = 2, u = 3 against both
    F = ss.pack_fingerprints(bits)
    F.setflags(write=False)
    return F


def _assert_fused(res, pattern, s, cutoff, dt, n):
    """`res` (a fused form) equals the CSR form fed by the matching producer at the same cutoff, and the reference on
    the host helper's similarity."""
    via_csr = ss.butina_clusters(pattern)
    assert np.array_equal(res.centre, via_csr.centre) and np.array_equal(res.label, via_csr.label)
    assert np.array_equal(res.size, via_csr.size)
    assert_result(res, R.ref_butina(s >= np.dtype(dt).type(cutoff)), n)


@pytest.mark.parametrize("dt", DTYPES)
def test_fingerprints_with_pairs_exactly_on_the_cutoff(dt):
    ss.init(0)
    F, cutoff = _fingerprints(), 0.5
    s = neighbour_ref.ref_similarity(F, None, dt)
    assert s[20, 21] == 0.5 and ((s == 0.5).sum() - (np.diag(s) == 0.5).sum()) >= 2
    res =ss.butina_clusters(fingerprints=F, cutoff=cutoff, dtype=dt)
    assert ss.path_last() == ["butina_csr", "tanimoto_csr_sym"]
    _assert_fused(res, ss.tanimoto_csr(F, alpha=cutoff, weighted=False, dtype=dt), s, cutoff, dt, 300)
    assert 1 < res.nclusters < 300


def test_fingerprints_from_device_memory():
    import torch
    ss.init(0)
    F = _fingerprints()
    want = ss.butina_clusters(fingerprints=F, cutoff=0.5)
    res = ss.butina_clusters(fingerprints=torch.from_numpy(F.view(np.int64).copy()).cuda(), cutoff=0.5)
    assert res.label.is_cuda
    assert_result(res, (want.centre, want.label, want.size), 300)


def _iris():
    path = os.path.join(os.path.dirname(__file__), "golden", "iris", "iris.features")
    with open(path) as f:
        F = np.array([[float(v) for v in l.split()[1:]] for l in f.read().splitlines()[1:]])
    assert F.shape == (150, 4)
    return F


@pytest.mark.parametrize("dt", DTYPES)
def test_features_on_iris(dt):
    ss.init(0)
    F, cutoff = _iris(), 0.9
    s = real_floor_ref.jaccard_s(F, None, dt)
    res = ss.butina_clusters(features=F, cutoff=cutoff, dtype=dt)
    assert ss.path_last() == ["butina_csr", "jaccard_csr_sym"]
    _assert_fused(res, ss.jaccard_csr(F, alpha=cutoff, weighted=False, dtype=dt), s, cutoff, dt, 150)
    assert 1 < res.nclusters < 150


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("metric", dot_ref.METRICS)
def test_vectors_once_per_metric(metric, dt):
    """200 x 24 integer-valued embeddings: their sums are exact in any order, so the host helper's similarity is the
    device's bit for bit, and integer_rows holds pairs at exactly 0.5 for every metric."""
    ss.init(0)
    X, cutoff = dot_ref.integer_rows(200, 24, 5), 0.5
    s = real_floor_ref.dot_s(X, None, metric, dt)
    assert ((s == 0.5).sum() - (np.diag(s) == 0.5).sum()) >= 2
    res = ss.butina_clusters(vectors=X, metric=metric, cutoff=cutoff, dtype=dt)
    assert ss.path_last() == ["butina_csr", "dot_csr_sym"]
    _assert_fused(res, ss.dot_csr(X, metric=metric, alpha=cutoff, weighted=False, dtype=dt), s, cutoff, dt, 200)
    assert 1 < res.nclusters < 200


def test_nan_cutoff_and_nan_features_are_refused():
    ss.init(0)
    F = _iris()
    bad = F.copy()
    bad[7, 2] = np.nan
    calls = [lambda: ss.butina_clusters(fingerprints=_fingerprints(), cutoff=np.nan),
             lambda: ss.butina_clusters(features=F, cutoff=np.nan),
             lambda: ss.butina_clusters(vectors=F, cutoff=np.nan),
             lambda: ss.butina_clusters(features=bad, cutoff=0.5),
             lambda: ss.butina_clusters(vectors=bad, cutoff=0.5, dtype=np.float64)]
    for call in calls:
        with pytest.raises(ss.SimSpreadError) as e:
            call()
        assert e.value.code == EINVAL
    with pytest.raises(ValueError):
        ss.butina_clusters(vectors=F, metric="euclid", cutoff=0.5)


# ------------------------------------------------------------------------------------------------ 3. folds and leakage
@pytest.mark.parametrize("name", ["random_p0.05", "hub", "path", "empty65", "directed_knn"])
def test_cluster_folds_equal_the_reference_and_keep_clusters_whole(name):
    ss.init(0)
    _, label, size = R.reference(name)
    for nf in (1, 2, 5, 7):
        fold = ss.cluster_folds(label, nf)
        assert fold.dtype == np.int32 and np.array_equal(fold, R.ref_folds(label, nf))
        assert all(len(set(fold[label == c])) == 1 for c in range(len(size)))
        load = np.bincount(fold, minlength=nf)
        assert load.max() - load.min() <= size.max()
    import torch
    dev = ss.cluster_folds(torch.from_numpy(np.array(label)).cuda(), 5)
    assert dev.is_cuda and np.array_equal(dev.cpu().numpy(), R.ref_folds(label, 5))


def test_cluster_folds_refusals():
    ss.init(0)
    lib = _lib.lib()
    label = np.array([0, 1, 2, 1], np.int32)
    fold = np.full(4, -7, np.int32)
    for nclusters, nfolds in ((3, 0), (2, 2), (3, -1)):                          # nfolds < 1; label 2 outside 0..1
        rc = lib.ss_cluster_folds(label.ctypes.data, 4, nclusters, nfolds, fold.ctypes.data, _lib.SS_MEM_HOST)
        assert rc == EINVAL and (fold == -7).all()
    label[0] = -1
    assert lib.ss_cluster_folds(label.ctypes.data, 4, 3, 2, fold.ctypes.data, _lib.SS_MEM_HOST) == EINVAL
    assert (fold == -7).all()
    assert ss.cluster_folds(np.zeros(0, np.int32), 3).shape == (0,)


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
@pytest.mark.parametrize("name,noise", [("random_p0.05", None), ("directed_knn", 11), ("hub", None)])
def test_cross_fold_edges_equal_numpy(name, noise, device):
    """A cluster split and a random split of the same graph; the pattern is counted as given (the directed one is not
    symmetric, and its noisy parts hold duplicates and diagonal entries, 1-based)."""
    ss.init(0)
    A = R.graphs()[name]
    n = A.shape[0]
    base = 0 if noise is None else 1
    ptr, idx = R.csr_parts(A, index_base=base, noise_seed=noise)
    label = R.reference(name)[1]
    splits = {"cluster": R.ref_folds(label, 5), "random": np.random.default_rng(2).integers(0, 5, n).astype(np.int32)}
    counts = {}
    for what, fold in splits.items():
        if device:
            import torch
            got = ss.cross_fold_edges((torch.from_numpy(ptr).cuda(), torch.from_numpy(idx).cuda()),
                                      torch.from_numpy(fold).cuda(), 5, index_base=base)
            assert got.is_cuda
            got = got.cpu().numpy()
        else:
            got = ss.cross_fold_edges((ptr, idx), fold, 5, index_base=base)
        assert got.dtype == np.int64 and np.array_equal(got, R.ref_cross_edges(ptr, idx, fold, 5, base)), what
        counts[what] = int(got.sum())
    assert ss.path_last() == ["cross_edges"]
    assert counts["cluster"] < counts["random"]                                  # which is what the split is for
    one = ss.cross_fold_edges((ptr, idx), np.zeros(n, np.int32), 1, index_base=base)
    assert np.array_equal(one, [0])


def test_cross_fold_edges_refuses_bad_folds():
    ss.init(0)
    lib = _lib.lib()
    ptr, idx = R.csr_parts(R.graphs()["k70"])
    count = np.full(3, -7, np.int64)
    for bad in (3, -1):
        fold = np.zeros(70, np.int32)
        fold[40] = bad
        rc = lib.ss_cluster_cross_edges(70, ptr.ctypes.data, idx.ctypes.data, 0, fold.ctypes.data, 3, count.ctypes.data,
                                        _lib.SS_MEM_HOST)
        assert rc == EINVAL and (count == -7).all()
    fold = np.zeros(70, np.int32)
    assert lib.ss_cluster_cross_edges(70, ptr.ctypes.data, idx.ctypes.data, 0, fold.ctypes.data, 0, count.ctypes.data,
                                      _lib.SS_MEM_HOST) == EINVAL
    assert np.array_equal(ss.cross_fold_edges(sp.csr_matrix((0, 0)), np.zeros(0, np.int32), 2), [0, 0])


def test_the_fold_vector_goes_straight_into_evaluate_kfold():
    """butina_clusters -> cluster_folds -> evaluate_kfold on a small fingerprint graph: the int32 vector is accepted as it
    is and gives what the identical numpy vector gives; split_clusters groups the names by the same folds."""
    ss.init(0)
    F = _fingerprints()
    rng = np.random.default_rng(4)
    Y = sp.random(300, 23, density=0.15, format="csr", random_state=rng)
    Y.data[:] = 1.0
    res = ss.butina_clusters(fingerprints=F, cutoff=0.5)
    fold = ss.cluster_folds(res.label, 3)
    assert fold.dtype == np.int32 and fold.flags.c_contiguous
    g = ss.DeviceGraph.from_fingerprints(None, F, Y, alpha=0.5, weighted=True)
    got = g.evaluate_kfold(fold, 3, L=5)
    want = g.evaluate_kfold(np.array(R.ref_folds(res.label, 3), dtype=np.int64), 3, L=5)
    assert got.shape == (300, 6) and np.array_equal(got.view(np.uint8), want.view(np.uint8))
    X = ss.tanimoto_csr(F, alpha=0.5, weighted=False)
    leak = ss.cross_fold_edges(X, fold, 3)
    assert np.array_equal(leak, R.ref_cross_edges(X.indptr, X.indices, fold, 3))
    y = ss.NamedMatrix(Y.toarray(), [f"s{i}" for i in range(300)], [f"t{j}" for j in range(23)])
    groups = ss.split_clusters(y, res.label, 3)
    assert [sorted(gr) for gr in groups] == [sorted(f"s{i}" for i in np.nonzero(fold == f)[0]) for f in range(3)]
    g.close()
