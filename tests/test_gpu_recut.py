"""Cutoff sweeps on the device: featurize on CSR (ss_cutoff_csr_*), graphs re-thresholded from a resident parent
(ss_graph_recut_*) and dense-similarity graphs re-thresholded in place (ss_graph_set_cutoff_*).

ss_cutoff_csr is checked bitwise against the host reference of recut_ref.py; a recut child bitwise against the graph the
parent's own constructor builds at the same cutoff (sizes, degrees, every score)."""
import ctypes as C

import numpy as np
import pytest
import scipy.sparse as sp

import simspread_jl_amd as ss
from recut_ref import assert_csr_bitwise, ref_cutoff_csr

pytestmark = pytest.mark.gpu

DTYPES = [np.float32, np.float64]


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint8)


def assert_same(a, b, what=""):
    assert a.shape == b.shape and a.dtype == b.dtype, what
    assert np.array_equal(_bits(a), _bits(b)), what


# ----------------------------------------------------------------------------------------------- 1. ss_cutoff_csr
def _rows_matrix(lengths, cols, seed):
    """A CSR whose row r stores lengths[r] values in (0, 1], a few of them exactly 1 and a few repeated."""
    rng = np.random.default_rng(seed)
    idx = [np.sort(rng.choice(cols, n, replace=False)) for n in lengths]
    ptr = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)
    nnz = int(ptr[-1])
    val = 1.0 - rng.random(nnz)                      # (0, 1]
    val[rng.random(nnz) < 0.1] = 1.0
    if nnz > 4:
        val[nnz // 2] = val[nnz // 3]
    return sp.csr_matrix((val, np.concatenate(idx).astype(np.int32) if nnz else np.zeros(0, np.int32), ptr),
                         shape=(len(lengths), cols))


def _random_matrix(n, density, seed):
    rng = np.random.default_rng(seed)
    m = sp.random(n, n, density=density, format="csr", random_state=rng)
    m.data = 1.0 - rng.random(m.nnz)
    m.data[rng.random(m.nnz) < 0.05] = 1.0
    m.sort_indices()
    return m


# mean row length 146 (one wave per row), 1 (groups of 4), ~30, ~10 and ~6 (groups of 32, 16 and 8 lanes)
MATRICES = {
    "rows": lambda: _rows_matrix([0, 1, 63, 64, 65, 129, 700], 900, 1),
    "one": lambda: sp.csr_matrix(np.array([[0.625]])),
    "3000": lambda: _random_matrix(3000, 0.01, 2),
    "g16": lambda: _random_matrix(500, 0.02, 3),
    "g8": lambda: _random_matrix(500, 0.012, 4),
    # mean ~4.5 (groups of 8) but one row of 500 > 32 * 8: the skew fallback to one wave per row
    "skew": lambda: _rows_matrix([2] * 100 + [500] + [3] * 100, 900, 5),
}


def _alphas(X, dt):
    v = np.unique(X.data.astype(dt))
    return [dt(v[len(v) // 2]),                          # exactly a stored value, in the graph precision: >= is inclusive
            np.nextafter(v.max(), dt(np.inf)),           # above the maximum: empty
            dt(v.min() / 2)]                             # below the minimum: the identity


@pytest.mark.parametrize("name", list(MATRICES))
def test_cutoff_csr_is_bitwise_the_host_reference(name):
    ss.init(0)
    X = MATRICES[name]()
    for dt in DTYPES:
        a_eq, a_hi, a_lo = _alphas(X, dt)
        assert (X.data.astype(dt) == a_eq).any()
        for weighted in (True, False):
            for alpha in (a_eq, a_hi, a_lo):
                got = ss.cutoff_csr(X, alpha, weighted=weighted, dtype=dt)        # size query, then fill
                assert ss.path_last() == ["cutoff_csr"]
                assert_csr_bitwise(got, ref_cutoff_csr(X, alpha, weighted, dt))
            assert ss.cutoff_csr(X, a_hi, weighted=weighted, dtype=dt).nnz == 0
        ident = ss.cutoff_csr(X, a_lo, weighted=True, dtype=dt)
        assert_csr_bitwise(ident, sp.csr_matrix((X.data.astype(dt), X.indices, X.indptr), shape=X.shape))


def _raw(lib, suf, ft, rows, cols, ip, ii, iv, base, alpha, weighted, optr, oidx, oval, cap, mem=0):
    nnz = C.c_int64(-1)
    p = lambda a: None if a is None else a.ctypes.data
    rc = getattr(lib, f"ss_cutoff_csr_{suf}")(rows, cols, p(ip), p(ii), p(iv), base, ft(alpha), weighted, p(optr),
                                              p(oidx), p(oval), cap, C.byref(nnz), mem)
    return rc, nnz.value


@pytest.mark.parametrize("suf,ft,dt", [("f32", C.c_float, np.float32), ("f64", C.c_double, np.float64)])
def test_cutoff_csr_protocol_null_values_index_base_and_errors(suf, ft, dt):
    lib = ss.init(0)
    X = MATRICES["rows"]()
    rows, cols = X.shape
    ip, ii, iv = X.indptr.astype(np.int64), X.indices.astype(np.int32), X.data.astype(dt)
    alpha = float(_alphas(X, dt)[0])
    want = ref_cutoff_csr(X, alpha, True, dt)
    assert 0 < want.nnz < X.nnz
    # size query: optr and nnz only
    optr = np.full(rows + 1, -3, np.int64)
    rc, nnz = _raw(lib, suf, ft, rows, cols, ip, ii, iv, 0, alpha, 1, optr, None, None, 0)
    assert rc == 0 and nnz == want.nnz and np.array_equal(optr, want.indptr)
    # capacity too small: SS_EINVAL, nnz still reported, nothing written
    oidx, oval = np.full(nnz, -5, np.int32), np.full(nnz, -5, dt)
    rc, nnz2 = _raw(lib, suf, ft, rows, cols, ip, ii, iv, 0, alpha, 1, optr, oidx, oval, nnz - 1)
    assert rc == -1 and nnz2 == nnz and (oidx == -5).all() and (oval == -5).all()
    assert "capacity" in lib.ss_last_error().decode()
    # exact capacity
    rc, _ = _raw(lib, suf, ft, rows, cols, ip, ii, iv, 0, alpha, 1, optr, oidx, oval, nnz)
    assert rc == 0
    assert_csr_bitwise(sp.csr_matrix((oval, oidx, optr), shape=X.shape), want)
    # oval == NULL: the indices alone
    oidx2 = np.full(nnz, -5, np.int32)
    rc, _ = _raw(lib, suf, ft, rows, cols, ip, ii, iv, 0, alpha, 1, optr, oidx2, None, nnz)
    assert rc == 0 and np.array_equal(oidx2, oidx)
    # 1-based input, 0-based output
    o1, i1, v1 = np.zeros(rows + 1, np.int64), np.full(nnz, -5, np.int32), np.full(nnz, -5, dt)
    rc, n1 = _raw(lib, suf, ft, rows, cols, ip + 1, ii + 1, iv, 1, alpha, 1, o1, i1, v1, nnz)
    assert rc == 0 and n1 == nnz
    assert_csr_bitwise(sp.csr_matrix((v1, i1, o1), shape=X.shape), want)
    # val == NULL: every stored value is 1 (kept at alpha = 1, dropped above it)
    ones = sp.csr_matrix((np.ones(X.nnz), X.indices, X.indptr), shape=X.shape)
    for w in (1, 0):
        o, i, v = np.zeros(rows + 1, np.int64), np.zeros(X.nnz, np.int32), np.zeros(X.nnz, dt)
        rc, n = _raw(lib, suf, ft, rows, cols, ip, ii, None, 0, 1.0, w, o, i, v, X.nnz)
        assert rc == 0 and n == X.nnz
        assert_csr_bitwise(sp.csr_matrix((v, i, o), shape=X.shape), ref_cutoff_csr(ones, 1.0, bool(w), dt))
        rc, n = _raw(lib, suf, ft, rows, cols, ip, ii, None, 0, 1.5, w, o, None, None, 0)
        assert rc == 0 and n == 0 and (o == 0).all()
    # alpha <= 0 and NaN are refused before anything is written
    for bad in (0.0, -0.5, float("nan")):
        o = np.full(rows + 1, -3, np.int64)
        rc, n = _raw(lib, suf, ft, rows, cols, ip, ii, iv, 0, bad, 1, o, None, None, 0)
        assert rc == -1 and n == -1 and (o == -3).all(), bad
        assert "alpha" in lib.ss_last_error().decode()
        with pytest.raises(ss.SimSpreadError) as e:
            ss.cutoff_csr(X, bad, dtype=dt)
        assert e.value.code == -1


@pytest.mark.parametrize("dt", DTYPES)
def test_cutoff_csr_device_memory_and_determinism(dt):
    import torch
    ss.init(0)
    X = MATRICES["3000"]()
    alpha = _alphas(X, dt)[0]
    parts = (torch.from_numpy(X.indptr.astype(np.int64)).cuda(), torch.from_numpy(X.indices.astype(np.int32)).cuda(),
             torch.from_numpy(X.data.astype(dt)).cuda())
    for weighted in (True, False):
        want = ref_cutoff_csr(X, alpha, weighted, dt)
        runs = []
        for _ in range(2):
            p, i, v = ss.cutoff_csr(parts, alpha, weighted=weighted, dtype=dt, shape=X.shape)
            runs.append((p.cpu().numpy(), i.cpu().numpy(), v.cpu().numpy()))
            assert_csr_bitwise(sp.csr_matrix((runs[-1][2], runs[-1][1], runs[-1][0]), shape=X.shape), want)
        for a, b in zip(*runs):
            assert_same(a, b, "two runs differ")
        host = ss.cutoff_csr(X, alpha, weighted=weighted, dtype=dt)
        assert_csr_bitwise(host, want)
    # val = None on the device: all ones
    p, i, v = ss.cutoff_csr((parts[0], parts[1], None), 1.0, weighted=True, dtype=dt, shape=X.shape)
    assert int(i.numel()) == X.nnz and bool((v == 1).all())


# ----------------------------------------------------------------------------------------------- 2. recut == fresh
def fingerprints(n, d, seed, zero_rows=()):
    """Bits drawn around a few prototypes (every cutoff keeps some pairs and drops others), an exact duplicate and
    all-zero rows included."""
    rng = np.random.default_rng(seed)
    k = max(1, n // 16)
    proto = rng.random((k, d)) < rng.uniform(0.05, 0.5, (k, 1))
    member = rng.integers(0, k, n)
    flip = rng.random((n, d)) < rng.uniform(0.0, 0.3, (n, 1))
    bits = proto[member] ^ flip
    if n > 3:
        bits[n // 2] = bits[n // 3]
    for z in zero_rows:
        if z < n:
            bits[z] = False
    return ss.pack_fingerprints(bits)


def _labels(ns, nt, seed):
    rng = np.random.default_rng(seed)
    Y = sp.random(ns, nt, density=4.0 / nt, random_state=rng, format="csr")
    Y.data[:] = 1.0
    return Y


def scores(g, fold=None):
    """Every score a sparse graph serves, as a dict of arrays (leave-one-out and k-fold need nq == 0: the library
    refuses them on a sparse graph with query rows)."""
    out = {"source": g.predict("source"), "source_clean": g.predict("source", clean=True)}
    if g.nq:
        out["query"] = g.predict("query")
        out["query_clean"] = g.predict("query", clean=True)
    else:
        out["loo"] = g.predict_loo(clean=False)
        out["loo_clean"] = g.predict_loo(clean=True)
        if fold is not None:
            out["kfold"] = g.predict_kfold_rows(fold, 5, clean=True)
    return out


def assert_graphs_equal(child, fresh, fold=None, what=""):
    info = lambda g: (g.nq, g.ns, g.nf, g.nt, g.nnz_xq, g.nnz_xs, g.nnz_ys)
    assert info(child) == info(fresh), (what, info(child), info(fresh))
    for a, b, name in zip(child.degrees(), fresh.degrees(), ("kf", "ks", "kt")):
        assert np.array_equal(a, b), (what, name)
    sc, sf = scores(child, fold), scores(fresh, fold)
    for key in sf:
        assert_same(sc[key], sf[key], (what, key))


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("nq", [0, 37])
@pytest.mark.parametrize("n", [65, 1000])
def test_recut_child_equals_the_fresh_fingerprint_graph(n, nq, dt):
    ss.init(0)
    d, nt = 150, 40
    Fs = fingerprints(n, d, seed=n + 1, zero_rows=(4, 17))
    Fq = fingerprints(nq, d, seed=n + 2, zero_rows=(0,)) if nq else None
    Y = _labels(n, nt, 5)
    fold = np.random.default_rng(6).integers(0, 5, n).astype(np.int32)
    parent = ss.DeviceGraph.from_fingerprints(Fq, Fs, Y, alpha=0.2, weighted=True, dtype=dt)
    nnz = []
    for alpha in (0.2, 0.5, 1.0):
        for weighted in (True, False):
            child = parent.recut(alpha, weighted)
            assert ss.path_last() == ["recut"]
            fresh = ss.DeviceGraph.from_fingerprints(Fq, Fs, Y, alpha=alpha, weighted=weighted, dtype=dt)
            assert_graphs_equal(child, fresh, fold, (alpha, weighted))
            nnz.append(child.nnz_xs)
            child.close()
            fresh.close()
    # the cutoffs differ in what they keep; alpha = 1 keeps only unit similarities (the binary operand variants)
    assert nnz[0] > nnz[2] > nnz[4] >= n - 2
    parent.close()


@pytest.mark.parametrize("dt", DTYPES)
def test_recut_child_equals_the_fresh_feature_graph(dt):
    ss.init(0)
    rng = np.random.default_rng(8)
    n, nq, d, nt = 300, 21, 12, 30
    Fs = rng.random((n, d)) * (rng.random((n, d)) < 0.6)
    Fs[7] = Fs[3]
    Fs[11] = 0
    Fq = rng.random((nq, d)) * (rng.random((nq, d)) < 0.6)
    Y = _labels(n, nt, 9)
    parent = ss.DeviceGraph.from_features(Fq, Fs, Y, alpha=0.2, weighted=True, dtype=dt)
    for alpha, weighted in ((0.2, True), (0.55, True), (0.55, False)):
        child = parent.recut(alpha, weighted)
        fresh = ss.DeviceGraph.from_features(Fq, Fs, Y, alpha=alpha, weighted=weighted, dtype=dt)
        assert 0 < fresh.nnz_xs <= parent.nnz_xs
        assert_graphs_equal(child, fresh, None, (alpha, weighted))
        child.close()
        fresh.close()
    parent.close()


@pytest.mark.parametrize("dt", DTYPES)
def test_recut_of_a_sparse_parent_is_featurize_on_the_stored_blocks(dt):
    ss.init(0)
    n, nq, nf, nt = 400, 33, 257, 30
    Xs = _random_matrix(n, 0.05, 10)[:, :nf].tocsr()
    Xq = _random_matrix(n, 0.05, 11)[:nq, :nf].tocsr()
    Y = _labels(n, nt, 12)
    parent = ss.DeviceGraph.from_sparse(Xq, Xs, Y, dtype=dt)
    a_eq = float(_alphas(Xs, dt)[0])
    for alpha, weighted in ((a_eq, True), (a_eq, False), (1.0, True)):
        child = parent.recut(alpha, weighted)
        fresh = ss.DeviceGraph.from_sparse(ref_cutoff_csr(Xq, alpha, weighted, dt), ref_cutoff_csr(Xs, alpha, weighted, dt),
                                           Y, dtype=dt)
        assert 0 < fresh.nnz_xs < parent.nnz_xs
        assert_graphs_equal(child, fresh, None, (alpha, weighted))
        child.close()
        fresh.close()
    parent.close()


# ----------------------------------------------------------------------------------------------- 3. independence
@pytest.mark.parametrize("dt", DTYPES)
def test_children_are_independent_of_the_parent(dt):
    ss.init(0)
    n = 300
    Fs = fingerprints(n, 150, seed=21, zero_rows=(2,))
    Y = _labels(n, 25, 22)
    fold = np.random.default_rng(23).integers(0, 5, n).astype(np.int32)
    parent = ss.DeviceGraph.from_fingerprints(None, Fs, Y, alpha=0.2, weighted=True, dtype=dt)
    before = scores(parent, fold)
    mid = parent.recut(0.4, True)
    direct = parent.recut(0.6, False)
    after = scores(parent, fold)
    for key in before:
        assert_same(after[key], before[key], ("parent changed", key))
    # a child of a child at a higher cutoff is the direct child
    grand = mid.recut(0.6, False)
    assert_graphs_equal(grand, direct, fold, "child of a child")
    # children outlive the parent
    want = scores(direct, fold)
    parent.close()
    mid.close()
    got = scores(grand, fold)
    for key in want:
        assert_same(got[key], want[key], ("after the parent was closed", key))
    assert_graphs_equal(direct, ss.DeviceGraph.from_fingerprints(None, Fs, Y, alpha=0.6, weighted=False, dtype=dt), fold)


# ----------------------------------------------------------------------------------------------- 4. refusals
def _similarities(ns, nq, seed, symmetric=True):
    """Raw similarities in (0, 1): Sq (nq x ns) and a symmetric Ss (ns x ns) with unit diagonal; symmetric=False: the
    iid matrix itself, element (s, f) source s against feature f."""
    rng = np.random.default_rng(seed)
    U = rng.random((ns, ns))
    Ss = (U + U.T) / 2 if symmetric else U
    np.fill_diagonal(Ss, 1.0)
    return rng.random((nq, ns)), Ss


def test_refusals():
    lib = ss.init(0)
    n = 40
    Y = _labels(n, 8, 31)
    sparse = ss.DeviceGraph.from_fingerprints(None, fingerprints(n, 70, seed=32), Y, alpha=0.3, dtype=np.float32)
    _, Ss = _similarities(n, 0, 33)
    dense = ss.DeviceGraph.from_similarity(None, Ss, Y, alpha=0.3, dtype=np.float32)
    B = sp.random(9, 9, density=0.4, format="csr", random_state=np.random.default_rng(34))
    general = ss.DeviceGraph.general(B[:2], B, B[:, :3].T.tocsr(), dtype=np.float32)

    def refused(call, code, *words):
        with pytest.raises(ss.SimSpreadError) as e:
            call()
        assert e.value.code == code, str(e.value)
        for w in words:
            assert w in str(e.value), str(e.value)

    refused(lambda: general.recut(0.5), -5, "general")
    refused(lambda: dense.recut(0.5), -5, "ss_graph_set_cutoff")
    refused(lambda: sparse.set_cutoff(0.5), -5, "ss_graph_recut")
    refused(lambda: general.set_cutoff(0.5), -5)
    for bad in (0.0, -1.0, float("nan")):
        refused(lambda: sparse.recut(bad), -1, "alpha")
    # the other precision's entry point
    h = C.c_void_p(0x1234)
    assert lib.ss_graph_recut_f64(sparse._h, C.c_double(0.5), 1, C.byref(h)) == -1
    assert "precision" in lib.ss_last_error().decode() and not h.value
    assert lib.ss_graph_set_cutoff_f64(dense._h, C.c_double(0.5), 1) == -1
    assert "precision" in lib.ss_last_error().decode()
    assert lib.ss_graph_recut_f32(sparse._h, C.c_float(0.5), 1, None) == -1
    # the refused handles still serve
    assert np.isfinite(sparse.predict_loo()).all() and np.isfinite(dense.predict_loo()).all()


# ----------------------------------------------------------------------------------------------- 5. set_cutoff
@pytest.mark.parametrize("dt", DTYPES)
def test_set_cutoff_gives_the_fresh_dense_similarity_graph(dt):
    ss.init(0)
    ns, nq, nt = 300, 40, 30
    Y = _labels(ns, nt, 42)
    fold = np.random.default_rng(43).integers(0, 5, ns).astype(np.int32)

    def served(g):
        out, paths = {}, {}
        for key, call in (("query", lambda: g.predict("query", clean=True)), ("source", lambda: g.predict("source")),
                          ("loo", lambda: g.predict_loo(clean=True)),
                          ("kfold", lambda: g.predict_kfold_rows(fold, 5, clean=True))):
            out[key] = call()
            paths[key] = ss.path_last()
        return out, paths

    for symmetric in (True, False):     # an asymmetric Ss: the recount reads columns for kf and rows for ks
        Sq, Ss = _similarities(ns, nq, 41, symmetric)
        g = ss.DeviceGraph.from_similarity(Sq, Ss, Y, alpha=0.3, weighted=True, dtype=dt)
        served(g)                                          # the handle has served (and cached operands) before the change
        nnz = []
        for alpha, weighted in ((0.6, True), (0.6, False), (0.9, True), (0.4, False), (0.3, True)):   # up and back down
            assert g.set_cutoff(alpha, weighted) is g
            fresh = ss.DeviceGraph.from_similarity(Sq, Ss, Y, alpha=alpha, weighted=weighted, dtype=dt)
            for a, b, name in zip(g.degrees(), fresh.degrees(), ("kf", "ks", "kt")):
                assert np.array_equal(a, b), (alpha, weighted, name)
            if not symmetric:
                kept = Ss.astype(dt) >= dt(alpha)
                kf, ks, _ = g.degrees()
                assert np.array_equal(kf, kept.sum(axis=0)) and not np.array_equal(kf, kept.sum(axis=1))
                assert np.array_equal(ks, kept.sum(axis=1) + np.diff(sp.csr_matrix(Y).indptr))
            nnz.append(int(g.degrees()[0].sum()))
            got, gpath = served(g)
            want, wpath = served(fresh)
            for key in want:
                assert_same(got[key], want[key], (alpha, weighted, key))
                assert gpath[key] == wpath[key], (alpha, weighted, key, gpath[key], wpath[key])
                assert any(t.startswith("transfer_dense") for t in gpath[key]), gpath[key]
            fresh.close()
        assert nnz[2] < nnz[0] < nnz[4] and nnz[0] == nnz[1]
        g.close()


# ----------------------------------------------------------------------------------------------- 6. a sweep end to end
def test_a_cutoff_sweep_evaluated_in_place():
    ss.init(0)
    n = 200
    Fs = fingerprints(n, 150, seed=51, zero_rows=(3,))
    Y = _labels(n, 30, 52)
    parent = ss.DeviceGraph.from_fingerprints(None, Fs, Y, alpha=0.25, weighted=True, dtype=np.float32)
    for alpha in (0.25, 0.45, 0.7):
        child = parent.recut(alpha, True)
        fresh = ss.DeviceGraph.from_fingerprints(None, Fs, Y, alpha=alpha, weighted=True, dtype=np.float32)
        got, want = child.evaluate_loo(clean=True), fresh.evaluate_loo(clean=True)
        assert got.shape == (n, 6)
        assert np.array_equal(got, want, equal_nan=True), alpha
