"""The real-valued feature route on the device: feature rows -> thresholded weighted Jaccard CSR -> graph.

Every CSR is checked bitwise against a host reference kept in this file (the two sums accumulated in the graph
precision one feature at a time, the division in that precision, the cutoff of featurize) and against the dense route
it replaces (ss_similarity_jaccard_* followed by the cutoff), graphs built from features against graphs built from the
reference CSR, the reference's iris fixture, and two sets at production size (one the dense route cannot hold)."""
import ctypes as C
import os

import numpy as np
import pytest
import scipy.sparse as sp

import simspread_jl_amd as ss

pytestmark = pytest.mark.gpu

ALPHAS = (0.0, 0.3, 0.7, 1.0)


# ----------------------------------------------------------------------------------------------- host reference
def ref_similarity(A, B, dt):
    """s = smin / smax (1 when smax == 0) for every pair of rows, both sums accumulated in dt one feature at a time in
    order -- the order of the device kernels (np.sum would add pairwise)."""
    A = np.asarray(A, dt)
    B = np.asarray(B, dt)
    na, nb, d = A.shape[0], B.shape[0], A.shape[1]
    out = np.empty((na, nb), dt)
    step = max(1, (1 << 23) // max(1, nb))
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        for r in range(0, na, step):
            a = A[r:r + step]
            smin = np.zeros((a.shape[0], nb), dt)
            smax = np.zeros((a.shape[0], nb), dt)
            for k in range(d):
                smin += np.minimum(a[:, k, None], B[None, :, k])
                smax += np.maximum(a[:, k, None], B[None, :, k])
            out[r:r + step] = np.where(smax == 0, dt(1), smin / np.where(smax == 0, dt(1), smax))
    return out


def ref_cut(s, alpha, weighted, dt):
    """featurize's cutoff as the dense assembly applies it: keep s >= alpha with a non-zero stored value."""
    v = s if weighted else np.ones_like(s)
    with np.errstate(invalid="ignore"):
        keep = (s >= dt(alpha)) & (v != 0)
    return sp.csr_matrix((v[keep], np.nonzero(keep)[1].astype(np.int32),
                          np.concatenate([[0], np.cumsum(keep.sum(axis=1))]).astype(np.int64)), shape=s.shape)


def dense_sym(F, dt):
    return ss.jaccard_similarity(np.asarray(F, dt), dtype=dt)


def dense_cross(Fa, Fb, dt):
    """The dense route for a cross block: the off-diagonal block of the stacked rows."""
    S = dense_sym(np.vstack([Fa, Fb]), dt)
    return np.ascontiguousarray(S[:Fa.shape[0], Fa.shape[0]:])


def features(n, d, seed, zero_rows=()):
    """Non-negative rows around a few prototypes with multiplicative noise (every alpha keeps some pairs and drops
    others), an exact duplicate, all-zero rows and some exact zeros."""
    rng = np.random.default_rng(seed)
    k = max(1, n // 16)
    proto = rng.random((k, d)) * (rng.random((k, d)) < 0.8)
    X = proto[rng.integers(0, k, n)] * np.exp(rng.normal(0, rng.uniform(0.0, 0.6, (n, 1)), (n, d)))
    if n > 3:
        X[n // 2] = X[n // 3]
    for z in zero_rows:
        if z < n:
            X[z] = 0
    return X


def assert_csr_equal(got, want):
    got, want = sp.csr_matrix(got), sp.csr_matrix(want)
    assert got.shape == want.shape
    assert np.array_equal(got.indptr, want.indptr)
    assert np.array_equal(got.indices, want.indices)
    assert got.data.dtype == want.data.dtype
    assert np.array_equal(got.data.view(np.uint8), want.data.view(np.uint8))   # bitwise


def to_csr(p, i, v, shape):
    return sp.csr_matrix((v.cpu().numpy(), i.cpu().numpy(), p.cpu().numpy()), shape=shape)


# ----------------------------------------------------------------------------------------------- 1. the case matrix
# n in {1, 63, 127, 128, 129, 1000, 4097}, d in {1, 4, 15, 16, 17, 64, 300}
CASES = [(1, 1), (63, 4), (127, 15), (128, 16), (129, 17), (1000, 64), (300, 300), (4097, 16), (129, 1)]


@pytest.mark.parametrize("n,d", CASES)
def test_jaccard_csr_matches_the_host_reference_and_the_dense_route(n, d):
    import torch
    ss.init(0)
    F = features(n, d, seed=n * 7 + d, zero_rows=(0, n - 1, 5))
    nb = max(1, n // 2 + 3)
    G = features(nb, d, seed=n + d + 1, zero_rows=(1,))
    for dt in (np.float32, np.float64):
        s_sym = ref_similarity(F, F, dt)
        s_x = ref_similarity(F, G, dt)
        S_dense = dense_sym(F, dt)
        assert np.array_equal(S_dense.view(np.uint8), s_sym.view(np.uint8)), "dense jaccard differs from the reference"
        X_dense = dense_cross(F, G, dt)
        assert np.array_equal(X_dense.view(np.uint8), s_x.view(np.uint8))
        for weighted in (True, False):
            for alpha in ALPHAS:
                want = ref_cut(s_sym, alpha, weighted, dt)
                got = ss.jaccard_csr(F, alpha=alpha, weighted=weighted, dtype=dt)
                assert_csr_equal(got, want)
                assert_csr_equal(got, ref_cut(S_dense, alpha, weighted, dt))
                assert ss.path_last() == ["jaccard_csr_sym"]
                got_x = ss.jaccard_csr(F, G, alpha=alpha, weighted=weighted, dtype=dt)
                assert_csr_equal(got_x, ref_cut(s_x, alpha, weighted, dt))
                assert_csr_equal(got_x, ref_cut(X_dense, alpha, weighted, dt))
                assert ss.path_last() == ["jaccard_csr_cross"]
        # device input gives the same arrays
        want_t = torch.float32 if dt == np.float32 else torch.float64
        Ft = torch.from_numpy(F).to(want_t).cuda()
        Gt = torch.from_numpy(G).to(want_t).cuda()
        p, i, v = ss.jaccard_csr(Ft, Gt, alpha=0.3, weighted=True, dtype=dt)
        assert_csr_equal(to_csr(p, i, v, (n, nb)), ref_cut(s_x, 0.3, True, dt))
        p, i, v = ss.jaccard_csr(Ft, alpha=0.7, weighted=False, dtype=dt)
        assert_csr_equal(to_csr(p, i, v, (n, n)), ref_cut(s_sym, 0.7, False, dt))


@pytest.mark.parametrize("dt", [np.float32, np.float64])
def test_leading_dimension_larger_than_n(dt):
    lib = ss.init(0)
    n, nb, d, lda, ldb = 300, 170, 33, 311, 200
    F, G = features(n, d, seed=1), features(nb, d, seed=2)
    A = np.full((d, lda), np.nan, dt)                  # column-major n x d with lda rows per column; padding is NaN
    A[:, :n] = F.T
    B = np.full((d, ldb), np.nan, dt)
    B[:, :nb] = G.T
    fn = getattr(lib, f"ss_similarity_jaccard_csr_{'f32' if dt == np.float32 else 'f64'}")
    ft = C.c_float if dt == np.float32 else C.c_double
    want = ref_cut(ref_similarity(F, G, dt), 0.3, True, dt)
    ptr = np.zeros(n + 1, np.int64)
    idx = np.zeros(want.nnz, np.int32)
    val = np.zeros(want.nnz, dt)
    nnz = C.c_int64(-1)
    assert fn(A.ctypes.data, n, lda, B.ctypes.data, nb, ldb, d, ft(0.3), 1, ptr.ctypes.data, idx.ctypes.data,
              val.ctypes.data, want.nnz, C.byref(nnz), 0) == 0
    assert_csr_equal(sp.csr_matrix((val, idx, ptr), shape=(n, nb)), want)
    # device memory, symmetric, the same padding
    import torch
    At = torch.from_numpy(A).cuda()
    want = ref_cut(ref_similarity(F, F, dt), 0.3, True, dt)
    pt = torch.zeros(n + 1, dtype=torch.int64, device="cuda")
    it = torch.zeros(want.nnz, dtype=torch.int32, device="cuda")
    vt = torch.zeros(want.nnz, dtype=At.dtype, device="cuda")
    assert fn(At.data_ptr(), n, lda, None, 0, 0, d, ft(0.3), 1, pt.data_ptr(), it.data_ptr(), vt.data_ptr(), want.nnz,
              C.byref(nnz), 1) == 0
    assert nnz.value == want.nnz
    assert_csr_equal(to_csr(pt, it, vt, (n, n)), want)


# ----------------------------------------------------------------------------------------------- 2. edge cases
@pytest.mark.parametrize("dt", [np.float32, np.float64])
def test_edge_cases_of_the_rule(dt):
    ss.init(0)
    X = np.zeros((4, 6))
    X[2, :3] = [1.0, 2.0, 0.5]
    X[3, 3:] = [1.0, 1.0, 4.0]                   # rows 2 and 3 share nothing: s = 0
    # alpha = 0 unweighted keeps every pair, zero rows against non-zero rows included
    assert (ss.jaccard_csr(X, alpha=0.0, weighted=False, dtype=dt).toarray() == 1).all()
    # weighted drops s = 0 (a stored zero is no edge)
    W = ss.jaccard_csr(X, alpha=0.0, weighted=True, dtype=dt)
    Wd = W.toarray()
    assert W.nnz == 6 and (W.data != 0).all()
    assert Wd[0, 1] == 1 and Wd[1, 0] == 1 and Wd[0, 0] == 1          # zero with zero: 1
    assert Wd[0, 2] == 0 and Wd[2, 0] == 0 and Wd[1, 3] == 0          # zero with non-zero: 0
    assert Wd[2, 3] == 0 and Wd[2, 2] == 1 and Wd[3, 3] == 1
    # d = 0: every pair has s = 1, as in the dense kernel
    E = np.zeros((5, 0))
    assert (ss.jaccard_csr(E, alpha=1.0, dtype=dt).toarray() == 1).all()
    assert (dense_sym(E, dt) == 1).all()
    assert (ss.jaccard_csr(E, np.zeros((3, 0)), alpha=0.5, dtype=dt).toarray() == 1).all()
    # alpha exactly equal to an attained s: >= is inclusive
    F = features(200, 9, seed=4)
    s = ref_similarity(F, F, dt)
    a = s[3, 17]
    got = ss.jaccard_csr(F, alpha=float(a), dtype=dt)
    assert got[3, 17] == a and got.nnz == int((s >= a).sum())
    assert_csr_equal(got, ref_cut(s, a, True, dt))


@pytest.mark.parametrize("dt", [np.float32, np.float64])
def test_duplicates_subnormals_negative_and_infinite_values_match_the_dense_route(dt):
    ss.init(0)
    rng = np.random.default_rng(8)
    tiny = np.finfo(dt).tiny
    cases = {
        "duplicates": np.repeat(rng.random((40, 7)), 5, axis=0),
        "subnormal": rng.random((150, 12)) * tiny * rng.choice([1e-3, 1e-1, 1.0, 1e3], (150, 1)),
        "negative": rng.normal(0, 1, (160, 10)),
        "infinite": np.where(rng.random((140, 6)) < 0.1, np.inf, rng.random((140, 6))) *
                    np.where(rng.random((140, 6)) < 0.2, -1, 1),
    }
    for name, F in cases.items():
        F = F.astype(dt)
        S = dense_sym(F, dt)
        s = ref_similarity(F, F, dt)
        # inf - inf sums give NaN similarities (dropped by the cutoff); the NaN's sign bit is the platform's own
        assert np.array_equal(np.isnan(S), np.isnan(s)), name
        assert np.array_equal(S[~np.isnan(S)].view(np.uint8), s[~np.isnan(s)].view(np.uint8)), name
        for alpha in (-0.5, 0.0, 0.5, 1.0):
            for weighted in (True, False):
                got = ss.jaccard_csr(F, alpha=alpha, weighted=weighted, dtype=dt)
                assert_csr_equal(got, ref_cut(S, alpha, weighted, dt))
        G = F[::-3].copy()
        got = ss.jaccard_csr(F, G, alpha=0.2, dtype=dt)
        assert_csr_equal(got, ref_cut(dense_cross(F, G, dt), 0.2, True, dt))
    # duplicate rows are exactly 1 with each other
    D = ss.jaccard_csr(cases["duplicates"].astype(dt), alpha=1.0, dtype=dt)
    assert D.nnz == 40 * 25


@pytest.mark.parametrize("dt", [np.float32, np.float64])
def test_nan_features_or_alpha_are_refused_before_anything_is_written(dt):
    import torch
    lib = ss.init(0)
    suf = "f32" if dt == np.float32 else "f64"
    fn = getattr(lib, f"ss_similarity_jaccard_csr_{suf}")
    ft = C.c_float if dt == np.float32 else C.c_double
    F = np.asfortranarray(features(300, 20, seed=5).astype(dt))
    ptr = np.full(301, -7, np.int64)
    idx = np.full(10, -7, np.int32)
    val = np.full(10, -7, dt)
    nnz = C.c_int64(-7)
    Fn = F.copy(order="F")
    Fn[299, 19] = np.nan                         # the last element
    for args in ((Fn, None, 0.5), (F, Fn, 0.5), (F, None, float("nan"))):
        a, b, alpha = args
        for out_idx in (None, idx.ctypes.data):
            rc = fn(a.ctypes.data, 300, 300, None if b is None else b.ctypes.data, 300, 300, 20, ft(alpha), 1,
                    ptr.ctypes.data, out_idx, None if out_idx is None else val.ctypes.data, 10, C.byref(nnz), 0)
            assert rc == -1, rc
            assert "NaN" in lib.ss_last_error().decode()
    assert nnz.value == -7 and (ptr == -7).all() and (idx == -7).all() and (val == -7).all()
    # device memory
    Ft = torch.from_numpy(np.ascontiguousarray(Fn.T)).cuda()     # (d, n) row-major = column-major n x d
    pt = torch.full((301,), -7, dtype=torch.int64, device="cuda")
    assert fn(Ft.data_ptr(), 300, 300, None, 0, 0, 20, ft(0.5), 1, pt.data_ptr(), None, None, 0, C.byref(nnz), 1) == -1
    assert nnz.value == -7 and (pt.cpu().numpy() == -7).all()
    with pytest.raises(ss.SimSpreadError) as e:
        ss.jaccard_csr(np.ascontiguousarray(Fn), alpha=0.5, dtype=dt)
    assert e.value.code == -1
    with pytest.raises(ss.SimSpreadError) as e:
        ss.DeviceGraph.from_features(None, np.ascontiguousarray(Fn), np.eye(300, 4), alpha=0.5, dtype=dt)
    assert e.value.code == -1


# ----------------------------------------------------------------------------------------------- 3. the size protocol
def test_size_protocol_capacity_and_memory_kinds():
    import torch
    lib = ss.init(0)
    F = np.asfortranarray(features(700, 30, seed=3, zero_rows=(2,)).astype(np.float32))
    fn = lib.ss_similarity_jaccard_csr_f32
    ptr = np.zeros(701, np.int64)
    nnz = C.c_int64(-1)
    assert fn(F.ctypes.data, 700, 700, None, 0, 0, 30, C.c_float(0.3), 1, ptr.ctypes.data, None, None, 0, C.byref(nnz),
              0) == 0
    want = ss.jaccard_csr(F, alpha=0.3)
    assert nnz.value == want.nnz > 0 and np.array_equal(ptr, want.indptr)
    # capacity too small: SS_EINVAL, nnz still reported, nothing written
    idx = np.full(nnz.value, -5, np.int32)
    val = np.full(nnz.value, -5, np.float32)
    nnz2 = C.c_int64(-1)
    rc = fn(F.ctypes.data, 700, 700, None, 0, 0, 30, C.c_float(0.3), 1, ptr.ctypes.data, idx.ctypes.data,
            val.ctypes.data, nnz.value - 1, C.byref(nnz2), 0)
    assert rc == -1 and nnz2.value == nnz.value
    assert (idx == -5).all() and (val == -5).all()
    # val == NULL: the pattern only
    rc = fn(F.ctypes.data, 700, 700, None, 0, 0, 30, C.c_float(0.3), 1, ptr.ctypes.data, idx.ctypes.data, None,
            nnz.value, C.byref(nnz2), 0)
    assert rc == 0 and np.array_equal(idx, want.indices) and (val == -5).all()
    # exact capacity
    rc = fn(F.ctypes.data, 700, 700, None, 0, 0, 30, C.c_float(0.3), 1, ptr.ctypes.data, idx.ctypes.data,
            val.ctypes.data, nnz.value, C.byref(nnz2), 0)
    assert rc == 0
    assert_csr_equal(sp.csr_matrix((val, idx, ptr), shape=(700, 700)), want)
    # device memory: the same CSR, and run to run bitwise repeatable
    Ft = torch.from_numpy(np.ascontiguousarray(F)).cuda()
    for _ in range(2):
        p, i, v = ss.jaccard_csr(Ft, alpha=0.3)
        assert np.array_equal(p.cpu().numpy(), ptr)
        assert np.array_equal(i.cpu().numpy(), idx)
        assert np.array_equal(v.cpu().numpy().view(np.uint32), val.view(np.uint32))
    # argument checks return codes, they do not abort
    args = dict(F=F.ctypes.data, n=700, ld=700, d=30, ptr=ptr.ctypes.data)

    def call(**kw):
        a = dict(args, **kw)
        return fn(a["F"], a["n"], a["ld"], None, 0, 0, a["d"], C.c_float(0.3), 1, a["ptr"], None, None, 0,
                  C.byref(nnz2), 0)
    assert call(d=-1) == -1
    assert call(ld=699) == -1
    assert call(F=None) == -1
    assert call(ptr=None) == -1
    assert call(n=1 << 31, ld=1 << 31) == -5


def test_nnz_of_2_to_the_31_is_refused_without_allocating_the_output():
    import torch
    lib = ss.init(0)
    n = 50_000
    Ft = torch.full((1, n), 0.25, dtype=torch.float32, device="cuda")     # n x 1 column-major, constant rows
    ptr = torch.full((n + 1,), -7, dtype=torch.int64, device="cuda")
    nnz = C.c_int64(-1)
    rc = lib.ss_similarity_jaccard_csr_f32(Ft.data_ptr(), n, n, None, 0, 0, 1, C.c_float(0.5), 1, ptr.data_ptr(), None,
                                           None, 0, C.byref(nnz), 1)
    assert rc == -5, rc
    assert nnz.value == n * n
    assert "2^31" in lib.ss_last_error().decode()
    assert (ptr.cpu().numpy() == -7).all()
    with pytest.raises(ss.SimSpreadError) as e:
        ss.jaccard_csr(Ft.t(), alpha=0.0, weighted=False)
    assert e.value.code == -5
    Y = (torch.zeros(n + 1, dtype=torch.int64, device="cuda"), torch.zeros(0, dtype=torch.int32, device="cuda"), None, 4)
    with pytest.raises(ss.SimSpreadError) as e:
        ss.DeviceGraph.from_features(None, Ft.t(), Y, alpha=0.0, weighted=False)
    assert e.value.code == -5


# ----------------------------------------------------------------------------------------------- 4. reference data
def test_iris_tutorial_graph_block():
    """docs/src/tutorial/fishers-flowers.jl:66,95-96 on the committed iris fixture: featurize(S, 0.9, true) with S the
    reference's own iris.simmat."""
    ss.init(0)
    here = os.path.join(os.path.dirname(__file__), "golden", "iris")

    def read(p):
        with open(os.path.join(here, p)) as f:
            lines = f.read().splitlines()
        return np.array([[float(v) for v in l.split()[1:]] for l in lines[1:]])
    F, S = read("iris.features"), read("iris.simmat")
    alpha = 0.9
    got = ss.jaccard_csr(F, alpha=alpha, weighted=True, dtype=np.float64)
    G = got.toarray()
    want = np.where(S >= alpha, S, 0.0)
    near = np.abs(S - alpha) <= 1e-12
    assert np.array_equal((G != 0)[~near], (want != 0)[~near])
    both = (G != 0) & (want != 0)
    assert np.abs(G[both] - want[both]).max() <= 1e-12
    assert_csr_equal(got, ref_cut(dense_sym(F, np.float64), alpha, True, np.float64))
    assert_csr_equal(got, ref_cut(ref_similarity(F, F, np.float64), alpha, True, np.float64))


# ----------------------------------------------------------------------------------------------- 5. graphs
def _labels(ns, nt, seed):
    rng = np.random.default_rng(seed)
    Y = sp.random(ns, nt, density=4.0 / nt, random_state=rng, format="csr")
    Y.data[:] = 1.0
    return Y


@pytest.mark.parametrize("dt,tol", [(np.float32, 1e-5), (np.float64, 1e-12)])
@pytest.mark.parametrize("weighted", [True, False])
def test_graph_from_features_equals_the_graph_from_the_reference_csr(dt, tol, weighted):
    from oracle import simspread_oracle as O
    ss.init(0)
    ns, nq, nt, d, alpha = 3000, 500, 300, 24, 0.55
    Fs = features(ns, d, seed=11, zero_rows=(4, 17))
    Fq = features(nq, d, seed=12, zero_rows=(0,))
    Xs = ref_cut(ref_similarity(Fs, Fs, dt), alpha, weighted, dt)
    Xq = ref_cut(ref_similarity(Fq, Fs, dt), alpha, weighted, dt)
    assert 0.001 < Xs.nnz / ns / ns < 0.5
    Y = _labels(ns, nt, 13)

    g = ss.DeviceGraph.from_features(Fq, Fs, Y, alpha=alpha, weighted=weighted, dtype=dt)
    assert ss.path_last() == ["jaccard_csr_sym", "jaccard_csr_cross"]
    assert (g.nq, g.ns, g.nf, g.nt, g.nnz_xq, g.nnz_xs) == (nq, ns, ns, nt, Xq.nnz, Xs.nnz)
    r = ss.DeviceGraph.from_sparse(Xq, Xs, Y, dtype=dt)
    for rows in ("query", "source"):
        got, want = g.predict(rows), r.predict(rows)
        assert np.array_equal(got.view(np.uint8), want.view(np.uint8)), rows
        ref = O.predict_factored(Xq.astype(np.float64), Xs.astype(np.float64), Y, rows)
        assert np.abs(got - ref).max() <= tol * np.abs(ref).max(), rows

    g3 = ss.DeviceGraph.from_features(None, Fs, Y, alpha=alpha, weighted=weighted, dtype=dt)
    assert ss.path_last() == ["jaccard_csr_sym"]
    r3 = ss.DeviceGraph.from_sparse(None, Xs, Y, dtype=dt)
    got, want = g3.predict_loo(clean=True), r3.predict_loo(clean=True)
    assert np.array_equal(got.view(np.uint8), want.view(np.uint8))
    qs = [0, 4, 17, ns // 2, ns - 1]
    ref = O.predict_loo_factored(Xs, Y, clean_flag=True, queries=qs)
    assert np.abs(got[qs] - ref).max() <= tol * np.abs(ref).max()
    fold = np.random.default_rng(5).integers(0, 7, ns).astype(np.int32)
    got, want = g3.predict_kfold(fold, 7, clean=True), r3.predict_kfold(fold, 7, clean=True)
    assert np.array_equal(got.view(np.uint8), want.view(np.uint8))
    got, want = g3.evaluate_loo(clean=True), r3.evaluate_loo(clean=True)
    assert np.array_equal(got.view(np.uint8), want.view(np.uint8))


def test_graph_from_device_features():
    import torch
    ss.init(0)
    ns, nq, nt, d, alpha = 1500, 200, 100, 16, 0.55
    Fs, Fq = features(ns, d, seed=21), features(nq, d, seed=22)
    Y = _labels(ns, nt, 23)
    for dt, tt in ((np.float32, torch.float32), (np.float64, torch.float64)):
        Xs = ref_cut(ref_similarity(Fs, Fs, dt), alpha, True, dt)
        Xq = ref_cut(ref_similarity(Fq, Fs, dt), alpha, True, dt)
        Yd = (torch.from_numpy(Y.indptr.astype(np.int64)).cuda(), torch.from_numpy(Y.indices.astype(np.int32)).cuda(),
              None, nt)
        g = ss.DeviceGraph.from_features(torch.from_numpy(Fq).to(tt).cuda(), torch.from_numpy(Fs).to(tt).cuda(), Yd,
                                         alpha=alpha, dtype=dt)
        r = ss.DeviceGraph.from_sparse(Xq, Xs, Y, dtype=dt)
        got, want = g.predict("query"), r.predict("query")
        assert np.array_equal(got.view(np.uint8), want.view(np.uint8))
        with pytest.raises(TypeError):
            ss.DeviceGraph.from_features(None, torch.from_numpy(Fs).cuda().to(torch.float16), Yd, alpha=alpha, dtype=dt)


# ----------------------------------------------------------------------------------------------- 6. at size
def clustered_features(n, d, clusters, seed, noise=0.05, dtype=np.float32):
    """Non-negative cluster prototypes with multiplicative noise: members of one cluster are ~0.9 similar, of different
    clusters ~0.55, so alpha = 0.85 keeps (almost exactly) the pairs inside a cluster -- sum of squared cluster sizes."""
    rng = np.random.default_rng(seed)
    proto = rng.random((clusters, d)) + 0.05
    member = rng.integers(0, clusters, n)
    X = np.empty((n, d), dtype)
    for r in range(0, n, 16384):
        m = member[r:r + 16384]
        X[r:r + 16384] = proto[m] * np.exp(rng.normal(0, noise, (len(m), d)))
    return X, member


def sample_rows(n, count, seed):
    rng = np.random.default_rng(seed)
    rows = {0, 1, n - 1, n - 2, 127, 128, 255, 256, n // 2 - 1, n // 2}
    rows |= {t * 128 + o for t in rng.integers(1, n // 128, 8) for o in (-1, 0)}
    while len(rows) < count:
        rows.add(int(rng.integers(0, n)))
    return np.array(sorted(r for r in rows if 0 <= r < n))[:count]


def test_100k_by_64_clustered_fp32_set():
    import torch
    from oracle import simspread_oracle as O
    ss.init(0)
    n, d, alpha = 100_000, 64, 0.85
    X, member = clustered_features(n, d, clusters=100, seed=2026)
    Xt = torch.from_numpy(X).cuda()
    p, i, v = ss.jaccard_csr(Xt, alpha=alpha, weighted=True, dtype=np.float32)
    torch.cuda.synchronize()
    sizes = np.bincount(member)
    implied = int((sizes.astype(np.int64) ** 2).sum())
    nnz = int(i.numel())
    assert 0.99 * implied <= nnz <= 1.01 * implied, (nnz, implied)
    A = sp.csr_matrix((v.cpu().numpy(), i.cpu().numpy(), p.cpu().numpy()), shape=(n, n))
    del p, i, v
    At = A.T.tocsr()
    At.sort_indices()
    assert np.array_equal(A.indptr, At.indptr) and np.array_equal(A.indices, At.indices)
    assert np.array_equal(A.data.view(np.uint32), At.data.view(np.uint32))
    del At
    assert (A.diagonal() == 1).all()
    rows = sample_rows(n, 256, 9)
    want = ref_cut(ref_similarity(X[rows], X, np.float32), alpha, True, np.float32)
    assert_csr_equal(A[rows], want)
    # the graph at size: a 2048-fold leave-one-out block, 8 folds against the factored oracle
    Y = _labels(n, 2000, 21)
    g = ss.DeviceGraph.from_features(None, Xt, (torch.from_numpy(Y.indptr.astype(np.int64)).cuda(),
                                                torch.from_numpy(Y.indices.astype(np.int32)).cuda(), None, 2000),
                                     alpha=alpha, weighted=True, dtype=np.float32)
    assert g.nnz_xs == nnz
    out = g.predict_loo(0, 2048, clean=True)
    assert np.isfinite(out).all()
    qs = [0, 1, 127, 128, 1000, 1500, 2046, 2047]
    ref = O.predict_loo_factored(A, Y, clean_flag=True, queries=qs)
    assert np.abs(out[qs] - ref).max() <= 1e-5 * np.abs(ref).max()


def test_200k_by_32_fp64_set_the_dense_route_cannot_hold():
    """200k rows: the dense fp64 similarity would be 320 GB."""
    import torch
    ss.init(0)
    n, d, alpha = 200_000, 32, 0.85
    X, member = clustered_features(n, d, clusters=400, seed=77, dtype=np.float64)
    Xt = torch.from_numpy(X).cuda()
    p, i, v = ss.jaccard_csr(Xt, alpha=alpha, weighted=True, dtype=np.float64)
    torch.cuda.synchronize()
    sizes = np.bincount(member)
    implied = int((sizes.astype(np.int64) ** 2).sum())
    nnz = int(i.numel())
    assert 0.99 * implied <= nnz <= 1.01 * implied, (nnz, implied)
    ptr = p.cpu().numpy()
    rows = sample_rows(n, 64, 10)
    starts, ends = ptr[rows], ptr[rows + 1]
    sel = np.concatenate([np.arange(s, e) for s, e in zip(starts, ends)])
    sel_t = torch.from_numpy(sel).cuda()
    got = sp.csr_matrix((v[sel_t].cpu().numpy(), i[sel_t].cpu().numpy(),
                         np.concatenate([[0], np.cumsum(ends - starts)])), shape=(len(rows), n))
    want = ref_cut(ref_similarity(X[rows], X, np.float64), alpha, True, np.float64)
    assert_csr_equal(got, want)
