"""The inner-product similarity route on the device: real-valued rows -> thresholded cosine / Tanimoto / Dice CSR (Gram
blocks on the matrix cores) -> graph.

The order of the three sums is the kernel's own, so general inputs are checked against the fp64 rule inside the derived
band of dot_ref.py (the pattern is exact outside it, and at most 1 % of the pairs lie inside); inputs whose sums are
exact in any order are checked bit for bit.  Everything else the contract fixes -- symmetry, the diagonal, alpha nesting,
repeatability, host against device input, the size protocol, graphs against graphs built from the same CSR, recut -- is
checked bitwise."""
import ctypes as C

import numpy as np
import pytest
import scipy.sparse as sp

import simspread_jl_amd as ss

import dot_ref as R
from dot_ref import assert_csr_equal, ref_cut, to_csr

pytestmark = pytest.mark.gpu

DTYPES = (np.float32, np.float64)


def suffix(dt):
    return "f32" if dt == np.float32 else "f64"


def tensor(X, dt):
    import torch
    return torch.from_numpy(np.ascontiguousarray(X)).to(torch.float32 if dt == np.float32 else torch.float64).cuda()


def check_structure(M, sym, alpha):
    n = M.shape[0]
    assert M.indptr[0] == 0 and (np.diff(M.indptr) >= 0).all() and M.indptr[n] == M.nnz == len(M.indices)
    inner = np.ones(max(M.nnz - 1, 0), bool)
    inner[M.indptr[1:-1][(M.indptr[1:-1] > 0) & (M.indptr[1:-1] < M.nnz)] - 1] = False     # row boundaries
    assert (np.diff(M.indices)[inner] > 0).all(), "idx not strictly ascending within a row"
    assert M.nnz == 0 or (0 <= M.indices.min() and M.indices.max() < M.shape[1])
    assert not np.isnan(M.data).any()
    if sym:
        T = M.T.tocsr()
        T.sort_indices()
        assert_csr_equal(T, M)
        if alpha <= 1:
            assert (M.diagonal() == 1).all()


def check_band(M, s64, alpha, weighted, dt, d):
    """Outside the band the pattern is exact; every stored value is within the band of s64 (exactly 1 when unweighted);
    at most 1 % of the pairs are inside the band, so the test cannot pass by leaving everything out.  Returns the
    largest |s_device - s64| over the stored entries."""
    band = R.band(dt, d)
    a = float(dt(alpha))
    rows = np.repeat(np.arange(M.shape[0]), np.diff(M.indptr))
    kept = np.zeros(M.shape, bool)
    kept[rows, M.indices] = True
    with np.errstate(invalid="ignore"):
        inb = np.abs(s64 - a) <= band
        want = (s64 >= a) & ((s64 != 0) if weighted else True)
    assert inb.mean() <= 0.01, inb.mean()
    assert np.array_equal(kept[~inb], want[~inb])
    sv = s64[rows, M.indices]
    if not weighted:
        assert (M.data == 1).all()
        return 0.0
    err = float(np.abs(M.data.astype(np.float64) - sv).max(initial=0.0))
    print(f"      max |s - s64| = {err:.3e}  band = {band:.3e}  in band {inb.mean():.4%}")
    assert err <= band, (err, band)
    return err


def combos(n):
    """(dtype, signed, metric) of one case: the full product, or for the largest n (16.8 M pairs per host reference) a
    subset that still has every metric, both dtypes and both input kinds."""
    full = [(dt, signed, m) for dt in DTYPES for signed in (False, True) for m in R.METRICS]
    if n <= 1000:
        return full
    return [(np.float32, False, "cosine"), (np.float64, True, "tanimoto"), (np.float32, True, "dice"),
            (np.float64, False, "cosine")]


# ----------------------------------------------------------------------------------------------- 1. the case matrix
@pytest.mark.parametrize("n,d", R.CASES)
def test_dot_csr_case_matrix(n, d):
    ss.init(0)
    nb = max(1, n // 2 + 3)
    inputs, sums = {}, {}
    for c, (dt, signed, metric) in enumerate(combos(n)):
        if signed not in inputs:
            inputs[signed] = R.case_inputs(n, d, signed)
        F, G = inputs[signed]
        if (dt, signed) not in sums:
            sums[(dt, signed)] = (R.sums64(F, F, dt), R.sums64(F, G, dt))
        s_sym = R.rule(*sums[(dt, signed)][0], metric, np.float64, sym=True)
        s_x = R.rule(*sums[(dt, signed)][1], metric, np.float64)
        print(f"  n={n} d={d} {dt.__name__} signed={signed} {metric}")
        if n <= 300:
            alphas = R.ALPHAS
        elif n <= 1000:
            alphas = (R.ALPHAS[c % 4], R.ALPHAS[(c + 2) % 4])
        else:
            alphas = (R.ALPHAS[c % 4],)
        if (n, d) == R.EXTRA_ALPHA_CASE and c == 0:
            alphas = alphas + R.EXTRA_ALPHAS
        for alpha in alphas:
            W = ss.dot_csr(F, metric=metric, alpha=alpha, weighted=True, dtype=dt)
            assert ss.path_last() == ["dot_csr_sym"]
            assert W.data.dtype == dt
            check_structure(W, True, alpha)
            check_band(W, s_sym, alpha, True, dt, d)
            X = ss.dot_csr(F, G, metric=metric, alpha=alpha, weighted=True, dtype=dt)
            assert ss.path_last() == ["dot_csr_cross"]
            assert X.shape == (n, nb)
            check_structure(X, False, alpha)
            check_band(X, s_x, alpha, True, dt, d)
            for Fb, Wt, s64 in ((None, W, s_sym), (G, X, s_x)):
                U = ss.dot_csr(F, Fb, metric=metric, alpha=alpha, weighted=False, dtype=dt)
                check_structure(U, Fb is None, alpha)
                assert (U.data == 1).all()
                if alpha > 0:      # the unweighted pattern is the weighted pattern, checked above
                    assert np.array_equal(U.indptr, Wt.indptr) and np.array_equal(U.indices, Wt.indices)
                else:              # at alpha <= 0 it also keeps s = 0
                    check_band(U, s64, alpha, False, dt, d)
        # alpha nesting, bitwise: the CSR at 0.7 is the cutoff of the device's own weighted CSR at 0.3
        for Fb in (None, G):
            lo = ss.dot_csr(F, Fb, metric=metric, alpha=0.3, weighted=True, dtype=dt)
            hi = ss.dot_csr(F, Fb, metric=metric, alpha=0.7, weighted=True, dtype=dt)
            keep = lo.data >= dt(0.7)
            rows = np.repeat(np.arange(n), np.diff(lo.indptr))
            ptr = np.concatenate([[0], np.cumsum(np.bincount(rows[keep], minlength=n))]).astype(np.int64)
            assert_csr_equal(hi, sp.csr_matrix((lo.data[keep], lo.indices[keep], ptr), shape=lo.shape))
            # two runs are bitwise equal; the device-input route gives the host-input route's bits
            assert_csr_equal(ss.dot_csr(F, Fb, metric=metric, alpha=0.3, weighted=True, dtype=dt), lo)
            p, i, v = ss.dot_csr(tensor(F, dt), None if Fb is None else tensor(Fb, dt), metric=metric, alpha=0.3,
                                 weighted=True, dtype=dt)
            assert_csr_equal(to_csr(p, i, v, lo.shape), lo)


# ----------------------------------------------------------------------------------------------- 2. exact inputs
@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("n,d", [(200, 9), (129, 300)])
def test_exactly_summable_inputs_are_bitwise_defined(n, d, dt):
    ss.init(0)
    X = R.integer_rows(n, d, seed=n + d)
    Z = R.integer_rows(n // 2 + 3, d, seed=n + d + 1)
    for metric in R.METRICS:
        e_sym = R.ref_exact(X, X, metric, dt, sym=True)
        e_x = R.ref_exact(X, Z, metric, dt)
        assert (e_sym == dt(0.5)).any() and (e_x == dt(0.5)).any()
        for alpha in (0.5, float(e_sym[3, 17]), 1.0, float(e_x[5, 2])):
            for weighted in (True, False):
                assert_csr_equal(ss.dot_csr(X, metric=metric, alpha=alpha, weighted=weighted, dtype=dt),
                                 ref_cut(e_sym, alpha, weighted, dt))
                assert_csr_equal(ss.dot_csr(X, Z, metric=metric, alpha=alpha, weighted=weighted, dtype=dt),
                                 ref_cut(e_x, alpha, weighted, dt))
        p, i, v = ss.dot_csr(tensor(X, dt), tensor(Z, dt), metric=metric, alpha=0.5, dtype=dt)
        assert_csr_equal(to_csr(p, i, v, e_x.shape), ref_cut(e_x, 0.5, True, dt))
        if metric != "cosine":     # duplicates are exactly 1
            D = ss.dot_csr(X, metric=metric, alpha=1.0, dtype=dt).toarray()
            assert D[n - 1, 3] == 1 and D[3, n - 2] == 1 and D[n // 2, n // 3] == 1


# ----------------------------------------------------------------------------------------------- 3. edge cases
@pytest.mark.parametrize("dt", DTYPES)
def test_edge_cases_of_the_rule(dt):
    ss.init(0)
    X = np.zeros((4, 6))
    X[2, :3] = [1.0, -2.0, 0.5]
    X[3, 3:] = [1.0, 1.0, 4.0]                   # rows 2 and 3 are orthogonal: s = 0
    for metric in R.METRICS:
        # alpha <= 0 unweighted keeps every pair, zero rows against non-zero rows and orthogonal rows included
        for alpha in (0.0, -0.5):
            assert (ss.dot_csr(X, metric=metric, alpha=alpha, weighted=False, dtype=dt).toarray() == 1).all()
        # weighted drops s = 0 (a stored zero is no edge)
        W = ss.dot_csr(X, metric=metric, alpha=-0.5, weighted=True, dtype=dt)
        Wd = W.toarray()
        assert W.nnz == 6 and (W.data == 1).all()
        assert Wd[0, 1] == 1 and Wd[1, 0] == 1 and Wd[0, 0] == 1          # zero with zero: 1
        assert Wd[0, 2] == 0 and Wd[2, 0] == 0 and Wd[1, 3] == 0          # zero with non-zero: 0
        assert Wd[2, 3] == 0 and Wd[2, 2] == 1 and Wd[3, 3] == 1          # orthogonal: 0
        # d = 0: every pair has s = 1
        E = np.zeros((5, 0))
        assert (ss.dot_csr(E, metric=metric, alpha=1.0, dtype=dt).toarray() == 1).all()
        assert (ss.dot_csr(E, np.zeros((3, 0)), metric=metric, alpha=0.5, dtype=dt).toarray() == 1).all()
        # opposite rows: cosine -1, kept at alpha = -1
        N = np.array([[3.0, 0.0, 4.0], [-3.0, 0.0, -4.0]])      # sqrt(25) * sqrt(25) is exact
        if metric == "cosine":
            got = ss.dot_csr(N, metric=metric, alpha=-1.0, dtype=dt).toarray()
            assert got[0, 1] == -1 and got[1, 0] == -1
    # infinite features: the NaN similarities are dropped, nothing stored is NaN
    Finf = np.array([[np.inf, 1.0], [1.0, 0.0], [0.0, 1.0], [2.0, 2.0]])
    for metric in R.METRICS:
        got = ss.dot_csr(Finf, metric=metric, alpha=-2.0, weighted=False, dtype=dt)
        assert not np.isnan(got.data).any() and got[0, 0] == 1 and got[1, 3] == 1
        assert got[0, 2] == 0                     # inf * 0 in g: s is NaN, dropped at any alpha


@pytest.mark.parametrize("dt", DTYPES)
def test_leading_dimension_larger_than_n_with_nan_padding(dt):
    import torch
    lib = ss.init(0)
    n, nb, d, lda, ldb = 300, 170, 9, 311, 200
    F, G = R.integer_rows(n, d, seed=1), R.integer_rows(nb, d, seed=2)
    A = np.full((d, lda), np.nan, dt)                  # column-major n x d with lda rows per column; padding is NaN
    A[:, :n] = F.T
    B = np.full((d, ldb), np.nan, dt)
    B[:, :nb] = G.T
    fn = getattr(lib, f"ss_similarity_dot_csr_{suffix(dt)}")
    ft = C.c_float if dt == np.float32 else C.c_double
    want = ref_cut(R.ref_exact(F, G, "tanimoto", dt), 0.3, True, dt)
    ptr = np.zeros(n + 1, np.int64)
    idx = np.zeros(want.nnz, np.int32)
    val = np.zeros(want.nnz, dt)
    nnz = C.c_int64(-1)
    assert fn(A.ctypes.data, n, lda, B.ctypes.data, nb, ldb, d, 1, ft(0.3), 1, ptr.ctypes.data, idx.ctypes.data,
              val.ctypes.data, want.nnz, C.byref(nnz), 0) == 0
    assert_csr_equal(sp.csr_matrix((val, idx, ptr), shape=(n, nb)), want)
    At = torch.from_numpy(A).cuda()
    want = ref_cut(R.ref_exact(F, F, "dice", dt, sym=True), 0.3, True, dt)
    pt = torch.zeros(n + 1, dtype=torch.int64, device="cuda")
    it = torch.zeros(want.nnz, dtype=torch.int32, device="cuda")
    vt = torch.zeros(want.nnz, dtype=At.dtype, device="cuda")
    assert fn(At.data_ptr(), n, lda, None, 0, 0, d, 2, ft(0.3), 1, pt.data_ptr(), it.data_ptr(), vt.data_ptr(), want.nnz,
              C.byref(nnz), 1) == 0
    assert nnz.value == want.nnz
    assert_csr_equal(to_csr(pt, it, vt, (n, n)), want)


@pytest.mark.parametrize("dt", DTYPES)
def test_nan_features_nan_alpha_and_bad_metric_are_refused_before_anything_is_written(dt):
    import torch
    lib = ss.init(0)
    fn = getattr(lib, f"ss_similarity_dot_csr_{suffix(dt)}")
    ft = C.c_float if dt == np.float32 else C.c_double
    F = np.asfortranarray(R.vectors(300, 20, seed=5, signed=True).astype(dt))
    ptr = np.full(301, -7, np.int64)
    idx = np.full(10, -7, np.int32)
    val = np.full(10, -7, dt)
    nnz = C.c_int64(-7)
    Fn = F.copy(order="F")
    Fn[299, 19] = np.nan                         # the last element
    for a, b, alpha, metric, word in ((Fn, None, 0.5, 0, "NaN"), (F, Fn, 0.5, 1, "NaN"), (F, None, float("nan"), 2, "NaN"),
                                      (F, None, 0.5, 3, "metric"), (F, None, 0.5, -1, "metric")):
        for out_idx in (None, idx.ctypes.data):
            rc = fn(a.ctypes.data, 300, 300, None if b is None else b.ctypes.data, 300, 300, 20, metric, ft(alpha), 1,
                    ptr.ctypes.data, out_idx, None if out_idx is None else val.ctypes.data, 10, C.byref(nnz), 0)
            assert rc == -1, rc
            assert word in lib.ss_last_error().decode()
    assert nnz.value == -7 and (ptr == -7).all() and (idx == -7).all() and (val == -7).all()
    # device memory
    Ft = torch.from_numpy(np.ascontiguousarray(Fn.T)).cuda()     # (d, n) row-major = column-major n x d
    pt = torch.full((301,), -7, dtype=torch.int64, device="cuda")
    assert fn(Ft.data_ptr(), 300, 300, None, 0, 0, 20, 0, ft(0.5), 1, pt.data_ptr(), None, None, 0, C.byref(nnz), 1) == -1
    assert nnz.value == -7 and (pt.cpu().numpy() == -7).all()
    for bad, alpha in ((np.ascontiguousarray(Fn), 0.5), (np.ascontiguousarray(F), float("nan"))):
        with pytest.raises(ss.SimSpreadError) as e:
            ss.dot_csr(bad, alpha=alpha, dtype=dt)
        assert e.value.code == -1
        with pytest.raises(ss.SimSpreadError) as e:
            ss.DeviceGraph.from_vectors(None, bad, np.eye(300, 4), alpha=alpha, dtype=dt)
        assert e.value.code == -1
        with pytest.raises(ss.SimSpreadError) as e:
            ss.DeviceGraph.from_vectors(np.ascontiguousarray(F[:7]), bad, np.eye(300, 4), alpha=alpha, metric="dice",
                                        dtype=dt)
        assert e.value.code == -1
    Yd = (torch.zeros(301, dtype=torch.int64, device="cuda"), torch.zeros(0, dtype=torch.int32, device="cuda"), None, 4)
    with pytest.raises(ss.SimSpreadError) as e:
        ss.DeviceGraph.from_vectors(None, tensor(Fn, dt), Yd, alpha=0.5, dtype=dt)
    assert e.value.code == -1
    with pytest.raises(ss.SimSpreadError) as e:
        ss.dot_csr(tensor(F, dt), tensor(Fn, dt), alpha=0.5, dtype=dt)
    assert e.value.code == -1
    # a bad metric through the graph constructor
    h = C.c_void_p()
    gfn = getattr(lib, f"ss_graph_create_vectors_{suffix(dt)}")
    yp = np.zeros(301, np.int64)
    assert gfn(0, 300, 4, 20, 7, None, 1, F.ctypes.data, 300, yp.ctypes.data, None, None, 0, ft(0.5), 1, 0,
               C.byref(h)) == -1
    assert h.value is None


# ----------------------------------------------------------------------------------------------- 4. the size protocol
def test_size_protocol_capacity_and_memory_kinds():
    import torch
    lib = ss.init(0)
    F = np.asfortranarray(R.vectors(700, 30, seed=3, signed=True, zero_rows=(2,)).astype(np.float32))
    fn = lib.ss_similarity_dot_csr_f32
    ptr = np.zeros(701, np.int64)
    nnz = C.c_int64(-1)
    assert fn(F.ctypes.data, 700, 700, None, 0, 0, 30, 0, C.c_float(0.3), 1, ptr.ctypes.data, None, None, 0,
              C.byref(nnz), 0) == 0
    want = ss.dot_csr(F, alpha=0.3)
    assert nnz.value == want.nnz > 0 and np.array_equal(ptr, want.indptr)
    # capacity too small: SS_EINVAL, nnz still reported, nothing written
    idx = np.full(nnz.value, -5, np.int32)
    val = np.full(nnz.value, -5, np.float32)
    nnz2 = C.c_int64(-1)
    rc = fn(F.ctypes.data, 700, 700, None, 0, 0, 30, 0, C.c_float(0.3), 1, ptr.ctypes.data, idx.ctypes.data,
            val.ctypes.data, nnz.value - 1, C.byref(nnz2), 0)
    assert rc == -1 and nnz2.value == nnz.value
    assert (idx == -5).all() and (val == -5).all()
    # val == NULL: the pattern only
    rc = fn(F.ctypes.data, 700, 700, None, 0, 0, 30, 0, C.c_float(0.3), 1, ptr.ctypes.data, idx.ctypes.data, None,
            nnz.value, C.byref(nnz2), 0)
    assert rc == 0 and np.array_equal(idx, want.indices) and (val == -5).all()
    # exact capacity
    rc = fn(F.ctypes.data, 700, 700, None, 0, 0, 30, 0, C.c_float(0.3), 1, ptr.ctypes.data, idx.ctypes.data,
            val.ctypes.data, nnz.value, C.byref(nnz2), 0)
    assert rc == 0
    assert_csr_equal(sp.csr_matrix((val, idx, ptr), shape=(700, 700)), want)
    # device memory: the same CSR, and run to run bitwise repeatable
    Ft = torch.from_numpy(np.ascontiguousarray(F)).cuda()
    for _ in range(2):
        p, i, v = ss.dot_csr(Ft, alpha=0.3)
        assert np.array_equal(p.cpu().numpy(), ptr)
        assert np.array_equal(i.cpu().numpy(), idx)
        assert np.array_equal(v.cpu().numpy().view(np.uint32), val.view(np.uint32))
    # argument checks return codes, they do not abort
    args = dict(F=F.ctypes.data, n=700, ld=700, d=30, ptr=ptr.ctypes.data)

    def call(**kw):
        a = dict(args, **kw)
        return fn(a["F"], a["n"], a["ld"], None, 0, 0, a["d"], 0, C.c_float(0.3), 1, a["ptr"], None, None, 0,
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
    rc = lib.ss_similarity_dot_csr_f32(Ft.data_ptr(), n, n, None, 0, 0, 1, 0, C.c_float(0.5), 1, ptr.data_ptr(), None,
                                       None, 0, C.byref(nnz), 1)
    assert rc == -5, rc
    assert nnz.value == n * n
    assert "2^31" in lib.ss_last_error().decode()
    assert (ptr.cpu().numpy() == -7).all()
    Y = (torch.zeros(n + 1, dtype=torch.int64, device="cuda"), torch.zeros(0, dtype=torch.int32, device="cuda"), None, 4)
    with pytest.raises(ss.SimSpreadError) as e:
        ss.DeviceGraph.from_vectors(None, Ft.t(), Y, alpha=0.5)
    assert e.value.code == -5


# ----------------------------------------------------------------------------------------------- 5. graphs
def _labels(ns, nt, seed):
    rng = np.random.default_rng(seed)
    Y = sp.random(ns, nt, density=4.0 / nt, random_state=rng, format="csr")
    Y.data[:] = 1.0
    return Y


@pytest.mark.parametrize("dt,tol", [(np.float32, 1e-5), (np.float64, 1e-12)])
@pytest.mark.parametrize("weighted", [True, False])
@pytest.mark.parametrize("metric,alpha", [("cosine", 0.6), ("tanimoto", 0.5)])
def test_graph_from_vectors_equals_the_graph_from_its_own_csr(metric, alpha, weighted, dt, tol):
    import torch
    from oracle import simspread_oracle as O
    ss.init(0)
    ns, nq, nt, d = 3000, 500, 300, 24
    Fs = R.vectors(ns, d, seed=11, signed=True, zero_rows=(4, 17))
    Fq = R.vectors(nq, d, seed=12, signed=True, zero_rows=(0,))
    Xs = ss.dot_csr(Fs, metric=metric, alpha=alpha, weighted=weighted, dtype=dt)
    Xq = ss.dot_csr(Fq, Fs, metric=metric, alpha=alpha, weighted=weighted, dtype=dt)
    assert 0.001 < Xs.nnz / ns / ns < 0.5
    Y = _labels(ns, nt, 13)

    g = ss.DeviceGraph.from_vectors(Fq, Fs, Y, alpha=alpha, metric=metric, weighted=weighted, dtype=dt)
    assert ss.path_last() == ["dot_csr_sym", "dot_csr_cross"]
    assert (g.nq, g.ns, g.nf, g.nt, g.nnz_xq, g.nnz_xs) == (nq, ns, ns, nt, Xq.nnz, Xs.nnz)
    r = ss.DeviceGraph.from_sparse(Xq, Xs, Y, dtype=dt)
    for rows in ("query", "source"):
        got, want = g.predict(rows), r.predict(rows)
        assert np.array_equal(got.view(np.uint8), want.view(np.uint8)), rows
        ref = O.predict_factored(Xq.astype(np.float64), Xs.astype(np.float64), Y, rows)
        assert np.abs(got - ref).max() <= tol * np.abs(ref).max(), rows
    # device-tensor inputs give the same graph
    Yd = (torch.from_numpy(Y.indptr.astype(np.int64)).cuda(), torch.from_numpy(Y.indices.astype(np.int32)).cuda(),
          None, nt)
    gd = ss.DeviceGraph.from_vectors(tensor(Fq, dt), tensor(Fs, dt), Yd, alpha=alpha, metric=metric, weighted=weighted,
                                     dtype=dt)
    assert (gd.nnz_xq, gd.nnz_xs) == (Xq.nnz, Xs.nnz)
    assert np.array_equal(gd.predict("query").view(np.uint8), g.predict("query").view(np.uint8))
    with pytest.raises(TypeError):
        ss.DeviceGraph.from_vectors(None, tensor(Fs, dt).to(torch.float16), Yd, alpha=alpha, metric=metric, dtype=dt)

    g3 = ss.DeviceGraph.from_vectors(None, Fs, Y, alpha=alpha, metric=metric, weighted=weighted, dtype=dt)
    assert ss.path_last() == ["dot_csr_sym"]
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


# ----------------------------------------------------------------------------------------------- 6. recut
@pytest.mark.parametrize("dt", DTYPES)
def test_recut_of_a_vector_graph_equals_a_fresh_graph(dt):
    ss.init(0)
    ns, nq, nt, d = 1500, 200, 100, 16
    Fs = R.vectors(ns, d, seed=21, signed=True, zero_rows=(3,))
    Fq = R.vectors(nq, d, seed=22, signed=True)
    Y = _labels(ns, nt, 23)
    parent = ss.DeviceGraph.from_vectors(Fq, Fs, Y, alpha=0.4, metric="cosine", weighted=True, dtype=dt)
    child = parent.recut(0.7)
    fresh = ss.DeviceGraph.from_vectors(Fq, Fs, Y, alpha=0.7, metric="cosine", weighted=True, dtype=dt)
    assert fresh.nnz_xs < parent.nnz_xs
    assert (child.nq, child.ns, child.nf, child.nt, child.nnz_xq, child.nnz_xs) == \
           (fresh.nq, fresh.ns, fresh.nf, fresh.nt, fresh.nnz_xq, fresh.nnz_xs)
    for a, b in zip(child.degrees(), fresh.degrees()):
        assert np.array_equal(a, b)
    for rows in ("query", "source"):
        assert np.array_equal(child.predict(rows).view(np.uint8), fresh.predict(rows).view(np.uint8))
    # leave-one-out needs the 3-layer graph
    parent3 = ss.DeviceGraph.from_vectors(None, Fs, Y, alpha=0.4, metric="cosine", weighted=True, dtype=dt)
    child3 = parent3.recut(0.7)
    fresh3 = ss.DeviceGraph.from_vectors(None, Fs, Y, alpha=0.7, metric="cosine", weighted=True, dtype=dt)
    assert child3.nnz_xs == fresh3.nnz_xs == fresh.nnz_xs
    assert np.array_equal(child3.predict_loo(clean=True).view(np.uint8), fresh3.predict_loo(clean=True).view(np.uint8))


# ----------------------------------------------------------------------------------------------- 7. many tiles
def test_20k_by_32_clustered_fp32_cosine():
    import torch
    ss.init(0)
    n, d, alpha = 20_000, 32, 0.965     # members of a cluster are >= 0.99 similar, of different clusters <= 0.94
    X, member = R.clustered_features(n, d, clusters=50, seed=2027)
    p, i, v = ss.dot_csr(torch.from_numpy(X).cuda(), metric="cosine", alpha=alpha, weighted=True, dtype=np.float32)
    torch.cuda.synchronize()
    sizes = np.bincount(member)
    implied = int((sizes.astype(np.int64) ** 2).sum())
    nnz = int(i.numel())
    assert 0.99 * implied <= nnz <= 1.01 * implied, (nnz, implied)
    A = to_csr(p, i, v, (n, n))
    check_structure(A, True, alpha)     # symmetry of the whole CSR, pattern and bits
    rows = R.sample_rows(n, 128, 9)
    s64 = R.ref_s64(X[rows], X, "cosine", np.float32)
    s64[np.arange(len(rows)), rows] = 1.0
    check_band(A[rows], s64, alpha, True, np.float32, d)
