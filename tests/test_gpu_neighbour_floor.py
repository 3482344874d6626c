"""The neighbour floor on the device (include/simspread_hip_neighbours.h): tau, the floor CSR, the graph and the query
sets, each bitwise against the host reference of the rule (tests/neighbour_ref.py).

The shapes are the smallest that reach every branch: n = 300, d = 167 is three 128-tiles with a ragged edge and
nwords = 3 (no multiple of the 8-word staging step); the forced rows give rows with fewer than k positives, ties at the
k-th value, rows with more than k entries, an asymmetric output and, at alpha = 0.7, rows the floor adds to and rows it
leaves alone (tests/test_neighbour_floor_cpu.py checks that the reference has them)."""
import ctypes as C
import functools

import numpy as np
import pytest
import scipy.sparse as sp

import neighbour_ref as R
import simspread_jl_amd as ss
from simspread_jl_amd import _lib

pytestmark = pytest.mark.gpu

DTYPES = [np.float32, np.float64]
KS = [1, 5, 33, 64]
ALPHAS = [0.7, np.inf]
EINVAL = -1
N, D, NQ, NT = 300, 167, 70, 23


def _suf(dt):
    return "f32" if np.dtype(dt) == np.float32 else "f64"


def _ct(dt):
    return C.c_float if np.dtype(dt) == np.float32 else C.c_double


def assert_same(a, b, what=""):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    assert a.shape == b.shape and a.dtype == b.dtype, what
    assert np.array_equal(a.view(np.uint8), b.view(np.uint8)), what


@functools.lru_cache(maxsize=None)
def _sets():
    """(Fs, Fq): the 300 sources of the case matrix and 70 queries: some near the sources, one all-zero, one a copy"""
    bits = R.case_bits(N, D)
    q = R.base_bits(NQ, D, seed=977)
    rng = np.random.default_rng(5)
    q[:30] = bits[rng.integers(0, N, 30)] ^ (rng.random((30, D)) < 0.05)
    q[3] = False
    q[4] = bits[7]
    return ss.pack_fingerprints(bits), ss.pack_fingerprints(q)


@functools.lru_cache(maxsize=None)
def _sims(dt):
    """(s_sym, s_cross) of the case matrix in precision dt, computed once"""
    Fs, Fq = _sets()
    s_sym, s_x = R.ref_similarity(Fs, None, dt), R.ref_similarity(Fq, Fs, dt)
    s_sym.setflags(write=False)
    s_x.setflags(write=False)
    return s_sym, s_x


@functools.lru_cache(maxsize=None)
def _labels():
    rng = np.random.default_rng(3)
    Y = sp.random(N, NT, density=0.15, format="csr", random_state=rng)
    Y.data[:] = 1.0
    Y.sort_indices()
    return Y


def _dev(F):
    import torch
    return None if F is None else torch.from_numpy(np.ascontiguousarray(F).view(np.int64)).cuda()


def _tau(Fa, Fb, k, dt, dev):
    if not dev:
        return ss.tanimoto_kth(Fa, Fb, k=k, dtype=dt)
    return ss.tanimoto_kth(_dev(Fa), _dev(Fb), k=k, dtype=dt).cpu().numpy()


def _floor(Fa, Fb, alpha, k, weighted, dt, dev):
    if not dev:
        return ss.tanimoto_csr(Fa, Fb, alpha=alpha, weighted=weighted, dtype=dt, min_neighbours=k)
    p, i, v = ss.tanimoto_csr(_dev(Fa), _dev(Fb), alpha=alpha, weighted=weighted, dtype=dt, min_neighbours=k)
    nb = (Fa if Fb is None else Fb).shape[0]
    return sp.csr_matrix((v.cpu().numpy(), i.cpu().numpy(), p.cpu().numpy()), shape=(Fa.shape[0], nb))


# ------------------------------------------------------------------------------------------------ 1. case matrix
@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("k", KS)
def test_tau_and_floor_csr_match_the_reference(k, dt):
    ss.init(0)
    Fs, Fq = _sets()
    s_sym, s_x = _sims(dt)
    tau_sym, tau_x = R.ref_kth(s_sym, k), R.ref_kth(s_x, k)
    for dev in (False, True):
        assert_same(_tau(Fs, None, k, dt, dev), tau_sym, ("tau sym", dev))
        assert ss.path_last() == ["tanimoto_kth"]
        assert_same(_tau(Fq, Fs, k, dt, dev), tau_x, ("tau cross", dev))
        for alpha in ALPHAS:
            for weighted in (True, False):
                R.assert_csr_equal(_floor(Fs, None, alpha, k, weighted, dt, dev), R.ref_floor(s_sym, alpha, k, weighted))
                assert ss.path_last() == ["tanimoto_csr_floor_sym"]
                R.assert_csr_equal(_floor(Fq, Fs, alpha, k, weighted, dt, dev), R.ref_floor(s_x, alpha, k, weighted))
                assert ss.path_last() == ["tanimoto_csr_floor_cross"]


# ------------------------------------------------------------------------------------ 2. column groups and the merge
@functools.lru_cache(maxsize=None)
def _wide():
    """70 rows against 2000 columns of 70 bits (16 column tiles: four groups of four) with heavy ties"""
    rows = R.base_bits(NQ, 70, seed=11)
    cols = R.base_bits(2000, 70, seed=12)
    cols[100:140] = rows[9]                    # 40 exact copies of one row, spread over two groups
    cols[1500:1520] = rows[9]
    rows[2] = False
    cols[[0, 777, 1999]] = False
    return ss.pack_fingerprints(rows), ss.pack_fingerprints(cols)


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("nb", [2000, 129])
def test_column_groups_and_merge(nb, dt):
    ss.init(0)
    Fa, Fb = _wide()
    Fb = Fb[:nb]
    s = R.ref_similarity(Fa, Fb, dt)
    for k in (5, 64):
        assert_same(_tau(Fa, Fb, k, dt, False), R.ref_kth(s, k), (nb, k))
        R.assert_csr_equal(_floor(Fa, Fb, np.inf, k, True, dt, False), R.ref_floor(s, np.inf, k, True))


# ------------------------------------------------------------------------------------------------ 3. k = 0
def _raw_floor_csr(Fa, Fb, alpha, k, weighted, dt):
    """ss_similarity_tanimoto_floor_csr_* itself, host arrays, by the size protocol"""
    fn = getattr(_lib.lib(), f"ss_similarity_tanimoto_floor_csr_{_suf(dt)}")
    na, nw = Fa.shape
    nb = na if Fb is None else Fb.shape[0]
    pb = None if Fb is None else Fb.ctypes.data
    ptr, nnz = np.zeros(na + 1, np.int64), C.c_int64(-1)
    head = (Fa.ctypes.data, na, pb, nb, nw, _ct(dt)(alpha), k, 1 if weighted else 0)
    _lib.check(fn(*head, ptr.ctypes.data, None, None, 0, C.byref(nnz), _lib.SS_MEM_HOST))
    idx, val = np.empty(max(nnz.value, 1), np.int32), np.empty(max(nnz.value, 1), dt)
    _lib.check(fn(*head, ptr.ctypes.data, idx.ctypes.data, val.ctypes.data, nnz.value, C.byref(nnz), _lib.SS_MEM_HOST))
    return sp.csr_matrix((val[:nnz.value], idx[:nnz.value], ptr), shape=(na, nb))


def _raw_graph(Fq, Fs, Y, alpha, k, weighted, dt):
    fn = getattr(_lib.lib(), f"ss_graph_create_fingerprint_floor_{_suf(dt)}")
    Y = sp.csr_matrix(Y)
    yp, yi, yv = Y.indptr.astype(np.int64), Y.indices.astype(np.int32), Y.data.astype(dt)
    h = C.c_void_p()
    nq = 0 if Fq is None else Fq.shape[0]
    _lib.check(fn(nq, Fs.shape[0], Y.shape[1], Fs.shape[1], None if Fq is None else Fq.ctypes.data, Fs.ctypes.data,
                  yp.ctypes.data, yi.ctypes.data, yv.ctypes.data, 0, _ct(dt)(alpha), k, 1 if weighted else 0,
                  _lib.SS_MEM_HOST, C.byref(h)))
    return ss.DeviceGraph(h, np.dtype(dt).type)


def _raw_queries(g, Fq, Fs, alpha, k, weighted):
    fn = getattr(_lib.lib(), f"ss_queries_create_fingerprint_floor_{_suf(g.dtype)}")
    h = C.c_void_p()
    _lib.check(fn(g._h, Fq.shape[0], Fs.shape[0], Fs.shape[1], Fq.ctypes.data, Fs.ctypes.data, _ct(g.dtype)(alpha), k,
                  1 if weighted else 0, _lib.SS_MEM_HOST, C.byref(h)))
    return ss.DeviceQueries(h, g)


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("n", [1, 63, 129])
def test_k0_is_the_plain_producer(n, dt):
    ss.init(0)
    Fs, Fq = _sets()
    Fs, Fq = np.ascontiguousarray(Fs[:n]), np.ascontiguousarray(Fq[:max(1, n // 2)])
    Y = _labels()[:n]
    for weighted in (True, False):
        want = ss.tanimoto_csr(Fs, alpha=0.3, weighted=weighted, dtype=dt)
        R.assert_csr_equal(_raw_floor_csr(Fs, None, 0.3, 0, weighted, dt), want)
        assert ss.path_last() == ["tanimoto_csr_sym"]
        want = ss.tanimoto_csr(Fq, Fs, alpha=0.3, weighted=weighted, dtype=dt)
        R.assert_csr_equal(_raw_floor_csr(Fq, Fs, 0.3, 0, weighted, dt), want)
        assert ss.path_last() == ["tanimoto_csr_cross"]
    plain = ss.DeviceGraph.from_fingerprints(Fq, Fs, Y, 0.3, dtype=dt)
    tags = ss.path_last()
    g0 = _raw_graph(Fq, Fs, Y, 0.3, 0, True, dt)
    assert ss.path_last() == tags == ["tanimoto_csr_sym", "tanimoto_csr_cross"]
    assert (g0.nnz_xq, g0.nnz_xs) == (plain.nnz_xq, plain.nnz_xs)
    assert_same(g0.predict("query", clean=True), plain.predict("query", clean=True))
    if n > 1:        # leave-one-out runs on the graph without queries
        assert_same(_raw_graph(None, Fs, Y, 0.3, 0, True, dt).predict_loo(),
                    ss.DeviceGraph.from_fingerprints(None, Fs, Y, 0.3, dtype=dt).predict_loo())
    q_plain = ss.DeviceQueries.from_fingerprints(plain, Fq, Fs, 0.3)
    q0 = _raw_queries(plain, Fq, Fs, 0.3, 0, True)
    assert ss.path_last() == ["tanimoto_csr_cross"]
    assert np.array_equal(q0.degrees(), q_plain.degrees())
    assert_same(plain.predict(queries=q0), plain.predict(queries=q_plain))


# ------------------------------------------------------------------------------------------------ 4. graph
@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("k,alpha,weighted", [(5, 0.7, True), (33, np.inf, False)])
def test_floor_graph_is_the_csr_graph_of_the_reference_blocks(k, alpha, weighted, dt):
    ss.init(0)
    Fs, Fq = _sets()
    s_sym, s_x = _sims(dt)
    Y = _labels()
    Xs, Xq = R.ref_floor(s_sym, alpha, k, weighted), R.ref_floor(s_x, alpha, k, weighted)
    want = ss.DeviceGraph.from_sparse(Xq, Xs, Y, dtype=dt)
    got = ss.DeviceGraph.from_fingerprints(Fq, Fs, Y, alpha, weighted=weighted, dtype=dt, min_neighbours=k)
    assert ss.path_last() == ["tanimoto_csr_floor_sym", "tanimoto_csr_floor_cross"]
    info = lambda g: (g.nq, g.ns, g.nf, g.nt, g.nnz_xq, g.nnz_xs, g.nnz_ys)
    assert info(got) == info(want) == (NQ, N, N, NT, Xq.nnz, Xs.nnz, Y.nnz)
    for a, b in zip(got.degrees(), want.degrees()):
        assert np.array_equal(a, b)
    for clean in (False, True):
        assert_same(got.predict("query", clean=clean), want.predict("query", clean=clean))
        assert_same(got.predict("source", clean=clean), want.predict("source", clean=clean))
    # leave-one-out runs on the graph without queries: all 300 folds
    want0 = ss.DeviceGraph.from_sparse(None, Xs, Y, dtype=dt)
    got0 = ss.DeviceGraph.from_fingerprints(None, Fs, Y, alpha, weighted=weighted, dtype=dt, min_neighbours=k)
    assert ss.path_last() == ["tanimoto_csr_floor_sym"]
    for clean in (False, True):
        assert_same(got0.predict_loo(clean=clean), want0.predict_loo(clean=clean))
    # device inputs build the same graph
    import torch
    Yd = (torch.from_numpy(Y.indptr.astype(np.int64)).cuda(), torch.from_numpy(Y.indices.astype(np.int32)).cuda(),
          torch.from_numpy(Y.data.astype(dt)).cuda(), NT)
    dev = ss.DeviceGraph.from_fingerprints(_dev(Fq), _dev(Fs), Yd, alpha, weighted=weighted, dtype=dt, min_neighbours=k)
    assert info(dev) == info(want)
    assert_same(dev.predict("query", clean=True), want.predict("query", clean=True))


# ------------------------------------------------------------------------------------------------ 5. query sets
@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("floor_graph", [False, True])
def test_floor_query_sets(floor_graph, dt):
    ss.init(0)
    k, alpha = 5, 0.7
    Fs, Fq = _sets()
    s_sym, s_x = _sims(dt)
    Y = _labels()
    Xq = R.ref_floor(s_x, alpha, k, True)
    Xs = R.ref_floor(s_sym, alpha, k if floor_graph else 0, True)
    fresh = ss.DeviceGraph.from_sparse(Xq, Xs, Y, dtype=dt)
    g = ss.DeviceGraph.from_fingerprints(None, Fs, Y, alpha, dtype=dt, min_neighbours=k if floor_graph else 0)
    info = lambda g: (g.nq, g.ns, g.nf, g.nt, g.nnz_xq, g.nnz_xs, g.nnz_ys)
    before = (info(g), g.degrees(), g.predict_loo(0, 40, clean=True))
    for dev in (False, True):
        q = ss.DeviceQueries.from_fingerprints(g, _dev(Fq) if dev else Fq, _dev(Fs) if dev else Fs, alpha,
                                               min_neighbours=k)
        assert ss.path_last() == ["tanimoto_csr_floor_cross"]
        assert (q.nq, q.nf, q.nnz) == (NQ, N, Xq.nnz)
        kq = q.degrees()
        assert np.array_equal(kq, np.diff(Xq.indptr))
        assert (kq >= np.minimum(k, R.positives(s_x))).all()        # nobody with a positive similarity is left out
        for clean in (False, True):
            assert_same(g.predict(clean=clean, queries=q), fresh.predict("query", clean=clean))
        assert_same(g.predict(row_begin=63, row_end=66, queries=q), fresh.predict("query", 63, 66))
        q.close()
    # the plain cut leaves queries without neighbours that the floor serves
    q_plain = ss.DeviceQueries.from_fingerprints(g, Fq, Fs, alpha)
    assert ((q_plain.degrees() == 0) & (R.positives(s_x) > 0)).any()
    after = (info(g), g.degrees(), g.predict_loo(0, 40, clean=True))
    assert before[0] == after[0]
    for a, b in zip(before[1], after[1]):
        assert np.array_equal(a, b)
    assert_same(before[2], after[2])


# ------------------------------------------------------------------------------------------------ 6. protocol
@pytest.mark.parametrize("dt", DTYPES)
def test_protocol_and_refusals(dt):
    ss.init(0)
    lib = _lib.lib()
    Fs, Fq = _sets()
    s_x = _sims(dt)[1]
    k, alpha = 5, 0.7
    want = R.ref_floor(s_x, alpha, k, True)
    csr = getattr(lib, f"ss_similarity_tanimoto_floor_csr_{_suf(dt)}")
    kth = getattr(lib, f"ss_similarity_tanimoto_kth_{_suf(dt)}")
    head = (Fq.ctypes.data, NQ, Fs.ctypes.data, N, Fs.shape[1])
    H = _lib.SS_MEM_HOST

    # size query, then a capacity that is too small: SS_EINVAL with *nnz set and idx / val untouched
    ptr, nnz = np.full(NQ + 1, -7, np.int64), C.c_int64(-1)
    _lib.check(csr(*head, _ct(dt)(alpha), k, 1, ptr.ctypes.data, None, None, 0, C.byref(nnz), H))
    assert nnz.value == want.nnz and np.array_equal(ptr, want.indptr)
    idx, val = np.full(want.nnz, -7, np.int32), np.full(want.nnz, -7, dt)
    nnz = C.c_int64(-1)
    assert csr(*head, _ct(dt)(alpha), k, 1, ptr.ctypes.data, idx.ctypes.data, val.ctypes.data, want.nnz - 1,
               C.byref(nnz), H) == EINVAL
    assert nnz.value == want.nnz and (idx == -7).all() and (val == -7).all()

    # bad k and NaN alpha: SS_EINVAL, nothing written, *out == NULL
    Y = _labels()
    yp, yi, yv = Y.indptr.astype(np.int64), Y.indices.astype(np.int32), Y.data.astype(dt)
    gcreate = getattr(lib, f"ss_graph_create_fingerprint_floor_{_suf(dt)}")
    qcreate = getattr(lib, f"ss_queries_create_fingerprint_floor_{_suf(dt)}")
    g = ss.DeviceGraph.from_fingerprints(None, Fs, Y, alpha, dtype=dt)
    for bad_k, bad_alpha in ((-1, alpha), (65, alpha), (5, np.nan), (0, np.nan)):
        ptr, nnz = np.full(NQ + 1, -7, np.int64), C.c_int64(-7)
        assert csr(*head, _ct(dt)(bad_alpha), bad_k, 1, ptr.ctypes.data, idx.ctypes.data, val.ctypes.data, want.nnz,
                   C.byref(nnz), H) == EINVAL
        assert (ptr == -7).all() and nnz.value == -7 and (idx == -7).all() and (val == -7).all()
        h = C.c_void_p(1)
        assert gcreate(NQ, N, NT, Fs.shape[1], Fq.ctypes.data, Fs.ctypes.data, yp.ctypes.data, yi.ctypes.data,
                       yv.ctypes.data, 0, _ct(dt)(bad_alpha), bad_k, 1, H, C.byref(h)) == EINVAL
        assert not h.value
        h = C.c_void_p(1)
        assert qcreate(g._h, NQ, N, Fs.shape[1], Fq.ctypes.data, Fs.ctypes.data, _ct(dt)(bad_alpha), bad_k, 1, H,
                       C.byref(h)) == EINVAL
        assert not h.value
    for bad_k in (-1, 0, 65):
        tau = np.full(NQ, -7, dt)
        assert kth(*head, bad_k, tau.ctypes.data, H) == EINVAL
        assert (tau == -7).all()

    # na == 0 and nb == 0
    tau = np.full(NQ, -7, dt)
    _lib.check(kth(Fq.ctypes.data, 0, Fs.ctypes.data, N, Fs.shape[1], k, tau.ctypes.data, H))
    assert (tau == -7).all()
    _lib.check(kth(Fq.ctypes.data, NQ, Fs.ctypes.data, 0, Fs.shape[1], k, tau.ctypes.data, H))
    assert_same(tau, np.zeros(NQ, dt))
    ptr, nnz = np.full(NQ + 1, -7, np.int64), C.c_int64(-1)
    _lib.check(csr(Fq.ctypes.data, NQ, Fs.ctypes.data, 0, Fs.shape[1], _ct(dt)(alpha), k, 1, ptr.ctypes.data, None, None,
                   0, C.byref(nnz), H))
    assert nnz.value == 0 and (ptr == 0).all()
    ptr, nnz = np.full(1, -7, np.int64), C.c_int64(-1)
    _lib.check(csr(Fq.ctypes.data, 0, Fs.ctypes.data, N, Fs.shape[1], _ct(dt)(alpha), k, 1, ptr.ctypes.data, None, None,
                   0, C.byref(nnz), H))
    assert nnz.value == 0 and ptr[0] == 0

    # two runs give identical bytes
    a, b = _floor(Fs, None, alpha, 33, True, dt, False), _floor(Fs, None, alpha, 33, True, dt, False)
    R.assert_csr_equal(a, b)
    assert_same(_tau(Fs, None, 33, dt, False), _tau(Fs, None, 33, dt, False))
