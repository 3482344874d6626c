"""The neighbour floor of the real-valued producers on the device (include/simspread_hip_neighbours_real.h): tau, the
floor CSR, the graphs and the query sets of the weighted-Jaccard and the inner-product producers, every comparison
bitwise.  Jaccard is bitwise defined by its sequential sums; the dot producer on integer-valued rows, where g, A and B
are exact in any order (tests/real_floor_ref.py).  On general real rows the dot floor is pinned against the plain cross
producer, whose code this feature leaves alone: selection, floor emit and plain emit must compute the same s.

The shapes are the smallest at which each mechanism can fail: n = 300 is three row and column tiles with a ragged last
tile of 44, d = 37 three staging steps with a ragged last one (odd against both MFMA k-steps), k = 33 crosses the fp64
rows-per-block switch, 3 x 1100 and 130 x 2000 give several column groups to merge.  tests/test_real_floor_cpu.py checks
that the reference inputs have short rows, ties, gained and untouched rows and an asymmetric result."""
import ctypes as C
import functools
import os

import numpy as np
import pytest
import scipy.sparse as sp

import dot_ref
import real_floor_ref as R
import simspread_jl_amd as ss
from simspread_jl_amd import _lib
from simspread_jl_amd.engine import SIM_METRICS

pytestmark = pytest.mark.gpu

DTYPES = [np.float32, np.float64]
EINVAL = -1
N, NQ, D, NT = R.N, R.NQ, R.D, 23
JACCARD = ("jaccard", None)
PRODUCERS = [JACCARD] + [("dot", m) for m in dot_ref.METRICS]
IDS = ["jaccard"] + list(dot_ref.METRICS)


def _suf(dt):
    return "f32" if np.dtype(dt) == np.float32 else "f64"


def _ct(dt):
    return C.c_float if np.dtype(dt) == np.float32 else C.c_double


def assert_same(a, b, what=""):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    assert a.shape == b.shape and a.dtype == b.dtype, what
    assert np.array_equal(a.view(np.uint8), b.view(np.uint8)), what


def _rows(P):
    """(sources, queries) of producer P's case matrix"""
    return (R.feature_rows(), R.feature_queries()) if P == JACCARD else (R.integer_sources(), R.integer_queries())


def _dense(P, A, B, dt):
    return R.jaccard_s(A, B, dt) if P == JACCARD else R.dot_s(A, B, P[1], dt)


@functools.lru_cache(maxsize=None)
def _sims(P, dt):
    """(s_sym, s_cross) of producer P's case matrix in precision dt, computed once"""
    Fs, Fq = _rows(P)
    s_sym, s_x = _dense(P, Fs, None, dt), _dense(P, Fq, Fs, dt)
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


def _dev(F, dt):
    import torch
    return None if F is None else torch.from_numpy(np.array(F, dtype=dt, order="C")).cuda()


def _tau(P, Fa, Fb, k, dt, dev=False):
    a, b = (_dev(Fa, dt), _dev(Fb, dt)) if dev else (Fa, Fb)
    t = ss.jaccard_kth(a, b, k=k, dtype=dt) if P == JACCARD else ss.dot_kth(a, b, metric=P[1], k=k, dtype=dt)
    return t.cpu().numpy() if dev else t


def _csr(P, Fa, Fb, alpha, k, weighted, dt, dev=False):
    """jaccard_csr / dot_csr with min_neighbours = k (k = 0: the plain entry point)"""
    a, b = (_dev(Fa, dt), _dev(Fb, dt)) if dev else (Fa, Fb)
    kw = dict(alpha=alpha, weighted=weighted, dtype=dt, min_neighbours=k)
    out = ss.jaccard_csr(a, b, **kw) if P == JACCARD else ss.dot_csr(a, b, metric=P[1], **kw)
    if not dev:
        return out
    p, i, v = out
    nb = (Fa if Fb is None else Fb).shape[0]
    return sp.csr_matrix((v.cpu().numpy(), i.cpu().numpy(), p.cpu().numpy()), shape=(Fa.shape[0], nb))


def _graph(P, Fq, Fs, Y, alpha, k, weighted, dt):
    if P == JACCARD:
        return ss.DeviceGraph.from_features(Fq, Fs, Y, alpha, weighted=weighted, dtype=dt, min_neighbours=k)
    return ss.DeviceGraph.from_vectors(Fq, Fs, Y, alpha, metric=P[1], weighted=weighted, dtype=dt, min_neighbours=k)


def _queries(P, g, Fq, Fs, alpha, k):
    if P == JACCARD:
        return ss.DeviceQueries.from_features(g, Fq, Fs, alpha, min_neighbours=k)
    return ss.DeviceQueries.from_vectors(g, Fq, Fs, alpha, metric=P[1], min_neighbours=k)


def _tags(P, floor):
    stem = "jaccard_csr" if P == JACCARD else "dot_csr"
    return [f"{stem}{'_floor' if floor else ''}_sym", f"{stem}{'_floor' if floor else ''}_cross"]


def _kth_tag(P):
    return ["jaccard_kth"] if P == JACCARD else ["dot_kth"]


# ------------------------------------------------------------------------------------------------ 1. case matrix
@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("k", R.KS)
@pytest.mark.parametrize("P", PRODUCERS, ids=IDS)
def test_tau_and_floor_csr_match_the_reference(P, k, dt):
    ss.init(0)
    Fs, Fq = _rows(P)
    s_sym, s_x = _sims(P, dt)
    tau_sym, tau_x = R.ref_kth(s_sym, k), R.ref_kth(s_x, k)
    sym_tag, cross_tag = _tags(P, True)
    for dev in (False, True):
        assert_same(_tau(P, Fs, None, k, dt, dev), tau_sym, ("tau sym", dev))
        assert ss.path_last() == _kth_tag(P)
        assert_same(_tau(P, Fq, Fs, k, dt, dev), tau_x, ("tau cross", dev))
        for alpha in R.ALPHAS:
            for weighted in (True, False):
                R.assert_csr_equal(_csr(P, Fs, None, alpha, k, weighted, dt, dev), R.ref_floor(s_sym, alpha, k, weighted))
                assert ss.path_last() == [sym_tag]
                R.assert_csr_equal(_csr(P, Fq, Fs, alpha, k, weighted, dt, dev), R.ref_floor(s_x, alpha, k, weighted))
                assert ss.path_last() == [cross_tag]


# ------------------------------------------------------------------------------------ 2. column groups and the merge
@functools.lru_cache(maxsize=None)
def _wide(P):
    """130 rows against 2000 columns (16 column tiles) with heavy ties; the first 3 rows x 1100 columns (9 tiles) are
    the three-groups-for-three-rows case"""
    if P == JACCARD:
        from test_gpu_jaccard_csr import features
        rows, cols = features(NQ, D, 21), features(2000, D, 22)
    else:
        rows, cols = dot_ref.integer_rows(NQ, D, 21), dot_ref.integer_rows(2000, D, 22)
    cols[100:140] = rows[2]                    # 40 exact copies of one row, then 20 more ten tiles on
    cols[1500:1520] = rows[2]
    rows[1] = 0
    cols[[0, 777, 1999]] = 0
    return rows, cols


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("na,nb", [(3, 1100), (130, 2000)])
@pytest.mark.parametrize("P", [JACCARD, ("dot", "cosine")], ids=["jaccard", "cosine"])
def test_column_groups_and_merge(P, na, nb, dt):
    ss.init(0)
    Fa, Fb = _wide(P)
    Fa, Fb = np.ascontiguousarray(Fa[:na]), np.ascontiguousarray(Fb[:nb])
    s = _dense(P, Fa, Fb, dt)
    for k in (5, 64):
        assert_same(_tau(P, Fa, Fb, k, dt), R.ref_kth(s, k), (na, nb, k))
        R.assert_csr_equal(_csr(P, Fa, Fb, np.inf, k, True, dt), R.ref_floor(s, np.inf, k, True))


# --------------------------------------------------------------------- 3. general real data for the dot producer
@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("metric", dot_ref.METRICS)
def test_dot_floor_on_real_data_sees_the_s_of_the_plain_cross_producer(metric, dt):
    """No independent bitwise reference exists for real-valued rows (the order of the Gram sums is the device's own), so
    the dense S comes from the plain cross producer, called with Fb given explicitly at alpha = -2: a missing entry is
    an exact 0.  For the self case the diagonal is set to 1.  tau and the floor CSR must equal the host rule on S."""
    ss.init(0)
    P = ("dot", metric)
    F = dot_ref.vectors(N, D, 17, signed=True, zero_rows=(0, 5))
    Q = dot_ref.vectors(NQ, D, 18, signed=True, zero_rows=(3,))
    S_self = np.ascontiguousarray(ss.dot_csr(F, F.copy(), metric=metric, alpha=-2.0, weighted=True, dtype=dt).toarray())
    assert ss.path_last() == ["dot_csr_cross"]
    np.fill_diagonal(S_self, dt(1))
    S_x = np.ascontiguousarray(ss.dot_csr(Q, F, metric=metric, alpha=-2.0, weighted=True, dtype=dt).toarray())
    assert S_self.dtype == dt and (S_self < 0).any()
    for k in (5, 33, 64):
        assert_same(_tau(P, F, None, k, dt), R.ref_kth(S_self, k), ("self", k))
        assert_same(_tau(P, Q, F, k, dt), R.ref_kth(S_x, k), ("cross", k))
        for alpha, weighted in ((0.7, True), (np.inf, True), (-0.5, True), (0.7, False)):
            R.assert_csr_equal(_csr(P, F, None, alpha, k, weighted, dt), R.ref_floor(S_self, alpha, k, weighted))
            R.assert_csr_equal(_csr(P, Q, F, alpha, k, weighted, dt), R.ref_floor(S_x, alpha, k, weighted))


# ------------------------------------------------------------------------------------------------ 4. k = 0
def _feature_args(F, dt, keep):
    """(pointer, rows, ld) of host rows in the library's column-major layout"""
    if F is None:
        return None, 0, 1
    a = np.asfortranarray(F, dtype=dt)
    keep.append(a)
    return a.ctypes.data, a.shape[0], max(a.shape[0], 1)


def _mid(P):
    return () if P == JACCARD else (SIM_METRICS[P[1]],)


def _raw_floor_csr(P, Fa, Fb, alpha, k, weighted, dt):
    """ss_similarity_{jaccard,dot}_floor_csr_* itself, host arrays, by the size protocol"""
    fn = getattr(_lib.lib(), f"ss_similarity_{P[0]}_floor_csr_{_suf(dt)}")
    keep = []
    pa, na, lda = _feature_args(Fa, dt, keep)
    pb, nb, ldb = _feature_args(Fb, dt, keep)
    if Fb is None:
        nb, ldb = na, lda
    ptr, nnz = np.zeros(na + 1, np.int64), C.c_int64(-1)
    head = (pa, na, lda, pb, nb, ldb, Fa.shape[1]) + _mid(P) + (_ct(dt)(alpha), k, 1 if weighted else 0)
    _lib.check(fn(*head, ptr.ctypes.data, None, None, 0, C.byref(nnz), _lib.SS_MEM_HOST))
    idx, val = np.empty(max(nnz.value, 1), np.int32), np.empty(max(nnz.value, 1), dt)
    _lib.check(fn(*head, ptr.ctypes.data, idx.ctypes.data, val.ctypes.data, nnz.value, C.byref(nnz), _lib.SS_MEM_HOST))
    return sp.csr_matrix((val[:nnz.value], idx[:nnz.value], ptr), shape=(na, nb))


def _label_args(Y, dt):
    Y = sp.csr_matrix(Y)
    return Y.indptr.astype(np.int64), Y.indices.astype(np.int32), Y.data.astype(dt)


def _raw_graph_call(P, Fq, Fs, Y, alpha, k, weighted, dt, h):
    name = "features" if P == JACCARD else "vectors"
    fn = getattr(_lib.lib(), f"ss_graph_create_{name}_floor_{_suf(dt)}")
    keep = []
    pq, nq, ldq = _feature_args(Fq, dt, keep)
    ps, ns, lds = _feature_args(Fs, dt, keep)
    yp, yi, yv = _label_args(Y, dt)
    return fn(nq, ns, Y.shape[1], Fs.shape[1], *_mid(P), pq, ldq, ps, lds, yp.ctypes.data, yi.ctypes.data, yv.ctypes.data,
              0, _ct(dt)(alpha), k, 1 if weighted else 0, _lib.SS_MEM_HOST, C.byref(h))


def _raw_graph(P, Fq, Fs, Y, alpha, k, weighted, dt):
    h = C.c_void_p()
    _lib.check(_raw_graph_call(P, Fq, Fs, Y, alpha, k, weighted, dt, h))
    return ss.DeviceGraph(h, np.dtype(dt).type)


def _raw_queries_call(P, g, Fq, Fs, alpha, k, weighted, h):
    name = "features" if P == JACCARD else "vectors"
    dt = g.dtype.type
    fn = getattr(_lib.lib(), f"ss_queries_create_{name}_floor_{_suf(dt)}")
    keep = []
    pq, nq, ldq = _feature_args(Fq, dt, keep)
    ps, ns, lds = _feature_args(Fs, dt, keep)
    return fn(g._h, nq, ns, Fs.shape[1], *_mid(P), pq, ldq, ps, lds, _ct(dt)(alpha), k, 1 if weighted else 0,
              _lib.SS_MEM_HOST, C.byref(h))


def _raw_queries(P, g, Fq, Fs, alpha, k, weighted):
    h = C.c_void_p()
    _lib.check(_raw_queries_call(P, g, Fq, Fs, alpha, k, weighted, h))
    return ss.DeviceQueries(h, g)


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("n", [1, 63, 129])
@pytest.mark.parametrize("P", [JACCARD, ("dot", "tanimoto")], ids=["jaccard", "tanimoto"])
def test_k0_is_the_plain_producer(P, n, dt):
    ss.init(0)
    Fs, Fq = _rows(P)
    Fs, Fq = np.ascontiguousarray(Fs[:n]), np.ascontiguousarray(Fq[:max(1, n // 2)])
    Y = _labels()[:n]
    alpha = 0.3
    sym_tag, cross_tag = _tags(P, False)
    for weighted in (True, False):
        want = _csr(P, Fs, None, alpha, 0, weighted, dt)
        R.assert_csr_equal(_raw_floor_csr(P, Fs, None, alpha, 0, weighted, dt), want)
        assert ss.path_last() == [sym_tag]
        want = _csr(P, Fq, Fs, alpha, 0, weighted, dt)
        R.assert_csr_equal(_raw_floor_csr(P, Fq, Fs, alpha, 0, weighted, dt), want)
        assert ss.path_last() == [cross_tag]
    plain = _graph(P, Fq, Fs, Y, alpha, 0, True, dt)
    tags = ss.path_last()
    g0 = _raw_graph(P, Fq, Fs, Y, alpha, 0, True, dt)
    assert ss.path_last() == tags == [sym_tag, cross_tag]
    assert (g0.nnz_xq, g0.nnz_xs) == (plain.nnz_xq, plain.nnz_xs)
    assert_same(g0.predict("query", clean=True), plain.predict("query", clean=True))
    if n > 1:        # leave-one-out runs on the graph without queries
        assert_same(_raw_graph(P, None, Fs, Y, alpha, 0, True, dt).predict_loo(),
                    _graph(P, None, Fs, Y, alpha, 0, True, dt).predict_loo())
    q_plain = _queries(P, plain, Fq, Fs, alpha, 0)
    q0 = _raw_queries(P, plain, Fq, Fs, alpha, 0, True)
    assert ss.path_last() == [cross_tag]
    assert np.array_equal(q0.degrees(), q_plain.degrees())
    assert_same(plain.predict(queries=q0), plain.predict(queries=q_plain))


# ------------------------------------------------------------------------------------------------ 5. graph
@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("P,k,alpha,weighted", [(JACCARD, 5, 0.9, True), (("dot", "cosine"), 33, np.inf, False)],
                         ids=["features", "vectors"])
def test_floor_graph_is_the_csr_graph_of_the_reference_blocks(P, k, alpha, weighted, dt):
    ss.init(0)
    Fs, Fq = _rows(P)
    s_sym, s_x = _sims(P, dt)
    Y = _labels()
    Xs, Xq = R.ref_floor(s_sym, alpha, k, weighted), R.ref_floor(s_x, alpha, k, weighted)
    want = ss.DeviceGraph.from_sparse(Xq, Xs, Y, dtype=dt)
    got = _graph(P, Fq, Fs, Y, alpha, k, weighted, dt)
    assert ss.path_last() == _tags(P, True)
    info = lambda g: (g.nq, g.ns, g.nf, g.nt, g.nnz_xq, g.nnz_xs, g.nnz_ys)
    assert info(got) == info(want) == (NQ, N, N, NT, Xq.nnz, Xs.nnz, Y.nnz)
    for a, b in zip(got.degrees(), want.degrees()):
        assert np.array_equal(a, b)
    for clean in (False, True):
        assert_same(got.predict("query", clean=clean), want.predict("query", clean=clean))
        assert_same(got.predict("source", clean=clean), want.predict("source", clean=clean))
    # leave-one-out runs on the graph without queries: all 300 folds
    want0 = ss.DeviceGraph.from_sparse(None, Xs, Y, dtype=dt)
    got0 = _graph(P, None, Fs, Y, alpha, k, weighted, dt)
    assert ss.path_last() == _tags(P, True)[:1]
    for clean in (False, True):
        assert_same(got0.predict_loo(clean=clean), want0.predict_loo(clean=clean))
    assert_same(got0.evaluate_loo(clean=True), want0.evaluate_loo(clean=True))
    # device inputs build the same graph
    import torch
    Yd = (torch.from_numpy(Y.indptr.astype(np.int64)).cuda(), torch.from_numpy(Y.indices.astype(np.int32)).cuda(),
          torch.from_numpy(Y.data.astype(dt)).cuda(), NT)
    dev = _graph(P, _dev(Fq, dt), _dev(Fs, dt), Yd, alpha, k, weighted, dt)
    assert info(dev) == info(want)
    assert_same(dev.predict("query", clean=True), want.predict("query", clean=True))


# ------------------------------------------------------------------------------------------------ 6. query sets
@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("floor_graph", [False, True], ids=["plain_graph", "floor_graph"])
@pytest.mark.parametrize("P,alpha", [(JACCARD, 0.9), (("dot", "dice"), 0.7)], ids=["features", "vectors"])
def test_floor_query_sets(P, alpha, floor_graph, dt):
    ss.init(0)
    k = 5
    Fs, Fq = _rows(P)
    s_sym, s_x = _sims(P, dt)
    Y = _labels()
    Xq = R.ref_floor(s_x, alpha, k, True)
    Xs = R.ref_floor(s_sym, alpha, k if floor_graph else 0, True)
    fresh = ss.DeviceGraph.from_sparse(Xq, Xs, Y, dtype=dt)
    g = _graph(P, None, Fs, Y, alpha, k if floor_graph else 0, True, dt)
    info = lambda g: (g.nq, g.ns, g.nf, g.nt, g.nnz_xq, g.nnz_xs, g.nnz_ys)
    before = (info(g), g.degrees(), g.predict_loo(0, 40, clean=True))
    for dev in (False, True):
        q = _queries(P, g, _dev(Fq, dt) if dev else Fq, _dev(Fs, dt) if dev else Fs, alpha, k)
        assert ss.path_last() == _tags(P, True)[1:]
        assert (q.nq, q.nf, q.nnz) == (NQ, N, Xq.nnz)
        kq = q.degrees()
        assert np.array_equal(kq, np.diff(Xq.indptr))
        assert (kq >= np.minimum(k, R.positives(s_x))).all()        # nobody with a positive similarity is left out
        for clean in (False, True):
            assert_same(g.predict(clean=clean, queries=q), fresh.predict("query", clean=clean))
        assert_same(g.predict(row_begin=63, row_end=66, queries=q), fresh.predict("query", 63, 66))
        assert_same(g.predict_loo(0, 40, clean=True), before[2])    # the graph's own results while the set is alive
        q.close()
    # the plain cut leaves queries without neighbours that the floor serves
    q_plain = _queries(P, g, Fq, Fs, alpha, 0)
    assert ((q_plain.degrees() == 0) & (R.positives(s_x) > 0)).any()
    after = (info(g), g.degrees(), g.predict_loo(0, 40, clean=True))
    assert before[0] == after[0]
    for a, b in zip(before[1], after[1]):
        assert np.array_equal(a, b)
    assert_same(before[2], after[2])


# ------------------------------------------------------------------------------------------------ 7. iris
def test_iris_floor_block_and_leave_one_out_degrees():
    """The reference tutorial's data path (150 x 4 features, so d is below one staging step): the floor CSR at k = 6,
    alpha = 0.95 equals the reference bitwise, and with its own column dropped every leave-one-out row keeps at least
    5 feature entries."""
    ss.init(0)
    path = os.path.join(os.path.dirname(__file__), "golden", "iris", "iris.features")
    with open(path) as f:
        F = np.array([[float(v) for v in l.split()[1:]] for l in f.read().splitlines()[1:]])
    assert F.shape == (150, 4)
    k, alpha = 6, 0.95
    for dt in DTYPES:
        s = R.jaccard_s(F, None, dt)
        want = R.ref_floor(s, alpha, k, True)
        got = _csr(JACCARD, F, None, alpha, k, True, dt)
        R.assert_csr_equal(got, want)
        assert_same(_tau(JACCARD, F, None, k, dt), R.ref_kth(s, k))
        assert (got.diagonal() == 1).all()
        assert (np.diff(got.indptr) - 1 >= 5).all()
        assert (np.diff(R.ref_cut(s, alpha, True).indptr) - 1 < 5).any()       # which alpha alone does not give


# ------------------------------------------------------------------------------------------------ 8. protocol
@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("P,alpha", [(JACCARD, 0.9), (("dot", "cosine"), 0.7)], ids=["jaccard", "cosine"])
def test_protocol_and_refusals(P, alpha, dt):
    ss.init(0)
    lib = _lib.lib()
    Fs, Fq = _rows(P)
    s_x = _sims(P, dt)[1]
    k = 5
    want = R.ref_floor(s_x, alpha, k, True)
    csr = getattr(lib, f"ss_similarity_{P[0]}_floor_csr_{_suf(dt)}")
    kth = getattr(lib, f"ss_similarity_{P[0]}_kth_{_suf(dt)}")
    keep = []
    pq, _, ldq = _feature_args(Fq, dt, keep)
    ps, _, lds = _feature_args(Fs, dt, keep)
    mid = _mid(P)
    H = _lib.SS_MEM_HOST

    def head(na=NQ, nb=N, d=D, mid=mid):
        return (pq, na, ldq, ps, nb, lds, d) + mid

    # size query, then a capacity that is too small: SS_EINVAL with *nnz set and idx / val untouched
    ptr, nnz = np.full(NQ + 1, -7, np.int64), C.c_int64(-1)
    _lib.check(csr(*head(), _ct(dt)(alpha), k, 1, ptr.ctypes.data, None, None, 0, C.byref(nnz), H))
    assert nnz.value == want.nnz and np.array_equal(ptr, want.indptr)
    idx, val = np.full(want.nnz, -7, np.int32), np.full(want.nnz, -7, dt)
    nnz = C.c_int64(-1)
    assert csr(*head(), _ct(dt)(alpha), k, 1, ptr.ctypes.data, idx.ctypes.data, val.ctypes.data, want.nnz - 1,
               C.byref(nnz), H) == EINVAL
    assert nnz.value == want.nnz and (idx == -7).all() and (val == -7).all()

    # bad k, NaN alpha, a NaN feature, an unknown metric: SS_EINVAL, nothing written, *out == NULL
    Y = _labels()
    g = _graph(P, None, Fs, Y, alpha, 0, True, dt)
    Fnan = np.array(Fq, dtype=dt)
    Fnan[17, 3] = np.nan
    bad = [(Fq, -1, alpha, P), (Fq, 65, alpha, P), (Fq, 5, np.nan, P), (Fq, 0, np.nan, P), (Fnan, 5, alpha, P)]
    if P != JACCARD:
        bad.append((Fq, 5, alpha, ("dot", None)))
    for Fbad, bad_k, bad_alpha, Pbad in bad:
        bmid = mid if Pbad == P else (7,)
        pbad, _, _ = _feature_args(Fbad, dt, keep)
        ptr, nnz = np.full(NQ + 1, -7, np.int64), C.c_int64(-7)
        assert csr(pbad, NQ, ldq, ps, N, lds, D, *bmid, _ct(dt)(bad_alpha), bad_k, 1, ptr.ctypes.data, idx.ctypes.data,
                   val.ctypes.data, want.nnz, C.byref(nnz), H) == EINVAL
        assert (ptr == -7).all() and nnz.value == -7 and (idx == -7).all() and (val == -7).all()
        yp, yi, yv = _label_args(Y, dt)
        name = "features" if P == JACCARD else "vectors"
        h = C.c_void_p(1)
        gcreate = getattr(lib, f"ss_graph_create_{name}_floor_{_suf(dt)}")
        assert gcreate(NQ, N, NT, D, *bmid, pbad, ldq, ps, lds, yp.ctypes.data, yi.ctypes.data, yv.ctypes.data, 0,
                       _ct(dt)(bad_alpha), bad_k, 1, H, C.byref(h)) == EINVAL
        assert not h.value
        h = C.c_void_p(1)
        qcreate = getattr(lib, f"ss_queries_create_{name}_floor_{_suf(dt)}")
        assert qcreate(g._h, NQ, N, D, *bmid, pbad, ldq, ps, lds, _ct(dt)(bad_alpha), bad_k, 1, H, C.byref(h)) == EINVAL
        assert not h.value
    pnan, _, _ = _feature_args(Fnan, dt, keep)
    cases = [(pq, -1, mid), (pq, 0, mid), (pq, 65, mid), (pnan, 5, mid)] + ([(pq, 5, (7,))] if P != JACCARD else [])
    for pbad, bad_k, bmid in cases:
        tau = np.full(NQ, -7, dt)
        assert kth(pbad, NQ, ldq, ps, N, lds, D, *bmid, bad_k, tau.ctypes.data, H) == EINVAL
        assert (tau == -7).all()

    # na == 0, nb == 0, d == 0
    tau = np.full(NQ, -7, dt)
    _lib.check(kth(*head(na=0), k, tau.ctypes.data, H))
    assert (tau == -7).all()
    _lib.check(kth(*head(nb=0), k, tau.ctypes.data, H))
    assert_same(tau, np.zeros(NQ, dt))
    for na, nb in ((NQ, 0), (0, N)):
        ptr, nnz = np.full(na + 1, -7, np.int64), C.c_int64(-1)
        _lib.check(csr(*head(na=na, nb=nb), _ct(dt)(alpha), k, 1, ptr.ctypes.data, None, None, 0, C.byref(nnz), H))
        assert nnz.value == 0 and (ptr == 0).all()
    _lib.check(kth(*head(d=0), 64, tau.ctypes.data, H))              # s = 1 everywhere: tau = 1 since nb >= k
    assert_same(tau, np.ones(NQ, dt))
    ptr, nnz = np.full(NQ + 1, -7, np.int64), C.c_int64(-1)
    _lib.check(csr(*head(d=0), _ct(dt)(np.inf), k, 1, ptr.ctypes.data, None, None, 0, C.byref(nnz), H))
    assert nnz.value == NQ * N and np.array_equal(ptr, np.arange(NQ + 1) * N)   # every pair ties at tau = 1

    # two runs give identical bytes
    a, b = _csr(P, Fs, None, alpha, 33, True, dt), _csr(P, Fs, None, alpha, 33, True, dt)
    R.assert_csr_equal(a, b)
    assert_same(_tau(P, Fs, None, 33, dt), _tau(P, Fs, None, 33, dt))
