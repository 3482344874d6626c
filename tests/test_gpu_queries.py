"""Query sets (ss_queries_*, ss_predict_queries_*): a batch of queries bound to a resident graph scores bit for bit like
the graph its constructor builds with those queries -- every constructor, range, layout and precision -- and leaves the
graph itself untouched."""
import ctypes as C

import numpy as np
import pytest
import scipy.sparse as sp

import simspread_jl_amd as ss
from simspread_jl_amd import _lib

pytestmark = pytest.mark.gpu

DTYPES = [np.float32, np.float64]
NS, NT = 193, 37                 # off the 128-pair producer tile and the 64-row slice
NQS = [0, 1, 65, 130]            # one batch on each side of a tile edge
EINVAL, EUNSUPPORTED = -1, -5


def assert_same(a, b, what=""):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    assert a.shape == b.shape and a.dtype == b.dtype, what
    assert np.array_equal(a.view(np.uint8), b.view(np.uint8)), what


def _labels(ns, nt, seed):
    rng = np.random.default_rng(seed)
    Y = sp.random(ns, nt, density=0.15, format="csr", random_state=rng)
    Y.data[:] = 1.0
    Y = Y.tolil()
    Y[:, 3] = 0.0                # a target nobody holds: clean! marks it
    Y = Y.tocsr()
    Y.eliminate_zeros()
    Y.sort_indices()
    return Y


def _sparse_blocks(nq, ns, seed, weighted=True):
    rng = np.random.default_rng(seed)

    def block(r):
        m = sp.random(r, ns, density=0.08, format="csr", random_state=rng)
        m.data = (0.5 + 0.5 * (1.0 - rng.random(m.nnz))) if weighted else np.ones(m.nnz)
        m.sort_indices()
        return m

    Xs = block(ns).tolil()
    Xs.setdiag(1.0)
    Xs = Xs.tocsr()
    Xs.sort_indices()
    return block(nq), Xs


def _ranges(nq):
    out = {(0, nq), (0, 0), (nq, nq), (nq // 2, nq), (0, (nq + 1) // 2)}
    if nq > 70:
        out |= {(63, 66), (1, nq - 1)}
    return sorted(out)


def _compare(fresh, g, q, nq, clean_values=(False, True)):
    """every range, both layouts, host and device outputs: g + q against the graph built with the queries"""
    import torch
    for lo, hi in _ranges(nq):
        for clean in clean_values:
            for layout in ("row", "col"):
                want = fresh.predict("query", lo, hi, clean=clean, layout=layout)
                got = g.predict(row_begin=lo, row_end=hi, clean=clean, layout=layout, queries=q)
                assert_same(got, want, (lo, hi, clean, layout))
    tt = torch.float32 if g.dtype == np.float32 else torch.float64
    for layout, shape in (("row", (nq, g.nt)), ("col", (g.nt, nq))):
        a = torch.full(shape, -7.0, dtype=tt, device="cuda")
        b = torch.full(shape, -7.0, dtype=tt, device="cuda")
        fresh.predict("query", 0, nq, clean=True, out=a, layout=layout)
        g.predict(row_begin=0, row_end=nq, clean=True, out=b, layout=layout, queries=q)
        torch.cuda.synchronize()
        ss._lib.check(ss._lib.lib().ss_synchronize())
        assert_same(b.cpu().numpy(), a.cpu().numpy(), ("device", layout))


# ------------------------------------------------------------------------------------------------ CSR
@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("nq", NQS)
def test_csr_query_set_is_bitwise_the_graph_built_with_the_queries(dt, nq):
    import torch
    ss.init(0)
    Xq, Xs = _sparse_blocks(nq, NS, 1 + nq)
    Ys = _labels(NS, NT, 2)
    fresh = ss.DeviceGraph.from_sparse(Xq, Xs, Ys, dtype=dt)
    g = ss.DeviceGraph.from_sparse(None, Xs, Ys, dtype=dt)
    info, deg = (g.nq, g.ns, g.nf, g.nt, g.nnz_xq, g.nnz_xs, g.nnz_ys), g.degrees()
    sets = [ss.DeviceQueries.from_sparse(g, Xq, index_base=0), ss.DeviceQueries.from_sparse(g, Xq, index_base=1)]
    ptr, idx, val = (Xq.indptr.astype(np.int64), Xq.indices.astype(np.int32), Xq.data.astype(dt))
    for base in (0, 1):
        dev = (torch.from_numpy(ptr + base).cuda(), torch.from_numpy(idx + np.int32(base)).cuda(),
               torch.from_numpy(val).cuda(), nq)
        sets.append(ss.DeviceQueries.from_sparse(g, dev, index_base=base))
    for k, q in enumerate(sets):
        assert (q.nq, q.nf, q.nnz) == (nq, NS, fresh.nnz_xq)
        assert np.array_equal(q.degrees(), np.diff(Xq.indptr))
        _compare(fresh, g, q, nq, clean_values=(False, True) if k == 0 else (True,))
    h = C.c_int64 * 7
    buf = h()
    _lib.check(_lib.lib().ss_graph_info(g._h, buf))
    assert tuple(int(v) for v in buf) == info
    for a, b in zip(g.degrees(), deg):
        assert np.array_equal(a, b)
    for q in sets:
        q.close()


# ------------------------------------------------------------------------------------------------ raw data
def _fingerprints(n, seed, nbits=130):
    rng = np.random.default_rng(seed)
    proto = rng.random((6, nbits)) < 0.4           # clusters: similarities spread over (0, 1]
    bits = proto[rng.integers(0, 6, n)] ^ (rng.random((n, nbits)) < 0.12)
    return ss.pack_fingerprints(bits)


def _features(n, d, seed):
    rng = np.random.default_rng(seed)
    return rng.integers(0, 5, (n, d)).astype(np.float64)       # small integers: exact in both precisions


RAW = {
    "fingerprint": dict(data=lambda n, seed: _fingerprints(n, seed), alpha=0.35,
                        graph=lambda Fq, Fs, Y, a, w, dt: ss.DeviceGraph.from_fingerprints(Fq, Fs, Y, a, weighted=w, dtype=dt),
                        queries=lambda g, Fq, Fs, a, w: ss.DeviceQueries.from_fingerprints(g, Fq, Fs, a, weighted=w),
                        tag="tanimoto_csr_cross"),
    "features": dict(data=lambda n, seed: _features(n, 5, seed), alpha=0.4,
                     graph=lambda Fq, Fs, Y, a, w, dt: ss.DeviceGraph.from_features(Fq, Fs, Y, a, weighted=w, dtype=dt),
                     queries=lambda g, Fq, Fs, a, w: ss.DeviceQueries.from_features(g, Fq, Fs, a, weighted=w),
                     tag="jaccard_csr_cross"),
}
for _m in ("cosine", "tanimoto", "dice"):
    RAW[f"vectors_{_m}"] = dict(
        data=lambda n, seed: _features(n, 7, seed), alpha=0.6,
        graph=lambda Fq, Fs, Y, a, w, dt, m=_m: ss.DeviceGraph.from_vectors(Fq, Fs, Y, a, metric=m, weighted=w, dtype=dt),
        queries=lambda g, Fq, Fs, a, w, m=_m: ss.DeviceQueries.from_vectors(g, Fq, Fs, a, metric=m, weighted=w),
        tag="dot_csr_cross")


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("kind", list(RAW))
def test_raw_data_query_sets_are_bitwise_the_constructor(kind, dt):
    ss.init(0)
    r = RAW[kind]
    Fs = r["data"](NS, 5)
    Ys = _labels(NS, NT, 6)
    for weighted in (True, False):
        g = r["graph"](None, Fs, Ys, r["alpha"], weighted, dt)
        for nq in NQS:
            Fq = r["data"](nq, 7 + nq)
            fresh = r["graph"](Fq, Fs, Ys, r["alpha"], weighted, dt)
            q = r["queries"](g, Fq, Fs, r["alpha"], weighted)
            if nq > 0:
                assert r["tag"] in ss.path_last()
            assert (q.nq, q.nf, q.nnz) == (nq, NS, fresh.nnz_xq)
            if nq == 130:
                assert 0 < q.nnz < nq * NS
            _compare(fresh, g, q, nq, clean_values=(True,))
            q.close()
            fresh.close()
        g.close()


@pytest.mark.parametrize("dt", DTYPES)
def test_query_degrees_are_the_row_counts_of_the_cross_similarity(dt):
    ss.init(0)
    Fs, Fq = _fingerprints(NS, 5), _fingerprints(130, 9)
    g = ss.DeviceGraph.from_fingerprints(None, Fs, _labels(NS, NT, 6), 0.35, dtype=dt)
    q = ss.DeviceQueries.from_fingerprints(g, Fq, Fs, 0.35)
    cross = ss.tanimoto_csr(Fq, Fs, alpha=0.35, dtype=dt)
    kq = q.degrees()
    assert np.array_equal(kq, np.diff(cross.indptr)) and kq.sum() == q.nnz
    import torch
    d = torch.full((130,), -1, dtype=torch.int64, device="cuda")
    _lib.check(_lib.lib().ss_queries_degrees(q._h, d.data_ptr(), _lib.SS_MEM_DEVICE))
    assert np.array_equal(d.cpu().numpy(), kq)


# ------------------------------------------------------------------------------------------------ sharing the graph
@pytest.mark.parametrize("dt", DTYPES)
def test_two_query_sets_alternate_and_the_graph_keeps_its_bits(dt):
    ss.init(0)
    Xa, Xs = _sparse_blocks(65, NS, 21)
    Xb, _ = _sparse_blocks(130, NS, 22)
    Ys = _labels(NS, NT, 23)
    g = ss.DeviceGraph.from_sparse(None, Xs, Ys, dtype=dt)
    # the graph on its own, before any query set exists
    loo0, deg0 = g.predict_loo(clean=True), g.degrees()
    fold = (np.arange(NS) % 5).astype(np.int32)
    kf0 = g.predict_kfold(fold, 5, clean=True)
    fa, fb = ss.DeviceGraph.from_sparse(Xa, Xs, Ys, dtype=dt), ss.DeviceGraph.from_sparse(Xb, Xs, Ys, dtype=dt)
    wa, wb = fa.predict(clean=True), fb.predict(clean=True)
    qa, qb = ss.DeviceQueries.from_sparse(g, Xa), ss.DeviceQueries.from_sparse(g, Xb)
    for _ in range(2):
        assert_same(g.predict(queries=qa, clean=True), wa)
        assert_same(g.predict_loo(clean=True), loo0)
        assert_same(g.predict(queries=qb, clean=True), wb)
    assert_same(g.predict_kfold(fold, 5, clean=True), kf0)
    for a, b in zip(g.degrees(), deg0):
        assert np.array_equal(a, b)
    qa.close()
    assert_same(g.predict(queries=qb, clean=True), wb)
    qb.close()
    assert_same(g.predict_loo(clean=True), loo0)
    assert_same(g.predict_kfold(fold, 5, clean=True), kf0)
    for a, b in zip(g.degrees(), deg0):
        assert np.array_equal(a, b)
    assert (g.nq, g.nnz_xq) == (0, 0)
    # a query set may outlive its graph
    qc = ss.DeviceQueries.from_sparse(g, Xa)
    g.close()
    assert qc.degrees().sum() == qc.nnz
    qc.close()


@pytest.mark.parametrize("dt", DTYPES)
def test_query_set_on_a_recut_child_is_the_constructor_at_the_childs_cutoff(dt):
    ss.init(0)
    Fs, Fq = _fingerprints(NS, 5), _fingerprints(130, 9)
    Ys = _labels(NS, NT, 6)
    parent = ss.DeviceGraph.from_fingerprints(None, Fs, Ys, 0.3, dtype=dt)
    child = parent.recut(0.45)
    fresh = ss.DeviceGraph.from_fingerprints(Fq, Fs, Ys, 0.45, dtype=dt)
    q = ss.DeviceQueries.from_fingerprints(child, Fq, Fs, 0.45)
    assert 0 < q.nnz == fresh.nnz_xq
    _compare(fresh, child, q, 130, clean_values=(True,))
    # bound to the child, not to its parent
    with pytest.raises(ss.SimSpreadError) as e:
        parent.predict(queries=q)
    assert e.value.code == EINVAL


@pytest.mark.parametrize("dt", DTYPES)
def test_several_transfer_batches(dt, monkeypatch):
    """ns = 2100: with the transfer block capped at its 1 MiB floor 130 rows take several stage-1 batches (fp64: 56 rows
    each, fp32: 120)"""
    ss.init(0)
    ns = 2100
    Xq, Xs = _sparse_blocks(130, ns, 31)
    Ys = _labels(ns, NT, 32)
    monkeypatch.setenv("SS_TRANSFER_BYTES", str(1 << 20))
    fresh = ss.DeviceGraph.from_sparse(Xq, Xs, Ys, dtype=dt)
    g = ss.DeviceGraph.from_sparse(None, Xs, Ys, dtype=dt)
    q = ss.DeviceQueries.from_sparse(g, Xq)
    want = fresh.predict(clean=True)
    assert ss.timing_last()["transfer_launches"] >= 2
    got = g.predict(queries=q, clean=True)
    assert ss.timing_last()["transfer_launches"] >= 2
    assert_same(got, want)
    monkeypatch.delenv("SS_TRANSFER_BYTES")
    assert_same(g.predict(queries=q, clean=True), want)       # one batch: the same bits
    assert_same(g.predict(row_begin=50, row_end=127, queries=q), fresh.predict("query", 50, 127))


@pytest.mark.parametrize("dt", DTYPES)
def test_target_topl_screens_a_query_set(dt):
    ss.init(0)
    Xq, Xs = _sparse_blocks(130, NS, 51)
    Ys = _labels(NS, NT, 52)
    yq = _labels(130, NT, 53)
    fresh = ss.DeviceGraph.from_sparse(Xq, Xs, Ys, dtype=dt)
    g = ss.DeviceGraph.from_sparse(None, Xs, Ys, dtype=dt)
    q = ss.DeviceQueries.from_sparse(g, Xq)
    a = ss.TargetTopL(NT, L=7, dtype=dt).add_predict(fresh, clean=True, y=yq, block_rows=50)
    b = ss.TargetTopL(NT, L=7, dtype=dt).add_predict(g, clean=True, y=yq, block_rows=64, queries=q)
    assert b.info()["rows"] == 130
    for x, y in zip(a.export(), b.export()):
        assert_same(np.asarray(x), np.asarray(y))


# ------------------------------------------------------------------------------------------------ refusals
def _raw_predict(lib, suf, g, q, lo, hi, out, ld):
    return getattr(lib, f"ss_predict_queries_{suf}")(g._h, q._h, lo, hi, 0, out.ctypes.data, ld, 0, _lib.SS_MEM_HOST)


@pytest.mark.parametrize("dt", DTYPES)
def test_refusals_leave_the_output_untouched(dt):
    lib = ss.init(0)
    suf = "f32" if dt == np.float32 else "f64"
    other = np.float64 if dt == np.float32 else np.float32
    osuf = "f64" if dt == np.float32 else "f32"
    Xq, Xs = _sparse_blocks(65, NS, 41)
    Ys = _labels(NS, NT, 42)
    g = ss.DeviceGraph.from_sparse(None, Xs, Ys, dtype=dt)
    g2 = ss.DeviceGraph.from_sparse(None, Xs, Ys, dtype=dt)      # same shape, another graph
    q = ss.DeviceQueries.from_sparse(g, Xq)
    out = np.full((65, NT), -7.0, dt)
    keep = out.copy()
    # a foreign graph
    assert _raw_predict(lib, suf, g2, q, 0, 65, out, NT) == EINVAL
    assert "another graph" in lib.ss_last_error().decode()
    # bad ranges, a short leading dimension
    for lo, hi in ((-1, 3), (3, 2), (0, 66)):
        assert _raw_predict(lib, suf, g, q, lo, hi, out, NT) == EINVAL
    assert _raw_predict(lib, suf, g, q, 0, 65, out, NT - 1) == EINVAL
    # mixed precision: the graph, the query set, the entry point
    go = ss.DeviceGraph.from_sparse(None, Xs, Ys, dtype=other)
    qo = ss.DeviceQueries.from_sparse(go, Xq)
    assert _raw_predict(lib, osuf, g, q, 0, 65, out, NT) == EINVAL
    assert _raw_predict(lib, suf, g, qo, 0, 65, out, NT) == EINVAL
    assert _raw_predict(lib, suf, go, qo, 0, 65, out, NT) == EINVAL
    assert_same(out, keep)
    assert _raw_predict(lib, suf, g, q, 0, 65, out, NT) == 0 and not np.array_equal(out, keep)
    # graphs that hold no CSR blocks
    rng = np.random.default_rng(43)
    S = rng.random((NS, NS))
    dense = ss.DeviceGraph.from_similarity(None, (S + S.T) / 2, Ys, 0.5, dtype=dt)
    B = sp.random(20, 20, density=0.3, format="csr", random_state=rng)
    general = ss.DeviceGraph.general(B[:3], B, B[:, :4].T.tocsr(), dtype=dt)
    dense_asym = ss.DeviceGraph.from_similarity(None, S, Ys, 0.5, dtype=dt)     # Ss need not be symmetric
    for bad, xq in ((dense, Xq), (dense_asym, Xq), (general, sp.csr_matrix((3, 20)))):
        with pytest.raises(ss.SimSpreadError) as e:
            ss.DeviceQueries.from_sparse(bad, xq)
        assert e.value.code == EUNSUPPORTED
    # raw data: Fs must be the graph's sources
    Fs, Fq = _fingerprints(NS, 5), _fingerprints(9, 9)
    gf = ss.DeviceGraph.from_fingerprints(None, Fs, Ys, 0.35, dtype=dt)
    with pytest.raises(ss.SimSpreadError) as e:
        ss.DeviceQueries.from_fingerprints(gf, Fq, Fs[:-1], 0.35)
    assert e.value.code == EINVAL
    with pytest.raises(ss.SimSpreadError) as e:
        ss.DeviceQueries.from_features(gf, _features(9, 5, 1), _features(NS + 1, 5, 2), 0.4)
    assert e.value.code == EINVAL
    h = C.c_void_p(123)
    ft = C.c_float if dt == np.float32 else C.c_double
    rc = getattr(lib, f"ss_queries_create_fingerprint_{suf}")(gf._h, 9, NS - 1, 3, Fq.ctypes.data, Fs.ctypes.data,
                                                             ft(0.35), 1, _lib.SS_MEM_HOST, C.byref(h))
    assert rc == EINVAL and not h.value
    # a graph whose features are not its sources takes no raw-data query set
    Xr, _ = _sparse_blocks(NS, 50, 44)                           # NS sources x 50 features
    gr = ss.DeviceGraph.from_sparse(None, Xr, Ys, dtype=dt)
    assert (gr.ns, gr.nf) == (NS, 50)
    with pytest.raises(ss.SimSpreadError) as e:
        ss.DeviceQueries.from_fingerprints(gr, Fq, Fs, 0.35)
    assert e.value.code == EINVAL
