"""Support lists (ss_support_*): which sources carry a score.

The transfer row T[r,:] is not exposed, so its bits come from the library itself through a probe graph: the same Xq and Xs
with labels Yp (ns x (ns + P)) that hold a single 1 in row s of column s plus nnz(Ys[s,:]) - 1 ones in columns >= ns, so
that every degree stage 1 uses is unchanged and the probe's score (r, s) is the one-term sum T[r,s] * 1.  The expected
lists are then numpy products in the graph's precision (support_ref.support_lists), compared bitwise."""
import ctypes as C

import numpy as np
import pytest
import scipy.sparse as sp

import simspread_jl_amd as ss
from simspread_jl_amd import _lib
from support_ref import support_lists, support_ref

pytestmark = pytest.mark.gpu

DTYPES = [np.float32, np.float64]
EINVAL, EUNSUPPORTED = -1, -5
U = {np.float32: 2.0 ** -24, np.float64: 2.0 ** -53}
TOL = {np.float32: 1e-5, np.float64: 1e-12}          # tests/test_gpu_parity.py, relative to the block's largest value
GAP = {np.float32: 2e-5, np.float64: 2e-12}


def assert_same(a, b, what=""):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    assert a.shape == b.shape and a.dtype == b.dtype, what
    assert np.array_equal(a.view(np.uint8), b.view(np.uint8)), what


def _x_blocks(nq, ns, density, seed):
    rng = np.random.default_rng(seed)

    def block(r):
        m = sp.random(r, ns, density=density, format="csr", random_state=rng)
        m.data = (0.5 + 0.5 * (1.0 - rng.random(m.nnz))).astype(np.float32).astype(np.float64)
        m.sort_indices()
        return m

    Xs = block(ns).tolil()
    Xs.setdiag(1.0)
    return block(nq), Xs


def _edge_graph(weighted_labels, seed=3, ns=150, nt=9, nq=40):
    """every source labelled; target 0 held by all 150 sources (more than two 64-entry steps), target 1 by none, target 2
    by one; sources (10, 11) and (40, 97) identical in features and labels: exact ties"""
    rng = np.random.default_rng(seed)
    Xq, Xs = _x_blocks(nq, ns, 0.1, seed)
    Y = (rng.random((ns, nt)) < 0.2).astype(np.float64)
    if weighted_labels:
        Y *= rng.choice([0.5, 1.0, 2.0, 0.75], size=Y.shape)
    Y[:, 0] = 1.0
    Y[:, 1] = 0.0
    Y[:, 2] = 0.0
    Y[77, 2] = 1.0
    for a, b in ((10, 11), (40, 97)):
        Xs[b, :] = Xs[a, :]
        Y[b, :] = Y[a, :]
    Xs = Xs.tocsr()
    Xs.sort_indices()
    return Xq, Xs, sp.csr_matrix(Y)


def _probe_labels(Ys):
    """Yp: a single 1 at (s, s) and nnz(Ys[s,:]) - 1 ones in columns >= ns"""
    ns = Ys.shape[0]
    cnt = np.diff(sp.csr_matrix(Ys).indptr)
    assert cnt.min() >= 1
    P = max(int(cnt.max()) - 1, 1)
    rows = np.concatenate([np.arange(ns)] + [np.full(c - 1, s) for s, c in enumerate(cnt)])
    cols = np.concatenate([np.arange(ns)] + [ns + np.arange(c - 1) for c in cnt])
    return sp.csr_matrix((np.ones(len(rows)), (rows, cols)), shape=(ns, ns + P))


def _transfer_bits(Xq, Xs, Ys, dt, loo_rows=None):
    """(T of the query rows, T of the leave-one-out folds loo_rows) in the graph's precision, from the library"""
    Yp = _probe_labels(Ys)
    ns = Ys.shape[0]
    gp = ss.DeviceGraph.from_sparse(Xq, Xs, Yp, dtype=dt)
    Tq = gp.predict("query")[:, :ns].copy()
    gp.close()
    Tl = None
    if loo_rows is not None:
        g0 = ss.DeviceGraph.from_sparse(None, Xs, Yp, dtype=dt)
        Tl = np.zeros((ns, ns), dt)
        for i in np.unique(loo_rows):
            Tl[i] = g0.predict_loo(int(i), int(i) + 1)[0, :ns]
        g0.close()
    return Tq, Tl


def _pairs(nrows, nt, n, seed, rows_from=None):
    rng = np.random.default_rng(seed)
    pool = np.arange(nrows) if rows_from is None else np.asarray(rows_from)
    rows = rng.choice(pool, n)                            # rows repeat
    targets = rng.integers(0, nt, n)
    targets[:6] = [0, 1, 2, 0, 1, 2]
    perm = rng.permutation(n)
    return rows[perm].astype(np.int64), targets[perm].astype(np.int32)


def _check_sums(contrib, nsupp, M, scores, rows, targets, kt, dt):
    full = nsupp <= M
    assert full.any()
    tot = contrib.astype(np.float64).sum(axis=1)
    mag = np.abs(contrib.astype(np.float64)).sum(axis=1)
    want = scores[rows, targets].astype(np.float64)
    bound = 2.0 * kt[targets] * U[dt] * mag
    assert (np.abs(tot - want)[full] <= bound[full]).all()


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("weighted_labels", [False, True])
def test_lists_are_bitwise_the_products_of_the_transfer_row(dt, weighted_labels):
    ss.init(0)
    Xq, Xs, Ys = _edge_graph(weighted_labels)
    ns, nt = Ys.shape
    nq = Xq.shape[0]
    kt = np.diff(sp.csc_matrix(Ys).indptr)
    assert (kt[0], kt[1], kt[2]) == (150, 0, 1)
    loo_rows = np.array([0, 1, 2, 10, 11, 40, 64, 77, 97, 149])
    Tq, Tl = _transfer_bits(Xq, Xs, Ys, dt, loo_rows)
    gq = ss.DeviceGraph.from_sparse(Xq, Xs, Ys, dtype=dt)            # its own query rows
    g0 = ss.DeviceGraph.from_sparse(None, Xs, Ys, dtype=dt)          # query sets and leave-one-out
    q = ss.DeviceQueries.from_sparse(g0, Xq)
    scores_q = gq.predict("query")
    scores_l = g0.predict_loo()
    for M in (1, 5, 64):
        rows, targets = _pairs(nq, nt, 120, 10 + M)
        want = support_lists(Tq, rows, Ys, targets, M)
        if M == 64:     # the exact ties are there and come in ascending source order
            c = want[1]
            assert ((c[:, :-1] == c[:, 1:]) & (c[:, :-1] != 0)).any()
        assert want[2].max() > 64 and want[2].min() == 0
        for g, qs in ((gq, None), (g0, q)):
            got = g.support(rows, targets, M=M, queries=qs)
            assert ss.path_last() == ["support", "transfer"]
            for a, b, name in zip(got, want, ("src", "contrib", "nsupp")):
                assert_same(a, b, (name, M, qs is not None))
            assert_same(g.support(rows, targets, M=M, queries=qs)[0], got[0], "repeatable")
        _check_sums(want[1], want[2], M, scores_q, rows, targets, kt, dt)
        rows, targets = _pairs(ns, nt, 60, 20 + M, rows_from=loo_rows)
        want = support_lists(Tl, rows, Ys, targets, M)
        got = g0.support(rows, targets, M=M, loo=True)
        assert ss.path_last() == ["support", "transfer_loo"]
        for a, b, name in zip(got, want, ("src", "contrib", "nsupp")):
            assert_same(a, b, ("loo", name, M))
        assert not (got[0] == rows[:, None]).any()
        _check_sums(want[1], want[2], M, scores_l, rows, targets, kt, dt)
    # device pair lists and outputs
    import torch
    rows, targets = _pairs(nq, nt, 50, 99)
    want = support_lists(Tq, rows, Ys, targets, 5)
    got = g0.support(torch.from_numpy(rows).cuda(), torch.from_numpy(targets).cuda(), M=5, queries=q)
    for a, b in zip(got, want):
        assert_same(a.cpu().numpy(), b)
    t = ss.timing_last()
    assert t["transfer_launches"] == 1 and t["total_ms"] > 0


@pytest.mark.parametrize("dt", DTYPES)
def test_long_label_row_and_several_batches(dt, monkeypatch):
    """ns = 5000 with a target every source holds (78 steps of 64 through one wave), and, with the transfer block capped
    at its 1 MiB floor, the distinct rows of the pair list in several stage-1 batches"""
    ss.init(0)
    ns, nt, nq = 5000, 6, 64
    rng = np.random.default_rng(5)
    Xq, Xs = _x_blocks(nq, ns, 0.004, 6)
    Xs = Xs.tocsr()
    Y = sp.random(ns, nt, density=0.01, format="lil", random_state=rng)
    Y[:, 0] = 1.0
    Ys = sp.csr_matrix(Y)
    Ys.data[:] = 1.0
    Tq, _ = _transfer_bits(Xq, Xs, Ys, dt)
    g = ss.DeviceGraph.from_sparse(Xq, Xs, Ys, dtype=dt)
    rows = np.concatenate([np.arange(nq), np.arange(nq)[::-1]]).astype(np.int64)
    targets = np.concatenate([np.zeros(nq), rng.integers(0, nt, nq)]).astype(np.int32)
    for M in (5, 64):
        want = support_lists(Tq, rows, Ys, targets, M)
        assert want[2].max() > 64
        got = g.support(rows, targets, M=M)
        for a, b, name in zip(got, want, ("src", "contrib", "nsupp")):
            assert_same(a, b, (name, M))
    monkeypatch.setenv("SS_TRANSFER_BYTES", str(1 << 20))        # 52 rows (fp32) / 26 rows (fp64) per batch
    got = g.support(rows, targets, M=64)
    assert ss.timing_last()["transfer_launches"] >= 2
    for a, b in zip(got, want):
        assert_same(a, b, "batched")


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("seed", [11, 12])
def test_against_the_fp64_reference_on_random_weighted_graphs(dt, seed):
    ss.init(0)
    ns, nq, nt, M = 150, 40, 9, 64
    Xq, Xs = _x_blocks(nq, ns, 0.08, seed)
    Xs = Xs.tocsr()
    rng = np.random.default_rng(seed)
    Ys = sp.csr_matrix((rng.random((ns, nt)) < 0.2) * rng.choice([0.5, 1.0, 2.0], size=(ns, nt)))
    g = ss.DeviceGraph.from_sparse(None, Xs, Ys, dtype=dt)
    q = ss.DeviceQueries.from_sparse(g, Xq)
    r, t = np.meshgrid(np.arange(nq), np.arange(nt), indexing="ij")
    cases = [(r.ravel(), t.ravel(), False)]
    r, t = np.meshgrid(np.arange(0, ns, 3), np.arange(nt), indexing="ij")
    cases.append((r.ravel(), t.ravel(), True))
    left_out = neighbours = 0
    for rows, targets, loo in cases:
        src, contrib, nsupp = g.support(rows, targets, M=M, queries=None if loo else q, loo=loo)
        rsrc, rcon, rn = support_ref(Xq, Xs, Ys, rows, targets, M, loo=loo)
        assert np.array_equal(nsupp, rn) and rn.max() <= M
        scale = np.abs(rcon).max()
        assert scale > 0
        assert np.abs(contrib.astype(np.float64) - rcon).max() <= TOL[dt] * scale
        assert np.array_equal(src >= 0, rsrc >= 0)
        for p in range(len(rows)):
            n = int(rn[p])
            if n == 0:
                continue
            c = rcon[p, :n]
            apart = (c[:-1] - c[1:]) > GAP[dt] * c[0]             # neighbouring reference contributions told apart
            neighbours += n - 1
            left_out += int((~apart).sum())
            sure = np.concatenate([[True], apart]) & np.concatenate([apart, [True]])
            assert np.array_equal(src[p, :n][sure], rsrc[p, :n][sure]), (p, loo)
            assert sorted(src[p, :n]) == sorted(rsrc[p, :n])
    assert neighbours > 1000
    assert left_out <= 0.02 * neighbours, (left_out, neighbours)


@pytest.mark.parametrize("suf,dt", [("f32", np.float32), ("f64", np.float64)])
def test_errors_write_nothing(suf, dt):
    lib = ss.init(0)
    Xq, Xs, Ys = _edge_graph(False)
    nq, nt = Xq.shape[0], Ys.shape[1]
    gq = ss.DeviceGraph.from_sparse(Xq, Xs, Ys, dtype=dt)
    g0 = ss.DeviceGraph.from_sparse(None, Xs, Ys, dtype=dt)
    q = ss.DeviceQueries.from_sparse(g0, Xq)
    fn = getattr(lib, f"ss_support_{suf}")
    n = 4
    src = np.full((n, 64), -5, np.int32)
    con = np.full((n, 64), -5.0, dt)
    cnt = np.full(n, -5, np.int32)
    keep = (src.copy(), con.copy(), cnt.copy())

    def call(g, qs, kind, rows, targets, M, npairs=n):
        r = np.asarray(rows, dtype=np.int64)
        t = np.asarray(targets, dtype=np.int32)
        return fn(g._h, None if qs is None else qs._h, kind, npairs, r.ctypes.data, t.ctypes.data, M, src.ctypes.data,
                  con.ctypes.data, cnt.ctypes.data, _lib.SS_MEM_HOST)

    ok_r, ok_t = [0, 1, 2, 3], [0, 1, 2, 0]
    assert call(gq, None, _lib.SS_ROWS_QUERY, ok_r, ok_t, 0) == EINVAL
    assert call(gq, None, _lib.SS_ROWS_QUERY, ok_r, ok_t, 65) == EINVAL
    assert call(gq, None, _lib.SS_ROWS_QUERY, [0, 1, nq, 3], ok_t, 5) == EINVAL
    assert call(gq, None, _lib.SS_ROWS_QUERY, [0, -1, 2, 3], ok_t, 5) == EINVAL
    assert call(gq, None, _lib.SS_ROWS_QUERY, ok_r, [0, 1, nt, 0], 5) == EINVAL
    assert call(gq, None, _lib.SS_ROWS_QUERY, ok_r, [0, -1, 2, 0], 5) == EINVAL
    assert call(g0, None, _lib.SS_ROWS_QUERY, ok_r, ok_t, 5) == EINVAL            # the graph has no query rows of its own
    assert call(g0, None, _lib.SS_ROWS_LOO, [0, 150, 2, 3], ok_t, 5) == EINVAL
    assert call(gq, None, _lib.SS_ROWS_LOO, ok_r, ok_t, 5) == EINVAL              # leave-one-out needs nq == 0
    assert call(g0, q, _lib.SS_ROWS_LOO, ok_r, ok_t, 5) == EINVAL                 # ... and q == NULL
    assert call(gq, q, _lib.SS_ROWS_QUERY, ok_r, ok_t, 5) == EINVAL               # q belongs to g0
    assert call(g0, q, 3, ok_r, ok_t, 5) == EINVAL
    assert call(g0, q, _lib.SS_ROWS_SOURCE, ok_r, ok_t, 5) == EUNSUPPORTED
    assert call(g0, q, _lib.SS_ROWS_QUERY, ok_r, ok_t, 5, npairs=-1) == EINVAL
    other = getattr(lib, "ss_support_f64" if suf == "f32" else "ss_support_f32")
    r, t = np.asarray(ok_r, np.int64), np.asarray(ok_t, np.int32)
    assert other(g0._h, q._h, 0, n, r.ctypes.data, t.ctypes.data, 5, src.ctypes.data, con.ctypes.data, cnt.ctypes.data,
                 0) == EINVAL
    rng = np.random.default_rng(1)
    S = rng.random((150, 150))
    dense = ss.DeviceGraph.from_similarity(S[:5], (S + S.T) / 2, Ys, 0.5, dtype=dt)
    assert call(dense, None, _lib.SS_ROWS_QUERY, ok_r, ok_t, 5) == EUNSUPPORTED
    dense_asym = ss.DeviceGraph.from_similarity(S[:5], S, Ys, 0.5, dtype=dt)     # Ss need not be symmetric
    assert call(dense_asym, None, _lib.SS_ROWS_QUERY, ok_r, ok_t, 5) == EUNSUPPORTED
    for a, b in zip((src, con, cnt), keep):
        assert_same(a, b)
    # no pairs: a no-op after the checks
    assert call(g0, q, _lib.SS_ROWS_QUERY, ok_r, ok_t, 5, npairs=0) == 0
    assert call(g0, q, _lib.SS_ROWS_QUERY, ok_r, ok_t, 65, npairs=0) == EINVAL
    for a, b in zip((src, con, cnt), keep):
        assert_same(a, b)
    assert call(g0, q, _lib.SS_ROWS_QUERY, ok_r, ok_t, 64) == 0
    assert 64 < cnt[0] <= 150 and cnt[1] == 0 and cnt[2] in (0, 1) and 64 < cnt[3] <= 150
    assert (src[0] >= 0).all() and (np.diff(con[0]) <= 0).all()
    assert (src[1] == -1).all() and (con[1] == 0).all()
