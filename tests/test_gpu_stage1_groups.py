"""Stage 1 between the batches of a neighbour group (simspread.jl_amd/csrc/transfer.hip): coefficient tables kept in the
handles (SS_TRANSFER_COEF: 0 = gather inv1[a] per group as before, 1 / unset = table, 2 = table + the tag coef_table in the
path note).  They may not change one bit of one score.

Coefficient tables: query rows (all rows, a range that does not start at 0, at least three transfer batches), a
DeviceQueries block and leave-one-out rows (all, a sub-range) on the exactly summable inputs of tests/sparse_ref.py equal
the fp64 oracle bit for bit under both paths, and the two paths equal each other; source rows (no exactly summable
builder: kt is arbitrary) and the ordinary inputs of band_graph are held to equality of the two paths.  predict_kfold
passes per-fold reciprocals and never takes a table.  Zero coefficients (a feature without a source; leave-one-out: a
feature whose only source is the held-out one, and the dropped feature) give the oracle's scores, also where a whole
group or row has no other neighbour.  A handle whose degrees or blocks change must not serve a table of the old ones:
recut children, their parents and query sets made before, and set_cutoff on a dense-similarity graph, against fresh
handles.

Groups full of tails: one chunk (ns = 256 = SC), power-of-two degrees.  With a table the bounds of a sub-row are loaded
whatever its coefficient and the length is zeroed afterwards, and the tails of a group are found from those lengths.
Query rows with 64 neighbours of which 40 and 48 have 128 sources (head, 16-entry tail, rest loop: 10 and 12 rounds of
tails), with exactly 8 / 9 and 16 / 17 long sub-rows (the rounds in flight during the heads, with values / pattern-only,
and one more), groups of 1, 63, 64 and 65 neighbours; leave-one-out rows of full blocks of 129 and 65 sources (64 long
sub-rows in a group, and the dropped feature, itself long, among them).  (These are the inputs that were written for
fetching the late rounds of a group in one flight, which was measured and not kept: DESIGN.md 4.1.)"""
import functools

import numpy as np
import pytest
import scipy.sparse as sp

import simspread_jl_amd as ss
from oracle import simspread_oracle as O

import sparse_ref as S

pytestmark = pytest.mark.gpu

SWITCHES = ("SS_TRANSFER_COEF", "SS_TRANSFER_COEF_BYTES", "SS_TRANSFER_CHUNK", "SS_TRANSFER_ORDER",
            "SS_TRANSFER_U", "SS_TRANSFER_DUAL", "SS_TRANSFER_BYTES", "SS_TRANSFER_V", "SS_TRANSFER_FIX1", "SS_TRANSFER_LD")
DTYPES = [np.float32, np.float64]
PARAMS = [pytest.param(dt, w, id=f"{np.dtype(dt).name}-{'weighted' if w else 'pattern-only'}") for dt in DTYPES
          for w in (True, False)]
NQ = 200   # SS_TRANSFER_BYTES = 2^20 holds 80 rows of 3000 fp32 sums (40 fp64): three batches and more


@pytest.fixture(scope="module", autouse=True)
def _init():
    ss.init(0)


@pytest.fixture
def env(monkeypatch):
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)

    def set_(**kw):
        for k, v in kw.items():
            if v is None:
                monkeypatch.delenv(k, raising=False)
            else:
                monkeypatch.setenv(k, str(v))
    return set_


def _graph(Xq, Xs, Ys, dtype):
    return ss.DeviceGraph.from_sparse(None if Xq is None else Xq.astype(dtype), Xs.astype(dtype), Ys.astype(dtype),
                                      dtype=dtype)


def _frozen(a):
    a.setflags(write=False)
    return a


def _both(env, run, tagged=True):
    """run() under SS_TRANSFER_COEF = 2 and = 0: the table path is tagged (or, tagged=False, is not taken), the gather
    path never; the two results are equal.  Returns the table path's."""
    env(SS_TRANSFER_COEF=2)
    got = run()
    assert ("coef_table" in ss.path_last()) == tagged, ss.path_last()
    env(SS_TRANSFER_COEF=0)
    ref = run()
    assert "coef_table" not in ss.path_last(), ss.path_last()
    env(SS_TRANSFER_COEF=None)
    np.testing.assert_array_equal(got, ref)
    return got


# ----------------------------------------------------------------------------- coefficient tables
@functools.lru_cache(maxsize=None)
def _query_case(elem, weighted):
    inp = S.exact_query_for(elem, None, nq=NQ, weighted=weighted)
    return dict(inp, want=_frozen(S.oracle_query(inp["Xq"], inp["Xs"], inp["Ys"])))


@functools.lru_cache(maxsize=None)
def _loo_case(weighted):
    inp = S.exact_loo(weighted)
    return dict(inp, want=_frozen(S.oracle_loo(inp["X"], inp["Y"])))


@pytest.mark.parametrize("U", [8, 4])
@pytest.mark.parametrize("dtype,weighted", PARAMS)
def test_query_rows_and_query_sets_from_the_table_equal_the_gather_path_and_the_oracle(dtype, weighted, U, env):
    env(SS_TRANSFER_U=U)
    inp = _query_case(np.dtype(dtype).itemsize, weighted)
    want = inp["want"]
    g = _graph(inp["Xq"], inp["Xs"], inp["Ys"], dtype)
    S.assert_bitwise(_both(env, lambda: g.predict("query")), want, dtype, "query rows")
    S.assert_bitwise(_both(env, lambda: g.predict("query", 13, 77)), want[13:77], dtype, "query rows [13, 77)")
    env(SS_TRANSFER_BYTES=1 << 20)
    S.assert_bitwise(_both(env, lambda: g.predict("query")), want, dtype, "query rows, three batches and more")
    env(SS_TRANSFER_BYTES=None)
    # a query set: other rows than the graph's own, in another order
    rows = np.arange(150, 40, -1)
    q = ss.DeviceQueries.from_sparse(g, inp["Xq"][rows].astype(dtype))
    S.assert_bitwise(_both(env, lambda: g.predict(queries=q)), want[rows], dtype, "query set")
    S.assert_bitwise(_both(env, lambda: g.predict(queries=q, row_begin=7, row_end=30)), want[rows][7:30], dtype,
                     "query set [7, 30)")
    # the graph's own rows after the query set's: each handle has its own table
    S.assert_bitwise(_both(env, lambda: g.predict("query", 0, 20)), want[:20], dtype, "query rows after the query set")
    # source rows (two terms, two tables): the two paths agree
    _both(env, lambda: g.predict("source", 0, 70))
    _both(env, lambda: g.predict("source", 2990, 3000))
    # a table above the cap is not built
    env(SS_TRANSFER_COEF_BYTES=16)
    g2 = _graph(inp["Xq"], inp["Xs"], inp["Ys"], dtype)
    S.assert_bitwise(_both(env, lambda: g2.predict("query", 0, 20), tagged=False), want[:20], dtype, "above the cap")
    q.close()
    g.close()
    g2.close()


@pytest.mark.parametrize("U", [8, 4])
@pytest.mark.parametrize("dtype,weighted", PARAMS)
def test_leave_one_out_rows_from_the_table_equal_the_gather_path_and_the_oracle(dtype, weighted, U, env):
    env(SS_TRANSFER_U=U)
    inp = _loo_case(weighted)
    g = _graph(None, inp["X"], inp["Y"], dtype)
    S.assert_bitwise(_both(env, lambda: g.predict_loo()), inp["want"], dtype, "leave-one-out")
    assert "transfer_loo" in ss.path_last()
    S.assert_bitwise(_both(env, lambda: g.predict_loo(37, 201)), inp["want"][37:201], dtype, "leave-one-out [37, 201)")
    g.close()


@pytest.mark.parametrize("dtype,weighted", PARAMS)
def test_kfold_keeps_the_gather_path(dtype, weighted, env):
    inp = S.exact_kfold(weighted)
    g = _graph(None, inp["X"], inp["Y"], dtype)
    g.predict("source", 0, 8)           # (the tables of the source rows exist: k-fold must not pick them up)
    got = _both(env, lambda: g.predict_kfold(inp["fold"], inp["nfolds"]), tagged=False)
    S.assert_bitwise(got, S.oracle_kfold(inp["X"], inp["Y"], inp["fold"]), dtype, "k-fold")
    got = _both(env, lambda: g.predict_kfold_rows(inp["fold"], inp["nfolds"], 0, 40), tagged=False)
    g.close()


@pytest.mark.parametrize("dtype,weighted", PARAMS)
def test_ordinary_inputs_give_the_same_bits_on_both_paths(dtype, weighted, env):
    inp = S.band_graph(weighted)
    g = _graph(inp["Xq"], inp["X"], inp["Y"], dtype)
    for U in (8, 4):
        env(SS_TRANSFER_U=U)
        _both(env, lambda: g.predict("query"))
        _both(env, lambda: g.predict("query", 5, 41))
        _both(env, lambda: g.predict("source"))
    g.close()
    g = _graph(None, inp["X"], inp["Y"], dtype)
    for U in (8, 4):
        env(SS_TRANSFER_U=U)
        _both(env, lambda: g.predict_loo())
        _both(env, lambda: g.predict_loo(100, 333))
    g.close()


# ----------------------------------------------------------------------------- zero coefficients
@pytest.mark.parametrize("dtype,weighted", PARAMS)
def test_query_entries_of_a_feature_without_a_source_are_not_visited(dtype, weighted, env):
    """Rows of a query set: the empty feature alone (a row whose neighbours all have coefficient 0), 64 ordinary features
    and the empty one (it has the highest id: alone in the second group), and the empty one among 20."""
    inp = _query_case(np.dtype(dtype).itemsize, weighted)
    Xs, Ys, empty = inp["Xs"], inp["Ys"], inp["empty_feature"]
    kf = np.asarray((Xs != 0).sum(axis=0)).ravel()
    assert kf[empty] == 0 and empty == Xs.shape[1] - 1
    rng = np.random.default_rng(21)
    live = np.flatnonzero((kf > 0) & (kf <= 16))
    rows = [np.array([empty]), np.concatenate((np.sort(rng.choice(live, 64, replace=False)), [empty])),
            np.concatenate((np.sort(rng.choice(live, 19, replace=False)), [empty])), np.array([], dtype=np.int64)]
    qr = np.concatenate([np.full(len(c), r) for r, c in enumerate(rows)])
    qc = np.concatenate(rows)
    Xq = sp.csr_matrix((S._weights(rng, len(qc), weighted), (qr, qc)), shape=(len(rows), Xs.shape[1]))
    want = S.oracle_query(Xq, Xs, Ys)
    assert not want[0].any() and want[1].any()
    g = _graph(inp["Xq"], Xs, Ys, dtype)
    q = ss.DeviceQueries.from_sparse(g, Xq.astype(dtype))
    S.assert_bitwise(_both(env, lambda: g.predict(queries=q)), want, dtype, "zero coefficients, query rows")
    q.close()
    g.close()


@functools.lru_cache(maxsize=None)
def _loo_zero_case(weighted, nt=120, seed=22):
    """Full blocks of 2^j + 1 sources as exact_loo builds them, and: a block of ONE source (kf = 1 and the dropped
    feature: its row has no other neighbour), and a feature n (a source without entries or labels) that source p alone
    names: kf[n] - 1 = 0 for the rows that are not n.  p gives one label back, so ks[p] - 1 stays a power of two."""
    rng = np.random.default_rng(seed)
    sizes = (1, 3, 5, 9, 17, 33, 65)
    X, Y = S._block_square(rng, sizes, weighted, lambda size: size - 1, nt)
    n = X.shape[0]
    p = 1 + 3 + 2                                     # a source of the block of five
    X = sp.lil_matrix(sp.block_diag((X, sp.csr_matrix((1, 1)))))
    X[p, n] = 0.75 if weighted else 1.0
    X = sp.csr_matrix(X)
    X.sort_indices()
    Y = sp.lil_matrix(sp.vstack((Y, sp.csr_matrix((1, nt)))))
    Y[p, Y.rows[p][0]] = 0.0
    Y = sp.csr_matrix(Y)
    Y.eliminate_zeros()
    Y.sort_indices()
    kf, ks, _ = O.degrees(X, Y)
    assert kf[n] == 1 and kf[0] == 1 and X[0].nnz == 1 and S.is_pow2(ks[p] - 1)
    return dict(X=X, Y=Y, p=p, want=_frozen(S.oracle_loo(X, Y)))


@pytest.mark.parametrize("dtype,weighted", PARAMS)
def test_leave_one_out_entries_with_no_other_source_and_the_dropped_feature_are_not_visited(dtype, weighted, env):
    inp = _loo_zero_case(weighted)
    want = inp["want"]
    assert not want[0].any() and not want[-1].any() and want[inp["p"]].any()
    g = _graph(None, inp["X"], inp["Y"], dtype)
    got = _both(env, lambda: g.predict_loo())
    assert np.isfinite(got).all()
    S.assert_bitwise(got, want, dtype, "zero coefficients, leave-one-out")
    g.close()


# ----------------------------------------------------------------------------- staleness
def _cut(M, alpha):
    M = sp.csr_matrix(M, copy=True)
    M.data[M.data < alpha] = 0.0
    M.eliminate_zeros()
    return M


@pytest.mark.parametrize("dtype", DTYPES, ids=["float32", "float64"])
def test_recut_children_parents_and_query_sets_serve_their_own_coefficients(dtype, env):
    env(SS_TRANSFER_COEF=2)
    inp = S.band_graph(True)
    Xq, X, Y = (inp[k].astype(dtype) for k in ("Xq", "X", "Y"))
    a1, a2 = 0.6, 0.8
    fresh = {}
    for a in (a1, a2):
        f = _graph(_cut(Xq, a), _cut(X, a), Y, dtype)
        fl = _graph(None, _cut(X, a), Y, dtype)
        fresh[a] = (f.predict("query"), f.predict("source"), fl.predict_loo())
        f.close()
        fl.close()
    root = _graph(Xq, X, Y, dtype)
    rootl = _graph(None, X, Y, dtype)
    p, pl = root.recut(a1), rootl.recut(a1)
    q = ss.DeviceQueries.from_sparse(p, _cut(Xq, a1))

    def check(g, gl, a):
        np.testing.assert_array_equal(g.predict("query"), fresh[a][0])
        assert "coef_table" in ss.path_last()
        np.testing.assert_array_equal(g.predict("source"), fresh[a][1])
        np.testing.assert_array_equal(gl.predict_loo(), fresh[a][2])
        assert "coef_table" in ss.path_last()

    check(p, pl, a1)                          # the tables of the parent at a1 exist now
    np.testing.assert_array_equal(p.predict(queries=q), fresh[a1][0])
    c, cl = p.recut(a2), pl.recut(a2)
    check(c, cl, a2)                          # the child at a2 builds its own
    check(p, pl, a1)                          # the parent is what it was
    np.testing.assert_array_equal(p.predict(queries=q), fresh[a1][0])   # and so is the query set made before the recut
    c2 = p.recut(a2)                          # a second child, the first one's tables long built
    check(c2, cl, a2)
    for h in (q, c, cl, c2, p, pl, root, rootl):
        h.close()


@pytest.mark.parametrize("dtype", DTYPES, ids=["float32", "float64"])
def test_set_cutoff_on_a_dense_similarity_graph_matches_a_fresh_handle(dtype, env):
    env(SS_TRANSFER_COEF=2)
    rng = np.random.default_rng(23)
    ns, nq, nt = 300, 40, 50
    Ss = rng.random((ns, ns))
    Ss = ((Ss + Ss.T) / 2).astype(np.float32).astype(np.float64)
    np.fill_diagonal(Ss, 1.0)
    Sq = rng.random((nq, ns)).astype(np.float32).astype(np.float64)
    Y = sp.random(ns, nt, density=0.1, format="csr", random_state=rng)
    Y.data[:] = 1.0

    def scores(g):
        return g.predict("query"), g.predict("source"), g.predict_loo()

    g = ss.DeviceGraph.from_similarity(Sq, Ss, Y, 0.6, weighted=True, dtype=dtype)
    scores(g)
    for alpha, weighted in ((0.8, True), (0.5, False), (0.6, True)):
        f = ss.DeviceGraph.from_similarity(Sq, Ss, Y, alpha, weighted=weighted, dtype=dtype)
        want = scores(f)
        f.close()
        for got, w in zip(scores(g.set_cutoff(alpha, weighted)), want):
            np.testing.assert_array_equal(got, w)
    g.close()


# ----------------------------------------------------------------------------- groups full of tails
NS1 = 256   # one chunk: SC = 256
NLONG, NSHORT = 80, 80


def _labels(rng, Xs, nt):
    """0/1 labels that make ks a power of two: 2^ceil(log2(rx + 1)) - rx per source among the first nt - 1 targets"""
    yr, yc = [], []
    for s, r in enumerate(np.diff(Xs.indptr)):
        n = S._pow2_at_least(r + 1) - int(r)
        yr.append(np.full(n, s))
        yc.append(rng.choice(nt - 1, size=n, replace=False))
    Ys = sp.csr_matrix((np.ones(sum(map(len, yc))), (np.concatenate(yr), np.concatenate(yc))), shape=(Xs.shape[0], nt))
    Ys.sort_indices()
    return Ys


@functools.lru_cache(maxsize=None)
def _tails_query_case(weighted, nt=400, seed=24):
    """Features 0 .. 79 have 128 sources (one sub-row: a head of 64, a tail of 16, 48 entries for the rest loop),
    features 80 .. 159 have 8, 16, 32 or 64.  Rows by name; their feature ids ascend, so `long features first` holds."""
    rng = np.random.default_rng(seed)
    nf = NLONG + NSHORT
    deg = [128] * NLONG + [int(d) for d in rng.choice((8, 16, 32, 64), size=NSHORT)]
    cols = np.concatenate([np.full(d, a) for a, d in enumerate(deg)])
    srcs = np.concatenate([rng.choice(NS1, size=d, replace=False) for d in deg])
    Xs = sp.csr_matrix((S._weights(rng, len(cols), weighted), (srcs, cols)), shape=(NS1, nf))
    Xs.sort_indices()
    Ys = _labels(rng, Xs, nt)
    longs, shorts = np.arange(NLONG), np.arange(NLONG, nf)

    def pick(nl, nshort):
        return np.concatenate((rng.choice(longs, nl, replace=False), rng.choice(shorts, nshort, replace=False)))

    rows = {"64 neighbours, 40 long": pick(40, 24), "64 neighbours, 48 long": pick(48, 16),
            "8 long": pick(8, 12), "9 long": pick(9, 12), "16 long": pick(16, 9), "17 long": pick(17, 9),
            "1 neighbour, long": pick(1, 0), "1 neighbour, short": pick(0, 1), "63 neighbours": pick(30, 33),
            "64 neighbours": pick(33, 31), "65 neighbours, a short one last": pick(35, 30),
            "65 neighbours, all long": pick(65, 0), "129 neighbours": pick(70, 59), "every feature": np.arange(nf),
            "every long feature": longs, "no neighbour": np.array([], dtype=np.int64)}
    qr = np.concatenate([np.full(len(c), r) for r, c in enumerate(rows.values())])
    qc = np.concatenate([np.asarray(c, dtype=np.int64) for c in rows.values()])
    Xq = sp.csr_matrix((S._weights(rng, len(qc), weighted), (qr, qc)), shape=(len(rows), nf))
    Xq.sort_indices()
    # what the names promise, one chunk, powers of two, and sums that are exact in fp32 in any order
    assert S.chunk_width(NS1, nf, Xs.nnz, 4) == (NS1, 1) == S.chunk_width(NS1, nf, Xs.nnz, 8)
    kf, ks, _ = O.degrees(Xs, Ys)
    assert S.is_pow2(kf).all() and S.is_pow2(ks).all()
    nlong = [(int((Xq[r].indices < NLONG).sum()), Xq[r].nnz) for r in range(Xq.shape[0])]
    names = list(rows)
    for name, want in (("64 neighbours, 40 long", (40, 64)), ("64 neighbours, 48 long", (48, 64)), ("8 long", (8, 20)),
                       ("9 long", (9, 21)), ("16 long", (16, 25)), ("17 long", (17, 26)), ("63 neighbours", (30, 63)),
                       ("64 neighbours", (33, 64)), ("65 neighbours, a short one last", (35, 65))):
        assert nlong[names.index(name)] == want, (name, nlong[names.index(name)])
    want = S.oracle_query(Xq, Xs, Ys)
    e = (8 if weighted else 0) + int(np.log2(kf.max())) + int(np.log2(ks.max()))
    acc = (Xq @ sp.diags(1.0 / kf) @ Xs.T).toarray()
    assert acc.max() * 2.0 ** (e - int(np.log2(ks.max()))) < 2 ** 24 and want.max() * 2.0 ** e < 2 ** 24
    assert (want * 2.0 ** e == np.round(want * 2.0 ** e)).all()
    return dict(Xq=Xq, Xs=Xs, Ys=Ys, want=_frozen(want), names=names)


@functools.lru_cache(maxsize=None)
def _tails_loo_case(weighted, nt=200, seed=25):
    """exact_loo's construction on 256 sources in one chunk: full blocks of 129, 65, 33, 17, 9 and 3 sources.  A row of
    the first block has 129 neighbours, 128 of them long (129 entries: head, tail, rest) and the dropped one."""
    rng = np.random.default_rng(seed)
    X, Y = S._block_square(rng, (129, 65, 33, 17, 9, 3), weighted, lambda size: size - 1, nt)
    assert X.shape[0] == NS1 and S.chunk_width(NS1, NS1, X.nnz, 4) == (NS1, 1) == S.chunk_width(NS1, NS1, X.nnz, 8)
    return dict(X=X, Y=Y, want=_frozen(S.oracle_loo(X, Y)))


@pytest.mark.parametrize("dtype,weighted", PARAMS)
def test_groups_full_of_tails_query_rows(dtype, weighted, env):
    inp = _tails_query_case(weighted)
    g = _graph(inp["Xq"], inp["Xs"], inp["Ys"], dtype)
    for U in (8, 4):
        env(SS_TRANSFER_U=U)
        got = _both(env, lambda: g.predict("query"))
        bits = np.uint32 if dtype is np.float32 else np.uint64
        for r in np.flatnonzero((got.view(bits) != inp["want"].astype(dtype).view(bits)).any(axis=1)):
            print(f"row {r} ({inp['names'][r]}) differs")
        S.assert_bitwise(got, inp["want"], dtype, f"many tails, query rows, U = {U}")
        S.assert_bitwise(_both(env, lambda: g.predict("query", 1, 4)), inp["want"][1:4], dtype, "rows [1, 4)")
    g.close()


@pytest.mark.parametrize("dtype,weighted", PARAMS)
def test_groups_full_of_tails_leave_one_out(dtype, weighted, env):
    inp = _tails_loo_case(weighted)
    g = _graph(None, inp["X"], inp["Y"], dtype)
    for U in (8, 4):
        env(SS_TRANSFER_U=U)
        S.assert_bitwise(_both(env, lambda: g.predict_loo()), inp["want"], dtype, f"many tails, LOO, U = {U}")
        S.assert_bitwise(_both(env, lambda: g.predict_loo(120, 200)), inp["want"][120:200], dtype,
                         "many tails, LOO [120, 200)")
    g.close()
