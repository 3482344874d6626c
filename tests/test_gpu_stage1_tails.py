"""Stage 1, the packed tails of long sub-rows (simspread.jl_amd/csrc/transfer.hip): entries 64..79 of up to four long
sub-rows of a batch come from one load pair, each tail is folded on its own, entries from position 80 on take the rest loop.

Graphs: ns = 2048 sources cut by SS_TRANSFER_CHUNK = 256 into 8 chunks.  Planted features have exactly 0, 1, 63, 64,
65, 79, 80, 81, 128, 129 and 200 sources inside chunk 0 (three features of every length above 64, so that a batch of 8
can hold 8 tails) and the rest of their power-of-two degree in one other chunk; the feature with the highest id has a
long sub-row in the last chunk, the last one the operand stores, so its packed tail load reaches into the slack.

Query rows (exactly summable inputs, as tests/sparse_ref.py builds them: degrees are powers of two, weights k/16, every
partial sum in any order is representable) equal the fp64 oracle bit for bit in fp32 and fp64: batches with 0, 1, 4, 5
and 8 tails, a tail in the last, partial batch of a row and of a second 64-neighbour group, rows with fewer
neighbours than a batch, the empty feature (coefficient 0: its bounds are never loaded), weighted and pattern-only,
under every batch size and the opt-in kernels that sum in floating point.  The same rows alone and inside a larger range
give the same bits.

Leave-one-out rows (the held-out source's own feature is long and takes coefficient 0: its bounds are not loaded, it
must not count as a tail), two-term source rows (a hub target gives the second operand long sub-rows too) and
predict_kfold_rows run on the square form of the same graph and stay within the per-score bands of
sparse_ref.band_graph_scores against the fp64 oracle, as the band tests of test_gpu_sparse.py do."""
import functools

import numpy as np
import pytest
import scipy.sparse as sp

import simspread_jl_amd as ss
from oracle import simspread_oracle as O

import sparse_ref as S

pytestmark = pytest.mark.gpu

NS, SC, NCH = 2048, 256, 8
LENGTHS = (0, 1, 63, 64, 65, 79, 80, 81, 128, 129, 200)       # sources of a planted feature inside chunk 0
SWITCHES = ("SS_TRANSFER_CHUNK", "SS_TRANSFER_ORDER", "SS_TRANSFER_U", "SS_TRANSFER_DUAL", "SS_CHUNK_SCHED",
            "SS_TRANSFER_BYTES", "SS_TRANSFER_V", "SS_TRANSFER_FIX", "SS_TRANSFER_FIX1", "SS_TRANSFER_LD",
            "SS_TRANSFER_ALIGN", "SS_TRANSFER_NW", "SS_TRANSFER_WIDE", "SS_TRANSFER_WIDE2", "SS_TRANSFER_QFLAT")
# name -> (switches, stage-1 tags, fp32 only)
KERNELS = {
    "U=8": ({"SS_TRANSFER_U": "8"}, {"transfer"}, False),
    "U=4": ({"SS_TRANSFER_U": "4"}, {"transfer"}, False),
    "U=16": ({"SS_TRANSFER_U": "16"}, {"transfer"}, False),
    "default": ({}, {"transfer"}, False),
    "dual": ({"SS_TRANSFER_DUAL": "1"}, {"transfer"}, False),
    "buffer loads, U=8": ({"SS_TRANSFER_LD": "1", "SS_TRANSFER_U": "8"}, {"transfer", "buffer_loads"}, True),
    "buffer loads, U=4": ({"SS_TRANSFER_LD": "1", "SS_TRANSFER_U": "4"}, {"transfer", "buffer_loads"}, True),
    "block kernel, U=8": ({"SS_TRANSFER_V": "2", "SS_TRANSFER_FIX": "0", "SS_TRANSFER_U": "8"}, {"transfer_block"}, False),
    "block kernel, U=4": ({"SS_TRANSFER_V": "2", "SS_TRANSFER_FIX": "0", "SS_TRANSFER_U": "4"}, {"transfer_block"}, False),
}
STAGE1_TAGS = {"transfer", "transfer_loo", "transfer_block", "buffer_loads", "fixed_point", "wide", "wide2", "qflat"}
DTYPES = [np.float32, np.float64]


def _kernel_params(names):
    return [pytest.param(dt, n, id=f"{np.dtype(dt).name}-{n}") for dt in DTYPES for n in names
            if not (KERNELS[n][2] and dt is np.float64)]


@pytest.fixture(scope="module", autouse=True)
def _init():
    ss.init(0)


@pytest.fixture
def switches(monkeypatch):
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)

    def set_(env):
        monkeypatch.setenv("SS_TRANSFER_CHUNK", str(SC))
        for k, v in env.items():
            monkeypatch.setenv(k, v)
    return set_


def _graph(Xq, Xs, Ys, dtype):
    return ss.DeviceGraph.from_sparse(None if Xq is None else Xq.astype(dtype), Xs.astype(dtype), Ys.astype(dtype),
                                      dtype=dtype)


# ----------------------------------------------------------------------------- the planted features
def _planted(rng):
    """[(length in chunk 0, sources)]: three features of every length above 64, two of the others; the degree is the
    next power of two (16 for length 0), the sources outside chunk 0 sit in one of the chunks 1..6."""
    out = []
    for n in LENGTHS:
        for _ in range(3 if n > 64 else 2):
            kf = 16 if n == 0 else S._pow2_at_least(n)
            c = int(rng.integers(1, NCH - 1))
            s = np.concatenate((rng.choice(SC, size=n, replace=False), c * SC + rng.choice(SC, size=kf - n, replace=False)))
            out.append((n, np.sort(s)))
    return out


def _labels(rng, Xs, nt, hub=None):
    """0/1 labels that make ks a power of two: 2^ceil(log2(rx + 1)) - rx per source among the first nt - 1 targets; hub:
    these sources get target 0 among theirs."""
    ns = Xs.shape[0]
    rx = np.diff(Xs.indptr)
    yr, yc = [], []
    for s in range(ns):
        n = S._pow2_at_least(rx[s] + 1) - int(rx[s])
        if hub is not None and hub[s]:
            c = np.concatenate(([0], 1 + rng.choice(nt - 2, size=n - 1, replace=False)))
        else:
            c = 1 + rng.choice(nt - 2, size=n, replace=False)
        yr.append(np.full(n, s))
        yc.append(c)
    Ys = sp.csr_matrix((np.ones(sum(map(len, yc))), (np.concatenate(yr), np.concatenate(yc))), shape=(ns, nt))
    Ys.sort_indices()
    return Ys


@functools.lru_cache(maxsize=None)
def _query_case(weighted, nf=320, nt=96, seed=11):
    """Xq, Xs, Ys, the oracle's scores and the rows by name.  Feature ids: the planted features are spread at random
    over 0 .. nf - 3; nf - 2 has no source; nf - 1 has 72 sources in the last chunk (and 56 in chunk 6)."""
    rng = np.random.default_rng(seed)
    planted = _planted(rng)
    ids = np.sort(rng.choice(nf - 2, size=len(planted), replace=False))
    rng.shuffle(ids)
    feat = {}
    for a, (n, s) in zip(ids, planted):
        feat[int(a)] = s
    for a in range(nf - 2):
        if a not in feat:
            feat[a] = rng.choice(NS, size=1 << int(rng.integers(0, 6)), replace=False)
    feat[nf - 1] = np.concatenate(((NCH - 1) * SC + rng.choice(SC, size=72, replace=False),
                                   (NCH - 2) * SC + rng.choice(SC, size=56, replace=False)))
    cols = np.concatenate([np.full(len(s), a) for a, s in feat.items()])
    srcs = np.concatenate(list(feat.values()))
    Xs = sp.csr_matrix((S._weights(rng, len(cols), weighted), (srcs, cols)), shape=(NS, nf))
    Xs.sort_indices()
    Ys = _labels(rng, Xs, nt)
    length = {int(a): n for a, (n, _) in zip(ids, planted)}
    longs = np.array(sorted(a for a, n in length.items() if n > 64))
    shorts = np.array(sorted(a for a in range(nf - 2) if length.get(a, 0) <= 64))
    every = np.array(sorted(length))

    def pick(nl, nshort, extra=()):
        return np.concatenate((rng.choice(longs, size=nl, replace=False), rng.choice(shorts, size=nshort, replace=False),
                               np.array(extra, dtype=np.int64)))

    def tail_last(nshort):
        """nshort short features and one long one with the highest id of the row"""
        a = int(longs[-1])
        return np.concatenate((rng.choice(shorts[shorts < a], size=nshort, replace=False), [a]))

    rows = {}
    for t in (0, 1, 4, 5, 8):
        rows[f"8 neighbours, {t} tails"] = pick(t, 8 - t)
    rows["16 neighbours, 8 tails"] = pick(8, 8)
    rows["every planted feature"] = every
    rows["every long feature and the last stored sub-row"] = np.concatenate((longs, [nf - 1]))
    rows["the last stored sub-row alone"] = np.array([nf - 1])
    rows["13 neighbours, the tail last"] = tail_last(12)
    rows["67 neighbours, the tail last"] = tail_last(66)
    rows["3 neighbours, 2 tails"] = pick(2, 1)
    rows["1 neighbour, a tail"] = pick(1, 0)
    rows["the empty feature and 3 tails"] = pick(3, 2, (nf - 2,))
    rows["the empty feature alone"] = np.array([nf - 2])
    rows["no neighbour"] = np.array([], dtype=np.int64)
    rows["130 neighbours, every long feature"] = np.union1d(longs, rng.choice(shorts, size=130 - len(longs), replace=False))
    names = list(rows)
    while len(rows) < 70:
        n = int(rng.integers(1, 41))
        rows[f"random {len(rows)}"] = np.union1d(rng.choice(longs, size=min(n, int(rng.integers(0, 9))), replace=False),
                                                 rng.choice(shorts, size=n, replace=False))
    qr = np.concatenate([np.full(len(c), q) for q, c in enumerate(rows.values())])
    qc = np.concatenate([np.asarray(c, dtype=np.int64) for c in rows.values()])
    Xq = sp.csr_matrix((S._weights(rng, len(qr), weighted), (qr, qc)), shape=(len(rows), nf))
    Xq.sort_indices()
    want = S.oracle_query(Xq, Xs, Ys)
    want.setflags(write=False)
    return dict(Xq=Xq, Xs=Xs, Ys=Ys, want=want, names=names, length=length, longs=longs, last=nf - 1, empty=nf - 2,
                weighted=weighted)


def _batch_tails(Xq, q, longs, U):
    """Tails per batch of U neighbours of row q (neighbours in column order, 64 to a group)."""
    c = Xq.indices[Xq.indptr[q]:Xq.indptr[q + 1]]
    is_long = np.isin(c, longs)
    return [int(is_long[g + u:min(g + u + U, g + 64)].sum()) for g in range(0, len(c), 64) for u in range(0, min(64, len(c) - g), U)]


def test_the_inputs_are_what_the_tests_say():
    """Sub-row lengths of chunk 0, powers of two, the exactness of every partial sum in fp32, the batches' tails, and the
    last stored sub-row (no device needed, but the cases below rest on it)."""
    for weighted in (True, False):
        inp = _query_case(weighted)
        Xq, Xs, Ys = inp["Xq"], inp["Xs"], inp["Ys"]
        assert S.chunk_width(NS, Xs.shape[1], Xs.nnz, 4, SC) == (SC, NCH) == S.chunk_width(NS, Xs.shape[1], Xs.nnz, 8, SC)
        in0 = np.asarray((Xs[:SC] != 0).sum(axis=0)).ravel()
        for a, n in inp["length"].items():
            assert in0[a] == n
        assert set(LENGTHS) <= set(in0.tolist()) and sorted(np.flatnonzero(in0 > 64)) == sorted(inp["longs"])
        kf, ks, _ = O.degrees(Xs, Ys)
        assert S.is_pow2(kf[kf > 0]).all() and S.is_pow2(ks).all() and kf[inp["empty"]] == 0
        # the last sub-row the operand stores (chunk-major, then by feature) is long
        last = np.asarray((Xs[(NCH - 1) * SC:] != 0).sum(axis=0)).ravel()
        assert last[inp["last"]] == 72 and inp["last"] == Xs.shape[1] - 1
        # every term is a multiple of 2^-e and the largest sums stay below 2^24 quanta: exact in any order in fp32
        e = (8 if weighted else 0) + int(np.log2(kf.max())) + int(np.log2(ks.max()))
        acc = (Xq @ sp.diags(np.where(kf > 0, 1.0 / np.maximum(kf, 1), 0.0)) @ Xs.T).toarray()
        assert acc.max() * 2.0 ** (e - int(np.log2(ks.max()))) < 2 ** 24 and inp["want"].max() * 2.0 ** e < 2 ** 24
        q = inp["want"] * 2.0 ** e
        assert (q == np.round(q)).all()
        names = inp["names"]
        for U, t in ((8, 0), (8, 1), (8, 4), (8, 5), (8, 8)):
            assert _batch_tails(Xq, names.index(f"8 neighbours, {t} tails"), inp["longs"], U) == [t]
        seen = {U: {t for q in range(Xq.shape[0]) for t in _batch_tails(Xq, q, inp["longs"], U)} for U in (4, 8)}
        assert seen[8] >= {0, 1, 4, 5, 8} and seen[4] >= {0, 1, 4}
        for name in ("13 neighbours, the tail last", "67 neighbours, the tail last"):
            assert _batch_tails(Xq, names.index(name), inp["longs"], 8)[-1] == 1
            assert (Xq[names.index(name)].nnz % 64) % 8 != 0


# ----------------------------------------------------------------------------- query rows, bit for bit
@pytest.mark.parametrize("weighted", [True, False], ids=["weighted", "pattern-only"])
@pytest.mark.parametrize("dtype,name", _kernel_params(list(KERNELS)))
def test_query_rows_with_tails_equal_the_oracle_bit_for_bit(dtype, name, weighted, switches):
    env, tags, _ = KERNELS[name]
    switches(env)
    inp = _query_case(weighted)
    want = inp["want"]
    g = _graph(inp["Xq"], inp["Xs"], inp["Ys"], dtype)
    got = g.predict("query")
    assert set(ss.path_last()) & STAGE1_TAGS == tags, ss.path_last()
    bits = np.uint32 if dtype is np.float32 else np.uint64
    w = want.astype(dtype)
    for q in np.flatnonzero((got.view(bits) != w.view(bits)).any(axis=1))[:8]:
        print(f"row {q} ({inp['names'][q] if q < len(inp['names']) else 'random'}) differs")
    S.assert_bitwise(got, want, dtype, f"query rows, {name}")
    # the same rows alone and inside a larger range: the sums of a row do not depend on its launch
    for a, b in ((0, 1), (4, 5), (6, 9), (13, 18), (9, 12)):
        S.assert_bitwise(g.predict("query", a, b), want[a:b], dtype, f"query rows [{a},{b}), {name}")
    g.close()


# ----------------------------------------------------------------------------- the other flavours, within their bands
@functools.lru_cache(maxsize=None)
def _square_case(weighted, nt=96, seed=12):
    """The planted features as features 0 .. of a square X (feature a is named after source a, non-zero diagonal), the
    other features short; target 0 is a label of 200 sources of chunk 0.  Rows 0 .. 69 are sources of chunk 0, members
    of about nine long features each, and most of them name their own long feature."""
    rng = np.random.default_rng(seed)
    planted = _planted(rng)
    ids = rng.permutation(len(planted))
    feat = {int(a): s for a, (_, s) in zip(ids, planted)}
    for a in range(NS):
        if a not in feat:
            feat[a] = rng.choice(NS, size=int(rng.integers(1, 7)), replace=False)
        feat[a] = np.union1d(feat[a], [a])
    cols = np.concatenate([np.full(len(s), a) for a, s in feat.items()])
    srcs = np.concatenate(list(feat.values()))
    vals = (1.0 - 0.5 * rng.random(len(cols))).astype(np.float32).astype(np.float64) if weighted else np.ones(len(cols))
    X = sp.csr_matrix((vals, (srcs, cols)), shape=(NS, NS))
    X.sort_indices()
    hub = np.zeros(NS, dtype=bool)
    hub[rng.choice(SC, size=200, replace=False)] = True
    Y = _labels(rng, X, nt, hub)
    fold = (np.arange(NS) % 5).astype(np.int32)
    rows = np.arange(70)
    in0 = np.asarray((X[:SC] != 0).sum(axis=0)).ravel()
    assert (in0[:len(planted)] > 64).sum() >= 20 and in0.max() >= 200
    ref = dict(loo=(S.oracle_loo(X, Y, rows), S.counts_loo(X, Y, rows)),
               source=(S.oracle_source(X, Y)[:70], tuple(c[:70] for c in S.counts_query(None, X, Y, source_rows=True))))
    return dict(X=X, Y=Y, fold=fold, ref=ref)


@functools.lru_cache(maxsize=None)
def _kfold_ref(weighted):
    """Rows 0 .. 69 of the 5-fold sweep: the oracle fold by fold on the graph without the fold's members."""
    inp = _square_case(weighted)
    X, Y, fold = inp["X"], inp["Y"], inp["fold"]
    want = np.zeros((70, Y.shape[1]))
    chain, addends = np.zeros_like(want), np.zeros_like(want)
    for phi in range(5):
        keep = np.flatnonzero(fold != phi)
        mem = np.flatnonzero(fold[:70] == phi)
        Xq, Xs, Ys = X[mem][:, keep], X[keep][:, keep], Y[keep]
        want[mem] = S.oracle_query(Xq, Xs, Ys)
        chain[mem], addends[mem] = S.counts_query(Xq, Xs, Ys)
    return want, (chain, addends)


@pytest.mark.parametrize("weighted", [True, False], ids=["weighted", "pattern-only"])
@pytest.mark.parametrize("dtype,name", _kernel_params(["U=8", "U=4"]))
def test_leave_one_out_source_and_kfold_rows_with_tails_within_their_bands(dtype, name, weighted, switches):
    switches(KERNELS[name][0])
    inp = _square_case(weighted)
    X, Y, fold = inp["X"], inp["Y"], inp["fold"]
    g = _graph(None, X, Y, dtype)

    def check(got, mode, want, counts):
        band = S.band_graph_scores(want, counts[0], counts[1], dtype, sell_chunks=1)
        S.assert_band(got, want, band, f"{mode}, {name}, {np.dtype(dtype).name}")

    check(g.predict_loo(0, 70), "leave-one-out", *inp["ref"]["loo"])
    assert "transfer_loo" in ss.path_last()
    whole = g.predict_loo(0, 70)
    np.testing.assert_array_equal(g.predict_loo(3, 11), whole[3:11])
    check(g.predict("source", 0, 70), "source rows", *inp["ref"]["source"])
    assert "transfer" in ss.path_last()
    np.testing.assert_array_equal(g.predict("source", 5, 6), g.predict("source", 0, 70)[5:6])
    check(g.predict_kfold_rows(fold, 5, 0, 70), "k-fold rows", *_kfold_ref(weighted))
    g.close()
