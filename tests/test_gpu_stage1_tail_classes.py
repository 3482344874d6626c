"""Stage 1, tails cut by column class (simspread.jl_amd/csrc/assemble.hip "class-pure tails", transfer.hip "tails"):
column j of a chunk has class j & 3, the sub-row of operand row a class a & 3; positions 64..79 of a long sub-row hold
only columns of the sub-row's class (or sentinels), a round of the kernel takes one long sub-row of each class and
folds the four tails in ONE plain read-add-write.  Long sub-rows of one class share no round; more than 16 of a class in
a group of 64 neighbours leave the slots and take the rest loop from position 64.

Main graph: ns = 2048 sources cut by SS_TRANSFER_CHUNK = 256 into 8 chunks.  Planted features have an exact number of
sources inside chunk 0 and the rest of their power-of-two degree in one other chunk:
  same class, same columns     five features of class 1 on the same 70 sources: five rounds, or addends are lost
  four classes, same columns   four features of the classes 0..3 on the same 72 sources: one round, one fold
  unbalanced classes           nine features of class 0, one of each other class: rounds with empty slots
  overflow                     twenty features of class 2 named by one row of 56 neighbours
  fillers                      class 2 with 80 sources, none in a class-2 column; 70 sources of which 3 in the class;
                               the feature with the highest id: 72 sources in the last chunk, 2 of its class -- the last
                               sub-row the operand stores, its tail load reaches into the slack
  lengths                      65, 79, 80, 81, 96 and 200 with random columns, one feature of every class each
A sub-row of 300 entries does not fit into a chunk of 256 columns: length 300 (above the 256 entries the bank schedule
used to cover), one feature of every class, lives in a graph of its own with ns = 4096 and SS_TRANSFER_CHUNK = 512.
The smallest chunk with tails, SS_TRANSFER_CHUNK = 68 (ns = 544), has a graph of its own with full sub-rows of 65..68
entries in every class.

Query rows (exactly summable inputs, as tests/sparse_ref.py builds them) equal the fp64 oracle bit for bit in fp32 and
fp64, weighted and pattern-only, under every kernel that takes tails and under SS_CHUNK_SCHED=0; the same rows alone and
inside a larger range give the same bits.  Leave-one-out rows, two-term source rows (a hub target gives the second
operand a long sub-row) and predict_kfold_rows run on the square form of the main graph within the per-score bands of
sparse_ref.band_graph_scores."""
import functools

import numpy as np
import pytest
import scipy.sparse as sp

import simspread_jl_amd as ss
from oracle import simspread_oracle as O

import sparse_ref as S

SWITCHES = ("SS_TRANSFER_CHUNK", "SS_TRANSFER_ORDER", "SS_TRANSFER_U", "SS_TRANSFER_DUAL", "SS_CHUNK_SCHED",
            "SS_TRANSFER_BYTES", "SS_TRANSFER_V", "SS_TRANSFER_FIX", "SS_TRANSFER_FIX1", "SS_TRANSFER_LD",
            "SS_TRANSFER_ALIGN", "SS_TRANSFER_NW", "SS_TRANSFER_WIDE", "SS_TRANSFER_WIDE2", "SS_TRANSFER_QFLAT",
            "SS_TRANSFER_COEF")
# name -> (switches, stage-1 tags, fp32 only)
KERNELS = {
    "default": ({}, {"transfer"}, False),
    "U=4": ({"SS_TRANSFER_U": "4"}, {"transfer"}, False),
    "U=8": ({"SS_TRANSFER_U": "8"}, {"transfer"}, False),
    "U=16": ({"SS_TRANSFER_U": "16"}, {"transfer"}, False),
    "dual": ({"SS_TRANSFER_DUAL": "1"}, {"transfer"}, False),
    "buffer loads": ({"SS_TRANSFER_LD": "1"}, {"transfer", "buffer_loads"}, True),
    "block kernel": ({"SS_TRANSFER_V": "2", "SS_TRANSFER_FIX": "0"}, {"transfer_block"}, False),
    "unscheduled": ({"SS_CHUNK_SCHED": "0"}, {"transfer"}, False),
}
STAGE1_TAGS = {"transfer", "transfer_loo", "transfer_block", "buffer_loads", "fixed_point", "wide", "wide2", "qflat"}
DTYPES = [np.float32, np.float64]
LENGTHS = (65, 79, 80, 81, 96, 200)
# graph -> (ns, SS_TRANSFER_CHUNK = SC, features)
GRAPHS = {"main": (2048, 256, 512), "length 300": (4096, 512, 128), "smallest chunk": (544, 68, 128)}


def _kernel_params(names):
    return [pytest.param(dt, n, id=f"{np.dtype(dt).name}-{n}") for dt in DTYPES for n in names
            if not (KERNELS[n][2] and dt is np.float64)]


@pytest.fixture(scope="module")
def device():
    ss.init(0)


@pytest.fixture
def switches(monkeypatch):
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)

    def set_(chunk, env):
        monkeypatch.setenv("SS_TRANSFER_CHUNK", str(chunk))
        for k, v in env.items():
            monkeypatch.setenv(k, v)
    return set_


def _graph(Xq, Xs, Ys, dtype):
    return ss.DeviceGraph.from_sparse(None if Xq is None else Xq.astype(dtype), Xs.astype(dtype), Ys.astype(dtype),
                                      dtype=dtype)


# ----------------------------------------------------------------------------- the planted features
def _columns(rng, SC, n, cls=None, in_class=None):
    """n columns of a chunk; in_class of them in class cls (cls None: at random)."""
    if cls is None:
        return np.sort(rng.choice(SC, size=n, replace=False))
    own = np.arange(cls, SC, 4)
    other = np.setdiff1d(np.arange(SC), own)
    return np.sort(np.concatenate((rng.choice(own, size=in_class, replace=False),
                                   rng.choice(other, size=n - in_class, replace=False))))


def _feature(rng, SC, nch, cols, chunk=0):
    """Sources of a feature: `cols` inside `chunk`, the rest of the next power of two in one other chunk."""
    kf = S._pow2_at_least(len(cols))
    others = [c for c in range(nch) if c != chunk and c != nch - 1]
    c = int(rng.choice(others))
    return np.sort(np.concatenate((chunk * SC + cols, c * SC + rng.choice(SC, size=kf - len(cols), replace=False))))


def _planted(rng, graph):
    """[(case, class, sources)] of one graph."""
    ns, SC, _ = GRAPHS[graph]
    nch = ns // SC
    f = lambda cols: _feature(rng, SC, nch, cols)
    out = []
    if graph == "length 300":
        return [("length 300", c, f(_columns(rng, SC, 300))) for c in range(4)]
    if graph == "smallest chunk":
        return [(f"length {n}", c, f(_columns(rng, SC, n))) for n in (65, 66, 67, 68) for c in range(4)]
    same = _columns(rng, SC, 70)
    out += [("same class, same columns", 1, f(same)) for _ in range(5)]
    same = _columns(rng, SC, 72)
    out += [("four classes, same columns", c, f(same)) for c in range(4)]
    out += [("unbalanced classes", 0, f(_columns(rng, SC, int(rng.integers(66, 80))))) for _ in range(9)]
    out += [("unbalanced classes", c, f(_columns(rng, SC, int(rng.integers(66, 80))))) for c in (1, 2, 3)]
    out += [("overflow", 2, f(_columns(rng, SC, (70, 85, 66, 100)[i % 4]))) for i in range(20)]
    out.append(("filler: none of its class", 2, f(_columns(rng, SC, 80, 2, 0))))
    out.append(("filler: 3 of its class", 1, f(_columns(rng, SC, 70, 1, 3))))
    out += [(f"length {n}", c, f(_columns(rng, SC, n))) for n in LENGTHS for c in range(4)]
    return out


def _labels(rng, Xs, nt, hub=None):
    """0/1 labels that make ks a power of two: 2^ceil(log2(rx + 1)) - rx per source among the targets 1 .. nt - 2; hub:
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


def _assign_ids(rng, planted, ids):
    """A feature id of the right class (id & 3) out of `ids` for every planted feature, in order of the list."""
    free = {c: list(rng.permutation([a for a in ids if a & 3 == c])) for c in range(4)}
    return [int(free[c].pop()) for _, c, _ in planted]


@functools.lru_cache(maxsize=None)
def _query_case(graph, weighted, nt=96, seed=21):
    """Xq, Xs, Ys, the oracle's scores, rows by name, and per planted feature (case, class, id).  Feature nf - 1, the
    highest id (class 3), has 72 sources in the last chunk, 2 of them in class-3 columns, and 56 in chunk 6 (smallest
    chunk: 66 and 62, columns at random)."""
    ns, SC, nf = GRAPHS[graph]
    nch = ns // SC
    rng = np.random.default_rng(seed + len(graph))
    planted = _planted(rng, graph)
    ids = _assign_ids(rng, planted, range(nf - 1))
    feat = {a: s for a, (_, _, s) in zip(ids, planted)}
    # (a chunk of 68 columns has no 64 outside a class: there the last sub-row is an ordinary long one)
    last_n = 72 if SC >= 128 else 66
    last_cols = _columns(rng, SC, last_n, 3, 2) if SC >= 128 else _columns(rng, SC, last_n)
    feat[nf - 1] = np.sort(np.concatenate(((nch - 1) * SC + last_cols,
                                           (nch - 2) * SC + rng.choice(SC, size=128 - last_n, replace=False))))
    shorts = np.array([a for a in range(nf - 1) if a not in feat])
    for a in shorts:
        feat[int(a)] = rng.choice(ns, size=1 << int(rng.integers(0, 6)), replace=False)
    cols = np.concatenate([np.full(len(s), a) for a, s in feat.items()])
    srcs = np.concatenate(list(feat.values()))
    Xs = sp.csr_matrix((S._weights(rng, len(cols), weighted), (srcs, cols)), shape=(ns, nf))
    Xs.sort_indices()
    Ys = _labels(rng, Xs, nt)
    by_case = {}
    for a, (case, _, _) in zip(ids, planted):
        by_case.setdefault(case, []).append(a)
    every = np.array(sorted(ids))
    rows = {case: np.array(sorted(a)) for case, a in by_case.items()}
    if graph == "main":
        rows["overflow"] = np.union1d(rows["overflow"], rng.choice(shorts, size=36, replace=False))   # 56 neighbours
        rows["fillers"] = np.array(sorted(by_case["filler: none of its class"] + by_case["filler: 3 of its class"] + [nf - 1]))
        rows["every length"] = np.array(sorted(a for n in LENGTHS for a in by_case[f"length {n}"]))
        # second groups of 64 neighbours: 64 short features with lower ids put the case's last long feature there
        for case in ("same class, same columns", "four classes, same columns", "unbalanced classes"):
            a = rows[case]
            low = shorts[shorts < a.max()]
            rows[case + ", 70 short neighbours"] = np.union1d(a, np.concatenate((rng.choice(low, size=64, replace=False),
                                                                               rng.choice(shorts[shorts > a.max()], size=6, replace=False))))
        rows["every planted feature"] = every
        rows["every planted feature and 100 short ones"] = np.union1d(every, rng.choice(shorts, size=100, replace=False))
    else:
        rows["every planted feature"] = every
        rows["every planted feature and 60 short ones"] = np.union1d(every, rng.choice(shorts, size=60, replace=False))
    rows["the last stored sub-row alone"] = np.array([nf - 1])
    rows["every planted feature and the last stored sub-row"] = np.concatenate((every, [nf - 1]))
    names = list(rows)
    while len(rows) < len(names) + 12:
        n = int(rng.integers(1, 41))
        rows[f"random {len(rows)}"] = np.union1d(rng.choice(every, size=min(len(every), int(rng.integers(0, 13))), replace=False),
                                                 rng.choice(shorts, size=n, replace=False))
    qr = np.concatenate([np.full(len(c), q) for q, c in enumerate(rows.values())])
    qc = np.concatenate([np.asarray(c, dtype=np.int64) for c in rows.values()])
    Xq = sp.csr_matrix((S._weights(rng, len(qr), weighted), (qr, qc)), shape=(len(rows), nf))
    Xq.sort_indices()
    want = S.oracle_query(Xq, Xs, Ys)
    want.setflags(write=False)
    return dict(Xq=Xq, Xs=Xs, Ys=Ys, want=want, names=names, by_case=by_case, last=nf - 1, weighted=weighted)


def _subrow(Xs, SC, a, chunk=0):
    """Chunk-local columns of the sub-row (chunk, feature a)."""
    col = sp.csc_matrix(Xs)[:, a].indices
    return np.sort(col[(col >= chunk * SC) & (col < (chunk + 1) * SC)]) - chunk * SC


def _tail(cols, a):
    """(tail length t, entries of the sub-row's class) of a long sub-row of feature a."""
    return min(len(cols) - 64, 16), int((cols & 3 == a & 3).sum())


def _class_counts(Xq, Xs, SC, q, chunk=0):
    """Per group of 64 neighbours of row q: long sub-rows of chunk `chunk` by class."""
    c = Xq.indices[Xq.indptr[q]:Xq.indptr[q + 1]]
    out = []
    for g in range(0, len(c), 64):
        cnt = [0, 0, 0, 0]
        for a in c[g:g + 64]:
            if len(_subrow(Xs, SC, a, chunk)) > 64:
                cnt[a & 3] += 1
        out.append(cnt)
    return out


def test_the_planted_inputs_are_what_the_cases_say():
    """Lengths, classes and class counts of the planted cases, the filler conditions, the last stored sub-row, powers of
    two and the exactness of every partial sum in fp32 (no device needed, but the cases below rest on it)."""
    for graph, (ns, SC, nf) in GRAPHS.items():
        nch = ns // SC
        for weighted in (True, False):
            inp = _query_case(graph, weighted)
            Xq, Xs, Ys, names, by_case = inp["Xq"], inp["Xs"], inp["Ys"], inp["names"], inp["by_case"]
            assert S.chunk_width(ns, nf, Xs.nnz, 4, SC) == (SC, nch) == S.chunk_width(ns, nf, Xs.nnz, 8, SC)
            kf, ks, _ = O.degrees(Xs, Ys)
            assert S.is_pow2(kf[kf > 0]).all() and S.is_pow2(ks).all()
            e = (8 if weighted else 0) + int(np.log2(kf.max())) + int(np.log2(ks.max()))
            acc = (Xq @ sp.diags(np.where(kf > 0, 1.0 / np.maximum(kf, 1), 0.0)) @ Xs.T).toarray()
            assert acc.max() * 2.0 ** (e - int(np.log2(ks.max()))) < 2 ** 24 and inp["want"].max() * 2.0 ** e < 2 ** 24
            q = inp["want"] * 2.0 ** e
            assert (q == np.round(q)).all()
            # the last sub-row the operand stores (chunk-major, then by feature): long, fewer of its class than its tail
            last = _subrow(Xs, SC, inp["last"], nch - 1)
            t, m = _tail(last, inp["last"])
            assert inp["last"] == nf - 1 and len(last) == (72 if SC >= 128 else 66) and (m == 2 < t or SC < 128)
            for case, ids in by_case.items():
                for a in ids:
                    if case.startswith("length "):
                        assert len(_subrow(Xs, SC, a)) == int(case.split()[1])
                if case.startswith("length "):
                    assert sorted(a & 3 for a in ids) == [0, 1, 2, 3]
            if graph == "smallest chunk":
                assert {len(_subrow(Xs, SC, a)) for ids in by_case.values() for a in ids} == {65, 66, 67, 68} and SC == 68
                continue
            if graph == "length 300":
                assert all(len(_subrow(Xs, SC, a)) == 300 for a in by_case["length 300"])
                continue
            same = by_case["same class, same columns"]
            cols = [_subrow(Xs, SC, a) for a in same]
            assert len(same) == 5 and {a & 3 for a in same} == {1} and len(cols[0]) == 70
            assert all((c == cols[0]).all() for c in cols)
            assert _class_counts(Xq, Xs, SC, names.index("same class, same columns")) == [[0, 5, 0, 0]]
            four = by_case["four classes, same columns"]
            cols = [_subrow(Xs, SC, a) for a in four]
            assert sorted(a & 3 for a in four) == [0, 1, 2, 3] and len(cols[0]) == 72 and all((c == cols[0]).all() for c in cols)
            assert _class_counts(Xq, Xs, SC, names.index("four classes, same columns")) == [[1, 1, 1, 1]]
            assert _class_counts(Xq, Xs, SC, names.index("unbalanced classes")) == [[9, 1, 1, 1]]
            over = names.index("overflow")
            assert Xq[over].nnz == 56 and _class_counts(Xq, Xs, SC, over) == [[0, 0, 20, 0]]
            beyond = sorted(by_case["overflow"])[16:]                  # without a slot: from position 64 in the rest loop
            assert {len(_subrow(Xs, SC, a)) for a in beyond} == {70, 85, 66, 100}
            (a,) = by_case["filler: none of its class"]
            assert a & 3 == 2 and len(_subrow(Xs, SC, a)) == 80 and _tail(_subrow(Xs, SC, a), a) == (16, 0)
            (a,) = by_case["filler: 3 of its class"]
            assert len(_subrow(Xs, SC, a)) == 70 and _tail(_subrow(Xs, SC, a), a) == (6, 3)
            # rows with a second group of 64 neighbours that holds long sub-rows
            for name in ("every planted feature", "every planted feature and 100 short ones",
                         "same class, same columns, 70 short neighbours"):
                groups = _class_counts(Xq, Xs, SC, names.index(name))
                assert len(groups) >= 2 and sum(groups[1]) > 0, (name, groups)


# ----------------------------------------------------------------------------- query rows, bit for bit
@pytest.mark.gpu
@pytest.mark.parametrize("weighted", [True, False], ids=["weighted", "pattern-only"])
@pytest.mark.parametrize("graph", list(GRAPHS))
@pytest.mark.parametrize("dtype,name", _kernel_params(list(KERNELS)))
def test_query_rows_with_class_tails_equal_the_oracle_bit_for_bit(dtype, name, graph, weighted, switches, device):
    env, tags, _ = KERNELS[name]
    switches(GRAPHS[graph][1], env)
    inp = _query_case(graph, weighted)
    want = inp["want"]
    g = _graph(inp["Xq"], inp["Xs"], inp["Ys"], dtype)
    got = g.predict("query")
    assert set(ss.path_last()) & STAGE1_TAGS == tags, ss.path_last()
    bits = np.uint32 if dtype is np.float32 else np.uint64
    w = want.astype(dtype)
    for q in np.flatnonzero((got.view(bits) != w.view(bits)).any(axis=1))[:8]:
        print(f"row {q} ({inp['names'][q] if q < len(inp['names']) else 'random'}) differs")
    S.assert_bitwise(got, want, dtype, f"query rows, {graph}, {name}")
    # the same rows alone and inside a larger range: the sums of a row do not depend on its launch
    n = got.shape[0]
    for a, b in ((0, 1), (1, 2), (2, 5), (3, 4), (n - 3, n)):
        S.assert_bitwise(g.predict("query", a, b), want[a:b], dtype, f"query rows [{a},{b}), {graph}, {name}")
    g.close()


# ----------------------------------------------------------------------------- the other flavours, within their bands
@functools.lru_cache(maxsize=None)
def _square_case(weighted, nt=96, seed=22):
    """The planted features of the main graph as features of a square X (feature a is named after source a, non-zero
    diagonal; ids below 128, so that the rows 0 .. 69 name many of them), the other features short; target 0 (class 0) is
    a label of 200 sources of chunk 0.  Rows 0 .. 69 are sources of chunk 0, members of many long features each."""
    ns, SC, _ = GRAPHS["main"]
    rng = np.random.default_rng(seed)
    planted = _planted(rng, "main")
    ids = _assign_ids(rng, planted, range(128))
    feat = {a: s for a, (_, _, s) in zip(ids, planted)}
    for a in range(ns):
        if a not in feat:
            feat[a] = rng.choice(ns, size=int(rng.integers(1, 7)), replace=False)
        feat[a] = np.union1d(feat[a], [a])
    cols = np.concatenate([np.full(len(s), a) for a, s in feat.items()])
    srcs = np.concatenate(list(feat.values()))
    vals = (1.0 - 0.5 * rng.random(len(cols))).astype(np.float32).astype(np.float64) if weighted else np.ones(len(cols))
    X = sp.csr_matrix((vals, (srcs, cols)), shape=(ns, ns))
    X.sort_indices()
    hub = np.zeros(ns, dtype=bool)
    hub[rng.choice(SC, size=200, replace=False)] = True
    Y = _labels(rng, X, nt, hub)
    fold = (np.arange(ns) % 5).astype(np.int32)
    rows = np.arange(70)
    in0 = np.asarray((X[:SC] != 0).sum(axis=0)).ravel()
    assert (in0[:128] > 64).sum() >= len(planted) and in0.max() >= 200
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


@pytest.mark.gpu
@pytest.mark.parametrize("weighted", [True, False], ids=["weighted", "pattern-only"])
@pytest.mark.parametrize("dtype,name", _kernel_params(["default", "U=4"]))
def test_leave_one_out_source_and_kfold_rows_with_class_tails_within_their_bands(dtype, name, weighted, switches, device):
    switches(GRAPHS["main"][1], KERNELS[name][0])
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
