"""The inputs of tests/test_gpu_sparse.py have the properties its assertions rely on (no device): the exactly summable
graphs are exactly summable, the structural edges the builders promise are there for every chunk width the GPU tests
use, and the rounding bands hold for a sequential fp32 model of the two stages while a single wrong entry leaves them."""
import functools

import numpy as np
import pytest
import scipy.sparse as sp

from oracle import simspread_oracle as O

import sparse_ref as S

MODES = [True, False]
IDS = ["weighted", "pattern-only"]


def _multiples(a, e):
    """Every element of a is a non-negative multiple of 2^-e below 2^24 quanta, and survives float32."""
    a = np.asarray(a, dtype=np.float64)
    q = a * 2.0 ** e
    return bool((q == np.round(q)).all() and (q >= 0).all() and q.max() < 2 ** 24
                and (a.astype(np.float32).astype(np.float64) == a).all())


@functools.lru_cache(maxsize=None)
def _query(elem, chunk, weighted, labels="random"):
    return S.exact_query_for(elem, chunk, weighted=weighted, labels=labels)


# ----------------------------------------------------------------------------- the sizing rule
def test_chunk_rule_restated():
    """chunk_width against hand-worked cases of graph_chunked (api.hip): mean degree 32 at ns = 3000 asks for 6000
    columns, capped at 5056 (fp32: one chunk) or 2496 (fp64: 2 -> 8 chunks of 376); SS_TRANSFER_CHUNK = 190 gives
    16 chunks of 188; the 488-source leave-one-out graph (mean degree 90.8) asks for 343 -> 2 -> 8 chunks of 64."""
    assert S.chunk_width(3000, 3000, 96000, 4) == (3000, 1)
    assert S.chunk_width(3000, 3000, 96000, 8) == (376, 8)
    assert S.chunk_width(3000, 3000, 96000, 4, 376) == (376, 8)
    assert S.chunk_width(3000, 3000, 96000, 4, 190) == (188, 16)
    assert S.chunk_width(3000, 3000, 96000, 4, 15) == (3000, 1)          # outside 16..8192: ignored
    assert S.chunk_width(488, 488, 44314, 4) == (64, 8)
    assert S.chunk_width(1, 1, 1, 4) == (4, 1)
    assert S.chunk_width(600, 600, 3600, 4, 38) == (40, 15)              # 16 asked for, 15 cut: no multiple of 8
    sizes = {"query": (S.QUERY_NS, 96000), "loo": (488, 44314), "kfold": (252, 252 * 36), "band": (608, 3648)}
    for family, (ns, nnz) in sizes.items():
        for elem in (4, 8):
            for n in (8, 16):
                assert S.chunk_width(ns, ns, nnz, elem, S.CHUNK_ENV[family][n])[1] == n, (family, n)
    assert S.transfer_batch_rows(170, 3000, 4, 1 << 20) == 80 and S.transfer_batch_rows(170, 3000, 8, 1 << 20) == 40


# ----------------------------------------------------------------------------- exactness
@pytest.mark.parametrize("labels", ["random", "hub", "private"])
@pytest.mark.parametrize("weighted", MODES, ids=IDS)
@pytest.mark.parametrize("chunk", S.QUERY_CHUNKS)
def test_query_inputs_are_exactly_summable(chunk, weighted, labels):
    for elem in ((4, 8) if chunk is None else (4,)):     # the switch cuts both precisions alike
        inp = _query(elem, chunk, weighted, labels)
        Xq, Xs, Ys, e = inp["Xq"], inp["Xs"], inp["Ys"], inp["e"]
        kf, ks, kt = O.degrees(Xs, Ys)
        assert S.is_pow2(kf[kf > 0]).all() and S.is_pow2(ks[ks > 0]).all()
        assert set(np.unique(Ys.data)) == {1.0}
        w = np.concatenate((Xq.data, Xs.data)) * 16
        assert ((w == np.round(w)) & (w >= 8) & (w <= 16)).all() if weighted else (w == 16).all()
        T = S.oracle_transfer(Xq, Xs, Ys)
        F = S.oracle_query(Xq, Xs, Ys)
        assert _multiples(F, e) and _multiples(T, e)
        assert _multiples(T * ks[None, :], e)              # the stage-1 sums before the division by ks
        assert np.count_nonzero(np.unique(F)) > (3000 if weighted else 1000)    # many distinct scores, decades apart
        assert F[F > 0].min() * 100 < F.max()
        if labels == "private":                            # score column s is the transfer element T[q][s]
            np.testing.assert_array_equal(F[:, :Xs.shape[0]], T)


@pytest.mark.parametrize("weighted", MODES, ids=IDS)
def test_loo_inputs_are_exactly_summable(weighted):
    inp = S.exact_loo(weighted)
    X, Y, e = inp["X"], inp["Y"], inp["e"]
    kf, ks, kt = O.degrees(X, Y)
    assert S.is_pow2(kf - 1).all() and S.is_pow2(ks - 1).all()
    assert (X.toarray() != 0).sum(axis=0).tolist() == kf.tolist()
    # every source that shares a feature with the held-out one owns its feature: ks - 1 is the only divisor in use
    P = (X != 0).astype(np.int64)
    assert ((P @ P.T) != 0).toarray().tolist() == (P != 0).toarray().tolist()
    F = S.oracle_loo(X, Y)
    assert _multiples(F, e) and F.max() > 0.1 and (not weighted or F.max() * 2.0 ** e > 2 ** 20)
    assert (kt == 0).sum() == 1 and X.shape[0] == 488


@pytest.mark.parametrize("weighted", MODES, ids=IDS)
def test_kfold_inputs_are_exactly_summable(weighted):
    inp = S.exact_kfold(weighted)
    X, Y, fold, e = inp["X"].toarray(), inp["Y"].toarray(), inp["fold"], inp["e"]
    for phi in range(inp["nfolds"]):
        keep = fold != phi
        kf, ks, _ = O.degrees(X[np.ix_(keep, keep)], Y[keep])
        assert (kf == 32).all() and (ks == 64).all()
    assert np.bincount(fold).tolist() == [28] * 9
    assert _multiples(S.oracle_kfold(X, Y, fold), e)


@pytest.mark.parametrize("weighted", MODES, ids=IDS)
def test_spmm_operands_are_exactly_summable(weighted):
    W, R = S.spmm_operands(weighted=weighted)
    n = np.diff(W.indptr)
    assert W.shape[0] % 64 != 0 and (n == 0).sum() > 40 and n.max() == W.shape[1]
    assert n[-1] == 1 and W.indices[-1] == W.shape[1] - 1
    assert np.abs(R * 16).max() == S.SPMM_RMAX and (R * 16 == np.round(R * 16)).all() and (R < 0).any()
    bound = S.spmm_quanta_bound(W)
    assert bound < 2 ** 24
    F, mag = W @ R, abs(W) @ np.abs(R)
    assert (F * 256 == np.round(F * 256)).all() and (mag * 256).max() <= bound
    assert (F.astype(np.float32).astype(np.float64) == F).all()


# ----------------------------------------------------------------------------- structural edges
@pytest.mark.parametrize("weighted", MODES, ids=IDS)
@pytest.mark.parametrize("chunk", S.QUERY_CHUNKS)
def test_query_inputs_hold_the_promised_edges(chunk, weighted):
    seen = set()
    for elem in ((4, 8) if chunk is None else (4,)):     # the switch cuts both precisions alike
        inp = _query(elem, chunk, weighted)
        Xq, Xs, Ys, SC = inp["Xq"], inp["Xs"], inp["Ys"], inp["SC"]
        ns, nt = Ys.shape
        assert (SC, inp["nchunks"]) == S.chunk_width(ns, Xs.shape[1], Xs.nnz, elem, chunk)
        lens = set(S.subrow_lengths(Xs, SC).tolist())
        assert S.promised_subrow_lengths(ns, SC) <= lens, (SC, sorted(S.promised_subrow_lengths(ns, SC) - lens))
        assert max(lens) <= SC
        seen |= {(SC, n) for n in lens}
        # the long sub-rows are read: every forced feature and the empty one are named by a row of at least 63 features
        nbr = np.diff(Xq.indptr)
        assert nbr[:len(S.NEIGHBOUR_EDGES)].tolist() == list(S.NEIGHBOUR_EDGES)
        long_rows = np.flatnonzero(nbr >= 63)
        named = set(np.concatenate([Xq.indices[Xq.indptr[q]:Xq.indptr[q + 1]] for q in long_rows]).tolist())
        assert set(inp["forced"].tolist()) <= named and inp["empty_feature"] in named
        kf, ks, kt = O.degrees(Xs, Ys)
        assert kf[inp["empty_feature"]] == 0 and ks[inp["isolated"]] == 0 and kt[-1] == 0 and (kt[:-1] > 0).all()
        assert nt > 64 and nt % 64 != 0
        assert Xq.shape[0] % 4 != 0 and Xq.shape[0] % 8 != 0
        hub = _query(elem, chunk, weighted, "hub")["Ys"]
        assert (hub != 0).sum(axis=0)[0, 0] > 0.98 * (ns - 1)          # far beyond SS_SELL_LMAX = 256: a split row
    if chunk == 376:     # the width at which every listed length exists, and a rolled tail of more than one pass
        assert {(376, n) for n in S.SUBROW_EDGES + (256,)} <= seen


def test_transfer_batches_and_fold_inputs_hold_their_edges():
    """Three transfer batches under SS_TRANSFER_BYTES = 2^20 at 170 rows of 3000 sources; the leave-one-out blocks are
    cut by the default chunks of 64 into sub-rows of 3..64 entries with blocks across a boundary."""
    assert -(-170 // S.transfer_batch_rows(170, S.QUERY_NS, 4, 1 << 20)) == 3
    assert -(-170 // S.transfer_batch_rows(170, S.QUERY_NS, 8, 1 << 20)) == 5
    X = S.exact_loo()["X"]
    lens = S.subrow_lengths(X, 64)
    assert lens.max() == 64 and lens.min() == 3 and len(set(lens.tolist())) > 8


# ----------------------------------------------------------------------------- band soundness
@functools.lru_cache(maxsize=None)
def _band_case(weighted):
    g = S.band_graph(weighted)
    Xq, X, Y, fold = g["Xq"], g["X"], g["Y"], g["fold"]
    ref = dict(query=(S.oracle_query(Xq, X, Y), S.counts_query(Xq, X, Y)),
               source=(S.oracle_source(X, Y), S.counts_query(None, X, Y, source_rows=True)),
               loo=(S.oracle_loo(X, Y), S.counts_loo(X, Y)),
               kfold=(S.oracle_kfold(X, Y, fold), S.counts_kfold(X, Y, fold)))
    return g, ref


SOURCE_ROWS = np.arange(1, 608, 5)       # the model walks source rows one addend at a time: every fifth row


def _emulate_mode(g, mode, dtype=np.float32, **defect):
    Xq, X, Y = g["Xq"], g["X"], g["Y"]
    if mode == "query":
        return S.emulate(Xq, X, Y, dtype, **defect)
    if mode == "source":
        return S.emulate(X[SOURCE_ROWS], X, Y, dtype, source_rows=SOURCE_ROWS, **defect)
    if mode == "loo":
        return S.emulate(X, X, Y, dtype, loo_rows=np.arange(X.shape[0]), **defect)
    return S.emulate_kfold(X, Y, g["fold"], dtype, **defect)


@pytest.mark.parametrize("weighted", MODES, ids=IDS)
@pytest.mark.parametrize("mode", ["query", "source", "loo", "kfold"])
def test_bands_hold_for_a_sequential_fp32_model_and_resolve_one_entry(mode, weighted):
    g, ref = _band_case(weighted)
    want, (chain, addends) = ref[mode]
    if mode == "source":
        want, chain, addends = want[SOURCE_ROWS], chain[SOURCE_ROWS], addends[SOURCE_ROWS]
    band = S.band_graph_scores(want, chain, addends, np.float32)
    assert np.median(chain[want > 0] + addends[want > 0]) <= 10         # low fill: a handful of terms per score
    assert (want > 0).sum() > 1000 and ((want == 0) == (band == 0)).all()
    got = _emulate_mode(g, mode)
    ratio = S.assert_band(got, want, band, f"model, {mode}")
    assert ratio > 0.01                                                  # the model does round
    L = g["Xq"] if mode == "query" else (g["X"][SOURCE_ROWS] if mode == "source" else g["X"])
    entry = S.used_entry(L, g["X"], g["Y"])
    for defect in (S.DEFECTS_LOO if mode == "loo" else S.DEFECTS):
        bad = _emulate_mode(g, mode, defect=defect, entry=entry)
        out = ~(np.abs(bad.astype(np.float64) - want) <= band)
        assert out.any(), f"{defect}: every score still inside its band"
    if mode == "loo":   # sources that share a feature with the held-out one without owning its feature: bit 0 and bit 1
        P = (g["X"] != 0).astype(np.int64)
        share = ((P @ P.T) != 0).toarray()
        owns = (P != 0).toarray()
        assert (share & ~owns).sum() > 1000 and (share & owns).sum() > 1000


@pytest.mark.parametrize("weighted", MODES, ids=IDS)
def test_spmm_band_holds_for_a_sequential_fp32_model(weighted):
    W, R = S.spmm_operands(weighted=weighted, exact=False)
    R = R.astype(np.float32).astype(np.float64)
    want, band = W @ R, S.band_spmm(W, R, np.float32, 3)
    got = np.zeros(want.shape, dtype=np.float32)
    R32 = R.astype(np.float32)
    for m in range(W.shape[0]):
        for p in range(W.indptr[m], W.indptr[m + 1]):
            got[m] = got[m] + np.float32(W.data[p]) * R32[W.indices[p]]
    S.assert_band(got, want, band, "model, W @ R")
    assert (band[np.diff(W.indptr) == 0] == 0).all()
    p = W.indptr[5]
    W2 = W.copy()
    W2.data[p] *= 2
    assert (~(np.abs(W2 @ R - want) <= band)).any()


@pytest.mark.parametrize("weighted", MODES, ids=IDS)
def test_defects_change_the_exact_inputs(weighted):
    """On the exact inputs the model in fp64 is the oracle, bit for bit; with any single defect it is not.  The entry
    sits in the longest planted sub-row (256 sources) and feeds scores of a query with 129 features."""
    inp = _query(4, 376, weighted)
    rows = np.array([10, 11, 20])
    L, Xs, Ys = inp["Xq"][rows], inp["Xs"], inp["Ys"]
    want = S.oracle_query(inp["Xq"], Xs, Ys)[rows]
    np.testing.assert_array_equal(S.emulate(L, Xs, Ys, np.float64), want)
    S.assert_bitwise(S.emulate(L, Xs, Ys, np.float32), want, np.float32, "fp32 model on exact inputs")
    entry = S.used_entry(L, Xs, Ys, long_row=True)
    assert np.diff(sp.csc_matrix(Xs).indptr)[entry[1]] == 256
    for defect in S.DEFECTS:
        assert (S.emulate(L, Xs, Ys, np.float64, defect=defect, entry=entry) != want).any(), defect
    loo = S.exact_loo(weighted)
    X, Y = loo["X"], loo["Y"]
    rows = np.array([0, 200, 487])
    want = S.oracle_loo(X, Y, rows)
    np.testing.assert_array_equal(S.emulate(X[rows], X, Y, np.float64, loo_rows=rows), want)
    entry = S.used_entry(X[rows], X, Y, long_row=True)
    for defect in S.DEFECTS_LOO:
        assert (S.emulate(X[rows], X, Y, np.float64, loo_rows=rows, defect=defect, entry=entry) != want).any(), defect
    kf = S.exact_kfold(weighted)
    want = S.oracle_kfold(kf["X"], kf["Y"], kf["fold"])
    np.testing.assert_array_equal(S.emulate_kfold(kf["X"], kf["Y"], kf["fold"], np.float64), want)
    entry = S.used_entry(kf["X"], kf["X"], kf["Y"])
    for defect in S.DEFECTS:
        bad = S.emulate_kfold(kf["X"], kf["Y"], kf["fold"], np.float64, defect=defect, entry=entry)
        assert (bad != want).any(), defect
