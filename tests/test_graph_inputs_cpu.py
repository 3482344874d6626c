"""What the assertions of tests/test_gpu_graph_inputs.py can see (no device): the restated split rule of csr_from_dense,
the shapes that force its arithmetic, the form the Julia binding hands over, the inputs with stored zeros, the exactly
summable graphs of extreme shape, the raw similarities whose cut is the exact graph -- and that every single defect a
graph constructor could have (tests/graph_input_ref.py: DEFECTS, BLOCK_DEFECTS, a transposed B) changes an entry count, a
degree or the bits of a score, or leaves the band of the directed general graph."""
import functools

import numpy as np
import pytest
import scipy.sparse as sp

from oracle import simspread_oracle as O

import graph_input_ref as G
import sparse_ref as S

MODES = [True, False]
IDS = ["weighted", "pattern-only"]


@functools.lru_cache(maxsize=None)
def _query(weighted):
    inp = S.exact_query_for(4, None, weighted=weighted)
    return inp, S.oracle_query(inp["Xq"], inp["Xs"], inp["Ys"])


def _same(a, b):
    a, b = sp.csr_matrix(a), sp.csr_matrix(b)
    return a.shape == b.shape and (a != b).nnz == 0


# ----------------------------------------------------------------------------- the split rule and the shapes
def test_dense_split_restated_and_every_path_reached():
    """dense_split against hand-worked cases of csr_from_dense (assemble.hip), and the shapes of the GPU tests between
    them reach every path of the rule."""
    assert G.dense_split(3000, 3000) == (22, 137, 123)
    assert G.dense_split(70, 3000) == (750, 4, 4)
    assert G.dense_split(3000, 300) == (22, 14, 6)
    assert G.dense_split(488, 488) == (122, 4, 4)
    assert G.dense_split(70000, 3) == (1, 3, 3)
    assert G.dense_split(1, 70001) == (1015, 69, 35)
    assert G.dense_split(150, 150) == (150, 1, 1)            # all the suite had before: one column per thread
    used = {}
    q = _query(True)[0]
    loo, kfold, tall, wide = S.exact_loo(), S.exact_kfold(), G.tall_graph(), G.wide_graph()
    for name, blocks in (("query", (q["Xq"], q["Xs"], q["Ys"])), ("loo", (loo["X"], loo["Y"])),
                         ("kfold", (kfold["X"], kfold["Y"])), ("tall", (tall["Xq"], tall["Xs"], tall["Ys"])),
                         ("wide", (wide["Xq"], wide["Xs"], wide["Ys"]))):
        for b in blocks:
            used[(name,) + b.shape] = G.dense_split(*b.shape)
    assert used[("query", 3000, 3000)] == (22, 137, 123) and used[("loo", 488, 488)] == (122, 4, 4)
    splits = set(used.values())
    assert any(cps > 1 and last < cps for _, cps, last in splits)              # a short last split
    assert any(cps == 1 and n > 1 for n, cps, _ in splits)                     # one column per thread
    assert used[("tall", 70000, 3)][0] == 1 and used[("tall", 70000, 4)][0] == 1      # nsplit = 1
    assert used[("wide", 1, 70001)] == (1015, 69, 35) and used[("wide", 8, 70001)] == (1015, 69, 35)   # the 1024 cap
    assert [G.small_query(n)["Xq"].shape[0] for n in (63, 64, 65)] == [63, 64, 65]     # around the 64-thread row block


# ----------------------------------------------------------------------------- the forms handed over
@pytest.mark.parametrize("weighted", MODES, ids=IDS)
def test_julia_form_is_the_matrix_itself(weighted):
    """The CSC of the transpose with 1-based colptr / rowval, built as julia/SimSpreadHIP.jl builds it, read as the
    1-based CSR the ABI takes, is M; stored zeros travel with it."""
    inp, _ = _query(weighted)
    for k, seed in (("Xq", 1), ("Xs", 2), ("Ys", 3)):
        for M in (inp[k], G.with_stored_zeros(inp[k], seed)):
            ptr, idx, val = G.julia_csr(M, np.float32)
            assert ptr.dtype == np.int64 and idx.dtype == np.int32 and val.dtype == np.float32
            assert ptr[0] == 1 and ptr[-1] == M.nnz + 1 and idx.min() >= 1 and idx.max() <= M.shape[1]
            back = G.from_triple(ptr, idx, val, M.shape, 1)
            assert back.nnz == M.nnz and _same(back, M)
            assert np.array_equal(back.indptr, M.indptr) and np.array_equal(back.indices, M.indices)
            p0, i0, v0 = G.csr_triple(M, np.float64, 0)
            assert np.array_equal(p0 + 1, ptr) and np.array_equal(i0 + 1, idx) and np.array_equal(v0, val)
            assert G.julia_csr(M, np.float32, pattern=True)[2] is None


@pytest.mark.parametrize("weighted", MODES, ids=IDS)
def test_stored_zeros_sit_where_the_compaction_can_go_wrong(weighted):
    inp, _ = _query(weighted)
    for k, seed in (("Xq", 1), ("Xs", 2), ("Ys", 3)):
        M, Z = inp[k], G.with_stored_zeros(inp[k], seed)
        zeros = Z.data == 0
        assert zeros.mean() > 0.3 and np.signbit(Z.data[zeros]).sum() > 10      # some are -0.0
        kept = sp.csr_matrix(Z, copy=True)
        kept.eliminate_zeros()
        assert kept.nnz == M.nnz and _same(kept, M) and np.array_equal(kept.indices, M.indices)
        pos = G.zero_positions(Z)
        assert len(pos) >= 12                                  # rows of more than 64 stored values
        first = sum(0 in p for p, n in pos.values())
        last = sum(n - 1 in p for p, n in pos.values())
        step = sum((63 in p) != (64 in p) for p, n in pos.values())       # a zero on one side of the 64-entry step only
        both = sum(63 in p and 64 in p for p, n in pos.values())
        assert first >= 5 and last >= 5 and (step >= 1 or both >= 5), (k, first, last, step, both)
        assert all(0 < len(p) < n for p, n in pos.values())    # zeros and kept entries in every such row


# ----------------------------------------------------------------------------- exactness of the graphs added here
def _exact(inp, bound_bits=24):
    Xq, Xs, Ys, e = inp["Xq"], inp["Xs"], inp["Ys"], inp["e"]
    kf, ks, kt = O.degrees(Xs, Ys)
    assert S.is_pow2(kf[kf > 0]).all() and S.is_pow2(ks[ks > 0]).all() and set(np.unique(Ys.data)) == {1.0}
    # the scores in quanta of 2^-e; the stage-1 sums before the (exact) division by ks in quanta of 2^-e * max(ks)
    sums = S.oracle_transfer(Xq, Xs, Ys) * ks[None, :]
    for a, ee in ((S.oracle_query(Xq, Xs, Ys), e), (sums, e - int(np.log2(ks.max())))):
        q = a * 2.0 ** ee
        assert (q == np.round(q)).all() and (q >= 0).all() and q.max() < 2 ** bound_bits
        assert (a.astype(np.float32).astype(np.float64) == a).all()
    return kf, ks, kt


@pytest.mark.parametrize("weighted", MODES, ids=IDS)
def test_graphs_of_extreme_shape_are_exactly_summable(weighted):
    tall = G.tall_graph(weighted)
    kf, ks, kt = _exact(tall)
    assert tall["Ys"].shape == (70000, 3) and kt[-1] == 0 and (kt[:-1] > 1000).all() and (ks == 0).any()
    assert np.count_nonzero(S.oracle_query(tall["Xq"], tall["Xs"], tall["Ys"])) >= 8
    wide = G.wide_graph(weighted)
    kf, ks, kt = _exact(wide)
    assert wide["Xq"].shape == (1, 70001) and set(np.unique(kf)) == {0, 1, 2, 4, 8} and (ks == 4096).all()
    assert kf[0] > 0 and kf[-1] > 0 and wide["Xq"][0, 0] != 0 and wide["Xq"][0, 70000] != 0 and kt[-1] == 0
    # every split of 69 columns has something to count, and entries of the query row sit in the short last split
    nz_per_split = np.bincount(wide["Xs"].indices // 69, minlength=1015)
    assert (nz_per_split > 0).all() and (wide["Xq"].indices >= 1014 * 69).sum() >= 1
    for n in (63, 64, 65):
        _exact(G.small_query(n, weighted))


@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("weighted", MODES, ids=IDS)
def test_raw_similarities_cut_to_the_exact_graph(weighted, dtype):
    """Kept entries exactly alpha, dropped entries exactly the precision's nextafter(alpha, 0); the cut is the graph."""
    inp = G.small_query(64, weighted)
    dt = np.dtype(dtype).type
    for k in ("Xq", "Xs"):
        raw = G.raw_similarities(inp[k], 0.5, weighted, dtype, 51)
        assert (raw.astype(dt).astype(np.float64) == raw).all()
        assert (raw == 0.5).any() and (raw == float(np.nextafter(dt(0.5), dt(0)))).sum() > 100
        assert ((raw > 0) & (raw < 0.5)).sum() > raw.size // 2
        cut = G.canonical_cut(raw, 0.5, weighted)
        assert _same(cut, inp[k]) and np.array_equal(cut.indices, inp[k].indices)
        assert (cut.toarray() == O.cutoff(raw, 0.5, weighted)).all()


@pytest.mark.parametrize("alpha", [0.0, -0.5, -1.0, 0.3])
@pytest.mark.parametrize("weighted", MODES, ids=IDS)
def test_canonical_cut_is_featurize_over_the_whole_domain(weighted, alpha):
    Sq, Ss, Y = G.domain_blocks()
    assert np.isnan(Ss).sum() > 500 and (Ss == 0).sum() > 2000 and np.signbit(Ss[Ss == 0]).sum() > 1000 and (Ss < 0).any()
    for D in (Sq, Ss):
        cut = G.canonical_cut(D, alpha, weighted)
        assert (cut.toarray() == O.cutoff(D, alpha, weighted)).all()
        assert cut.nnz == np.count_nonzero(O.cutoff(D, alpha, weighted))
        if not weighted and alpha <= 0:                        # zeros of either sign are edges, and the negatives >= alpha
            assert (cut.toarray()[D == 0] == 1).all() and cut.nnz == (D >= alpha).sum() > (D > 0).sum() + 500
        if not weighted and alpha == -1.0:
            assert cut.nnz == (~np.isnan(D)).sum()             # full rows but for NaN
        if weighted and alpha < 0:
            assert (cut.data < 0).any() and cut.nnz == ((D >= alpha) & (D != 0)).sum()
    cy = G.canonical_cut(Y, None, True)
    assert cy.nnz == np.count_nonzero(Y) < (Y == 0).sum() and np.signbit(Y[Y == 0]).any() and (cy.data < 0).any()


# ----------------------------------------------------------------------------- the general graph
@pytest.mark.parametrize("weighted", MODES, ids=IDS)
def test_general_blocks_give_the_oracle(weighted):
    """The literal L * spread(B) * spread(B)[:, targets] on the block matrix is the factored oracle, bit for bit on exact
    inputs; B is A without the query edges and is symmetric (a transposed operand would pass here: the directed case)."""
    inp = G.small_query(63, weighted)
    Xq, Xs, Ys = inp["Xq"], inp["Xs"], inp["Ys"]
    L, B, Wt, k = G.general_blocks(Xq, Xs, Ys)
    nq, nf = Xq.shape
    ns, nt = Ys.shape
    n = nq + ns + nf + nt
    assert B.shape == (n, n) and (B != B.T).nnz == 0 and B[:nq].nnz == 0 and B[:, :nq].nnz == 0
    assert L.shape == (nq, n) and _same(L[:, nq + ns:nq + ns + nf], Xq) and L.nnz == Xq.nnz
    assert _same(Wt.T, B[:, n - nt:]) and _same(Wt[:, nq:nq + ns], Ys.T)
    kf, ks, kt = O.degrees(Xs, Ys)
    assert np.array_equal(k, np.concatenate((np.zeros(nq, int), ks, kf, kt)))
    got = G.general_reference(L, B, np.arange(n - nt, n))
    np.testing.assert_array_equal(got, S.oracle_query(Xq, Xs, Ys))
    A = sp.vstack([L, B[nq:]])                                 # the reference's own block form, densified
    names = list(range(n))
    lit = O.predict(O.Named(A.toarray(), names, names), O.Named(B.toarray(), names, names),
                    O.Named(np.zeros((nq, nt)), names[:nq], names[n - nt:])).array
    np.testing.assert_array_equal(lit, got)


def test_directed_general_graph_band_holds_and_sees_a_transposed_operand():
    d = G.directed_graph()
    L, B, cols = d["L"], d["B"], d["cols"]
    k = np.diff(B.indptr)
    assert B.shape == (600, 600) and k[7] == 0 and np.diff(sp.csc_matrix(B).indptr)[11] == 0 and k.max() == 6
    oneway = (B != 0).astype(int) - (B != 0).astype(int).multiply((B.T != 0).astype(int))
    assert oneway.nnz > 3000                                   # B[i,j] != 0 = B[j,i]
    assert (B.data > 0).all() and (B.data.astype(np.float32).astype(np.float64) == B.data).all()
    assert 11 in cols and _same(d["Wt"], B[:, cols].T)
    want = G.general_reference(L, B, cols)
    np.testing.assert_allclose(want, L.toarray() @ O.spread(B.toarray()) @ O.spread(B.toarray())[:, cols], rtol=1e-13)
    assert want.size > 600 and (want > 0).sum() > 200 and (want[:, list(cols).index(11)] == 0).all()
    band = G.general_band(L, B, cols, want, np.float32)
    assert ((band == 0) == (want == 0)).all() and (band[want > 0] < 40 * S.U32 * want[want > 0]).all()
    ratio = S.assert_band(G.emulate_general(L, B, cols, np.float32), want, band, "model, directed general graph")
    assert ratio > 0.01
    for stage in (1, 2):
        bad = G.emulate_general(L, B, cols, np.float32, transposed=(stage,)).astype(np.float64)
        outside = ~(np.abs(bad - want) <= band) & (want > 0)
        assert outside.sum() >= (want > 0).sum() / 2, (stage, int(outside.sum()), int((want > 0).sum()))


# ----------------------------------------------------------------------------- single defects
def _detected(base, want, M, blocks, changed):
    """A graph differs from the exact one in what a handle shows: an entry count, a degree or the bits of a score."""
    if not G.same_shown(base, G.shown(*blocks)):
        return True
    if changed == "Xq":                                        # degrees and weights unchanged: still exactly summable
        got = np.asarray(sp.csr_matrix(blocks[0]) @ M)
    else:
        got = S.oracle_query(*blocks)
    return bool((got != want).any())


def test_every_single_defect_changes_a_count_a_degree_or_a_score():
    """A dropped entry, an entry moved one column, an entry assigned to the next row (200 sampled entries per block, the
    first and last of the longest row among them), indices left 1-based, one split written at the next split's offset:
    none goes unseen by info, degrees and the oracle's bits."""
    inp, want = _query(True)
    blocks = {k: inp[k] for k in ("Xq", "Xs", "Ys")}
    base = G.shown(*blocks.values())
    kf, ks, kt = base[1:]
    M = np.asarray((sp.diags(O._inv_count(kf)) @ inp["Xs"].T @ sp.diags(O._inv_count(ks)) @ inp["Ys"]).todense())
    np.testing.assert_array_equal(np.asarray(inp["Xq"] @ M), want)      # any order of exact sums: the oracle's bits
    applied = {}
    for name, blk in blocks.items():
        picks = G.sample_entries(blk, 200, 91)
        r = int(np.argmax(np.diff(blk.indptr)))
        assert len(picks) >= 200 and blk.indptr[r] in picks and blk.indptr[r + 1] - 1 in picks
        for defect in G.DEFECTS:
            for p in picks:
                bad = G.apply_defect(blk, defect, int(p))
                if bad is None:
                    continue
                if name == "Xq" and kf[blk.indices[p]] == 0 and defect != "dropped entry":
                    continue        # an edge to a feature without sources carries nothing: no score depends on its place
                assert bad.nnz == blk.nnz - (defect == "dropped entry")
                applied[(name, defect)] = applied.get((name, defect), 0) + 1
                assert _detected(base, want, M, list(dict(blocks, **{name: bad}).values()), name), (name, defect, int(p))
        shifted = G.one_based_read_as_zero_based(blk)
        if shifted is not None:                                 # (None: an index leaves the matrix and the block is refused)
            assert _detected(base, want, M, list(dict(blocks, **{name: shifted}).values()), name), (name, "1-based")
        applied[(name, "1-based")] = shifted is not None
        nsplit, cps, _ = G.dense_split(*blk.shape)
        rng = np.random.default_rng(92)
        n = 0
        for p in rng.choice(blk.nnz, 400, replace=False):
            r = int(np.searchsorted(blk.indptr, p, side="right")) - 1
            late = G.split_written_late(blk, r, int(blk.indices[p]) // cps)
            if late is None:
                continue
            bad = sp.csr_matrix(late, shape=blk.shape)
            n += 1
            assert _detected(base, want, M, list(dict(blocks, **{name: bad}).values()), name), (name, "late split", r)
            if n >= 60:
                break
        applied[(name, "late split")] = n
    assert all(applied[(k, d)] >= 150 for k in blocks for d in G.DEFECTS), applied
    assert all(applied[(k, "late split")] >= 40 for k in blocks), applied
    assert applied[("Xs", "1-based")] and applied[("Ys", "1-based")], applied
