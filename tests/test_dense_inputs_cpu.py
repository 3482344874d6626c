"""CPU-side checks of the inputs of tests/test_gpu_dense.py (no GPU): for every input builder the stated preconditions
hold, the faithful plane model of dense_ref.py passes the very assertion the GPU test applies to the device result, and
every single defect of the model (a kept plane product dropped, a plane of either side zeroed, the two lo pairs reading
the wrong source plane) violates that assertion on at least half of the non-zero scores.  The orientation of the source
similarity has defects of its own (dense_ref.TRANSPOSE_DEFECTS: an index pair of Ss swapped somewhere): on every
symmetric input each is bit-identical to the correct result, on the symmetric=False inputs each violates the assertion
on at least a tenth of the non-zero scores of every mode it applies to.  These are conditions on the
inputs: a builder that cannot meet them is changed, not the threshold."""
import hashlib

import numpy as np
import pytest
import scipy.sparse as sp

from oracle import simspread_oracle as O

import dense_ref as R

MIN_SHARE = 0.5
MIN_SHARE_T = 0.10      # the transpositions of dense_ref.TRANSPOSE_DEFECTS (a has mismatch hits 2 p (1 - p) of the pairs)


def _pow2(d):
    d = np.asarray(d, dtype=np.int64)
    return bool(((d > 0) & ((d & (d - 1)) == 0)).all())


def _share(bad, want):
    nz = want != 0
    return bad[nz].mean()


def _check_mutants(weighted, run, violations, want):
    """run(**defect) -> model scores; violations(scores) -> boolean mask of the GPU test's assertion."""
    assert (want != 0).mean() >= 0.10
    for name, defect in R.mutants(weighted).items():
        share = _share(violations(run(**defect)), want)
        assert share >= MIN_SHARE, f"defect '{name}' is visible on only {share:.1%} of the non-zero scores"


# ----------------------------------------------------------------------------- the model itself
def test_planes_are_an_exact_split_into_bf16_values():
    rng = np.random.default_rng(0)
    x = np.concatenate([rng.standard_normal(4096).astype(np.float32), rng.random(4096).astype(np.float32) * 1e-3,
                        np.float32([0.0, 1.0, -1.0, 0.4, 1.0 / 3.0, 0.5 + 2.0 ** -10 + 2.0 ** -19])])
    hi, mid, lo = R.planes(x)
    for p in (hi, mid, lo):
        assert ((p.view(np.uint32) & 0xFFFF) == 0).all()               # bf16 values
    assert (hi.astype(np.float64) + mid.astype(np.float64) + lo.astype(np.float64) == x.astype(np.float64)).all()
    # round to nearest even on a tie: 1 + 2^-8 is half way between bf16 neighbours 1 and 1 + 2^-7
    assert R.bf16_rne(np.float32([1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -8])).tolist() == [1.0, 1.0 + 2.0 ** -6]
    f = R._family(rng, 1000)
    fh, fm, fl = R.planes(f)
    assert (fh == 0.5).all() and (fm == 2.0 ** -10).all() and set(np.unique(fl * 2.0 ** 19)) == {-1.0, 0.0, 1.0}


def test_source_row_and_fold_references_equal_the_oracles_own_forms():
    inp = R.random_inputs(20, 61, True, seed=5)
    X, Y = R.cut(inp["Ss"], inp["alpha"], True), inp["Y"].astype(np.float64)
    rows = np.r_[0:7, 50:61]
    full = O.predict_factored(None, X, sp.csr_matrix(Y), rows="source")
    np.testing.assert_allclose(R.oracle_source(X, Y, rows), full[rows], rtol=1e-13, atol=0)
    loo = O.predict_loo_factored(X, Y)
    np.testing.assert_allclose(R.oracle_folds(X, Y, np.arange(61)), loo, rtol=1e-13, atol=1e-300)
    for a, b in zip(R.terms_loo(X, Y, rows), R.terms_folds(X, Y, np.arange(61), rows=rows)):
        np.testing.assert_allclose(a, b, rtol=1e-13, atol=1e-300)
    np.testing.assert_allclose(R.terms_loo(X, Y, rows)[0], loo[rows], rtol=1e-13, atol=1e-300)   # no negative weights here
    np.testing.assert_allclose(R.oracle_folds(X, Y, np.arange(61), rows=rows), loo[rows], rtol=1e-13, atol=1e-300)


# ----------------------------------------------------------------------------- tier 1: exactly summable inputs
def _check_exact_inputs(mode, alpha_edge, symmetric):
    inp = R.exact_inputs(mode, alpha_edge=alpha_edge, symmetric=symmetric)
    Ss, Sq, Y, alpha = inp["Ss"], inp["Sq"], inp["Y"], inp["alpha"]
    ns = Ss.shape[0]
    X, Xq = R.cut(Ss, alpha, True), R.cut(Sq, alpha, True)
    Y64 = Y.astype(np.float64)
    # preconditions
    if symmetric:
        assert (Ss == Ss.T).all()
    else:       # every pair inside a block differs from its mirror, and so does most of the filler
        same_block = inp["block"][:, None] == inp["block"][None, :]
        off = same_block & ~np.eye(ns, dtype=bool)
        assert off.any() and (Ss != Ss.T)[off].all() and (X != X.T)[off].all() and (Ss != Ss.T)[~same_block].mean() > 0.5
        if mode == "loo":
            assert np.bincount(inp["block"]).min() >= 3
    assert (np.count_nonzero(Y, axis=0) == 1).all()                                   # one source per target
    below = np.nextafter(np.float32(alpha), np.float32(0))
    assert (Ss == below).any() and (Sq == below).any()                                # one ulp below alpha: cut
    assert (X[inp["block"][:, None] != inp["block"][None, :]] == 0).all()             # nothing kept outside the blocks
    assert (X[inp["block"][:, None] == inp["block"][None, :]] != 0).all()
    if alpha_edge:
        assert (Ss == np.float32(alpha)).any() and (Sq == np.float32(alpha)).any()    # exactly alpha: kept
    assert (np.abs(np.r_[Xq, X]) @ np.abs(X).T).max() < 16.0                          # < 2^24 units of 2^-20
    kf, ks, _ = O.degrees(sp.csr_matrix(X), sp.csr_matrix(Y64))
    if mode == "query":
        assert _pow2(kf) and _pow2(ks)
        want = R.oracle_query(Xq, X, Y64)
        run = lambda **d: R.plane_scores(Xq, X, Y, True, **d)
    elif mode == "loo":
        assert _pow2(kf - 1) and _pow2(ks - 1)                                        # has = 1 wherever T is non-zero
        want = O.predict_loo_factored(X, Y64)
        np.testing.assert_array_equal(R.oracle_folds(X, Y64, np.arange(ns)), want)
        run = lambda rows=None, **d: R.plane_scores_folds(X, Y, np.arange(ns), True, rows=rows, **d)
    else:
        fold = inp["fold"]
        for phi in range(9):
            keep = fold != phi
            fkf, fks, _ = O.degrees(sp.csr_matrix(X[np.ix_(keep, keep)]), sp.csr_matrix(Y64[keep]))
            assert set(fkf) == {32} and set(fks) == {64}
        want = R.oracle_folds(X, Y64, fold)
        run = lambda rows=None, **d: R.plane_scores_folds(X, Y, fold, True, rows=rows, **d)
    assert (want != 0).mean() >= 0.10
    # the faithful model: representable in fp32, equal to float32(oracle), and not by a lucky rounding
    model = run()
    assert (model.astype(np.float32).astype(np.float64) == model).all()
    R.assert_bitwise(model.astype(np.float32), want, f"model {mode}")
    ulp = np.spacing(np.abs(model.astype(np.float32))).astype(np.float64)
    assert (np.abs(want - model) <= 0.25 * ulp).all()
    # every single defect
    if mode == "query":
        _check_mutants(True, run, lambda s: R.bitwise_violations(s.astype(np.float32), want), want)
    else:
        rows = np.arange(0, ns, 4)
        _check_mutants(True, lambda **d: run(rows=rows, **d),
                       lambda s: R.bitwise_violations(s.astype(np.float32), want[rows]), want[rows])
    return inp, X, Xq, want


@pytest.mark.parametrize("alpha_edge", [False, True])
@pytest.mark.parametrize("mode", ["query", "loo", "kfold"])
def test_exact_inputs_are_exact_and_resolve_every_plane_product(mode, alpha_edge):
    _check_exact_inputs(mode, alpha_edge, True)


@pytest.mark.parametrize("alpha_edge", [False, True])
@pytest.mark.parametrize("mode", ["query", "loo", "kfold"])
def test_asymmetric_exact_inputs_are_exact_and_show_a_transposed_operand_in_every_row(mode, alpha_edge):
    """The asymmetric-value tier 1 keeps every property of the symmetric one, and a device that reads the source-side
    operand as Ss[f, s], or the whole Ss transposed, changes at least one bit of every non-zero score row.  The pattern
    is symmetric here (all pairs of a block), so the defects of the degrees cannot show and are not asked to."""
    inp, X, Xq, want = _check_exact_inputs(mode, alpha_edge, False)
    Y = inp["Y"]
    kw = dict(Xq=Xq) if mode == "query" else dict(fold=inp["fold"]) if mode == "kfold" else {}
    ok = R.transposed_scores(mode, X, Y, **kw)
    assert (ok.astype(np.float32) == want.astype(np.float32)).all()    # the device form is the oracle on these inputs
    rows_nz = (want != 0).any(axis=1)
    assert rows_nz.mean() > 0.9
    for defect in ("source_operand_transposed", "input_transposed"):
        got = R.transposed_scores(mode, X, Y, defect=defect, **kw)
        changed = R.bitwise_violations(got.astype(np.float32), want).any(axis=1)
        assert changed[rows_nz].all(), (defect, int((~changed[rows_nz]).sum()))
    for defect in ("has_transposed", "degrees_swapped", "fold_recount_transposed"):
        if mode in R.TRANSPOSE_DEFECTS[defect]:
            assert (R.transposed_scores(mode, X, Y, defect=defect, **kw) == ok).all()


# ----------------------------------------------------------------------------- tier 2: derived bands
def _check_single_feature_inputs(symmetric):
    inp = R.single_feature_inputs(symmetric=symmetric)
    X, Xq = R.cut(inp["Ss"], inp["alpha"], False), R.cut(inp["Sq"], inp["alpha"], False)
    Y = inp["Y"]
    assert (np.count_nonzero(Xq, axis=1) == 1).all() and (np.count_nonzero(Y, axis=0) == 1).all()
    kf, ks, _ = O.degrees(sp.csr_matrix(X), sp.csr_matrix(Y.astype(np.float64)))
    assert (~np.isin(np.r_[kf, ks], 2 ** np.arange(12))).mean() > 0.9 and len(set(kf)) > 20   # arbitrary degrees
    want = R.oracle_query(Xq, X, Y)
    band = R.band_single_term(want)
    run = lambda **d: R.plane_scores(Xq, X, Y, False, **d)
    R.assert_band(run(), want, band, "model, one feature per row")
    R.assert_band(run().astype(np.float32), want, band, "model rounded to fp32")
    _check_mutants(False, run, lambda s: R.band_violations(s, want, band), want)
    return inp, X, Xq, want, band


def test_single_feature_inputs_resolve_the_planes_of_one_reciprocal():
    inp, X, _, _, _ = _check_single_feature_inputs(True)
    assert (inp["Ss"] == inp["Ss"].T).all()
    _assert_defects_invisible("query", X, inp["Y"], Xq=R.cut(inp["Sq"], inp["alpha"], False))


def test_asymmetric_single_feature_inputs_show_every_transposition():
    """kf a column count, ks a row count, one term per score: each transposition leaves 4 * 2^-24 of the score."""
    inp, X, Xq, want, band = _check_single_feature_inputs(False)
    _assert_asymmetric_pattern(X)
    assert (np.count_nonzero(X, axis=0) != np.count_nonzero(X, axis=1)).mean() > 0.8
    _assert_defects_visible("query", X, inp["Y"], want, band, Xq=Xq)


def _assert_asymmetric_pattern(X):
    one_sided = (X != 0) & (X.T == 0)
    assert one_sided.sum() >= 0.2 * np.count_nonzero(X - np.diag(np.diag(X)))


def _assert_defects_invisible(mode, X, Y, **kw):
    """On a symmetric Ss every transposition computes the correct device's bits: the gap the asymmetric inputs close."""
    assert (X == X.T).all()
    ok = R.transposed_scores(mode, X, Y, **kw)
    for defect, modes in R.TRANSPOSE_DEFECTS.items():
        if mode in modes:
            got = R.transposed_scores(mode, X, Y, defect=defect, **kw)
            assert got.tobytes() == ok.tobytes(), (mode, defect)
    return ok


def _assert_defects_visible(mode, X, Y, want, band, **kw):
    """The correct device form is the oracle (far inside the band); every defect that applies to `mode` leaves the band
    on at least MIN_SHARE_T of the non-zero scores."""
    ok = R.transposed_scores(mode, X, Y, **kw)
    np.testing.assert_allclose(ok, want, rtol=1e-13, atol=1e-300)
    assert not R.band_violations(ok, want, band).any()
    seen = 0
    for defect, modes in R.TRANSPOSE_DEFECTS.items():
        if mode in modes:
            share = _share(R.band_violations(R.transposed_scores(mode, X, Y, defect=defect, **kw), want, band), want)
            assert share >= MIN_SHARE_T, f"{mode}: '{defect}' is visible on only {share:.1%} of the non-zero scores"
            seen += 1
    assert seen >= 3


def _random_case(nq, ns, weighted, mode, symmetric):
    inp = R.random_inputs(nq, ns, weighted, mode, symmetric=symmetric)
    alpha, Ss, Sq, Y = inp["alpha"], inp["Ss"], inp["Sq"], inp["Y"]
    X, Xq = R.cut(Ss, alpha, weighted), R.cut(Sq, alpha, weighted)
    assert (np.count_nonzero(Y, axis=0) == 1).all()
    at = Ss == np.float32(alpha)
    assert at.any() and (X[at] != 0).all() and Sq[0, 1] == np.float32(alpha) and Xq[0, 1] != 0    # exactly alpha: kept
    if symmetric:
        assert (Ss == Ss.T).all()
    else:
        assert (X.T[at] == 0).all()                                                   # ... on one side only
        _assert_asymmetric_pattern(X)
    return inp, X, Xq, Y, np.count_nonzero(X, axis=0)


@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("shape", [(37, 321), (129, 256), (200, 130)])
def test_random_inputs_and_their_bands(shape, weighted):
    nq, ns = shape

    def case(mode):
        return _random_case(nq, ns, weighted, mode, True)

    band = lambda t: R.band_general(*t, dropped_products=weighted)
    # query rows: model inside the band, every defect outside it; source rows of the same graph.  (The fold modes of these
    # inputs serve the shapes and offsets of tier 3: a fold's row is non-zero only at the targets of its few neighbours,
    # below the 10 % that a defect check needs; the defects of the fold modes are resolved by the tier-1 inputs.)
    inp, X, Xq, Y, kf = case("query")
    if weighted:
        assert (kf == 0).any() and _pow2(kf[kf > 0]) and len(set(kf)) >= 4           # fl(x * fl(1/kf)) is exact
    else:
        assert (~np.isin(kf, 2 ** np.arange(12))).mean() > 0.8 and len(set(kf)) > 10  # arbitrary degrees
    want, bq = R.oracle_query(Xq, X, Y), band(R.terms(Xq, X, Y))
    run = lambda **d: R.plane_scores(Xq, X, Y, weighted, **d)
    R.assert_band(run(), want, bq, f"model query {shape} weighted={weighted}")
    _check_mutants(weighted, run, lambda s: R.band_violations(s, want, bq), want)
    rows = np.concatenate([np.arange(a, b) for a, b in R.row_ranges(ns)[1:]])
    R.assert_band(R.plane_scores_source(X, Y, weighted, rows), R.oracle_source(X, Y, rows),
                  band(R.terms_source(X, Y, rows)), "model source rows")
    # leave-one-out
    inp, X, Xq, Y, kf = case("loo")
    if weighted:
        assert (kf == 0).any() and _pow2(kf[kf > 0] - 1)                             # fl(x * fl(1/(kf - 1))) is exact
    loo, rows = np.arange(ns), rows[::3]
    R.assert_band(R.plane_scores_folds(X, Y, loo, weighted, rows=rows), R.oracle_folds(X, Y, loo, rows=rows),
                  band(R.terms_loo(X, Y, rows)), "model leave-one-out")
    # k-fold
    inp, X, Xq, Y, kf = case("kfold")
    fold = inp["fold"]
    assert set(fold) == set(range(inp["nfolds"]))
    if weighted:
        for phi in range(3):
            fkf = np.count_nonzero(X[np.ix_(fold != phi, fold != phi)], axis=0)
            assert _pow2(fkf[fkf > 0])
    R.assert_band(R.plane_scores_folds(X, Y, fold, weighted), R.oracle_folds(X, Y, fold),
                  band(R.terms_folds(X, Y, fold)), "model k-fold")


@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("shape", [(37, 321), (129, 256), (130, 260), (200, 130)])
def test_asymmetric_random_inputs_their_bands_and_every_transposition(shape, weighted):
    """random_inputs(symmetric=False) keeps what the symmetric inputs promise (an entry exactly at alpha, one source per
    target, edge-less sources and exact feature scaling when weighted, the plane model inside the band in every mode),
    has an asymmetric pattern with row degrees that differ from the column degrees, and shows each transposition of
    TRANSPOSE_DEFECTS outside the GPU test's band on at least a tenth of the non-zero scores of every mode it applies
    to.  The same defects are bit-identical to the correct form on the symmetric inputs."""
    nq, ns = shape
    band = lambda t: R.band_general(*t, dropped_products=weighted)
    rows = np.concatenate([np.arange(a, b) for a, b in R.row_ranges(ns)[1:]])
    for mode in ("query", "loo", "kfold"):
        inp, X, Xq, Y, kf = _random_case(nq, ns, weighted, mode, False)
        fold = inp["fold"]
        assert (kf != np.count_nonzero(X, axis=1)).mean() > 0.5                       # column degree != row degree
        if not weighted:
            assert (~np.isin(kf, 2 ** np.arange(12))).mean() > 0.8 and len(set(kf)) > 10  # arbitrary degrees
        if weighted:
            assert (kf == 0).sum() >= 3
            if mode == "kfold":
                for phi in range(3):
                    fkf = np.count_nonzero(X[np.ix_(fold != phi, fold != phi)], axis=0)
                    assert _pow2(fkf[fkf > 0])
            else:
                assert _pow2(kf[kf > 0] - (mode == "loo")) and len(set(kf)) >= 4
        sym = _random_case(nq, ns, weighted, mode, True)
        if mode == "query":
            want, bq = R.oracle_query(Xq, X, Y), band(R.terms(Xq, X, Y))
            R.assert_band(R.plane_scores(Xq, X, Y, weighted), want, bq, "model query, asymmetric")
            _assert_defects_visible("query", X, Y, want, bq, Xq=Xq)
            _assert_defects_invisible("query", sym[1], sym[3], Xq=sym[2])
            want, bs = R.oracle_source(X, Y, rows), band(R.terms_source(X, Y, rows))
            R.assert_band(R.plane_scores_source(X, Y, weighted, rows), want, bs, "model source rows, asymmetric")
            _assert_defects_visible("source", X, Y, want, bs, rows=rows)
            _assert_defects_invisible("source", sym[1], sym[3], rows=rows)
        elif mode == "loo":
            tl = R.terms_loo(X, Y, rows)
            for a, b in zip(tl, R.terms_folds(X, Y, np.arange(ns), rows=rows)):       # the identity on asymmetric input
                np.testing.assert_allclose(a, b, rtol=1e-13, atol=1e-300)
            want = R.oracle_folds(X, Y, np.arange(ns), rows=rows)
            np.testing.assert_allclose(O.predict_loo_factored(X, Y.astype(np.float64), queries=rows), want, rtol=1e-13,
                                       atol=1e-300)
            R.assert_band(R.plane_scores_folds(X, Y, np.arange(ns), weighted, rows=rows[::3]), want[::3],
                          band(R.terms_loo(X, Y, rows[::3])), "model leave-one-out, asymmetric")
            _assert_defects_visible("loo", X, Y, want, band(tl), rows=rows)
            _assert_defects_invisible("loo", sym[1], sym[3], rows=rows)
        else:
            want, bk = R.oracle_folds(X, Y, fold), band(R.terms_folds(X, Y, fold))
            R.assert_band(R.plane_scores_folds(X, Y, fold, weighted), want, bk, "model k-fold, asymmetric")
            _assert_defects_visible("kfold", X, Y, want, bk, fold=fold)
            _assert_defects_invisible("kfold", sym[1], sym[3], fold=sym[0]["fold"])


@pytest.mark.parametrize("alpha_edge", [False, True])
@pytest.mark.parametrize("mode", ["query", "loo", "kfold"])
def test_transpositions_are_invisible_on_the_symmetric_exact_inputs(mode, alpha_edge):
    inp = R.exact_inputs(mode, alpha_edge=alpha_edge)
    X, Xq = R.cut(inp["Ss"], inp["alpha"], True), R.cut(inp["Sq"], inp["alpha"], True)
    kw = dict(Xq=Xq) if mode == "query" else dict(fold=inp["fold"]) if mode == "kfold" else {}
    _assert_defects_invisible(mode, X, inp["Y"], **kw)


def _digest(inp):
    h = hashlib.sha256()
    for key in sorted(inp):
        if isinstance(inp[key], np.ndarray):
            a = np.ascontiguousarray(inp[key])
            h.update(f"{key} {a.dtype} {a.shape}".encode())
            h.update(a.tobytes())
    return h.hexdigest()


def test_the_symmetric_generators_return_their_earlier_arrays():
    """symmetric=True (the default) draws what the builders drew before the keyword existed: digests of every array of
    one input of each builder, recorded from the builders as they were."""
    assert _digest(R.exact_inputs("query")) == "ba3d6916cfc035d3e51b6817f3d905815766d0209944867b75c1cd7023e16aa5"
    assert _digest(R.exact_inputs("loo")) == "bfbfa203b95730cc70565e80be89240bd3195a05b13b21a2c1fd83af0d3c1a07"
    assert _digest(R.exact_inputs("kfold", symmetric=True)) == "e69338406613688ed7f5e8f228c22f6a4ddfc5600eda2b3a7a08831a288c1d90"
    assert _digest(R.single_feature_inputs()) == "a23a964a71b44bb47a7eaad7faeeef6d04960322341c97196a54015d1fd23bf3"
    assert _digest(R.random_inputs(129, 256, False)) == "26e7562863f1a2594bd263ce51e3ed198f4386fda8c72cbf893381344804780a"
    assert _digest(R.random_inputs(129, 256, True, "loo")) == "06aa3067366a67e6e2d3f348373169f75fe855342418cfa0c0c05c76d9eba025"
    assert _digest(R.random_inputs(37, 321, True, "kfold", symmetric=True)) == "811d4baf6c1ced95f638e62a0bc1e574e657c777e619ebf90f397092d3fac92c"
    assert _digest(R.random_inputs(200, 130, True, "query")) == "2c846071a13747811dec5105e8fc6b9f574f6e1742922d1b441d3b279105b583"


def test_row_ranges_cover_every_alignment_and_length():
    for ns in (130, 256, 260, 321, 2176):
        rr = R.row_ranges(ns)
        assert {a % 4 for a, _ in rr} == {0, 1, 2, 3}
        assert all(0 <= a < b <= ns for a, b in rr) and rr[-1][1] == ns
        lens = [b - a for a, b in rr]
        assert 128 in lens and 129 in lens and min(lens) < 4
