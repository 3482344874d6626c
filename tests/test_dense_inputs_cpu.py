"""CPU-side checks of the inputs of tests/test_gpu_dense.py (no GPU): for every input builder the stated preconditions
hold, the faithful plane model of dense_ref.py passes the very assertion the GPU test applies to the device result, and
every single defect of the model (a kept plane product dropped, a plane of either side zeroed, the two lo pairs reading
the wrong source plane) violates that assertion on at least half of the non-zero scores.  These are conditions on the
inputs: a builder that cannot meet them is changed, not the threshold."""
import numpy as np
import pytest
import scipy.sparse as sp

from oracle import simspread_oracle as O

import dense_ref as R

MIN_SHARE = 0.5


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
@pytest.mark.parametrize("alpha_edge", [False, True])
@pytest.mark.parametrize("mode", ["query", "loo", "kfold"])
def test_exact_inputs_are_exact_and_resolve_every_plane_product(mode, alpha_edge):
    inp = R.exact_inputs(mode, alpha_edge=alpha_edge)
    Ss, Sq, Y, alpha = inp["Ss"], inp["Sq"], inp["Y"], inp["alpha"]
    ns = Ss.shape[0]
    X, Xq = R.cut(Ss, alpha, True), R.cut(Sq, alpha, True)
    Y64 = Y.astype(np.float64)
    # preconditions
    assert (Ss == Ss.T).all()
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


# ----------------------------------------------------------------------------- tier 2: derived bands
def test_single_feature_inputs_resolve_the_planes_of_one_reciprocal():
    inp = R.single_feature_inputs()
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


@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("shape", [(37, 321), (129, 256), (200, 130)])
def test_random_inputs_and_their_bands(shape, weighted):
    nq, ns = shape

    def case(mode):
        inp = R.random_inputs(nq, ns, weighted, mode)
        alpha, Ss, Sq, Y = inp["alpha"], inp["Ss"], inp["Sq"], inp["Y"]
        X, Xq = R.cut(Ss, alpha, weighted), R.cut(Sq, alpha, weighted)
        assert (Ss == Ss.T).all() and (np.count_nonzero(Y, axis=0) == 1).all()
        at = Ss == np.float32(alpha)
        assert at.any() and (X[at] != 0).all() and Sq[0, 1] == np.float32(alpha) and Xq[0, 1] != 0    # exactly alpha: kept
        return inp, X, Xq, Y, np.count_nonzero(X, axis=0)

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


def test_row_ranges_cover_every_alignment_and_length():
    for ns in (130, 256, 260, 321, 2176):
        rr = R.row_ranges(ns)
        assert {a % 4 for a, _ in rr} == {0, 1, 2, 3}
        assert all(0 <= a < b <= ns for a, b in rr) and rr[-1][1] == ns
        lens = [b - a for a, b in rr]
        assert 128 in lens and 129 in lens and min(lens) < 4
