"""The oracle against the reference's own known-answer tests (test/runtests.jl) and
against itself (literal dense form == factored sparse form == LOO identity)."""
import os

import numpy as np
import pytest
import scipy.sparse as sp

from oracle import simspread_oracle as O
from oracle.simspread_oracle import Named


def test_k_kat(kats):
    M = np.array(kats["k"]["M"], dtype=float)
    assert int(O.k(M[0])) == 0
    assert O.k(M).ravel().tolist() == kats["k"]["row_degrees"]
    assert O.k(M).shape == (4, 1)


def test_cutoff_kats(kats):
    c = kats["cutoff"]
    x, y, z = c["x"], np.array(c["y"]).reshape(-1, 1), np.array(c["z"])
    for case in c["cases"]:
        a = case["alpha"]
        assert O.cutoff(x, a, False) == pytest.approx(case["x_bin"])
        assert O.cutoff(x, a, True) == pytest.approx(case["x_w"])
        np.testing.assert_allclose(O.cutoff(y, a, False).ravel(), case["y_bin"])
        np.testing.assert_allclose(O.cutoff(y, a, True).ravel(), case["y_w"])
        np.testing.assert_allclose(O.cutoff(z, a, False), case["z_bin"])
        np.testing.assert_allclose(O.cutoff(z, a, True), case["z_w"])


def test_cutoff_inclusive():
    assert O.cutoff(0.5, 0.5, False) == 1.0
    assert O.cutoff(np.nextafter(0.5, 0), 0.5, False) == 0.0


def test_featurize_kat(kats):
    f = kats["featurize"]
    M0 = Named(f["M0"], f["rows"], f["cols"])
    u = O.featurize(M0, f["alpha"], False)
    w = O.featurize(M0, f["alpha"], True)
    assert u.cols == f["out_cols"] and w.cols == f["out_cols"]
    np.testing.assert_array_equal(u.array, f["unweighted"])
    np.testing.assert_array_equal(w.array, f["weighted"])


def test_construct_kat(kats):
    c = kats["construct"]
    X = Named(c["X"], c["X_rows"], c["X_cols"])
    y = Named(c["y"], c["y_rows"], c["y_cols"])
    A, B = O.construct_queries(y, X, c["queries"])
    assert A.rows == c["node_order"] and A.cols == c["node_order"]
    assert B.rows == c["node_order"] and B.cols == c["node_order"]
    np.testing.assert_array_equal(A.array, A.array.T)
    assert not B.array[0].any() and not B.array[:, 0].any()
    X2 = Named(c["X"], c["X_rows"], c["X_rows"])  # features named like sources
    with pytest.raises(AssertionError, match=c["same_names_message"]):
        O.construct_queries(y, X2, c["queries"])
    X3 = Named(c["row_mismatch_X"], c["row_mismatch_rows"], c["X_cols"])
    with pytest.raises(AssertionError, match=c["row_mismatch_message"]):
        O.construct_queries(y, X3, c["queries"])


def test_spread_kat(kats):
    s = kats["spread"]
    # Julia's `≈` on arrays is norm-based: norm(x-y) <= rtol*max(norm(x), norm(y))
    got, want = O.spread(np.array(s["M"], float)), np.array(s["W"])
    assert np.linalg.norm(got - want) <= s["rtol"] * max(np.linalg.norm(got), np.linalg.norm(want))
    np.testing.assert_allclose(got, [[1, 0, 0], [0.5, 0.5, 0], [1 / 3, 1 / 3, 1 / 3]], rtol=1e-15)


def test_spread_zero_degree_rows_give_zero():
    W = O.spread(np.array([[0.0, 0.0], [2.0, 0.5]]))
    np.testing.assert_array_equal(W, [[0, 0], [1.0, 0.25]])  # count, not weight sum


def test_predict_kat_exact(kats):
    p = kats["predict"]
    A = Named(p["A"], p["names"], p["names"])
    B = Named(p["B"], p["names"], p["names"])
    y = Named(p["y"], p["y_rows"], p["y_cols"])
    yhat = O.predict(A, B, y)
    assert yhat.rows == p["y_rows"] and yhat.cols == p["y_cols"]
    assert (yhat.array == np.array(p["yhat"])).all()  # reference uses exact ==


def test_clean_kat(kats):
    c = kats["clean"]
    A = Named(c["A"], c["names"], c["names"])
    y = Named(c["y"], c["y_rows"], c["y_cols"])
    yhat = Named(c["yhat_in"], c["y_rows"], c["y_cols"])
    O.clean(yhat, A, y)
    np.testing.assert_array_equal(yhat.array, c["yhat_out"])


def _random_named(seed, nq=5, ns=17, nf=17, nt=7, weighted=True):  # Nf == Ns: the reference name check needs it (quirk 6)
    rng = np.random.default_rng(seed)
    def m(r, c, d):
        a = (rng.random((r, c)) < d) * (rng.random((r, c)) * 0.5 + 0.5 if weighted else 1.0)
        return a
    Xq, Xs, Ys = m(nq, nf, 0.4), m(ns, nf, 0.4), (rng.random((ns, nt)) < 0.3).astype(float)
    Xs[:, 2] = 0.0     # a zero-degree feature
    Xs[3, :] = 0.0     # an isolated source
    Ys[3, :] = 0.0
    Ys[:, 1] = 0.0     # a zero-degree target
    q = [f"q{i}" for i in range(nq)]
    s = [f"s{i}" for i in range(ns)]
    f = [f"f{i}" for i in range(nf)]
    t = [f"t{i}" for i in range(nt)]
    return (Named(Xq, q, f), Named(Xs, s, f), Named(Ys, s, t),
            Named(np.zeros((nq, nt)), q, t))


@pytest.mark.parametrize("seed,weighted", [(1, True), (2, False), (3, True)])
def test_literal_equals_factored(seed, weighted):
    Xq, Xs, Ys, yq = _random_named(seed, weighted=weighted)
    A, B = O.construct_split(Ys, yq, Xs, Xq)
    lit_q = O.predict(A, B, yq).array
    lit_s = O.predict(A, B, Ys).array
    np.testing.assert_allclose(O.predict_factored(Xq.array, Xs.array, Ys.array, "query"), lit_q, rtol=1e-12, atol=1e-15)
    np.testing.assert_allclose(O.predict_factored(Xq.array, Xs.array, Ys.array, "source"), lit_s, rtol=1e-12, atol=1e-15)
    A3 = O.construct_single(Ys, Xs)
    np.testing.assert_allclose(O.predict_single(A3, Ys).array, lit_s, rtol=1e-12, atol=1e-15)


def _iid_similarity(rng, n):
    """An asymmetric source similarity: iid U(0, 1), unit diagonal.  Element (s, f) is source s against feature f."""
    S = rng.random((n, n))
    np.fill_diagonal(S, 1.0)
    return S


def _assert_orientation_matters(X, form, want, tol=1e-3):
    """The cut pattern has one-sided pairs, and `form` on the transposed X is far from the literal result (the clean!
    markers aside): an input regenerated as symmetric, or a form that reads X[f, s], cannot pass."""
    X = np.asarray(X)
    assert ((X != 0) & (X.T == 0)).sum() >= 10
    other = form(np.ascontiguousarray(X.T))
    assert np.abs(other - want)[want != -99.0].max() > tol


def _literal_loo(X, Y, names, queries=None):
    """construct(y, X, [name]) -> predict -> clean! for every source (or those of `queries`), one fold at a time."""
    out = []
    for i in (range(len(names)) if queries is None else queries):
        A, B = O.construct_queries(Y, X, [names[i]])
        yq = Y.sub([names[i]], Y.cols)
        yhat = O.predict(A, B, yq)
        O.clean(yhat, A, yq)
        out.append(yhat.array[0])
    return np.array(out)


@pytest.mark.parametrize("seed,weighted", [(4, True), (5, False)])
def test_loo_identity(seed, weighted):
    rng = np.random.default_rng(seed)
    n, nt = 24, 6
    names = [f"d{i:02d}" for i in range(n)]
    for symmetric in (True, False):
        if symmetric:
            S = rng.random((n, n)); S = (S + S.T) / 2; np.fill_diagonal(S, 1.0)
        else:
            S = _iid_similarity(rng, n)
        X = O.featurize(Named(S, names, names), 0.55, weighted)
        Y = Named((rng.random((n, nt)) < 0.25).astype(float), names, [f"t{i}" for i in range(nt)])
        Y.array[:, 2] = 0.0; Y.array[5, 2] = 1.0   # target whose only edge is source 5 -> clean! case
        fast = O.predict_loo_factored(X.array, Y.array, clean_flag=True)
        lit = _literal_loo(X, Y, names)
        np.testing.assert_allclose(fast, lit, rtol=1e-12, atol=1e-15)
        assert fast[5, 2] == -99.0
        if not symmetric:
            _assert_orientation_matters(X.array, lambda Xt: O.predict_loo_factored(Xt, Y.array, clean_flag=True), lit)


def test_feature_filter_strips_all_leading_f():
    # quirk: lstrip(f, 'f') removes every leading 'f' (src/core.jl:152)
    names = ["foo", "bar", "oo"]
    X = Named(np.ones((3, 3)), names, ["f" + n for n in names])
    y = Named(np.eye(3), names, ["t0", "t1", "t2"])
    A, _ = O.construct_queries(y, X, ["oo"])
    # "ffoo" -> "oo" and "foo" -> "oo": both feature columns vanish, only "fbar" stays
    assert A.rows == ["oo", "foo", "bar", "fbar", "t0", "t1", "t2"]


def _iris():
    here = os.path.join(os.path.dirname(__file__), "golden", "iris")
    def read(p):
        with open(os.path.join(here, p)) as f:
            lines = f.read().splitlines()
        cols = lines[0].split()
        rows = [l.split()[0] for l in lines[1:]]
        vals = np.array([[float(v) for v in l.split()[1:]] for l in lines[1:]])
        return rows, cols, vals
    rows, fc, F = read("iris.features")
    _, cc, C = read("iris.classes")
    mn = np.minimum(F[:, None, :], F[None, :, :]).sum(-1)
    mx = np.maximum(F[:, None, :], F[None, :, :]).sum(-1)
    return rows, cc, mn / mx, C


def test_iris_simmat_matches_reference_file():
    p = os.path.join(os.path.dirname(__file__), "golden", "iris", "iris.simmat")
    rows, _, S, _ = _iris()
    with open(p) as f:
        lines = f.read().splitlines()
    ref = np.array([[float(v) for v in l.split()[1:]] for l in lines[1:]])
    np.testing.assert_allclose(S, ref, rtol=0, atol=1e-14)


def test_iris_single_loo_fold_literal_vs_factored():
    rows, cc, S, C = _iris()
    X = O.featurize(Named(S, rows, rows), 0.9, True)
    Y = Named(C, rows, cc)
    fast = O.predict_loo_factored(X.array, Y.array, clean_flag=True, queries=[0, 77, 149])
    for o, i in enumerate([0, 77, 149]):
        A, B = O.construct_queries(Y, X, [rows[i]])
        yq = Y.sub([rows[i]], cc)
        yhat = O.predict(A, B, yq)
        O.clean(yhat, A, yq)
        np.testing.assert_allclose(fast[o], yhat.array[0], rtol=1e-12, atol=1e-15)
    assert A.array.shape == (302, 302)


def test_name_check_needs_equal_counts():
    # quirk 6: element-wise compare of the sorted name vectors -> DimensionMismatch unless Nf == Ns
    X = Named(np.ones((3, 2)), ["a", "b", "c"], ["fx", "fy"])
    y = Named(np.ones((3, 1)), ["a", "b", "c"], ["t"])
    with pytest.raises(ValueError, match="DimensionMismatch"):
        O.construct_single(y, X)


def test_loo_dense_form_equals_factored_form():
    """predict_loo_dense (used to check the dense-similarity regime at sizes where a sparse copy of a 90 % full
    matrix is impractical) against predict_loo_factored, weighted and unweighted, with an isolated target; on an
    asymmetric similarity both also against the literal fold loop."""
    rng = np.random.default_rng(5)
    n, nt = 60, 17
    S = rng.random((n, n)); S = np.triu(S, 1); S = S + S.T; np.fill_diagonal(S, 1.0)
    Y = (rng.random((n, nt)) < 0.15).astype(np.float64)
    Y[:, 3] = 0.0
    Y[5, 4] = 1.0; Y[:5, 4] = 0.0; Y[6:, 4] = 0.0          # a target whose only edge belongs to one query
    names = [f"d{i:02d}" for i in range(n)]
    Yn = Named(Y, names, [f"t{i}" for i in range(nt)])
    for symmetric in (True, False):
        if not symmetric:
            S = _iid_similarity(rng, n)
        for alpha, weighted in ((0.1, True), (0.5, False), (0.9, True)):
            X = O.cutoff(S, alpha, weighted)
            a = O.predict_loo_dense(X, Y, clean_flag=True)
            b = O.predict_loo_factored(X, Y, clean_flag=True)
            assert np.abs(a - b).max() < 1e-13
            assert ((a == -99) == (b == -99)).all()
            if not symmetric:
                lit = _literal_loo(Named(X, names, ["f" + c for c in names]), Yn, names)
                np.testing.assert_allclose(a, lit, rtol=1e-12, atol=1e-15)
                np.testing.assert_allclose(b, lit, rtol=1e-12, atol=1e-15)
                _assert_orientation_matters(X, lambda Xt: O.predict_loo_dense(Xt, Y, clean_flag=True), lit)


def test_c_oracle_equals_python_oracle():
    """oracle/factored.c (the checker of the full-size GPU tests and bench.py's cpu_baseline) against the numpy
    factored form it restates, on a seeded graph with a zero-degree feature, an isolated source and weighted edges."""
    from oracle import c_oracle
    Xq, Xs, Ys = O.synth_bipartite(70, 90, 90, 41, 0.08, 0.06, seed=11, weighted=True, dtype=np.float64)
    Xs = Xs.tolil(); Xs[:, 7] = 0.0; Xs[12, :] = 0.0; Xs = Xs.tocsr(); Xs.eliminate_zeros()
    Ys = Ys.tolil(); Ys[12, :] = 0.0; Ys = Ys.tocsr(); Ys.eliminate_zeros()
    want = O.predict_factored(Xq, Xs, Ys, "query")
    got = c_oracle.predict_query(Xq, Xs, Ys)
    assert np.abs(got - want).max() <= 1e-15 * max(1.0, np.abs(want).max()) * 64
    prep = c_oracle.Prepared(Xq, Xs, Ys)
    assert np.array_equal(prep.predict(3, 40), got[3:40])       # prepared form == one-shot form, any row block
    assert np.array_equal(prep.predict(threads=1), got)
    prep.close()


def _loo_edge_graph(seed, n=240, nt=70):
    """A square weighted X and labels Y with the corner cases of the leave-one-out identity: a feature of degree 1
    (kf - 1 = 0 for its one query), a source whose only edge is to itself, a target whose only edge is one query
    (clean!), an empty label row, an all-zero target, and an explicitly stored zero in X."""
    import scipy.sparse as sp
    rng = np.random.default_rng(seed)
    X = sp.random(n, n, density=0.05, format="lil", random_state=rng)
    X.setdiag(1.0)
    X[:, 17] = 0.0; X[40, 17] = 0.8             # feature 17 has degree 1: its only source is 40
    X[23, :] = 0.0; X[:, 23] = 0.0; X[23, 23] = 1.0   # source 23: only edge is to itself
    X = X.tocsr()
    X.data = 0.5 + 0.5 * rng.random(X.nnz)
    X.data[X.indptr[5] + 1] = 0.0                # an explicitly stored zero is no edge
    Y = sp.random(n, nt, density=0.06, format="lil", random_state=rng)
    Y[:, 4] = 0.0; Y[71, 4] = 1.0                # target 4: only edge is source 71
    Y[:, 6] = 0.0                                # target 6: no edge at all
    Y[23, :] = 0.0; Y[100, :] = 0.0              # empty label rows
    Y = Y.tocsr()
    Y.data[:] = 1.0
    return X, Y


@pytest.mark.parametrize("seed", [1, 2])
def test_c_loo_equals_python_loo(seed):
    """oracle_predict_loo_rows (the checker of the at-size leave-one-out GPU tests) against predict_loo_factored, with
    and without clean!, and the same rows from any block split as from one whole-range call."""
    from oracle import c_oracle
    X, Y = _loo_edge_graph(seed)
    n = X.shape[0]
    prep = c_oracle.PreparedLoo(X, Y)
    for clean in (False, True):
        want = O.predict_loo_factored(X, Y, clean_flag=clean)
        got = prep.predict(clean=clean)
        np.testing.assert_allclose(got, want, rtol=1e-14, atol=0)
        assert np.array_equal(got == 0, want == 0)
        if clean:
            assert got[71, 4] == -99.0 and (got[:, 6] == -99.0).all() and (got[:, 4] == -99).sum() == 1
        # blocks starting and ending mid-range, a single row, an empty block, one thread
        for i0, i1 in ((0, 1), (3, 97), (40, 41), (97, 203), (203, n), (17, 17)):
            assert np.array_equal(prep.predict(i0, i1, clean=clean), got[i0:i1]), (i0, i1)
        assert np.array_equal(prep.predict(5, 150, clean=clean, threads=1), got[5:150])
    assert (got[23] == np.where(got[23] == -99, -99, 0)).all()     # a source linked to nothing else scores 0
    prep.close()
    np.testing.assert_array_equal(c_oracle.predict_loo(X, Y, 10, 30, clean=True), got[10:30])
    # the pattern above is one-sided almost everywhere, and the orientation matters to both forms
    for form in (lambda Xt: O.predict_loo_factored(Xt, Y, clean_flag=True),
                 lambda Xt: c_oracle.predict_loo(sp.csr_matrix(Xt), Y, clean=True)):
        _assert_orientation_matters(X.toarray(), form, got)


@pytest.mark.parametrize("seed,weighted", [(1, True), (2, False)])
def test_c_loo_equals_the_literal_loop_on_an_asymmetric_similarity(seed, weighted):
    """oracle_predict_loo_rows against the literal construct -> predict -> clean! loop on an iid similarity with unit
    diagonal: which of X[s, q] and X[q, s] lowers a source's degree is visible here and nowhere on a symmetric X."""
    from oracle import c_oracle
    rng = np.random.default_rng(seed)
    n, nt = 40, 9
    names = [f"d{i:02d}" for i in range(n)]
    Yarr = (rng.random((n, nt)) < 0.2).astype(float)
    Yarr[:, 2] = 0.0; Yarr[5, 2] = 1.0
    Yn = Named(Yarr, names, [f"t{i}" for i in range(nt)])
    for alpha in (0.55, 0.9):
        X = O.cutoff(_iid_similarity(rng, n), alpha, weighted)
        lit = _literal_loo(Named(X, names, ["f" + c for c in names]), Yn, names)
        prep = c_oracle.PreparedLoo(sp.csr_matrix(X), sp.csr_matrix(Yarr))
        got = prep.predict(clean=True)
        prep.close()
        np.testing.assert_allclose(got, lit, rtol=1e-12, atol=1e-15)
        assert np.array_equal(got == -99, lit == -99) and got[5, 2] == -99.0
        np.testing.assert_allclose(O.predict_loo_factored(X, Yarr, clean_flag=True), lit, rtol=1e-12, atol=1e-15)
        _assert_orientation_matters(X, lambda Xt: c_oracle.predict_loo(sp.csr_matrix(Xt), sp.csr_matrix(Yarr), clean=True), lit)


def test_c_loo_missing_symbol_is_a_rebuild_error(monkeypatch):
    from oracle import c_oracle

    class Old:                               # a liboracle.so built before the leave-one-out form existed
        pass
    monkeypatch.setattr(c_oracle, "_lib", Old())
    X, Y = _loo_edge_graph(1, n=120, nt=10)
    with pytest.raises(RuntimeError, match="rebuild the oracle"):
        c_oracle.PreparedLoo(X, Y)


def test_blocked_dense_loo_equals_per_fold_dense_loo():
    """predict_loo_dense_blocked (the checker of every C4 fold at 20k) against predict_loo_dense, at block sizes that do
    and do not divide the fold list, on a 90 % full and a sparse cutoff, weighted and not, with an isolated target; on
    an asymmetric similarity also against the literal fold loop."""
    rng = np.random.default_rng(9)
    n, nt = 150, 31
    S = rng.random((n, n)); S = np.triu(S, 1); S = S + S.T; np.fill_diagonal(S, 1.0)
    Y = (rng.random((n, nt)) < 0.1).astype(np.float64)
    Y[:, 3] = 0.0
    Y[:, 4] = 0.0; Y[33, 4] = 1.0
    Y[50] = 0.0
    qs = list(range(7, 140))
    names = [f"d{i:03d}" for i in range(n)]
    Yn = Named(Y, names, [f"t{i}" for i in range(nt)])
    lit_rows = [7, 33, 50, 91, 139]
    for symmetric in (True, False):
        if not symmetric:
            S = _iid_similarity(rng, n)
        for alpha, weighted in ((0.1, True), (0.1, False), (0.9, True)):
            X = O.cutoff(S, alpha, weighted)
            want = O.predict_loo_dense(X, Y, clean_flag=True, queries=qs)
            for block in (1, 16, 50, 512):
                got = O.predict_loo_dense_blocked(X, Y, clean_flag=True, queries=qs, block=block)
                np.testing.assert_allclose(got, want, rtol=1e-13, atol=0)
                assert np.array_equal(got == -99, want == -99) and np.array_equal(got == 0, want == 0)
            assert (want[33 - 7, 4] == -99)
            np.testing.assert_allclose(O.predict_loo_dense_blocked(X, Y, block=64), O.predict_loo_dense(X, Y),
                                       rtol=1e-13, atol=0)
            if not symmetric:
                lit = _literal_loo(Named(X, names, ["f" + c for c in names]), Yn, names, queries=lit_rows)
                blocked = lambda Xt: O.predict_loo_dense_blocked(Xt, Y, clean_flag=True, queries=lit_rows, block=2)
                np.testing.assert_allclose(blocked(X), lit, rtol=1e-13, atol=1e-14)
                _assert_orientation_matters(X, blocked, lit)


def test_kfold_query_form_equals_the_literal_fold_loop():
    """c_oracle.predict_kfold (the checker of k-fold at 10k sources) against the reference's literal fold loop
    (construct(y, X, members) -> predict -> clean!) on the dense block graph, with a target whose edges all sit in one
    fold and an empty fold, on a symmetric and on an asymmetric similarity."""
    from oracle import c_oracle
    rng = np.random.default_rng(13)
    n, nt, k = 70, 19, 6
    names = [f"d{i:02d}" for i in range(n)]; tn = [f"t{i}" for i in range(nt)]
    for symmetric in (True, False):
        if symmetric:
            S = rng.random((n, n)); S = (S + S.T) / 2; np.fill_diagonal(S, 1.0)
        else:
            S = _iid_similarity(rng, n)
        Xn = O.featurize(Named(S, names, names), 0.7, True)
        Yarr = (rng.random((n, nt)) < 0.15).astype(float)
        Yarr[:, 2] = 0; Yarr[8, 2] = 1; Yarr[11, 2] = 1
        Yn = Named(Yarr, names, tn)
        fold = rng.integers(0, k - 1, size=n); fold[8] = fold[11] = 1        # fold k-1 stays empty
        want = np.zeros((n, nt))
        for phi in range(k):
            idx = [i for i in range(n) if fold[i] == phi]
            if not idx:
                continue
            members = [names[i] for i in idx]
            A, B = O.construct_queries(Yn, Xn, members)
            yq = Yn.sub(members, tn)
            yh = O.predict(A, B, yq); O.clean(yh, A, yq)
            want[idx] = yh.array
        got = c_oracle.predict_kfold(Xn.array, Yarr, fold, k, clean=True)
        np.testing.assert_allclose(got, want, rtol=1e-12, atol=1e-15)
        assert np.array_equal(got == -99, want == -99) and (got[8, 2] == -99) and (got[11, 2] == -99)
        np.testing.assert_allclose(c_oracle.predict_kfold(Xn.array, Yarr, fold, k), want * (want != -99), rtol=1e-12, atol=1e-15)
        if not symmetric:
            _assert_orientation_matters(Xn.array, lambda Xt: c_oracle.predict_kfold(Xt, Yarr, fold, k, clean=True), want)


def _helper_block():
    rng = np.random.default_rng(3)
    want = rng.random((40, 300)) * (rng.random((40, 300)) < 0.3)
    want[:, 7] = -99.0
    return want


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_compare_block_accepts_rounding_and_catches_subtle_errors(dtype):
    """The shared comparison of the at-size tests passes a block rounded to the result precision, and fails on each
    subtle error a kernel could make: one entry off by 1e-3 of itself, one contribution-carrying entry lost, two
    neighbouring rows exchanged, one clean! marker lost."""
    from block_compare import compare_block
    want = _helper_block()
    ok = want.astype(dtype)
    m = compare_block(ok, want, dtype, "rounded")
    assert m["elem"] <= (6e-8 if dtype == np.float32 else 1.2e-16)
    r, c = np.argwhere(want > 0)[5]

    def bad(f):
        g = ok.astype(np.float64).copy()
        f(g)
        with pytest.raises(AssertionError):
            compare_block(g, want, dtype, "perturbed")

    bad(lambda g: g.__setitem__((r, c), g[r, c] * (1 + 1e-3)))
    bad(lambda g: g.__setitem__((r, c), 0.0))
    bad(lambda g: g.__setitem__(slice(10, 12), g[[11, 10]]))
    bad(lambda g: g.__setitem__((3, 7), 0.0))
    bad(lambda g: g.__setitem__((r, c), np.nan))
    bad(lambda g: g.__setitem__(tuple(np.argwhere(want == 0)[0]), 1e-30))
