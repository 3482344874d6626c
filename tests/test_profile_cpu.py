"""Host side of the cutoff profiles (include/simspread_hip_profile.h), no GPU: the numpy restatement of the rule
(profile_ref.py) on hand-worked cases, the host-side members of CutoffProfile against brute force, and the refusals the
Python layer makes before it needs a device."""
import numpy as np
import pytest

import simspread_jl_amd as ss

import profile_ref as P

F32, F64 = np.float32, np.float64


def test_the_rule_on_a_hand_worked_matrix():
    S = np.array([[1.0, 0.5, 0.0, np.nan],
                  [0.5, 1.0, 0.25, -0.5],
                  [0.0, 0.25, 1.0, 0.0]], F32)
    cuts = np.array([-np.inf, -0.5, 0.0, 0.25, 0.5, 0.5, 1.0, 2.0, np.inf], F32)
    total, rows = P.profile_ref(S, cuts, weighted=True)
    # weighted: the zeros never count (v = 0), the NaN never counts
    assert rows.tolist() == [[2, 2, 2, 2, 2, 2, 1, 0, 0], [4, 4, 3, 3, 2, 2, 1, 0, 0], [2, 2, 2, 2, 1, 1, 1, 0, 0]]
    assert total.tolist() == [8, 8, 7, 7, 5, 5, 3, 0, 0] and total.dtype == np.int64 and rows.dtype == np.int32
    total, rows = P.profile_ref(S, cuts, weighted=False)
    # not weighted: v = 1, so a zero counts where s >= cut; the NaN still counts for none
    assert rows.tolist() == [[3, 3, 3, 2, 2, 2, 1, 0, 0], [4, 4, 3, 3, 2, 2, 1, 0, 0], [4, 4, 4, 2, 1, 1, 1, 0, 0]]
    assert total.tolist() == [11, 11, 10, 7, 5, 5, 3, 0, 0]
    # empty shapes
    for shape in ((0, 5), (5, 0), (0, 0)):
        total, rows = P.profile_ref(np.zeros(shape, F64), np.array([0.0, 1.0]), True)
        assert total.tolist() == [0, 0] and rows.shape == (shape[0], 2) and not rows.any()


def test_the_rule_is_the_cut_of_the_producers_reference_at_every_alpha():
    """profile_ref against the cutoff the producers' own host reference applies (neighbour_ref.ref_cut: keep iff
    s >= alpha and v != 0), cut by cut."""
    from neighbour_ref import ref_cut
    rng = np.random.default_rng(3)
    S = rng.integers(-4, 5, (37, 23)).astype(F32) / F32(4)
    cuts = np.array([-1.0, -0.25, 0.0, 0.0, 0.25, 0.5, 1.0, 1.5], F32)
    for weighted in (True, False):
        total, rows = P.profile_ref(S, cuts, weighted)
        for b, c in enumerate(cuts):
            M = ref_cut(S, float(c), weighted)
            assert total[b] == M.nnz and np.array_equal(rows[:, b], np.diff(M.indptr))


def test_tanimoto_dense_is_the_fingerprint_rule():
    bits = np.array([[1, 1, 0, 0], [1, 0, 0, 0], [0, 0, 0, 0], [0, 0, 0, 0], [1, 1, 1, 0]])
    F = ss.pack_fingerprints(bits)
    for T in (F32, F64):
        S = P.tanimoto_dense(F, None, T)
        assert S.dtype == T and S[0, 1] == T(1) / T(2) and S[0, 4] == T(2) / T(3) and S[1, 4] == T(1) / T(3)
        assert S[2, 3] == 1 and S[2, 2] == 1 and S[2, 0] == 0 and np.array_equal(S, S.T)
        X = P.tanimoto_dense(F[:2], F[2:], T)
        assert X.shape == (2, 3) and np.array_equal(X, S[:2, 2:])


def _profile(symmetric, seed=0, na=41, nb=29, ncuts=7):
    rng = np.random.default_rng(seed)
    nb = na if symmetric else nb
    cuts = np.sort(rng.choice(np.array([-0.5, 0.0, 0.1, 0.3, 0.5, 0.9, 1.0, 1.0, 1.5]), ncuts, replace=False)).astype(F32)
    S = rng.integers(0, 11, (na, nb)).astype(F32) / F32(10)
    if symmetric:
        S = np.maximum(S, S.T)
        np.fill_diagonal(S, 1)
    S[3] = 0                                   # a row without neighbours (but for its diagonal when symmetric)
    if symmetric:
        S[:, 3] = 0
        S[3, 3] = 1
    total, rows = P.profile_ref(S, cuts, True)
    return ss.CutoffProfile(cuts, total, rows, (na, nb), symmetric), S


@pytest.mark.parametrize("symmetric", [False, True])
def test_cutoff_profile_helpers_against_brute_force(symmetric):
    p, S = _profile(symmetric)
    na, nb = p.shape
    assert p.nnz.dtype == np.int64 and p.degrees.dtype == np.int32 and p.degrees.shape == (na, p.cuts.size)
    assert np.allclose(p.fill(), P.fill_ref(p.nnz, p.shape), rtol=0, atol=0)
    for k in (1, 2, 5, nb + 1):
        assert p.coverage(k).tolist() == P.coverage_ref(p.degrees, p.cuts, k)
        if symmetric:
            assert p.coverage(k, exclude_self=True).tolist() == P.coverage_ref(p.degrees, p.cuts, k, True)
    if symmetric:
        # the diagonal is what exclude_self takes away: coverage of the matrix without it, cut by cut
        off = S.copy()
        np.fill_diagonal(off, 0)
        _, rows = P.profile_ref(off, p.cuts, True)
        assert p.coverage(exclude_self=True).tolist() == ((rows >= 1).mean(axis=0)).tolist()
        assert p.coverage()[0] == 1.0 and p.coverage(exclude_self=True)[p.cuts <= 1].max() < 1.0  # row 3: only itself
    else:
        with pytest.raises(ValueError):
            p.coverage(exclude_self=True)
    for budget in (-1, 0, 1, int(p.nnz[2]), int(p.nnz[2]) - 1, int(p.nnz[0]), 10 ** 12):
        got, want = p.alpha_for_nnz(budget), P.alpha_for_nnz_ref(p.cuts.tolist(), p.nnz.tolist(), budget)
        assert got == want and (got is None or isinstance(got, float))
    for k in (0, 0.5, 1, 3.25, nb):
        assert p.alpha_for_mean_degree(k) == P.alpha_for_mean_degree_ref(p.cuts.tolist(), p.nnz.tolist(), na, k)
    assert p.alpha_for_nnz(-1) is None and p.alpha_for_nnz(int(p.nnz[0])) == p.cuts[0]


def test_cutoff_profile_of_empty_shapes():
    cuts = np.array([0.0, 0.5], F64)
    for shape in ((0, 4), (4, 0), (0, 0)):
        p = ss.CutoffProfile(cuts, np.zeros(2, np.int64), np.zeros((shape[0], 2), np.int32), shape)
        assert p.fill().tolist() == [0.0, 0.0] and p.coverage().tolist() == [0.0, 0.0]
        assert p.alpha_for_nnz(0) == 0.0 and p.alpha_for_mean_degree(1) == 0.0


def test_python_refuses_bad_cuts_metric_and_storage_without_a_device():
    """Every one of these raises before the library is asked for a device (on a machine without one the device's own
    error would be a SimSpreadError, which is none of the types below)."""
    F = ss.pack_fingerprints(np.eye(5, 70))
    X = np.arange(12.0).reshape(4, 3)
    profiles = ((ss.tanimoto_profile, (F,)), (ss.jaccard_profile, (X,)), (ss.dot_profile, (X,)),
                (ss.tanimoto_profile, (F, F)), (ss.jaccard_profile, (X, X)), (ss.dot_profile, (X, X)))
    bad = ([0.5, 0.3], [0.1, float("nan")], [float("nan")], [], [0.01 * b for b in range(33)], [[0.1, 0.2]])
    for fn, args in profiles:
        for cuts in bad:
            for dtype in (F32, F64):
                with pytest.raises(ValueError):
                    fn(*args, cuts=cuts, dtype=dtype)
        with pytest.raises(TypeError):
            fn(*args)                                      # no cuts at all
    for storage in ("bf16", "f16"):
        for cuts in bad:
            with pytest.raises(ValueError):
                ss.dot_profile(X, cuts=cuts, storage=storage)
        with pytest.raises(TypeError):
            ss.dot_profile(X, cuts=[0.5], storage=storage, dtype=F64)
    with pytest.raises(ValueError):
        ss.dot_profile(X, metric="euclid", cuts=[0.5])
    with pytest.raises(ValueError):
        ss.dot_profile(X, cuts=[0.5], storage="fp8")
    # cuts are compared in the graph's dtype: these two are distinct and ascending in fp64, equal (legal) in fp32
    from simspread_jl_amd import engine
    c = engine._profile_cuts([0.1, 0.1 + 1e-12], F32)
    assert c.dtype == F32 and c[0] == c[1]
    assert engine._profile_cuts([-np.inf, 0.0, 0.0, np.inf], F64).tolist() == [-np.inf, 0.0, 0.0, np.inf]
    assert engine._profile_cuts(0.5, F32).tolist() == [0.5] and engine.PROFILE_CUTS_MAX == 32
