"""Cutoff profiles on the device (include/simspread_hip_profile.h, csrc/cut_profile.hip): for every cut, total[b] and
rows[i, b] are the nnz and the row degrees of the matching plain producer at alpha = cuts[b].

Every comparison is exact equality of integers; there is no tolerance.  The reference is twofold: the producer's own
idx == NULL size query (ptr, nnz) at each cut -- unchanged code, pinned elsewhere -- and, for fingerprints, profile_ref
on a numpy S, where c / u is one correctly rounded division and numpy reproduces the device's bits in both precisions.

Shapes are the smallest that reach every edge of a 128-tile pass: one row, one short of a tile, one past a tile, three
row tiles (a triangle of six tiles with mirrored ones), six column tiles against two row tiles, word counts on both
sides of the 8 words of a staging step, feature counts on both sides of the 16 (fp32 / fp64) and 64 (16-bit) columns of
one."""
import ctypes as C

import numpy as np
import pytest

import simspread_jl_amd as ss

import dot_ref as R
import profile_ref as P

pytestmark = pytest.mark.gpu

F32, F64 = np.float32, np.float64
SUF = {F32: "f32", F64: "f64"}
CT = {F32: C.c_float, F64: C.c_double}
METRIC_CODE = {"cosine": 0, "tanimoto": 1, "dice": 2}
SENT = -7


# ----------------------------------------------------------------------------------------------- the two sides of a check
def producer(lib, kind, suf, head, na, alpha, weighted, ctype):
    """(nnz, row degrees) of the plain producer's size query (idx == NULL) on host operands."""
    fn = getattr(lib, f"ss_similarity_{kind}_csr_{suf}")
    ptr = np.zeros(na + 1, np.int64)
    nnz = C.c_int64(-1)
    rc = fn(*head, ctype(alpha), weighted, ptr.ctypes.data, None, None, 0, C.byref(nnz), 0)
    assert rc == 0, lib.ss_last_error()
    assert ptr[0] == 0 and ptr[na] == nnz.value
    return nnz.value, np.diff(ptr)


def profile(lib, kind, suf, head, na, cuts, weighted, want_rows=True, expect=0):
    """(total, rows) of one profile call on host operands; the outputs start sentinel-filled."""
    fn = getattr(lib, f"ss_similarity_{kind}_profile_{suf}")
    total = np.full(max(len(cuts), 1), SENT, np.int64)
    rows = np.full((na, max(len(cuts), 1)), SENT, np.int32)
    rc = fn(*head, cuts.ctypes.data, len(cuts), weighted, total.ctypes.data, rows.ctypes.data if want_rows else None, 0)
    assert rc == expect, (rc, lib.ss_last_error())
    return total, rows


def check_against_producer(lib, kind, suf, head, na, cuts, ctype, tag, weights=(1, 0)):
    """The contract, for every cut and both values of `weighted`; returns the weighted profile."""
    first = None
    for weighted in weights:
        total, rows = profile(lib, kind, suf, head, na, cuts, weighted)
        assert ss.path_last() == [tag]
        seen = {}
        for b, c in enumerate(cuts):
            key = float(c)
            if key not in seen:
                seen[key] = producer(lib, kind, suf, head, na, c, weighted, ctype)
            nnz, deg = seen[key]
            assert total[b] == nnz, (kind, suf, weighted, b, c)
            assert np.array_equal(rows[:, b], deg), (kind, suf, weighted, b, c)
        assert np.array_equal(total, rows.astype(np.int64).sum(axis=0))
        if first is None:
            first = (total, rows)
    return first


def addr(a):
    return None if a is None else a.ctypes.data


# ----------------------------------------------------------------------------------------------- 1. fingerprints
def fp_rows(n, nwords, seed):
    """Packed rows around a few prototypes; from nine rows on: two all-zero rows (u == 0: s = 1), rows {0}, {0, 1},
    {0, 1, 2} (similarities exactly 1/2, 1/3 and 2/3) and a duplicated row (s = 1)."""
    rng = np.random.default_rng(seed)
    d = 64 * nwords
    protos = rng.random((max(1, n // 16), d)) < 0.3
    bits = protos[rng.integers(0, protos.shape[0], n)] ^ (rng.random((n, d)) < 0.05)
    if n >= 9:
        bits[:5] = False
        bits[2, 0] = bits[3, :2] = bits[4, :3] = True
        bits[5] = bits[6]
    return ss.pack_fingerprints(bits)


def fp_cuts(T):
    return np.array([-np.inf, -0.5, 0.0, T(1) / T(3), T(1) / T(2), T(1) / T(2), 0.7, 1.0, 1.5, np.inf], T)


@pytest.mark.parametrize("na", [1, 127, 129, 300])
def test_fingerprint_profiles_are_the_producer_and_the_numpy_rule(na):
    lib = ss.init(0)
    for nwords in (1, 3, 9):
        Fa = fp_rows(na, nwords, seed=na + nwords)
        others = [None] + [fp_rows(nb, nwords, seed=na + nwords + nb) for nb in (1, 200, 641)]
        for Fb in others:
            nb = na if Fb is None else Fb.shape[0]
            head = (addr(Fa), na, addr(Fb), 0 if Fb is None else nb, nwords)
            for T in (F32, F64):
                cuts = fp_cuts(T)
                S = P.tanimoto_dense(Fa, Fb, T)
                if na >= 9 and nb >= 9:
                    assert (S == T(1) / T(3)).any() and (S == T(1) / T(2)).any() and (S[0, :5] == [1, 1, 0, 0, 0]).all()
                for weighted in (1, 0):
                    total, rows = profile(lib, "tanimoto", SUF[T], head, na, cuts, weighted)
                    assert ss.path_last() == ["tanimoto_profile"]
                    want_total, want_rows = P.profile_ref(S, cuts, bool(weighted))
                    assert np.array_equal(total, want_total) and np.array_equal(rows, want_rows)
                    assert rows.dtype == np.int32 and total.dtype == np.int64
                # and the producer itself; both weights on the symmetric and the widest cross shape
                both = Fb is None or nb == 641
                check_against_producer(lib, "tanimoto", SUF[T], head, na, cuts, CT[T], "tanimoto_profile",
                                       weights=(1, 0) if both else (1,))


def test_one_cut_and_thirty_two_cuts_and_the_python_mirror():
    import torch
    ss.init(0)
    Fa, Fb = fp_rows(300, 3, seed=1), fp_rows(200, 3, seed=2)
    for T in (F32, F64):
        S_sym, S_x = P.tanimoto_dense(Fa, None, T), P.tanimoto_dense(Fa, Fb, T)
        for cuts in ([0.4], np.linspace(0.0, 1.0, 32), [1 / 3] * 32, [-np.inf] * 3 + [np.inf] * 3):
            c = np.asarray(cuts, T)
            for weighted in (True, False):
                p = ss.tanimoto_profile(Fa, cuts=cuts, weighted=weighted, dtype=T)
                total, rows = P.profile_ref(S_sym, c, weighted)
                assert isinstance(p, ss.CutoffProfile) and p.symmetric and p.shape == (300, 300)
                assert p.cuts.dtype == T and np.array_equal(p.cuts, c)
                assert p.nnz.dtype == np.int64 and np.array_equal(p.nnz, total)
                assert p.degrees.dtype == np.int32 and np.array_equal(p.degrees, rows)
                q = ss.tanimoto_profile(Fa, Fb, cuts=cuts, weighted=weighted, dtype=T)
                total, rows = P.profile_ref(S_x, c, weighted)
                assert not q.symmetric and q.shape == (300, 200)
                assert np.array_equal(q.nnz, total) and np.array_equal(q.degrees, rows)
        # the helpers on a device result: every row has itself; without itself the two all-zero rows keep each other
        p = ss.tanimoto_profile(Fa, cuts=[0.0, 0.5, 1.0, 1.5], dtype=T)
        assert p.coverage().tolist() == [1.0, 1.0, 1.0, 0.0]
        assert p.coverage(exclude_self=True)[2] == ((p.degrees[:, 2] - 1) >= 1).mean() > 0
        assert p.alpha_for_nnz(int(p.nnz[1])) == 0.5 and p.alpha_for_nnz(-1) is None
        assert p.fill()[0] == p.nnz[0] / 90000.0
    # device input: CUDA degrees, the same numbers
    ta, tb = (torch.from_numpy(F.view(np.int64)).cuda() for F in (Fa, Fb))
    for Fb_h, Fb_d in ((None, None), (Fb, tb)):
        h = ss.tanimoto_profile(Fa, Fb_h, cuts=fp_cuts(F32))
        d = ss.tanimoto_profile(ta, Fb_d, cuts=fp_cuts(F32))
        assert d.degrees.is_cuda and d.degrees.dtype == torch.int32 and isinstance(d.nnz, np.ndarray)
        assert np.array_equal(d.nnz, h.nnz) and np.array_equal(d.degrees.cpu().numpy(), h.degrees)
        assert d.coverage().tolist() == h.coverage().tolist()


# ----------------------------------------------------------------------------------------------- 2. weighted Jaccard
def jaccard_rows(n, d, seed):
    """Small non-negative integers with many zeros (so that exact similarities such as 1/2 and 1/3 occur), two all-zero
    rows (the all-zero pair: smax == 0, s = 1) and a duplicated row."""
    rng = np.random.default_rng(seed)
    X = rng.integers(0, 4, (n, d)).astype(np.float64) * (rng.random((n, d)) < 0.7)
    if n >= 9:
        X[1] = X[4] = 0
        X[5] = X[6]
    return X


def colmajor(X, T):
    return np.asfortranarray(X, dtype=T)


@pytest.mark.parametrize("d", [1, 5, 17])
def test_jaccard_profiles_are_the_producer(d):
    lib = ss.init(0)
    for na, nb in ((129, None), (300, None), (130, 257), (1, 200)):
        for T in (F32, F64):
            A = colmajor(jaccard_rows(na, d, seed=na + d), T)
            B = None if nb is None else colmajor(jaccard_rows(nb, d, seed=na + d + 1), T)
            head = (addr(A), na, na, addr(B), nb or 0, nb or 0, d)
            cuts = np.array([-np.inf, -1.0, 0.0, T(1) / T(3), T(1) / T(2), T(1) / T(2), 0.75, 1.0, 2.0, np.inf], T)
            total, rows = check_against_producer(lib, "jaccard", SUF[T], head, na, cuts, CT[T], "jaccard_profile")
            cols = nb or na
            if na >= 9 and cols >= 9:
                assert rows[1, 7] >= 2                      # the all-zero pair keeps s = 1
            assert total[0] == total[1] < na * cols         # weighted: the pairs with s = 0 never count
            p = ss.jaccard_profile(np.asarray(A), None if B is None else np.asarray(B), cuts=cuts, dtype=T)
            assert np.array_equal(p.nnz, total) and np.array_equal(p.degrees, rows) and p.shape == (na, cols)


# ----------------------------------------------------------------------------------------------- 3. inner products
@pytest.mark.parametrize("metric", R.METRICS)
@pytest.mark.parametrize("d", [3, 16, 33])
def test_dot_profiles_are_the_producer(d, metric):
    lib = ss.init(0)
    m = METRIC_CODE[metric]
    for na, nb in ((200, None), (300, None), (129, 300), (1, 129)):
        Xa = R.vectors(na, d, seed=na + d, signed=True, zero_rows=(0, 7) if na > 7 else ())
        Xb = None if nb is None else R.vectors(nb, d, seed=na + d + 1, signed=True, zero_rows=(2,))
        for T in (F32, F64):
            A = colmajor(Xa, T)
            B = None if Xb is None else colmajor(Xb, T)
            head = (addr(A), na, na, addr(B), nb or 0, nb or 0, d, m)
            cuts = np.array([-np.inf, -1.0, -0.25, 0.0, 0.0, 0.3, 0.6, np.nextafter(T(1), T(0)), 1.0, np.nextafter(T(1), T(2)),
                             np.inf], T)
            total, rows = check_against_producer(lib, "dot", SUF[T], head, na, cuts, CT[T], "dot_profile")
            if nb is None:
                # the symmetric diagonal is exactly 1: every row counts itself at the cut 1 but not just above it
                assert (rows[:, 8] >= 1).all() and total[10] == 0
                assert (rows[:, 8] - rows[:, 9] >= 1).all()
                assert rows[0, 8] == 2 and rows[7, 8] == 2          # the two all-zero rows: den == 0, s = 1
                assert rows[0, 3] == 2                              # and s = 0 against every other row: not weighted in
            p = ss.dot_profile(Xa, Xb, metric=metric, cuts=cuts, dtype=T)
            assert np.array_equal(p.nnz, total) and np.array_equal(p.degrees, rows)


# ----------------------------------------------------------------------------------------------- 4. 16-bit rows
def to_bits(X, storage):
    if storage == "bf16":
        return ss.to_bf16_bits(np.asarray(X, np.float64))
    return np.asarray(X, np.float64).astype(np.float16).view(np.uint16)


def strided(bits, ld, shift):
    """Row i at element shift + i * ld of a buffer that ends with the last row; NaN patterns everywhere else."""
    n, d = bits.shape
    buf = np.full(shift + (n - 1) * ld + d, 0x7FFF, np.uint16)
    for i in range(n):
        buf[shift + i * ld: shift + i * ld + d] = bits[i]
    return buf


@pytest.mark.parametrize("storage", ["bf16", "f16"])
@pytest.mark.parametrize("d", [4, 64, 72])
def test_h16_profiles_are_the_producer_whatever_the_layout(d, storage):
    import torch
    lib = ss.init(0)
    code = {"bf16": 0, "f16": 1}[storage]
    fn = lib.ss_similarity_dot_profile_h16
    cuts = np.array([-np.inf, -0.5, 0.0, 0.3, 0.3, 0.6, 1.0, np.nextafter(F32(1), F32(2)), np.inf], F32)
    na, nb = 200, 300
    ba = to_bits(R.vectors(na, d, seed=d, signed=True, zero_rows=(0, 7)), storage)
    bb = to_bits(R.vectors(nb, d, seed=d + 1, signed=True, zero_rows=(2,)), storage)
    ld_odd = d + 3                                             # ld % 8 != 0 for d in {4, 64, 72}
    assert ld_odd % 8 != 0
    dev = {}
    for name, bits in (("a", ba), ("b", bb)):
        dev[name, "aligned"] = (torch.from_numpy(bits.view(np.int16)).cuda(), 0, d)
        dev[name, "odd"] = (torch.from_numpy(strided(bits, ld_odd, 1).view(np.int16)).cuda(), 1, ld_odd)
    for metric in R.METRICS:
        m = METRIC_CODE[metric]
        for Fb in (None, bb):
            cols = na if Fb is None else nb
            head = (addr(ba), na, d, addr(Fb), 0 if Fb is None else nb, 0 if Fb is None else d, d, code, m)
            total, rows = check_against_producer(lib, "dot", "h16", head, na, cuts, C.c_float, "dot_h16_profile")
            if Fb is None:
                assert (rows[:, 6] - rows[:, 7] >= 1).all() and total[8] == 0 and rows[0, 6] == 2
            # device memory: an aligned block and the same rows at an odd element offset with ld % 8 != 0
            for la, lb in (("aligned", "aligned"), ("odd", "odd"), ("aligned", "odd")):
                ta, offa, lda = dev["a", la]
                tb, offb, ldb = dev["b", lb]
                assert ta.data_ptr() % 16 == 0
                t = torch.full((len(cuts),), SENT, dtype=torch.int64, device="cuda")
                r = torch.full((na, len(cuts)), SENT, dtype=torch.int32, device="cuda")
                pb = None if Fb is None else tb.data_ptr() + 2 * offb
                rc = fn(ta.data_ptr() + 2 * offa, na, lda, pb, 0 if Fb is None else nb, 0 if Fb is None else ldb, d, code, m,
                        cuts.ctypes.data, len(cuts), 1, t.data_ptr(), r.data_ptr(), 1)
                assert rc == 0, lib.ss_last_error()
                assert np.array_equal(t.cpu().numpy(), total) and np.array_equal(r.cpu().numpy(), rows), (la, lb, metric)
        p = ss.dot_profile(ba, bb, metric=metric, cuts=cuts, storage=storage)
        assert ss.path_last() == ["dot_h16_profile"] and p.shape == (na, nb)
        assert np.array_equal(p.nnz, total) and np.array_equal(p.degrees, rows)
    # a 16-bit CUDA tensor selects the route by its dtype
    tdt = torch.bfloat16 if storage == "bf16" else torch.float16
    pt = ss.dot_profile(dev["a", "aligned"][0].view(tdt), cuts=cuts)
    assert ss.path_last() == ["dot_h16_profile"] and pt.degrees.is_cuda
    ph = ss.dot_profile(ba, cuts=cuts, storage=storage)
    assert np.array_equal(pt.nnz, ph.nnz) and np.array_equal(pt.degrees.cpu().numpy(), ph.degrees)


# ----------------------------------------------------------------------------------------------- 5. memory kinds, NULL rows
def _operands():
    """One operand set per entry point: (kind, suffix) -> ([A, B] host arrays in the library's layout,
    head(pa, pb) -> the arguments before the cuts (pb None: symmetric), T)."""
    na, nb, d = 200, 130, 9
    F, G = fp_rows(na, 3, seed=5), fp_rows(nb, 3, seed=6)
    X, Y = R.vectors(na, d, seed=7, signed=True, zero_rows=(3,)), R.vectors(nb, d, seed=8, signed=True)
    sets = {}
    for T in (F32, F64):
        sets["tanimoto", SUF[T]] = ([F, G], lambda a, b: (a, na, b, nb if b else 0, 3), T)
        sets["jaccard", SUF[T]] = ([colmajor(np.abs(X), T), colmajor(np.abs(Y), T)],
                                   lambda a, b: (a, na, na, b, nb if b else 0, nb if b else 0, d), T)
        sets["dot", SUF[T]] = ([colmajor(X, T), colmajor(Y, T)],
                               lambda a, b: (a, na, na, b, nb if b else 0, nb if b else 0, d, 1), T)
    sets["dot", "h16"] = ([to_bits(X, "bf16"), to_bits(Y, "bf16")],
                          lambda a, b: (a, na, d, b, nb if b else 0, d if b else 0, d, 0, 2), F32)
    return sets, na, nb


def dev_copy(a):
    """The array's bytes, in memory order, on the device."""
    import torch
    return torch.from_numpy(np.frombuffer(a.tobytes(order="A"), np.uint8).copy()).cuda()


def test_host_and_device_memory_null_rows_and_repeatability():
    import torch
    lib = ss.init(0)
    sets, na, nb = _operands()
    for (kind, suf), (arrays, head, T) in sets.items():
        cuts = np.array([-1.0, 0.0, 0.2, 0.5, 0.5, 1.0], T)
        fn = getattr(lib, f"ss_similarity_{kind}_profile_{suf}")
        tens = [dev_copy(a) for a in arrays]
        for cross in (False, True):
            hh = head(addr(arrays[0]), addr(arrays[1]) if cross else None)
            total, rows = profile(lib, kind, suf, hh, na, cuts, 1)
            assert total[1] > 0 and (total[:-1] >= total[1:]).all()
            # rows == NULL: the totals alone
            t2, r2 = profile(lib, kind, suf, hh, na, cuts, 1, want_rows=False)
            assert np.array_equal(t2, total) and (r2 == SENT).all()
            # twice the same
            t3, r3 = profile(lib, kind, suf, hh, na, cuts, 1)
            assert np.array_equal(t3, total) and np.array_equal(r3, rows)
            # device memory (cuts stay on the host)
            dh = head(tens[0].data_ptr(), tens[1].data_ptr() if cross else None)
            for want_rows in (True, False):
                t = torch.full((len(cuts),), SENT, dtype=torch.int64, device="cuda")
                r = torch.full((na, len(cuts)), SENT, dtype=torch.int32, device="cuda")
                rc = fn(*dh, cuts.ctypes.data, len(cuts), 1, t.data_ptr(), r.data_ptr() if want_rows else None, 1)
                assert rc == 0, lib.ss_last_error()
                assert np.array_equal(t.cpu().numpy(), total), (kind, suf, cross)
                assert np.array_equal(r.cpu().numpy(), rows) if want_rows else (r.cpu().numpy() == SENT).all()


# ----------------------------------------------------------------------------------------------- 6. refusals, empty cases
def test_every_refusal_leaves_the_outputs_untouched():
    import torch
    lib = ss.init(0)
    sets, na, nb = _operands()
    nan = float("nan")
    bad_cuts = ([], list(np.linspace(0, 1, 33)), [0.1, nan, 0.5], [nan], [0.5, 0.4], [0.0, 1.0, 0.999])
    for (kind, suf), (arrays, head, T) in sets.items():
        fn = getattr(lib, f"ss_similarity_{kind}_profile_{suf}")
        hh = head(addr(arrays[0]), addr(arrays[1]))
        refused = [(hh, np.asarray(c, T)) for c in bad_cuts]
        good = np.array([0.1, 0.5], T)
        if kind != "tanimoto":                                   # a NaN feature where the producer refuses one
            for side in (0, 1):
                poisoned = [a.copy() for a in arrays]
                if suf == "h16":
                    poisoned[side][-1, -1] = 0x7FC0
                else:
                    poisoned[side][-1, -1] = nan
                h2 = head(addr(poisoned[0]), addr(poisoned[1]))
                total, rows = profile(lib, kind, suf, h2, na, good, 1, expect=-1)
                assert (total == SENT).all() and (rows == SENT).all() and "NaN" in lib.ss_last_error().decode()
        if kind == "dot":
            mi = 7 if suf != "h16" else 8
            for metric in (-1, 3):
                refused.append((tuple(metric if i == mi else v for i, v in enumerate(hh)), good))
            if suf == "h16":
                for storage in (-1, 2):
                    refused.append((tuple(storage if i == 7 else v for i, v in enumerate(hh)), good))
        for h2, cuts in refused:
            total, rows = profile(lib, kind, suf, h2, na, cuts, 1, expect=-1)
            assert (total == SENT).all() and (rows == SENT).all(), (kind, suf, cuts)
        # device memory: sentinels stay on the device too
        t = torch.full((2,), SENT, dtype=torch.int64, device="cuda")
        r = torch.full((na, 2), SENT, dtype=torch.int32, device="cuda")
        tens = [dev_copy(a) for a in arrays]
        d1 = head(tens[0].data_ptr(), tens[1].data_ptr())
        c = np.array([0.5, 0.4], T)
        assert fn(*d1, c.ctypes.data, 2, 1, t.data_ptr(), r.data_ptr(), 1) == -1
        if kind != "tanimoto":
            bad = arrays[1].copy()
            bad[0, 0] = 0x7FC0 if suf == "h16" else nan
            tb = dev_copy(bad)
            assert fn(*head(tens[0].data_ptr(), tb.data_ptr()), good.ctypes.data, 2, 1, t.data_ptr(), r.data_ptr(), 1) == -1
        assert (t.cpu().numpy() == SENT).all() and (r.cpu().numpy() == SENT).all()
        # total == NULL and an unknown mem are refused as everywhere
        assert fn(*hh, good.ctypes.data, 2, 1, None, None, 0) == -1
        assert fn(*hh, good.ctypes.data, 2, 1, None, None, 5) == -1
    # the python mirror passes a device refusal on
    X = np.ones((4, 3))
    X[2, 1] = nan
    for call in (lambda: ss.jaccard_profile(X, cuts=[0.5]), lambda: ss.dot_profile(X, cuts=[0.5]),
                 lambda: ss.dot_profile(X, cuts=[0.5], storage="bf16")):
        with pytest.raises(ss.SimSpreadError) as e:
            call()
        assert e.value.code == -1


def test_empty_cases():
    lib = ss.init(0)
    dummy = np.zeros(16, np.uint64)
    for T in (F32, F64):
        cuts = np.array([-1.0, 0.5, 1.0, 1.5], T)
        F = fp_rows(130, 2, seed=9)
        # na == 0: total is all zero
        total, rows = profile(lib, "tanimoto", SUF[T], (addr(dummy), 0, addr(F), 130, 2), 0, cuts, 1)
        assert total.tolist() == [0, 0, 0, 0]
        total, rows = profile(lib, "tanimoto", SUF[T], (addr(dummy), 0, None, 0, 2), 0, cuts, 1)
        assert total.tolist() == [0, 0, 0, 0]
        # nb == 0: everything is zero
        total, rows = profile(lib, "tanimoto", SUF[T], (addr(F), 130, addr(dummy), 0, 2), 130, cuts, 1)
        assert total.tolist() == [0, 0, 0, 0] and not rows.any()
        X = colmajor(R.vectors(130, 4, seed=1, signed=False), T)
        for kind, extra in (("jaccard", ()), ("dot", (0,))):
            total, rows = profile(lib, kind, SUF[T], (addr(X), 130, 130, addr(dummy), 0, 1, 4) + extra, 130, cuts, 1)
            assert total.tolist() == [0, 0, 0, 0] and not rows.any()
            # d == 0: s = 1 everywhere, by the producers' own rule
            total, rows = profile(lib, kind, SUF[T], (addr(dummy), 130, 130, None, 0, 0, 0) + extra, 130, cuts, 1)
            assert total.tolist() == [130 * 130] * 3 + [0] and (rows[:, :3] == 130).all() and not rows[:, 3].any()
            total, rows = profile(lib, kind, SUF[T], (addr(dummy), 130, 130, addr(dummy), 3, 3, 0) + extra, 130, cuts, 0)
            assert total.tolist() == [390] * 3 + [0] and (rows[:, :3] == 3).all()
    cuts = np.array([-1.0, 0.5, 1.0, 1.5], F32)
    for storage in (0, 1):
        total, rows = profile(lib, "dot", "h16", (addr(dummy), 130, 1, None, 0, 0, 0, storage, 0), 130, cuts, 1)
        assert total.tolist() == [130 * 130] * 3 + [0] and (rows[:, :3] == 130).all()
        total, rows = profile(lib, "dot", "h16", (addr(dummy), 0, 4, addr(dummy), 5, 4, 4, storage, 0), 0, cuts, 1)
        assert total.tolist() == [0, 0, 0, 0]
