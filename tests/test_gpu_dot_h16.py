"""The 16-bit route of the inner-product producer on the device (include/simspread_hip_half.h, csrc/dot_tile_h16.hpp):
bf16 / fp16 rows, row-major -> thresholded cosine / Tanimoto / Dice CSR on v_mfma_f32_32x32x16_{bf16,f16} -> graph.

"Widened inputs" always means the fp32 values of the exact 16-bit patterns the device received.  Inputs whose sums are
exact in any order are checked bit for bit, against the exact host rule and against the fp32 producer on the widened
inputs; that is the test of the operand lane map, of the k pairing of the two sides and of rows against columns (the data
are asymmetric).  General inputs are checked against the fp64 rule on the widened inputs inside a band.

band16(d) = 8 (d + 4) eps_fp32 is derived, not measured.  Every product of two 16-bit values is exact in fp32, so g
carries only the error of d - 1 fp32 additions.  dot_ref.band = 4 (d + 4) eps allows half an ulp per accumulated term
(round to nearest; see dot_ref.py for the way through the three formulas and the epilogue's roundings).  How the 16-bit
matrix instruction rounds inside its accumulation is not documented; if it aligns and truncates instead of rounding, a
term costs up to one full ulp instead of half of one.  One ulp per term is twice the fp32 band: 8 (d + 4) eps.  The cap
that at most 1 % of the pairs may lie inside the band stays; on the host these inputs, rounded to bf16 and fp16, give at
most 0.66 % over all metrics and alphas (at (257, 512))."""
import ctypes as C

import numpy as np
import pytest
import scipy.sparse as sp

import simspread_jl_amd as ss

import dot_ref as R
from dot_ref import assert_csr_equal, ref_cut, to_csr
from test_gpu_dot_csr import check_structure

pytestmark = pytest.mark.gpu

STORAGES = ("bf16", "f16")
CODE = {"bf16": 0, "f16": 1}
F32 = np.float32
NAN_PATTERN = 0x7FFF           # a NaN in both formats
METRIC_CODE = {"cosine": 0, "tanimoto": 1, "dice": 2}


def band16(d):
    return 8.0 * (d + 4) * float(np.finfo(F32).eps)


def to_bits(X, storage):
    """The patterns the device receives: X rounded to the storage, nearest even."""
    if storage == "bf16":
        return ss.to_bf16_bits(np.asarray(X, np.float64))
    with np.errstate(over="ignore"):
        return np.asarray(X, np.float64).astype(np.float16).view(np.uint16)


def widen(bits, storage):
    bits = np.ascontiguousarray(bits, np.uint16)
    if storage == "bf16":
        return (bits.astype(np.uint32) << 16).view(F32)
    return bits.view(np.float16).astype(F32)


def int_rows(n, d, seed):
    """dot_ref.integer_rows; below its four leading columns (d < 4) plain integers in -3 .. 3 with a zero row and
    duplicates."""
    if d >= 4:
        return R.integer_rows(n, d, seed)
    X = np.random.default_rng(seed).integers(-3, 4, (n, d)).astype(np.float64)
    X[7] = 0
    X[n // 2] = X[n // 3]
    X[n - 1] = X[3]
    return X


def check_band16(M, s64, alpha, weighted, d):
    """check_band of test_gpu_dot_csr.py with band16: outside the band the pattern is exact, every stored value is within
    the band of s64, at most 1 % of the pairs are inside the band.  Returns the largest |s_device - s64|."""
    band = band16(d)
    a = float(F32(alpha))
    rows = np.repeat(np.arange(M.shape[0]), np.diff(M.indptr))
    kept = np.zeros(M.shape, bool)
    kept[rows, M.indices] = True
    with np.errstate(invalid="ignore"):
        inb = np.abs(s64 - a) <= band
        want = (s64 >= a) & ((s64 != 0) if weighted else True)
    assert inb.mean() <= 0.01, inb.mean()
    assert np.array_equal(kept[~inb], want[~inb])
    if not weighted:
        assert (M.data == 1).all()
        return 0.0
    err = float(np.abs(M.data.astype(np.float64) - s64[rows, M.indices]).max(initial=0.0))
    assert err <= band, (err, band)
    return err


# ----------------------------------------------------------------------------------------------- 1. exact, bit for bit
@pytest.mark.parametrize("n,d", [(129, 1), (131, 9), (128, 16), (129, 17), (130, 33), (200, 65), (300, 300)])
def test_exact_inputs_are_bitwise_the_rule_and_the_fp32_route(n, d):
    ss.init(0)
    X = int_rows(n, d, seed=n + d)
    Z = int_rows(n // 2 + 3, d, seed=n + d + 1)
    for storage in STORAGES:
        bx, bz = to_bits(X, storage), to_bits(Z, storage)
        assert np.array_equal(widen(bx, storage), X) and np.array_equal(widen(bz, storage), Z)      # exact in the format
        for metric in R.METRICS:
            e_sym = R.ref_exact(X, X, metric, F32, sym=True)
            e_x = R.ref_exact(X, Z, metric, F32)
            for alpha in R.ALPHAS:
                for weighted in (True, False):
                    S = ss.dot_csr(bx, metric=metric, alpha=alpha, weighted=weighted, storage=storage)
                    assert ss.path_last() == ["dot_h16_sym"]
                    assert_csr_equal(S, ref_cut(e_sym, alpha, weighted, F32))
                    assert_csr_equal(S, ss.dot_csr(X.astype(F32), metric=metric, alpha=alpha, weighted=weighted))
                    Xc = ss.dot_csr(bx, bz, metric=metric, alpha=alpha, weighted=weighted, storage=storage)
                    assert ss.path_last() == ["dot_h16_cross"]
                    assert_csr_equal(Xc, ref_cut(e_x, alpha, weighted, F32))
                    assert_csr_equal(Xc, ss.dot_csr(X.astype(F32), Z.astype(F32), metric=metric, alpha=alpha,
                                                    weighted=weighted))
            if d >= 4:      # the pairs whose similarity is exactly 0.5 are there at alpha = 0.5
                i, j = {"cosine": (10, 11), "tanimoto": (12, 13), "dice": (12, 14)}[metric]
                assert e_sym[i, j] == F32(0.5) and e_x[i, j] == F32(0.5)
                S = ss.dot_csr(bx, metric=metric, alpha=0.5, storage=storage).toarray()
                assert S[i, j] == F32(0.5) and S[j, i] == F32(0.5)
                assert ss.dot_csr(bx, bz, metric=metric, alpha=0.5, storage=storage).toarray()[i, j] == F32(0.5)


# ----------------------------------------------------------------------------------------------- 2. general inputs
BAND_CASES = [(1, 1), (63, 4), (127, 15), (128, 16), (129, 17), (130, 33), (200, 65), (1000, 64), (300, 300), (4097, 16),
              (257, 512)]
WORST = {}      # metric -> largest |s - s64| / band16 seen, printed per case (the table of DESIGN 4.19)


def combos16(n):
    """combos of test_gpu_dot_csr.py with the storage in the place of the dtype."""
    full = [(st, signed, m) for st in STORAGES for signed in (False, True) for m in R.METRICS]
    if n <= 1000:
        return full
    return [("bf16", False, "cosine"), ("f16", True, "tanimoto"), ("bf16", True, "dice"), ("f16", False, "cosine")]


@pytest.mark.parametrize("n,d", BAND_CASES)
def test_general_inputs_stay_in_the_band_of_the_fp64_rule_on_the_widened_inputs(n, d):
    ss.init(0)
    nb = max(1, n // 2 + 3)
    inputs, sums = {}, {}
    worst = {m: 0.0 for m in R.METRICS}
    for c, (storage, signed, metric) in enumerate(combos16(n)):
        if signed not in inputs:
            inputs[signed] = R.case_inputs(n, d, signed)
        if (storage, signed) not in sums:
            bf, bg = (to_bits(A, storage) for A in inputs[signed])
            wf, wg = widen(bf, storage), widen(bg, storage)
            sums[(storage, signed)] = (bf, bg, R.sums64(wf, wf, F32), R.sums64(wf, wg, F32))
        bf, bg, sm_sym, sm_x = sums[(storage, signed)]
        s_sym = R.rule(*sm_sym, metric, np.float64, sym=True)
        s_x = R.rule(*sm_x, metric, np.float64)
        if n <= 300:
            alphas = R.ALPHAS
        elif n <= 1000:
            alphas = (R.ALPHAS[c % 4], R.ALPHAS[(c + 2) % 4])
        else:
            alphas = (R.ALPHAS[c % 4],)
        for alpha in alphas:
            W = ss.dot_csr(bf, metric=metric, alpha=alpha, weighted=True, storage=storage)
            assert W.data.dtype == F32 and W.shape == (n, n)
            check_structure(W, True, alpha)
            worst[metric] = max(worst[metric], check_band16(W, s_sym, alpha, True, d) / band16(d))
            X = ss.dot_csr(bf, bg, metric=metric, alpha=alpha, weighted=True, storage=storage)
            assert X.shape == (n, nb)
            check_structure(X, False, alpha)
            worst[metric] = max(worst[metric], check_band16(X, s_x, alpha, True, d) / band16(d))
            for Fb, Wt in ((None, W), (bg, X)):
                U = ss.dot_csr(bf, Fb, metric=metric, alpha=alpha, weighted=False, storage=storage)
                assert (U.data == 1).all()
                assert np.array_equal(U.indptr, Wt.indptr) and np.array_equal(U.indices, Wt.indices)
    for m in R.METRICS:
        WORST[m] = max(WORST.get(m, 0.0), worst[m])
    print(f"  n={n} d={d}: max |s - s64| / band16 " + "  ".join(f"{m} {worst[m]:.4f}" for m in R.METRICS)
          + "   so far " + "  ".join(f"{m} {WORST[m]:.4f}" for m in R.METRICS))


# ----------------------------------------------------------------------------------------------- 3. the layout contract
def _strided(bits, ld, shift):
    """A buffer that starts `shift` elements before row 0, holds row i at shift + i * ld and ENDS with the last element of
    the last row; everything that is not a feature is a NaN pattern."""
    n, d = bits.shape
    buf = np.full(shift + (n - 1) * ld + d, NAN_PATTERN, np.uint16)
    for i in range(n):
        buf[shift + i * ld: shift + i * ld + d] = bits[i]
    return buf


def _raw_csr(lib, mem, a, na, lda, b, nb, ldb, d, storage, metric, alpha):
    """ss_similarity_dot_csr_h16 through ctypes: a, b are (buffer, element offset) of numpy (mem 0) or CUDA int16 tensors
    (mem 1); b None: symmetric."""
    import torch
    fn = lib.ss_similarity_dot_csr_h16

    def address(x):
        if x is None:
            return None
        buf, off = x
        return (buf.data_ptr() if mem else buf.ctypes.data) + 2 * off
    pa, pb = address(a), address(b)
    head = (pa, na, lda, pb, nb if b is not None else 0, ldb if b is not None else 0, d, CODE[storage],
            METRIC_CODE[metric], C.c_float(alpha), 1)
    nnz = C.c_int64(-1)
    cols = nb if b is not None else na
    if mem:
        ptr = torch.zeros(na + 1, dtype=torch.int64, device="cuda")
        assert fn(*head, ptr.data_ptr(), None, None, 0, C.byref(nnz), 1) == 0, lib.ss_last_error()
        idx = torch.zeros(max(nnz.value, 1), dtype=torch.int32, device="cuda")
        val = torch.zeros(max(nnz.value, 1), dtype=torch.float32, device="cuda")
        assert fn(*head, ptr.data_ptr(), idx.data_ptr(), val.data_ptr(), nnz.value, C.byref(nnz), 1) == 0
        torch.cuda.synchronize()
        return to_csr(ptr, idx[:nnz.value], val[:nnz.value], (na, cols))
    ptr = np.zeros(na + 1, np.int64)
    assert fn(*head, ptr.ctypes.data, None, None, 0, C.byref(nnz), 0) == 0, lib.ss_last_error()
    idx = np.zeros(max(nnz.value, 1), np.int32)
    val = np.zeros(max(nnz.value, 1), F32)
    assert fn(*head, ptr.ctypes.data, idx.ctypes.data, val.ctypes.data, nnz.value, C.byref(nnz), 0) == 0
    return sp.csr_matrix((val[:nnz.value], idx[:nnz.value], ptr), shape=(na, cols))


@pytest.mark.parametrize("storage", STORAGES)
def test_layout_contract_any_base_any_ld_nan_padding_and_no_read_past_the_last_row(storage):
    import torch
    lib = ss.init(0)
    n, d, alpha = 300, 65, 0.5
    F, G = R.case_inputs(n, d, signed=True)
    bf, bg = to_bits(F, storage), to_bits(G, storage)
    nb = bg.shape[0]
    for metric in ("cosine", "tanimoto"):
        want_sym = ss.dot_csr(bf, metric=metric, alpha=alpha, storage=storage)          # contiguous, aligned copies
        want_x = ss.dot_csr(bf, bg, metric=metric, alpha=alpha, storage=storage)
        assert want_sym.nnz > n and want_x.nnz > 0
        for ld, shift in ((d, 0), (d + 3, 1), (72, 0), (72, 8), (80, 4)):
            ha, hb = _strided(bf, ld, shift), _strided(bg, ld, shift)
            for mem in (1, 0):
                if mem:
                    a, b = (torch.from_numpy(x.view(np.int16)).cuda() for x in (ha, hb))
                    assert a.data_ptr() % 16 == 0 and a.numel() == shift + (n - 1) * ld + d
                else:
                    a, b = ha, hb
                assert_csr_equal(_raw_csr(lib, mem, (a, shift), n, ld, None, 0, 0, d, storage, metric, alpha), want_sym)
                assert_csr_equal(_raw_csr(lib, mem, (a, shift), n, ld, (b, shift), nb, ld, d, storage, metric, alpha),
                                 want_x)
        # an aligned side against an unaligned one
        a = torch.from_numpy(_strided(bf, 72, 0).view(np.int16)).cuda()
        b = torch.from_numpy(_strided(bg, d + 3, 1).view(np.int16)).cuda()
        assert_csr_equal(_raw_csr(lib, 1, (a, 0), n, 72, (b, 1), nb, d + 3, d, storage, metric, alpha), want_x)


# ----------------------------------------------------------------------------------------------- 4. refusals
def test_refusals_come_before_anything_is_written_and_the_size_protocol():
    import torch
    lib = ss.init(0)
    fn = lib.ss_similarity_dot_csr_h16
    n, d = 300, 20
    X = R.vectors(n, d, seed=5, signed=True)
    ptr = np.full(n + 1, -7, np.int64)
    idx = np.full(10, -7, np.int32)
    val = np.full(10, -7, F32)
    nnz = C.c_int64(-7)

    def call(a, b, storage, metric, alpha, lda=d, out_idx=None, mem=0, p=None):
        return fn(a, n, lda, b, n if b else 0, d if b else 0, d, storage, metric, C.c_float(alpha), 1,
                  ptr.ctypes.data if p is None else p, out_idx, None if out_idx is None else val.ctypes.data, 10,
                  C.byref(nnz), mem)
    for storage, nanbits in (("bf16", 0x7FC0), ("f16", 0x7E00)):
        good = to_bits(X, storage)
        bad = good.copy()
        bad[n - 1, d - 1] = nanbits                       # the last element
        neg = good.copy()
        neg[0, 0] = nanbits | 0x8001                      # a negative NaN with a payload
        code = CODE[storage]
        cases = ((bad, None, code, 0, 0.5, d, "NaN"), (good, bad, code, 1, 0.5, d, "NaN"), (neg, None, code, 2, 0.5, d, "NaN"),
                 (good, None, code, 2, float("nan"), d, "NaN"), (good, None, code, 7, 0.5, d, "metric"),
                 (good, None, code, -1, 0.5, d, "metric"), (good, None, 2, 0, 0.5, d, "storage"),
                 (good, None, -1, 0, 0.5, d, "storage"), (good, None, code, 0, 0.5, d - 1, "leading"))
        for a, b, st, metric, alpha, lda, word in cases:
            for out_idx in (None, idx.ctypes.data):
                rc = call(a.ctypes.data, None if b is None else b.ctypes.data, st, metric, alpha, lda, out_idx)
                assert rc == -1, (rc, word)
                assert word in lib.ss_last_error().decode(), (word, lib.ss_last_error())
        assert nnz.value == -7 and (ptr == -7).all() and (idx == -7).all() and (val == -7).all()
        # device memory
        bt = torch.from_numpy(bad.view(np.int16)).cuda()
        pt = torch.full((n + 1,), -7, dtype=torch.int64, device="cuda")
        assert call(bt.data_ptr(), None, code, 0, 0.5, mem=1, p=pt.data_ptr()) == -1
        assert nnz.value == -7 and (pt.cpu().numpy() == -7).all()
        # the python mirror and the graph constructors
        with pytest.raises(ss.SimSpreadError) as e:
            ss.dot_csr(bad, alpha=0.5, storage=storage)
        assert e.value.code == -1
        with pytest.raises(ss.SimSpreadError) as e:
            ss.DeviceGraph.from_vectors(good[:7], bad, np.eye(n, 4), alpha=0.5, storage=storage)
        assert e.value.code == -1
        h = C.c_void_p()
        yp = np.zeros(n + 1, np.int64)
        assert lib.ss_graph_create_vectors_h16(0, n, 4, d, code, 7, None, d, good.ctypes.data, d, yp.ctypes.data, None, None,
                                               0, C.c_float(0.5), 1, 0, C.byref(h)) == -1
        assert h.value is None
        # the size protocol
        want = ss.dot_csr(good, alpha=0.3, storage=storage)
        p2 = np.zeros(n + 1, np.int64)
        n1, n2 = C.c_int64(-1), C.c_int64(-1)
        head = (good.ctypes.data, n, d, None, 0, 0, d, code, 0, C.c_float(0.3), 1)
        assert fn(*head, p2.ctypes.data, None, None, 0, C.byref(n1), 0) == 0
        assert n1.value == want.nnz > n and np.array_equal(p2, want.indptr)
        i2 = np.full(n1.value, -5, np.int32)
        v2 = np.full(n1.value, -5, F32)
        rc = fn(*head, p2.ctypes.data, i2.ctypes.data, v2.ctypes.data, n1.value - 1, C.byref(n2), 0)     # capacity too small
        assert rc == -1 and n2.value == n1.value and (i2 == -5).all() and (v2 == -5).all()
        assert fn(*head, p2.ctypes.data, i2.ctypes.data, None, n1.value, C.byref(n2), 0) == 0            # the pattern only
        assert np.array_equal(i2, want.indices) and (v2 == -5).all()
        assert fn(*head, p2.ctypes.data, i2.ctypes.data, v2.ctypes.data, n1.value, C.byref(n2), 0) == 0
        assert_csr_equal(sp.csr_matrix((v2, i2, p2), shape=(n, n)), want)
        assert fn(None, n, d, None, 0, 0, d, code, 0, C.c_float(0.3), 1, p2.ctypes.data, None, None, 0, C.byref(n2), 0) == -1
        assert fn(good.ctypes.data, 1 << 31, d, None, 0, 0, d, code, 0, C.c_float(0.3), 1, p2.ctypes.data, None, None, 0,
                  C.byref(n2), 0) == -5


# ----------------------------------------------------------------------------------------------- 5. edges of the rule
@pytest.mark.parametrize("storage", STORAGES)
def test_edge_cases_of_the_rule(storage):
    ss.init(0)
    X = np.zeros((4, 6))
    X[2, :3] = [1.0, -2.0, 0.5]
    X[3, 3:] = [1.0, 1.0, 4.0]                   # rows 2 and 3 are orthogonal: s = 0
    for metric in R.METRICS:
        for alpha in (0.0, -0.5):
            assert (ss.dot_csr(X, metric=metric, alpha=alpha, weighted=False, storage=storage).toarray() == 1).all()
        W = ss.dot_csr(X, metric=metric, alpha=-0.5, weighted=True, storage=storage)
        Wd = W.toarray()
        assert W.nnz == 6 and (W.data == 1).all()
        assert Wd[0, 1] == 1 and Wd[1, 0] == 1 and Wd[0, 0] == 1          # zero with zero: 1
        assert Wd[0, 2] == 0 and Wd[2, 0] == 0 and Wd[1, 3] == 0          # zero with non-zero: 0
        assert Wd[2, 3] == 0 and Wd[2, 2] == 1 and Wd[3, 3] == 1          # orthogonal: 0
        E = np.zeros((5, 0))                                              # d = 0: every pair has s = 1
        assert (ss.dot_csr(E, metric=metric, alpha=1.0, storage=storage).toarray() == 1).all()
        assert (ss.dot_csr(E, np.zeros((3, 0)), metric=metric, alpha=0.5, storage=storage).toarray() == 1).all()
    N = np.array([[3.0, 0.0, 4.0], [-3.0, 0.0, -4.0]])                    # antiparallel, sqrt(25) * sqrt(25) is exact
    got = ss.dot_csr(N, metric="cosine", alpha=-1.0, storage=storage).toarray()
    assert got[0, 1] == -1 and got[1, 0] == -1
    # an infinite feature: its NaN similarities are dropped, every other pair is what it is without that row
    Finf = np.array([[np.inf, 1.0], [1.0, 0.0], [0.0, 1.0], [2.0, 2.0]])
    for metric in R.METRICS:
        got = ss.dot_csr(Finf, metric=metric, alpha=-2.0, weighted=False, storage=storage)
        assert not np.isnan(got.data).any() and got[0, 0] == 1 and got[1, 3] == 1
        assert got[0, 2] == 0                     # inf * 0 in g: s is NaN, dropped at any alpha
        rest = ss.dot_csr(Finf[1:], metric=metric, alpha=-2.0, weighted=True, storage=storage)
        full = ss.dot_csr(Finf, metric=metric, alpha=-2.0, weighted=True, storage=storage)
        assert_csr_equal(full[1:, 1:], rest)


# ----------------------------------------------------------------------------------------------- 6. graph and queries
def _labels(ns, nt, seed):
    rng = np.random.default_rng(seed)
    Y = sp.random(ns, nt, density=4.0 / nt, random_state=rng, format="csr")
    Y.data[:] = 1.0
    return Y


def _same_bits(a, b):
    return a.shape == b.shape and np.array_equal(a.view(np.uint8), b.view(np.uint8))


@pytest.mark.parametrize("metric,alpha", [("cosine", 0.6), ("tanimoto", 0.5)])
@pytest.mark.parametrize("storage", STORAGES)
def test_graph_and_queries_from_16_bit_vectors(storage, metric, alpha):
    import torch
    ss.init(0)
    ns, nq, nt, d = 600, 150, 40, 48
    Fs = to_bits(R.vectors(ns, d, seed=11, signed=True, zero_rows=(4, 17)), storage)
    Fq = to_bits(R.vectors(nq, d, seed=12, signed=True, zero_rows=(0,)), storage)
    Y = _labels(ns, nt, 13)
    kw = dict(alpha=alpha, metric=metric, weighted=True, storage=storage)
    Xs = ss.dot_csr(Fs, **kw)
    Xq = ss.dot_csr(Fq, Fs, **kw)
    assert 0.001 < Xs.nnz / ns / ns < 0.5 and Xq.nnz > 0

    g = ss.DeviceGraph.from_vectors(Fq, Fs, Y, **kw)
    assert ss.path_last() == ["dot_h16_sym", "dot_h16_cross"]
    assert g.dtype == np.float32
    assert (g.nq, g.ns, g.nf, g.nt, g.nnz_xq, g.nnz_xs) == (nq, ns, ns, nt, Xq.nnz, Xs.nnz)
    r = ss.DeviceGraph.from_sparse(Xq, Xs, Y, dtype=F32)
    for rows in ("query", "source"):
        assert _same_bits(g.predict(rows), r.predict(rows)), rows
    g3 = ss.DeviceGraph.from_vectors(None, Fs, Y, **kw)
    assert ss.path_last() == ["dot_h16_sym"]
    r3 = ss.DeviceGraph.from_sparse(None, Xs, Y, dtype=F32)
    assert _same_bits(g3.predict_loo(clean=True), r3.predict_loo(clean=True))

    # a query set on the graph built without queries, and on a graph another constructor built
    for graph in (g3, r3):
        q = ss.DeviceQueries.from_vectors(graph, Fq, Fs, **kw)
        assert ss.path_last() == ["dot_h16_cross"]
        assert (q.nq, q.nnz) == (nq, Xq.nnz)
        assert _same_bits(graph.predict(queries=q), g.predict("query"))
        q.close()

    # recut equals a fresh build at the higher alpha
    hi = dict(kw, alpha=alpha + 0.2)
    child, fresh = g.recut(alpha + 0.2), ss.DeviceGraph.from_vectors(Fq, Fs, Y, **hi)
    assert 0 < fresh.nnz_xs < g.nnz_xs
    assert (child.nnz_xq, child.nnz_xs) == (fresh.nnz_xq, fresh.nnz_xs)
    for rows in ("query", "source"):
        assert _same_bits(child.predict(rows), fresh.predict(rows)), rows

    # device tensors of the storage's dtype: the same graph, the same query set
    tdt = torch.bfloat16 if storage == "bf16" else torch.float16
    ts, tq = (torch.from_numpy(b.view(np.int16)).cuda().view(tdt) for b in (Fs, Fq))
    Yd = (torch.from_numpy(Y.indptr.astype(np.int64)).cuda(), torch.from_numpy(Y.indices.astype(np.int32)).cuda(), None, nt)
    gd = ss.DeviceGraph.from_vectors(tq, ts, Yd, **kw)
    assert (gd.nnz_xq, gd.nnz_xs) == (Xq.nnz, Xs.nnz)
    assert _same_bits(gd.predict("query"), g.predict("query"))
    qd = ss.DeviceQueries.from_vectors(g3, tq, ts, alpha=alpha, metric=metric)          # storage by the dtype
    assert _same_bits(g3.predict(queries=qd), g.predict("query"))
    with pytest.raises(TypeError):
        ss.DeviceGraph.from_vectors(tq, ts, Yd, **dict(kw, storage="f16" if storage == "bf16" else "bf16"))

    # exact inputs: the whole graph is bitwise the fp32 graph
    Is, Iq = R.integer_rows(ns, d, seed=31), R.integer_rows(nq, d, seed=32)
    gi = ss.DeviceGraph.from_vectors(to_bits(Iq, storage), to_bits(Is, storage), Y, **kw)
    gf = ss.DeviceGraph.from_vectors(Iq, Is, Y, alpha=alpha, metric=metric, weighted=True, dtype=F32)
    assert ss.path_last() == ["dot_csr_sym", "dot_csr_cross"]
    assert (gi.nnz_xq, gi.nnz_xs) == (gf.nnz_xq, gf.nnz_xs) and gi.nnz_xs > ns
    for a, b in zip(gi.degrees(), gf.degrees()):
        assert np.array_equal(a, b)
    for rows in ("query", "source"):
        assert _same_bits(gi.predict(rows), gf.predict(rows)), rows


@pytest.mark.parametrize("storage", STORAGES)
def test_row_strided_cuda_views_are_read_in_place(storage):
    import torch
    ss.init(0)
    n, d = 300, 48
    tdt = torch.bfloat16 if storage == "bf16" else torch.float16
    wide = np.full((n, 64), NAN_PATTERN, np.uint16)                       # NaN patterns beside the view
    wide[:, :d] = to_bits(R.vectors(n, d, seed=41, signed=True), storage)
    Xw = torch.from_numpy(wide.view(np.int16)).cuda().view(tdt)
    view = Xw[:, :d]
    assert view.stride() == (64, 1) and not view.is_contiguous()
    keep = []
    from simspread_jl_amd import engine
    ptr, rows, cols, ld = engine._features_h16(view, CODE[storage], True, keep)
    assert (ptr, rows, cols, ld) == (Xw.data_ptr(), n, d, 64)               # no copy
    want = ss.dot_csr(np.ascontiguousarray(wide[:, :d]), alpha=0.5, storage=storage)
    for X in (view, view.contiguous()):
        p, i, v = ss.dot_csr(X, alpha=0.5)                                 # storage by the dtype
        assert ss.path_last() == ["dot_h16_sym"]
        assert_csr_equal(to_csr(p, i, v, (n, n)), want)
    p, i, v = ss.dot_csr(view[:100], view.t().contiguous().t()[100:], metric="dice", alpha=0.4, storage=storage)
    assert_csr_equal(to_csr(p, i, v, (100, n - 100)),
                     ss.dot_csr(wide[:100, :d], np.ascontiguousarray(wide[100:, :d]), metric="dice", alpha=0.4,
                                storage=storage))
