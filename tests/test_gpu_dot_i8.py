"""The int8 route of the inner-product producer on the device (include/simspread_hip_int8.h, csrc/dot_tile_i8.hpp): rows
of signed bytes, row-major -> thresholded cosine / Tanimoto / Dice CSR on v_mfma_i32_32x32x32_i8 -> graph, with the
neighbour floor.

g, A and B are exact integers on this route, so s is a pure function of the inputs and EVERY comparison here is bitwise:
against the host rule (dot_i8_ref.ref_s: exact int64 sums, one int64 -> float32 conversion each, dot_ref.rule in
float32; the keep and floor rules of neighbour_ref) and, where the floating-point routes are exact too, against them.
The two sides of the cross blocks hold different data, so a wrong operand lane map, k pairing or row / column swap
cannot pass."""
import ctypes as C

import numpy as np
import pytest
import scipy.sparse as sp

import simspread_jl_amd as ss

import dot_i8_ref as I
import dot_ref as R
import real_floor_ref as FR
from dot_ref import to_csr
from real_floor_ref import assert_csr_equal, ref_cut, ref_floor, ref_kth

pytestmark = pytest.mark.gpu

F32 = np.float32
METRIC_CODE = {"cosine": 0, "tanimoto": 1, "dice": 2}
ALPHAS = (0.3, 0.5, 0.9)
# the tile edge, the chunk edge at 16, the MFMA slice at 32, the step at 128 with a ragged last step, 33 tiles for the
# triangle enumeration, and sums above 2^24 (d = 2048), where the integer-to-float conversion rounds
CASES = [(129, 1), (131, 15), (128, 16), (129, 17), (130, 33), (200, 129), (300, 300), (4097, 16), (130, 2048)]
D_EXACT_ON_THE_FLOAT_ROUTES = 1040


def _pattern_of(W):
    """The pattern-only CSR that goes with the weighted CSR W at alpha > 0 (then every kept s is positive: the same
    pattern, every value 1)."""
    return sp.csr_matrix((np.ones_like(W.data), W.indices, W.indptr), shape=W.shape)


# ----------------------------------------------------------------------------------------------- 1. the rule, bit for bit
@pytest.mark.parametrize("metric", R.METRICS)
@pytest.mark.parametrize("n,d", CASES)
def test_every_input_is_the_rule_bit_for_bit(n, d, metric):
    ss.init(0)
    F, G = I.case_inputs(n, d)
    assert F.min() == -128 and F.max() == 127 and not F[7].any() and np.array_equal(F[n // 2], F[n // 3])
    sm_sym, sm_x = I.sums(F, F), I.sums(F, G)
    if d > 1024:       # the conversion to float32 rounds: some Gram value and some norm are not float32 numbers
        for g, a, _ in (sm_sym, sm_x):
            off = g[~np.eye(*g.shape, dtype=bool)] if g.shape[0] == g.shape[1] else g
            assert (off.astype(F32).astype(np.int64) != off).any() and (a.astype(F32).astype(np.int64) != a).any()
    s_sym, s_x = I.ref_s(F, None, metric, sm_sym), I.ref_s(F, G, metric, sm_x)
    if d >= 4:          # the pairs whose similarity is exactly 0.5
        i, j = {"cosine": (10, 11), "tanimoto": (12, 13), "dice": (12, 14)}[metric]
        assert s_sym[i, j] == F32(0.5) and s_sym[j, i] == F32(0.5)
    exact_elsewhere = d <= D_EXACT_ON_THE_FLOAT_ROUTES
    wide_f, wide_g = F.astype(F32), G.astype(F32)
    for Fb, wide_b, s, tag, plain in ((None, None, s_sym, "dot_i8_sym", "dot_csr_sym"),
                                      (G, wide_g, s_x, "dot_i8_cross", "dot_csr_cross")):
        off_diag = s if Fb is not None else s[~np.eye(n, dtype=bool)]
        assert (off_diag >= F32(0.5)).any() and (off_diag < F32(0.5)).any()
        for alpha in ALPHAS:
            want = ref_cut(s, alpha, True)
            W = ss.dot_csr(F, Fb, metric=metric, alpha=alpha, weighted=True, storage="i8")
            assert ss.path_last() == [tag]
            assert_csr_equal(W, want)
            U = ss.dot_csr(F, Fb, metric=metric, alpha=alpha, weighted=False, storage="i8")
            assert_csr_equal(U, ref_cut(s, alpha, False) if n <= 300 else _pattern_of(want))
            if exact_elsewhere:
                for weighted, mine in ((True, W), (False, U)):
                    assert_csr_equal(ss.dot_csr(F, Fb, metric=metric, alpha=alpha, weighted=weighted, storage="bf16"),
                                     mine)
                    assert_csr_equal(ss.dot_csr(wide_f, wide_b, metric=metric, alpha=alpha, weighted=weighted), mine)
                    assert ss.path_last() == [plain]


def test_pattern_only_reference_is_the_rule_itself():
    """_pattern_of(ref_cut(s, alpha, True)) is ref_cut(s, alpha, False) at every alpha of this file (host only; it is here
    so that the shortcut of the test above is itself pinned)."""
    F, G = I.case_inputs(131, 15)
    for metric in R.METRICS:
        for s in (I.ref_s(F, None, metric), I.ref_s(F, G, metric)):
            for alpha in ALPHAS:
                assert_csr_equal(_pattern_of(ref_cut(s, alpha, True)), ref_cut(s, alpha, False))


# ----------------------------------------------------------------------------------------------- 2. the neighbour floor
@pytest.mark.parametrize("k", [1, 5, 33, 64])
@pytest.mark.parametrize("n,d", [(300, 33), (131, 15)])
def test_floor_is_the_rule_bit_for_bit(n, d, k):
    ss.init(0)
    F, G, Q = I.floor_inputs(n, d)
    for metric in R.METRICS:
        for Fa, Fb, sym in ((F, None, True), (Q, G, False)):
            s = I.ref_s(Fa, Fb, metric)
            # both kinds of row are there: a tie at the k-th value, and fewer than k positives (against itself a row
            # always has its diagonal, so k = 1 has no short row in the symmetric block)
            assert len(FR.tied_rows(s, k)) > 0
            assert (FR.positives(s) < k).any() or (sym and k == 1)
            assert len(FR.gained_rows(s, np.inf, k)) > 0 and (k == 1 or len(FR.gained_rows(s, 0.5, k)) > 0)
            tau = ss.dot_kth_i8(Fa, Fb, metric=metric, k=k)
            assert ss.path_last() == ["dot_i8_kth"]
            want_tau = ref_kth(s, k)
            assert tau.dtype == F32 and np.array_equal(tau.view(np.uint32), want_tau.view(np.uint32))
            for alpha in (0.5, np.inf):
                for weighted in (True, False):
                    M = ss.dot_csr(Fa, Fb, metric=metric, alpha=alpha, weighted=weighted, storage="i8", min_neighbours=k)
                    assert ss.path_last() == ["dot_i8_floor_sym" if sym else "dot_i8_floor_cross"]
                    assert_csr_equal(M, ref_floor(s, alpha, k, weighted))
                    again = ss.dot_csr(Fa, Fb, metric=metric, alpha=alpha, weighted=weighted, storage="i8",
                                       min_neighbours=k)
                    assert_csr_equal(again, M)                                  # two runs: the same bits
            assert np.array_equal(ss.dot_kth_i8(Fa, Fb, metric=metric, k=k).view(np.uint32),
                                  tau.view(np.uint32))


def test_k_zero_is_the_plain_producer_with_the_plain_tags():
    lib = ss.init(0)
    F, G, Q = I.floor_inputs(131, 15)
    for Fa, Fb, tag in ((F, None, "dot_i8_sym"), (Q, G, "dot_i8_cross")):
        plain = ss.dot_csr(Fa, Fb, metric="tanimoto", alpha=0.5, storage="i8")
        assert ss.path_last() == [tag]
        got = ss.dot_csr(Fa, Fb, metric="tanimoto", alpha=0.5, storage="i8", min_neighbours=0)
        assert ss.path_last() == [tag]
        assert_csr_equal(got, plain)
        raw = _raw_csr(lib, 0, (Fa, 0), Fa.shape[0], 15, None if Fb is None else (Fb, 0),
                       0 if Fb is None else Fb.shape[0], 15, 15, "tanimoto", 0.5, 0)
        assert ss.path_last() == [tag]
        assert_csr_equal(raw, plain)
        if Fb is None:                                     # the triangle grid mirrors the bits
            D = plain.toarray()
            assert np.array_equal(D.view(np.uint32), D.T.copy().view(np.uint32)) and (D.diagonal() == 1).all()


# ----------------------------------------------------------------------------------------------- 3. the layout contract
def _strided(X, ld, shift):
    """A byte buffer that starts `shift` bytes before row 0, holds row i at shift + i * ld and ENDS with the last byte of
    the last row; every byte that is not a feature is -128."""
    n, d = X.shape
    buf = np.full(shift + (n - 1) * ld + d, -128, np.int8)
    for i in range(n):
        buf[shift + i * ld: shift + i * ld + d] = X[i]
    return buf


def _raw_csr(lib, mem, a, na, lda, b, nb, ldb, d, metric, alpha, k, weighted=1):
    """ss_similarity_dot_csr_i8 through ctypes: a, b are (buffer, byte offset) of numpy (mem 0) or CUDA int8 tensors
    (mem 1); b None: symmetric."""
    import torch
    fn = lib.ss_similarity_dot_csr_i8

    def address(x):
        if x is None:
            return None
        buf, off = x
        return (buf.data_ptr() if mem else buf.ctypes.data) + off
    head = (address(a), na, lda, address(b), nb if b is not None else 0, ldb if b is not None else 0, d,
            METRIC_CODE[metric], C.c_float(alpha), k, weighted)
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


@pytest.mark.parametrize("k", [0, 5])
def test_layout_contract_any_base_any_ld_padding_and_no_read_past_the_last_row(k):
    import torch
    lib = ss.init(0)
    n, d, alpha, metric = 300, 65, 0.5, "cosine"
    F, G = I.case_inputs(n, d)
    nb = G.shape[0]
    want_sym = ss.dot_csr(F, metric=metric, alpha=alpha, storage="i8", min_neighbours=k)   # contiguous copies
    want_x = ss.dot_csr(F, G, metric=metric, alpha=alpha, storage="i8", min_neighbours=k)
    assert_csr_equal(want_sym, ref_floor(I.ref_s(F, None, metric), alpha, k, True))
    assert_csr_equal(want_x, ref_floor(I.ref_s(F, G, metric), alpha, k, True))
    assert want_sym.nnz > n and want_x.nnz > 0
    # ld = d, d + 5 and d rounded up to 16; bases + 0, + 1, + 3 and + 16 bytes; (80, 0) and (80, 16) allow 16-byte loads
    for ld, shift in ((d, 0), (d + 5, 1), (d + 5, 3), (80, 0), (80, 16), (80, 3)):
        ha, hb = _strided(F, ld, shift), _strided(G, ld, shift)
        for mem in (1, 0):
            if mem:
                a, b = torch.from_numpy(ha).cuda(), torch.from_numpy(hb).cuda()
                assert a.data_ptr() % 16 == 0 and a.numel() == shift + (n - 1) * ld + d      # ends with the last row
            else:
                a, b = ha, hb
            assert_csr_equal(_raw_csr(lib, mem, (a, shift), n, ld, None, 0, 0, d, metric, alpha, k), want_sym)
            assert_csr_equal(_raw_csr(lib, mem, (a, shift), n, ld, (b, shift), nb, ld, d, metric, alpha, k), want_x)
    # an aligned side against an unaligned one
    a = torch.from_numpy(_strided(F, 80, 0)).cuda()
    b = torch.from_numpy(_strided(G, d + 5, 1)).cuda()
    assert_csr_equal(_raw_csr(lib, 1, (a, 0), n, 80, (b, 1), nb, d + 5, d, metric, alpha, k), want_x)


# ----------------------------------------------------------------------------------------------- 4. refusals
def test_refusals_come_before_anything_is_written_and_the_size_protocol():
    import torch
    lib = ss.init(0)
    fn, kth = lib.ss_similarity_dot_csr_i8, lib.ss_similarity_dot_kth_i8
    n, d = 300, 20
    X, _ = I.case_inputs(n, d)
    ptr = np.full(n + 1, -7, np.int64)
    idx = np.full(10, -7, np.int32)
    val = np.full(10, -7, F32)
    tau = np.full(n, -7, F32)
    nnz = C.c_int64(-7)

    def call(d_, metric, alpha, k, lda=d, out_idx=None, mem=0, p=None, a=None):
        return fn(X.ctypes.data if a is None else a, n, lda, None, 0, 0, d_, metric, C.c_float(alpha), k, 1,
                  ptr.ctypes.data if p is None else p, out_idx, None if out_idx is None else val.ctypes.data, 10,
                  C.byref(nnz), mem)
    # d = 131072 is refused before anything is read: the rows hold 20 bytes each
    cases = ((131072, 0, 0.5, 0, 131072, "131071"), (d, 0, float("nan"), 0, d, "NaN"), (d, 3, 0.5, 0, d, "metric"),
             (d, -1, 0.5, 0, d, "metric"), (d, 0, 0.5, 65, d, "k ="), (d, 0, 0.5, -1, d, "k ="),
             (d, 0, 0.5, 0, d - 1, "leading"))
    for d_, metric, alpha, k, lda, word in cases:
        for out_idx in (None, idx.ctypes.data):
            assert call(d_, metric, alpha, k, lda, out_idx) == -1, word
            assert word in lib.ss_last_error().decode(), (word, lib.ss_last_error())
    for d_, metric, k, word in ((d, 0, 0, "k ="), (d, 0, 65, "k ="), (d, 3, 5, "metric"), (131072, 0, 5, "131071")):
        assert kth(X.ctypes.data, n, max(d_, d), None, 0, 0, d_, metric, k, tau.ctypes.data, 0) == -1, word
        assert word in lib.ss_last_error().decode(), (word, lib.ss_last_error())
    assert nnz.value == -7 and (ptr == -7).all() and (idx == -7).all() and (val == -7).all() and (tau == -7).all()
    # device memory
    xt = torch.from_numpy(np.array(X)).cuda()
    pt = torch.full((n + 1,), -7, dtype=torch.int64, device="cuda")
    assert call(d, 3, 0.5, 0, mem=1, p=pt.data_ptr(), a=xt.data_ptr()) == -1
    assert call(131072, 0, 0.5, 0, lda=131072, mem=1, p=pt.data_ptr(), a=xt.data_ptr()) == -1
    assert nnz.value == -7 and (pt.cpu().numpy() == -7).all()
    # the python mirror and the graph constructors
    with pytest.raises(ss.SimSpreadError) as e:
        ss.dot_csr(X, alpha=float("nan"), storage="i8")
    assert e.value.code == -1
    h = C.c_void_p()
    yp = np.zeros(n + 1, np.int64)
    for metric, k in ((7, 0), (0, 65)):
        assert lib.ss_graph_create_vectors_i8(0, n, 4, d, metric, None, d, X.ctypes.data, d, yp.ctypes.data, None, None, 0,
                                              C.c_float(0.5), k, 1, 0, C.byref(h)) == -1
        assert h.value is None
    # the size protocol
    want = ss.dot_csr(X, alpha=0.3, storage="i8")
    p2 = np.zeros(n + 1, np.int64)
    n1, n2 = C.c_int64(-1), C.c_int64(-1)
    head = (X.ctypes.data, n, d, None, 0, 0, d, 0, C.c_float(0.3), 0, 1)
    assert fn(*head, p2.ctypes.data, None, None, 0, C.byref(n1), 0) == 0                            # idx == NULL
    assert n1.value == want.nnz > n and np.array_equal(p2, want.indptr)
    i2 = np.full(n1.value, -5, np.int32)
    v2 = np.full(n1.value, -5, F32)
    rc = fn(*head, p2.ctypes.data, i2.ctypes.data, v2.ctypes.data, n1.value - 1, C.byref(n2), 0)   # capacity < nnz
    assert rc == -1 and n2.value == n1.value and (i2 == -5).all() and (v2 == -5).all()
    assert fn(*head, p2.ctypes.data, i2.ctypes.data, None, n1.value, C.byref(n2), 0) == 0           # the pattern only
    assert np.array_equal(i2, want.indices) and (v2 == -5).all()
    assert fn(*head, p2.ctypes.data, i2.ctypes.data, v2.ctypes.data, n1.value, C.byref(n2), 0) == 0
    assert_csr_equal(sp.csr_matrix((v2, i2, p2), shape=(n, n)), want)
    assert fn(None, n, d, None, 0, 0, d, 0, C.c_float(0.3), 0, 1, p2.ctypes.data, None, None, 0, C.byref(n2), 0) == -1
    assert fn(X.ctypes.data, 1 << 31, d, None, 0, 0, d, 0, C.c_float(0.3), 0, 1, p2.ctypes.data, None, None, 0,
              C.byref(n2), 0) == -5


def test_empty_inputs():
    ss.init(0)
    E = np.zeros((5, 0), np.int8)
    for metric in R.METRICS:                               # d == 0: every pair has s = 1
        assert (ss.dot_csr(E, metric=metric, alpha=1.0, storage="i8").toarray() == 1).all()
        assert (ss.dot_csr(E, np.zeros((3, 0), np.int8), metric=metric, alpha=0.5, storage="i8").toarray() == 1).all()
        M = ss.dot_csr(E, np.zeros((3, 0), np.int8), metric=metric, alpha=np.inf, storage="i8", min_neighbours=2)
        assert M.shape == (5, 3) and (M.toarray() == 1).all()          # every value ties at tau = 1
        assert (ss.dot_kth_i8(E, metric=metric, k=5) == 1).all()
        assert (ss.dot_kth_i8(E, metric=metric, k=6) == 0).all()
    X, _ = I.case_inputs(131, 15)
    none = np.zeros((0, 15), np.int8)
    for k in (0, 3):
        A = ss.dot_csr(none, X, alpha=0.5, storage="i8", min_neighbours=k)                  # na == 0
        assert A.shape == (0, 131) and A.nnz == 0
        B = ss.dot_csr(X, none, alpha=0.5, storage="i8", min_neighbours=k)                  # nb == 0
        assert B.shape == (131, 0) and B.nnz == 0 and not B.indptr.any()
        S = ss.dot_csr(none, alpha=0.5, storage="i8", min_neighbours=k)
        assert S.shape == (0, 0) and S.nnz == 0
    assert ss.dot_kth_i8(none, X, k=3).shape == (0,)
    tau = ss.dot_kth_i8(X, none, k=3)                                            # as dot_kth_f32: tau = 0
    assert tau.shape == (131,) and not tau.any()


# ----------------------------------------------------------------------------------------------- 5. graph and queries
def _labels(ns, nt, seed):
    rng = np.random.default_rng(seed)
    Y = sp.random(ns, nt, density=4.0 / nt, random_state=rng, format="csr")
    Y.data[:] = 1.0
    return Y


def _same_bits(a, b):
    return a.shape == b.shape and np.array_equal(a.view(np.uint8), b.view(np.uint8))


@pytest.mark.parametrize("k", [0, 3])
def test_graph_and_queries_from_int8_vectors(k):
    import torch
    ss.init(0)
    ns, nq, nt, d, alpha, metric = 200, 60, 30, 48, 0.6, "cosine"
    Fs = I.rows(ns, d, seed=11)
    Fq = I.rows(nq, d, seed=12)
    Fq[30:] = Fs[:30]                                     # queries that have close sources
    Y = _labels(ns, nt, 13)
    Xs = ref_floor(I.ref_s(Fs, None, metric), alpha, k, True)          # the reference CSR, from the host rule
    Xq = ref_floor(I.ref_s(Fq, Fs, metric), alpha, k, True)
    assert Xs.nnz > ns and Xq.nnz > 0
    kw = dict(alpha=alpha, metric=metric, weighted=True, storage="i8", min_neighbours=k)
    tags = ["dot_i8_floor_sym", "dot_i8_floor_cross"] if k else ["dot_i8_sym", "dot_i8_cross"]

    g = ss.DeviceGraph.from_vectors(Fq, Fs, Y, **kw)
    assert ss.path_last() == tags
    assert g.dtype == np.float32
    assert (g.nq, g.ns, g.nf, g.nt, g.nnz_xq, g.nnz_xs) == (nq, ns, ns, nt, Xq.nnz, Xs.nnz)
    r = ss.DeviceGraph.from_sparse(Xq, Xs, Y, dtype=F32)
    for rows in ("query", "source"):
        assert _same_bits(g.predict(rows), r.predict(rows)), rows
    g3 = ss.DeviceGraph.from_vectors(None, Fs, Y, **kw)
    assert ss.path_last() == tags[:1]
    r3 = ss.DeviceGraph.from_sparse(None, Xs, Y, dtype=F32)
    assert _same_bits(g3.predict_loo(clean=True), r3.predict_loo(clean=True))

    for graph in (g3, r3):                                 # a query set on a graph of either constructor
        q = ss.DeviceQueries.from_vectors(graph, Fq, Fs, **kw)
        assert ss.path_last() == tags[1:]
        assert (q.nq, q.nnz) == (nq, Xq.nnz)
        assert _same_bits(graph.predict(queries=q), r.predict("query"))
        q.close()

    # torch.int8 CUDA tensors: the same graph, the same query set
    ts, tq = torch.from_numpy(Fs).cuda(), torch.from_numpy(Fq).cuda()
    Yd = (torch.from_numpy(Y.indptr.astype(np.int64)).cuda(), torch.from_numpy(Y.indices.astype(np.int32)).cuda(), None, nt)
    gd = ss.DeviceGraph.from_vectors(tq, ts, Yd, **kw)
    assert (gd.nnz_xq, gd.nnz_xs) == (Xq.nnz, Xs.nnz)
    assert _same_bits(gd.predict("query"), r.predict("query"))
    qd = ss.DeviceQueries.from_vectors(g3, tq, ts, **kw)
    assert _same_bits(g3.predict(queries=qd), r.predict("query"))
    # other integer-valued arrays are converted exactly; the route is taken only when named
    gi = ss.DeviceGraph.from_vectors(Fq.astype(np.int32), Fs.astype(np.float64), Y, **kw)
    assert _same_bits(gi.predict("query"), r.predict("query"))
    ss.DeviceGraph.from_vectors(Fq, Fs, Y, alpha=alpha, metric=metric, min_neighbours=k)
    assert ss.path_last() == (["dot_csr_floor_sym", "dot_csr_floor_cross"] if k else ["dot_csr_sym", "dot_csr_cross"])


def test_row_strided_cuda_views_are_read_in_place():
    import torch
    ss.init(0)
    n, d = 300, 48
    wide = np.full((n, 64), -128, np.int8)
    wide[:, :d] = I.rows(n, d, seed=41)
    Xw = torch.from_numpy(wide).cuda()
    view = Xw[:, :d]
    assert view.stride() == (64, 1) and not view.is_contiguous()
    keep = []
    from simspread_jl_amd import engine
    assert engine._features_i8(view, True, keep) == (Xw.data_ptr(), n, d, 64)               # no copy
    off = Xw[:, 3:3 + d]                                                                    # a misaligned base
    assert engine._features_i8(off, True, keep) == (Xw.data_ptr() + 3, n, d, 64)
    want = ss.dot_csr(np.ascontiguousarray(wide[:, :d]), alpha=0.5, storage="i8")
    assert_csr_equal(want, ref_cut(I.ref_s(np.ascontiguousarray(wide[:, :d]), None, "cosine"), 0.5, True))
    for X in (view, view.contiguous()):
        p, i, v = ss.dot_csr(X, alpha=0.5, storage="i8")
        assert ss.path_last() == ["dot_i8_sym"]
        assert_csr_equal(to_csr(p, i, v, (n, n)), want)
    tau = ss.dot_kth_i8(view, k=5)
    assert tau.is_cuda and np.array_equal(tau.cpu().numpy(), ss.dot_kth_i8(np.ascontiguousarray(wide[:, :d]), k=5))
    p, i, v = ss.dot_csr(view[:100], view.t().contiguous().t()[100:], metric="dice", alpha=0.4, storage="i8",
                         min_neighbours=2)
    assert_csr_equal(to_csr(p, i, v, (100, n - 100)),
                     ss.dot_csr(wide[:100, :d], np.ascontiguousarray(wide[100:, :d]), metric="dice", alpha=0.4,
                                storage="i8", min_neighbours=2))
    with pytest.raises(ValueError):
        ss.dot_csr(view.to(torch.float32) + 0.5, alpha=0.5, storage="i8")
