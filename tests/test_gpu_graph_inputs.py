"""The layer that turns a caller's matrices into a handle, route by route: ss_graph_create_csr_* / _dense_* / _general_*,
the label CSR of the other constructors, ss_spmat_create_csr_*, the element-wise ABI and the refusals of bad CSR.

Nothing reads a handle's CSR back.  A handle is judged by ss_graph_info, ss_graph_degrees and the bits of every score it
serves, on the exactly summable graphs of tests/sparse_ref.py (tests/graph_input_ref.py adds two of extreme shape): there
float32(oracle) -- for fp64 the oracle itself -- is the only correct answer, so a dropped, doubled, shifted or misplaced
entry changes the bits, a count or a degree (tests/test_graph_inputs_cpu.py proves it defect by defect).  Where inputs
are not exactly summable (source rows, the domain cases) the handle is compared bit for bit with the base-0 host
from_sparse handle of the canonical CSR computed in numpy.  Every handle is fresh.  The only tolerances are the
gamma(k) bands of the directed general graph."""
import ctypes as C
import functools

import numpy as np
import pytest
import scipy.sparse as sp

import simspread_jl_amd as ss
from oracle import simspread_oracle as O

import graph_input_ref as G
import sparse_ref as S

pytestmark = pytest.mark.gpu

DTYPES = [np.float32, np.float64]
D_IDS = ["f32", "f64"]
WEIGHTED = [True, False]
W_IDS = ["weighted", "pattern-only"]
MEMS = [G.HOST, G.DEVICE]
M_IDS = ["host", "device"]
ROUTES = [(0, G.HOST), (1, G.HOST), (0, G.DEVICE), (1, G.DEVICE)]
WORST = {}


@pytest.fixture(scope="module", autouse=True)
def _init():
    ss.init(0)


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32 if a.dtype == np.float32 else np.uint64)


def _same_bits(got, want, label):
    assert got.dtype == want.dtype and got.shape == want.shape, (label, got.dtype, got.shape, want.shape)
    bad = _bits(got) != _bits(want)
    assert not bad.any(), f"{label}: {int(bad.sum())} of {bad.size} scores differ from the canonical handle's bits"


def _cleaned(want, mask):
    out = want.copy()
    out[np.broadcast_to(mask, out.shape)] = -99.0
    return out


# ----------------------------------------------------------------------------- cases (inputs and references, built once)
BUILDERS = {
    "query": lambda w: S.exact_query_for(4, None, weighted=w),
    "tall": G.tall_graph,
    "wide": G.wide_graph,
    "q63": lambda w: G.small_query(63, w),
    "q64": lambda w: G.small_query(64, w),
    "q65": lambda w: G.small_query(65, w),
}


@functools.lru_cache(maxsize=None)
def _case(name, weighted):
    inp = BUILDERS[name](weighted)
    want = S.oracle_query(inp["Xq"], inp["Xs"], inp["Ys"])
    want.setflags(write=False)
    return inp, want


@functools.lru_cache(maxsize=None)
def _canonical_source(name, weighted, dtype):
    """Source rows of the base-0 host from_sparse handle of the case (not exactly summable: the target path divides by
    kt)."""
    inp, _ = _case(name, weighted)
    g = ss.DeviceGraph.from_sparse(inp["Xq"].astype(dtype), inp["Xs"].astype(dtype), inp["Ys"].astype(dtype), dtype=dtype)
    out = g.predict("source")
    g.close()
    out.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def _loo_case(weighted):
    inp = S.exact_loo(weighted)
    want = S.oracle_loo(inp["X"], inp["Y"])
    want.setflags(write=False)
    return inp, want


@functools.lru_cache(maxsize=None)
def _kfold_case(weighted):
    inp = S.exact_kfold(weighted)
    want = S.oracle_kfold(inp["X"], inp["Y"], inp["fold"])
    want.setflags(write=False)
    return inp, want


# ----------------------------------------------------------------------------- what every route is held to
def _check_shown(g, Xq, Xs, Ys, label):
    ns, nf = Xs.shape
    nq = 0 if Xq is None else Xq.shape[0]
    nz, kf, ks, kt = G.shown(sp.csr_matrix((0, nf)) if Xq is None else Xq, Xs, Ys)
    assert (g.nq, g.ns, g.nf, g.nt) == (nq, ns, nf, Ys.shape[1]), label
    assert (g.nnz_xq, g.nnz_xs, g.nnz_ys) == nz, (label, (g.nnz_xq, g.nnz_xs, g.nnz_ys), nz)
    for got, want, which in zip(g.degrees(), (kf, ks, kt), ("kf", "ks", "kt")):
        np.testing.assert_array_equal(got, want, err_msg=f"{label}: {which}")


def _check_query_handle(g, name, weighted, dtype, label):
    """info, degrees; predict("query") whole, on a sub-range with begin % 8 != 0 and with clean! against the oracle's
    bits; predict("source") whole and on a sub-range against the canonical handle's."""
    inp, want = _case(name, weighted)
    _check_shown(g, inp["Xq"], inp["Xs"], inp["Ys"], label)
    nq, ns = inp["Xq"].shape[0], inp["Xs"].shape[0]
    S.assert_bitwise(g.predict("query"), want, dtype, f"{label}: query rows")
    a = 5 if nq > 8 else 1
    b = min(nq, a + 13)
    if b > a:
        S.assert_bitwise(g.predict("query", a, b), want[a:b], dtype, f"{label}: query rows [{a},{b})")
    mask = S.clean_mask(inp["Ys"])
    assert mask.any()
    S.assert_bitwise(g.predict("query", clean=True), _cleaned(want, mask), dtype, f"{label}: query rows, clean")
    canon = _canonical_source(name, weighted, dtype)
    _same_bits(g.predict("source"), canon, f"{label}: source rows")
    a, b = (13, 77) if ns > 77 else (3, ns)
    _same_bits(g.predict("source", a, b), canon[a:b], f"{label}: source rows [{a},{b})")
    g.close()


def _check_three_layer(make, weighted, dtype, label):
    """A 3-layer route: make(X, Y) builds a fresh handle; predict_loo (whole, a sub-range, clean) and
    predict_kfold_rows (whole, a sub-range) against the oracle's bits."""
    inp, want = _loo_case(weighted)
    X, Y = inp["X"], inp["Y"]
    g = make(X, Y)
    _check_shown(g, None, X, Y, f"{label}: leave-one-out graph")
    S.assert_bitwise(g.predict_loo(), want, dtype, f"{label}: leave-one-out")
    S.assert_bitwise(g.predict_loo(61, 70), want[61:70], dtype, f"{label}: leave-one-out rows [61,70)")
    mask = S.clean_mask(Y, np.arange(X.shape[0]))
    S.assert_bitwise(g.predict_loo(clean=True), _cleaned(want, mask), dtype, f"{label}: leave-one-out, clean")
    g.close()
    inp, want = _kfold_case(weighted)
    X, Y, fold = inp["X"], inp["Y"], inp["fold"]
    g = make(X, Y)
    _check_shown(g, None, X, Y, f"{label}: k-fold graph")
    S.assert_bitwise(g.predict_kfold_rows(fold, inp["nfolds"]), want, dtype, f"{label}: k-fold rows")
    S.assert_bitwise(g.predict_kfold_rows(fold, inp["nfolds"], 29, 70), want[29:70], dtype, f"{label}: k-fold rows [29,70)")
    g.close()


# ============================================================================= 1. CSR routes
def _pattern(weighted, explicit):
    """val == NULL for the labels, and for all three blocks of the pattern-only graph; `explicit`: every value passed."""
    if explicit:
        return (False, False, False)
    return (False, False, True) if weighted else (True, True, True)


@pytest.mark.parametrize("base,mem", ROUTES, ids=[f"base{b}-{M_IDS[m]}" for b, m in ROUTES])
@pytest.mark.parametrize("weighted", WEIGHTED, ids=W_IDS)
@pytest.mark.parametrize("dtype", DTYPES, ids=D_IDS)
def test_csr_route_query_graph(dtype, weighted, base, mem):
    """ss_graph_create_csr_* with index_base 0 / 1 (1: the CSC of the transpose as the Julia binding builds it), host /
    device memory, NULL and explicit values."""
    inp, _ = _case("query", weighted)
    for explicit in (False, True):
        g = G.graph_csr(inp["Xq"], inp["Xs"], inp["Ys"], dtype, base, mem, _pattern(weighted, explicit))
        _check_query_handle(g, "query", weighted, dtype, f"csr base {base} {M_IDS[mem]} explicit={explicit}")


@pytest.mark.parametrize("base,mem", ROUTES, ids=[f"base{b}-{M_IDS[m]}" for b, m in ROUTES])
@pytest.mark.parametrize("weighted", WEIGHTED, ids=W_IDS)
@pytest.mark.parametrize("dtype", DTYPES, ids=D_IDS)
def test_csr_route_three_layer_graph(dtype, weighted, base, mem):
    """nq = 0 with xq_* NULL and as a valid one-element pointer array."""
    for xq in ("null", "one"):
        make = lambda X, Y: G.graph_csr(None, X, Y, dtype, base, mem, _pattern(weighted, xq == "one"), xq=xq)
        _check_three_layer(make, weighted, dtype, f"csr base {base} {M_IDS[mem]} xq={xq}")


@pytest.mark.parametrize("weighted", WEIGHTED, ids=W_IDS)
@pytest.mark.parametrize("dtype", DTYPES, ids=D_IDS)
def test_csr_route_drops_stored_zeros(dtype, weighted):
    """A third of the stored values are 0.0 or -0.0, first, last and across the 64-entry steps of rows that store more
    than 64: the handle is the handle of the graph without them."""
    inp, _ = _case("query", weighted)
    Z = {k: G.with_stored_zeros(inp[k], seed) for k, seed in (("Xq", 1), ("Xs", 2), ("Ys", 3))}
    assert Z["Xs"].nnz > 1.4 * inp["Xs"].nnz and Z["Ys"].nnz > 1.4 * inp["Ys"].nnz
    for base, mem in ROUTES:
        g = G.graph_csr(Z["Xq"], Z["Xs"], Z["Ys"], dtype, base, mem)
        _check_query_handle(g, "query", weighted, dtype, f"stored zeros, base {base} {M_IDS[mem]}")


@pytest.mark.parametrize("weighted", WEIGHTED, ids=W_IDS)
@pytest.mark.parametrize("dtype", DTYPES, ids=D_IDS)
def test_spmat_routes_equal_w_times_r(dtype, weighted):
    """ss_spmat_create_csr_* in the 1-based and device forms: W @ R at B = 1, 5, 64 equals the fp64 product bit for bit."""
    W, R = S.spmm_operands(weighted=weighted)
    want = W @ R
    for base, mem in ROUTES:
        for pattern in ((False, True) if not weighted else (False,)):
            w = G.spmat(W, dtype, base, mem, pattern)
            for B in (1, 5, 64):
                got = w.spmm(np.ascontiguousarray(R[:, :B]).astype(dtype))
                S.assert_bitwise(got, want[:, :B], dtype, f"W @ R, base {base} {M_IDS[mem]}, B = {B}")
            w.close()


# ============================================================================= 2. dense-block route
@functools.lru_cache(maxsize=4)
def _dense_case(name, weighted):
    inp, _ = _case(name, weighted)
    return tuple(inp[k].toarray() for k in ("Xq", "Xs", "Ys"))


@pytest.mark.parametrize("mem", MEMS, ids=M_IDS)
@pytest.mark.parametrize("weighted", WEIGHTED, ids=W_IDS)
@pytest.mark.parametrize("dtype", DTYPES, ids=D_IDS)
@pytest.mark.parametrize("name", ["query", "q63", "q64", "q65", "tall", "wide"])
def test_dense_route_without_cutoff(name, dtype, weighted, mem):
    """ss_graph_create_dense_* with apply_cutoff = 0 on the densified exact graphs, ld = rows + 5 with NaN padding.  The
    3000-source graph: 22 splits of 137 columns (last 123), 750 of 4, 22 of 14 (last 6); 63 / 64 / 65 query rows; the
    70 000 x 3 label block (one split); one query x 70 001 features (1015 splits of 69, last 35)."""
    blocks = G.dense_blocks(_dense_case(name, weighted), dtype, mem)
    g = ss.DeviceGraph.from_dense(*blocks, dtype=dtype, ld_pad=G.LD_PAD)
    del blocks
    _check_query_handle(g, name, weighted, dtype, f"dense {name} {M_IDS[mem]}")


@pytest.mark.parametrize("mem", MEMS, ids=M_IDS)
@pytest.mark.parametrize("weighted", WEIGHTED, ids=W_IDS)
@pytest.mark.parametrize("dtype", DTYPES, ids=D_IDS)
def test_dense_route_three_layer_graph(dtype, weighted, mem):
    """Sq == NULL; the 488-source leave-one-out graph (122 splits of 4) and the 252-source k-fold graph (one column per
    split)."""
    def make(X, Y):
        blocks = G.dense_blocks((None, X.toarray(), Y.toarray()), dtype, mem)
        return ss.DeviceGraph.from_dense(*blocks, dtype=dtype, ld_pad=G.LD_PAD)
    _check_three_layer(make, weighted, dtype, f"dense {M_IDS[mem]}")


@functools.lru_cache(maxsize=2)
def _raw_case(weighted, dtype):
    inp, _ = _case("query", weighted)
    return (G.raw_similarities(inp["Xq"], 0.5, weighted, dtype, 51), G.raw_similarities(inp["Xs"], 0.5, weighted, dtype, 52),
            inp["Ys"].toarray())


@pytest.mark.parametrize("mem", MEMS, ids=M_IDS)
@pytest.mark.parametrize("weighted", WEIGHTED, ids=W_IDS)
@pytest.mark.parametrize("dtype", DTYPES, ids=D_IDS)
def test_dense_route_with_cutoff(dtype, weighted, mem):
    """apply_cutoff = 1 at alpha = 0.5 on raw similarities whose cut is the exact graph: kept entries equal to alpha,
    dropped ones equal to nextafter(alpha, 0) in the graph precision."""
    blocks = G.dense_blocks(_raw_case(weighted, dtype), dtype, mem)
    g = ss.DeviceGraph.from_dense(*blocks, alpha=0.5, weighted=weighted, dtype=dtype, ld_pad=G.LD_PAD)
    del blocks
    _check_query_handle(g, "query", weighted, dtype, f"dense cutoff {M_IDS[mem]}")


@pytest.mark.parametrize("alpha", [0.0, -0.5, -1.0, 0.3])
@pytest.mark.parametrize("weighted", WEIGHTED, ids=W_IDS)
@pytest.mark.parametrize("dtype", DTYPES, ids=D_IDS)
def test_dense_route_input_domain(dtype, weighted, alpha):
    """NaN is no edge; unweighted, alpha <= 0 keeps zeros and the negatives >= alpha (alpha = -1: full rows); weighted, a
    zero of either sign is no edge and a negative weight keeps its sign.  Against the from_sparse handle of the canonical cut."""
    Sq, Ss, Y = G.domain_blocks()
    cq, cs = G.canonical_cut(Sq, alpha, weighted), G.canonical_cut(Ss, alpha, weighted)
    cy = G.canonical_cut(Y, None, True)
    if not weighted and alpha <= 0:
        assert cs.nnz == int((Ss >= alpha).sum()) > int((Ss > 0).sum()) and (cs.data == 1).all()
    if not weighted and alpha == -1.0:
        assert cs.nnz == int((~np.isnan(Ss)).sum())          # full rows but for NaN
    if weighted and alpha < 0:
        assert (cs.data < 0).any() and cs.nnz < int((Ss >= alpha).sum())
    canon = ss.DeviceGraph.from_sparse(cq.astype(dtype), cs.astype(dtype), cy.astype(dtype), dtype=dtype)
    want = [canon.predict("query"), canon.predict("source"), canon.predict("query", 3, 20, clean=True)]
    canon.close()
    for mem in MEMS:
        blocks = G.dense_blocks((Sq, Ss, Y), dtype, mem)
        g = ss.DeviceGraph.from_dense(*blocks, alpha=alpha, weighted=weighted, dtype=dtype, ld_pad=G.LD_PAD)
        label = f"domain alpha={alpha} {M_IDS[mem]}"
        _check_shown(g, cq, cs, cy, label)
        _same_bits(g.predict("query"), want[0], label + ": query rows")
        _same_bits(g.predict("source"), want[1], label + ": source rows")
        _same_bits(g.predict("query", 3, 20, clean=True), want[2], label + ": query rows [3,20), clean")
        assert (want[2] == -99).any()
        g.close()


# ============================================================================= 3. general graph
@functools.lru_cache(maxsize=None)
def _general_case(weighted):
    inp, want = _case("query", weighted)
    return G.general_blocks(inp["Xq"], inp["Xs"], inp["Ys"]) + (want, S.clean_mask(inp["Ys"]))


@pytest.mark.parametrize("base", [0, 1])
@pytest.mark.parametrize("weighted", WEIGHTED, ids=W_IDS)
@pytest.mark.parametrize("dtype", DTYPES, ids=D_IDS)
def test_general_graph_exact(dtype, weighted, base):
    """B the block matrix of the exact query graph (6370 nodes, never densified), L = A[queries, :], Wt = B[:, targets]':
    the oracle's bits in both precisions; the degrees are the row counts of B."""
    L, B, Wt, k, want, mask = _general_case(weighted)
    for mem in MEMS:
        g = G.create_general(B.shape[0], L, B, Wt, dtype, base, mem)
        label = f"general base {base} {M_IDS[mem]}"
        assert (g.nq, g.ns, g.nf, g.nt) == (L.shape[0], B.shape[0], B.shape[0], Wt.shape[0])
        assert (g.nnz_xq, g.nnz_xs, g.nnz_ys) == (L.nnz, B.nnz, Wt.nnz)
        kf, ks, kt = g.degrees()
        np.testing.assert_array_equal(kf, k)
        np.testing.assert_array_equal(ks, k)
        np.testing.assert_array_equal(kt, np.diff(Wt.indptr))
        S.assert_bitwise(g.predict("query"), want, dtype, label)
        S.assert_bitwise(g.predict("query", 5, 18), want[5:18], dtype, label + ", rows [5,18)")
        S.assert_bitwise(g.predict("query", clean=True), _cleaned(want, mask), dtype, label + ", clean")
        g.close()


@pytest.mark.parametrize("dtype", DTYPES, ids=D_IDS)
def test_general_graph_directed_within_its_bands(dtype):
    """A directed B (B != B', an empty row and an empty column), arbitrary rows of A and arbitrary columns of B against
    the literal L * spread(B) * spread(B)[:, cols] in fp64: gamma(k) per score, no margin, structural zeros exact.  A
    transposed operand in either stage leaves the band on most scores (test_graph_inputs_cpu.py)."""
    d = G.directed_graph()
    want = G.general_reference(d["L"], d["B"], d["cols"])
    band = G.general_band(d["L"], d["B"], d["cols"], want, dtype)
    assert want.size > 600 and (want > 0).sum() > 200 and (want == 0).sum() > 200
    for base, mem in ROUTES:
        g = G.create_general(d["B"].shape[0], d["L"], d["B"], d["Wt"], dtype, base, mem)
        np.testing.assert_array_equal(g.degrees()[0], np.diff(d["B"].indptr))
        ratio = S.assert_band(g.predict("query"), want, band, f"directed general graph, {np.dtype(dtype).name}")
        WORST[np.dtype(dtype).name] = max(WORST.get(np.dtype(dtype).name, 0.0), ratio)
        g.close()
    print(f"[graph inputs] directed general graph, largest error / band so far: {WORST}")


def test_general_graph_refuses_source_rows_and_leave_one_out():
    d = G.directed_graph()
    g = G.create_general(d["B"].shape[0], d["L"], d["B"], d["Wt"], np.float32, 0, G.HOST)
    for call in (lambda: g.predict("source"), lambda: g.predict_loo()):
        with pytest.raises(ss.SimSpreadError) as e:
            call()
        assert e.value.code == G.SS_EINVAL
    g.close()


# ============================================================================= 4. label CSR of the other constructors
def _other_inputs(kind, dtype):
    rng = np.random.default_rng(61)
    nq, ns, nt = 40, 300, 40
    Y = sp.random(ns, nt - 1, density=0.08, format="csr", random_state=rng)
    Y.data[:] = 1.0
    Y = sp.csr_matrix(sp.hstack([Y, sp.csr_matrix((ns, 1))]))
    Y.sort_indices()
    if kind == "similarity":
        Ss = rng.random((ns, ns))
        Ss = ((Ss + Ss.T) / 2).astype(np.float32).astype(np.float64)
        np.fill_diagonal(Ss, 1.0)
        return rng.random((nq, ns)).astype(np.float32).astype(np.float64), Ss, Y, dict(alpha=0.7)
    if kind == "fingerprint":
        return (ss.pack_fingerprints(rng.random((nq, 200)) < 0.3), ss.pack_fingerprints(rng.random((ns, 200)) < 0.3), Y,
                dict(alpha=0.2))
    if kind == "features":
        return rng.random((nq, 12)).astype(dtype), rng.random((ns, 12)).astype(dtype), Y, dict(alpha=0.5)
    return (rng.standard_normal((nq, 16)).astype(dtype), rng.standard_normal((ns, 16)).astype(dtype), Y,
            dict(alpha=0.2, metric="cosine"))


def _other_make(kind, Fq, Fs, Y, dtype, base, mem, kw):
    import torch
    make = {"similarity": ss.DeviceGraph.from_similarity, "fingerprint": ss.DeviceGraph.from_fingerprints,
            "features": ss.DeviceGraph.from_features, "vectors": ss.DeviceGraph.from_vectors}[kind]
    ptr, idx, val = G.csr_triple(Y, dtype, base)
    labels = (ptr, idx, val, Y.shape[1])
    if mem == G.DEVICE:
        labels = tuple(torch.from_numpy(a).cuda() for a in (ptr, idx, val)) + (Y.shape[1],)
        to = lambda F: None if F is None else torch.from_numpy(
            F.view(np.int64) if kind == "fingerprint" else np.asarray(F, dtype=dtype)).cuda()
        Fq, Fs = to(Fq), to(Fs)
    elif base == 0:
        labels = Y.astype(dtype)
    return make(Fq, Fs, labels, dtype=dtype, index_base=base, **kw)


@pytest.mark.parametrize("kind", ["similarity", "fingerprint", "features", "vectors"])
@pytest.mark.parametrize("dtype", DTYPES, ids=D_IDS)
def test_label_csr_of_the_other_constructors(dtype, kind):
    """1-based labels (the Julia form; host and device) give the 0-based host handle bit for bit: info, degrees,
    predict("query") on the graph with queries, predict_loo(clean=True) on the one without; the dense-similarity
    graph also with ldq, lds larger than the row counts and NaN in the padding."""
    Fq, Fs, Y, kw = _other_inputs(kind, dtype)

    def seen(base, mem, **extra):
        g = _other_make(kind, Fq, Fs, Y, dtype, base, mem, dict(kw, **extra))
        out = [(g.nq, g.ns, g.nf, g.nt, g.nnz_ys), g.degrees(), g.predict("query")]
        g.close()
        g = _other_make(kind, None, Fs, Y, dtype, base, mem, dict(kw, **extra))
        out += [g.degrees(), g.predict_loo(clean=True)]
        g.close()
        return out

    ref = seen(0, G.HOST)
    assert ref[0][4] == Y.nnz and (ref[4] == -99).any() and np.count_nonzero(ref[2]) > 0
    np.testing.assert_array_equal(ref[1][2], np.diff(sp.csc_matrix(Y).indptr))
    variants = [(1, G.HOST, {}), (0, G.DEVICE, {}), (1, G.DEVICE, {})]
    if kind == "similarity":
        variants += [(1, G.HOST, dict(ld_pad=7)), (1, G.DEVICE, dict(ld_pad=7))]
    for base, mem, extra in variants:
        got = seen(base, mem, **extra)
        label = f"{kind} base {base} {M_IDS[mem]} {extra}"
        assert got[0] == ref[0], label
        for a, b in zip(got[1] + got[3], ref[1] + ref[3]):
            np.testing.assert_array_equal(a, b, err_msg=label)
        _same_bits(got[2], ref[2], label + ": query rows")
        _same_bits(got[4], ref[4], label + ": leave-one-out, clean")


# ============================================================================= 5. element-wise ABI
SHAPES = [(1, 1), (63, 5), (64, 64), (65, 3), (257, 129), (1, 1000), (1000, 1)]


def _elementwise_values(rows, cols, dt, alpha, seed):
    """alpha exactly, its two neighbours, 0, -0, negatives, NaN and ordinary values."""
    rng = np.random.default_rng(seed)
    a = dt(alpha)
    special = np.array([a, np.nextafter(a, dt(0)), np.nextafter(a, dt(2)), 0.0, -0.0, -a, -1.5, np.nan, 1.0, 2.5], dtype=dt)
    X = (rng.random((rows, cols)) * 2 - 0.5).astype(dt)
    pick = rng.random((rows, cols)) < 0.6
    X[pick] = special[rng.integers(0, len(special), size=int(pick.sum()))]
    if rows > 2:
        X[2] = 0.0                                       # a row of degree 0
    return X


@pytest.mark.parametrize("mem", MEMS, ids=M_IDS)
@pytest.mark.parametrize("shape", SHAPES, ids=[f"{r}x{c}" for r, c in SHAPES])
@pytest.mark.parametrize("dtype", DTYPES, ids=D_IDS)
def test_elementwise_abi_equals_numpy(dtype, shape, mem):
    """ss_cutoff_*, ss_row_degree_*, ss_spread_* with ld = ldo = rows + 3 and NaN padding: equal to numpy with ==, the
    output's padding untouched.  spread is G / k in the same precision, correctly rounded."""
    dt = np.dtype(dtype).type
    alpha = 0.4375
    X = _elementwise_values(*shape, dt, alpha, 71)
    rows, cols = shape
    for weighted in WEIGHTED:
        got, full = G.elementwise("cutoff", X, dt, mem, alpha=alpha, weighted=weighted)
        with np.errstate(invalid="ignore"):
            want = np.where(X >= dt(alpha), X if weighted else dt(1), dt(0)).astype(dt)
        assert got.dtype == want.dtype and (got == want).all(), f"cutoff weighted={weighted}"
        assert (full[:, rows:] == -7).all(), "cutoff wrote into the padding of its output"
    deg, _ = G.elementwise("row_degree", X, dt, mem)
    k = np.count_nonzero(X, axis=1).astype(np.int64)            # (NaN is non-zero, as in k(G))
    np.testing.assert_array_equal(deg, k)
    got, full = G.elementwise("spread", X, dt, mem)
    with np.errstate(invalid="ignore", divide="ignore"):
        want = np.where(k[:, None] > 0, X / np.maximum(k, 1).astype(dt)[:, None], dt(0)).astype(dt)
    nan = np.isnan(want)
    assert (np.isnan(got) == nan).all() and (got[~nan] == want[~nan]).all(), "spread"
    assert (full[:, rows:] == -7).all(), "spread wrote into the padding of its output"


@pytest.mark.parametrize("dtype", DTYPES, ids=D_IDS)
def test_dense_cutoff_and_csr_cutoff_agree_on_the_non_zeros(dtype):
    dt = np.dtype(dtype).type
    rng = np.random.default_rng(72)
    M = sp.random(65, 129, density=0.3, format="csr", random_state=rng)
    M.data = (1.0 - rng.random(M.nnz)).astype(dt).astype(np.float64)
    M.sort_indices()
    alpha = float(np.sort(M.data)[M.nnz // 2])
    for weighted in WEIGHTED:
        cut = ss.cutoff_csr(M, alpha, weighted=weighted, dtype=dt)
        got, _ = G.elementwise("cutoff", M.toarray(), dt, G.HOST, alpha=alpha, weighted=weighted)
        nz = sp.csr_matrix(got)
        nz.sort_indices()
        assert 0 < nz.nnz < M.nnz and (M.data == alpha).any()
        assert np.array_equal(nz.indptr, cut.indptr) and np.array_equal(nz.indices, cut.indices)
        assert nz.data.dtype == cut.data.dtype and (nz.data == cut.data).all()


# ============================================================================= 6. refusals
def _refusal_block(rows, cols, seed):
    """A plain block: row 1 has 130 entries, the others 3, the last 4 (0-based arrays)."""
    rng = np.random.default_rng(seed)
    n = [3] * rows
    n[1], n[-1] = 130, 4
    idx = np.concatenate([np.sort(rng.choice(cols - 1, k, replace=False)) for k in n]).astype(np.int32)
    ptr = np.concatenate(([0], np.cumsum(n))).astype(np.int64)
    return ptr, idx


def _bad_inputs(ptr, idx, cols, base):
    """name -> (ptr, idx, index_base passed, word of the message); every array in the base the call announces.  The
    entry count ptr[rows] is never changed, so no reader is sent past the arrays."""
    p, i = ptr + base, idx + np.int32(base)
    out = {}
    b = p[1] - base
    j = i.copy(); j[[b + 63, b + 64]] = j[[b + 64, b + 63]]
    out["unsorted pair at 63 / 64 of a 130-entry row"] = (p, j, base, "strictly increasing")
    j = i.copy(); j[-1] = j[-2]
    out["duplicate in the last two entries"] = (p, j, base, "strictly increasing")
    j = i.copy(); j[p[2] - base - 1] = cols + base
    out["index equal to cols (+ base)"] = (p, j, base, "out of range")
    if base == 1:
        j = i.copy(); j[p[3] - base] = 0
        out["index 0 at base 1"] = (p, j, base, "out of range")
    q = p.copy(); q[3] = q[2] - 2
    assert q[3] >= base and q[-1] == p[-1]
    out["pointer that decreases in the middle"] = (q, i, base, "monotone")
    q = p.copy(); q[0] = base + 1
    out["ptr[0] != index_base"] = (q, i, base, "index_base")
    out["index_base = 2"] = (p, i, 2, "index_base must be 0 or 1")
    return out


@pytest.mark.parametrize("dtype", DTYPES, ids=D_IDS)
def test_bad_inputs_are_refused_and_leave_the_library_usable(dtype):
    """Every bad CSR through ss_graph_create_csr_* (in each of the three blocks) and ss_spmat_create_csr_*, host and
    device, base 0 and 1: SS_EINVAL, *out NULL, a message that names the reason; dense ld < rows likewise.  The check
    kernel refuses each of them before any other kernel reads the block.  A correct call afterwards gives the oracle's
    bits."""
    nq, ns, nf, nt = 5, 6, 200, 150
    shapes = [(nq, nf), (ns, nf), (ns, nt)]
    good = [_refusal_block(r, c, 80 + k) for k, (r, c) in enumerate(shapes)]
    lib = ss._lib.lib()
    for base, mem in ROUTES:
        ok = [(p + base, i + np.int32(base), None) for p, i in good]
        rc, h = G.create_csr((nq, ns, nf, nt), *ok, dtype, base, mem)
        assert rc == 0 and h.value
        lib.ss_graph_destroy(h)
        for k, (rows, cols) in enumerate(shapes):
            for name, (p, i, b, word) in _bad_inputs(*good[k], cols, base).items():
                blocks = list(ok)
                blocks[k] = (p, i, None)
                rc, h = G.create_csr((nq, ns, nf, nt), *blocks, dtype, b, mem)
                label = f"{name}, block {k}, base {base}, {M_IDS[mem]}"
                assert rc == G.SS_EINVAL and h.value is None, (label, rc, h.value)
                assert word in G.last_error(), (label, G.last_error())
                if k == 1:
                    rc, h = G.create_spmat((rows, cols), (p, i, None), dtype, b, mem)
                    assert rc == G.SS_EINVAL and h.value is None, ("spmat: " + label, rc, h.value)
                    assert word in G.last_error(), ("spmat: " + label, G.last_error())
    # dense blocks with ld < rows, each block in turn
    ft = C.c_float if np.dtype(dtype) == np.float32 else C.c_double
    fn = getattr(lib, f"ss_graph_create_dense_{'f32' if np.dtype(dtype) == np.float32 else 'f64'}")
    for mem in MEMS:
        buf = G.Buffers(mem)
        ptrs = [buf(np.zeros((c, r), dtype=dtype)) for r, c in shapes]
        buf.ready()
        for k in range(3):
            ld = [nq, ns, ns]
            ld[k] -= 1
            h = C.c_void_p(0xdead)
            rc = fn(nq, ns, nf, nt, ptrs[0], ld[0], ptrs[1], ld[1], ptrs[2], ld[2], 0, ft(0), 1, mem, C.byref(h))
            assert rc == G.SS_EINVAL and h.value is None and "ld < rows" in G.last_error(), (k, mem, rc, G.last_error())
    g = G.graph_csr(*(_case("q64", True)[0][k] for k in ("Xq", "Xs", "Ys")), dtype, 1, G.HOST)
    _check_query_handle(g, "q64", True, dtype, "after the refusals")
