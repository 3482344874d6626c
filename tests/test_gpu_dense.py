"""The dense-similarity regime (from_similarity) element by element, for every stage-1 engine: the 128 x 128 bf16 plane
kernel, the 256 x 256 bf16 ring kernel, the fp32-input MFMA kernel with 128- and 256-row tiles, and the fp64 kernel.

Tier 1: exactly summable weighted inputs.  Every partial sum any order can form is exact in fp32, so the plane engines
        must return float32(oracle) bit for bit and the fp64 engine the oracle itself; each of the six kept plane
        products is visible on its own (tests/test_dense_inputs_cpu.py shows that dropping any one changes the result).
Tier 2: derived element-wise bands, never the block maximum: 4 * 2^-24 of the score for the single-term unweighted
        inputs, (n + 2) * 2^-24 * sum|terms| in general (+ 2^-24 * sum|terms| for the three dropped plane products).
Tier 3: the shapes, row offsets and alignments that choose between vector and scalar loads, paired and single fp64
        accesses, full and partial tiles, and a last tile group that is one block wide.
Tier 4: the input domain: NaN similarities, alpha = 0, alpha < 0, zeros and negative weights, against O.cutoff.

Orientation: element (s, f) of Ss is source s (row) against feature f (column), and Ss need not be symmetric.  Every
tier runs again on dense_ref's symmetric=False inputs: tier 1 with Ss[i, j] != Ss[j, i] inside every block, the bands
on an asymmetric pattern whose row and column degrees differ, the degrees after set_cutoff, and one graph handed over
from numpy, from a CUDA tensor and with a padded leading dimension.  tests/test_dense_inputs_cpu.py shows that every
swap of the two indices (dense_ref.TRANSPOSE_DEFECTS) is invisible on the symmetric inputs and leaves the band on a
tenth or more of the scores of the asymmetric ones.

Every predict call asserts the engine's tag in ss.path_last().  References are computed once per input and shared by the
engines; inputs, bands and assertions live in tests/dense_ref.py."""
import functools

import numpy as np
import pytest
import scipy.sparse as sp

import simspread_jl_amd as ss
from oracle import simspread_oracle as O

import dense_ref as R
from test_gpu_parity import assert_close

pytestmark = pytest.mark.gpu

SWITCHES = ("SS_DENSE_BF16", "SS_DENSE_RING", "SS_DENSE_TILE")
# engine -> (precision, switches, tag of predict / predict_loo, tag of predict_kfold)
# (k-fold in fp32 always runs on the bf16 planes; small blocks take the 128 x 128 kernel unless the ring is forced)
ENGINES = {
    "bf16-128": (np.float32, {"SS_DENSE_RING": "0"}, "transfer_dense_bf16_128", "transfer_dense_bf16_128"),
    "bf16-ring": (np.float32, {"SS_DENSE_RING": "1"}, "transfer_dense_bf16_ring", "transfer_dense_bf16_ring"),
    "fp32-mfma": (np.float32, {"SS_DENSE_BF16": "0"}, "transfer_dense_f32_mfma", "transfer_dense_bf16_128"),
    "fp32-mfma-256": (np.float32, {"SS_DENSE_BF16": "0", "SS_DENSE_TILE": "256"}, "transfer_dense_f32_mfma_256",
                      "transfer_dense_bf16_128"),
    "fp64": (np.float64, {}, "transfer_dense_f64_mfma", "transfer_dense_f64_mfma"),
}
ALL_TAGS = {t for e in ENGINES.values() for t in e[2:]}
WORST = {}      # engine -> largest error / band seen so far (printed, recorded in DESIGN.md section 5)
WORST_ASYM = {}  # the same on the asymmetric inputs


@pytest.fixture(scope="module", autouse=True)
def _init():
    ss.init(0)


@pytest.fixture
def engine(request, monkeypatch):
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)
    dtype, env, tag, tag_kfold = ENGINES[request.param]
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    return dict(name=request.param, dtype=dtype, tag=tag, tag_kfold=tag_kfold, planes=request.param.startswith("bf16"))


def all_engines(fn):
    return pytest.mark.parametrize("engine", list(ENGINES), indirect=True)(fn)


def _tag(want):
    """The last call went through `want` and through no other stage-1 engine."""
    path = ss.path_last()
    assert want in path and not (ALL_TAGS - {want}) & set(path), (want, path)


def _graph(inp, weighted, eng):
    g = ss.DeviceGraph.from_similarity(inp["Sq"], inp["Ss"], sp.csr_matrix(inp["Y"]), alpha=inp["alpha"],
                                       weighted=weighted, dtype=eng["dtype"])
    return g


def _check_degrees(g, X, Y):
    kf, ks, kt = g.degrees()
    okf, oks, okt = O.degrees(sp.csr_matrix(X), sp.csr_matrix(np.asarray(Y, dtype=np.float64)))
    np.testing.assert_array_equal(kf, okf)
    np.testing.assert_array_equal(ks, oks)
    np.testing.assert_array_equal(kt, okt)


def _check_band(eng, got, want, terms, label, weighted, planes=None, worst=None):
    """fp32 engines: element-wise band; fp64: the suite's 1e-12 of the block's largest score."""
    if eng["dtype"] == np.float64:
        assert_close(got, want, np.float64)
        return
    worst = WORST if worst is None else worst
    planes = eng["planes"] if planes is None else planes
    key = eng["name"] if planes == eng["planes"] else eng["name"] + " (k-fold: bf16 planes)"
    ratio = R.assert_band(got, want, R.band_general(*terms, dropped_products=planes and weighted),
                          f"{eng['name']} {label}")
    worst[key] = max(worst.get(key, 0.0), ratio)
    print(f"[dense] worst so far{' (asymmetric inputs)' if worst is WORST_ASYM else ''}: {worst}")


# ----------------------------------------------------------------------------- tier 1
@functools.lru_cache(maxsize=None)
def _exact_case(mode, alpha_edge, symmetric=True):
    inp = R.exact_inputs(mode, alpha_edge=alpha_edge, symmetric=symmetric)
    X, Xq, Y = R.cut(inp["Ss"], inp["alpha"], True), R.cut(inp["Sq"], inp["alpha"], True), inp["Y"]
    ns = X.shape[0]
    if mode == "query":
        want, terms = R.oracle_query(Xq, X, Y), R.terms(Xq, X, Y)
    elif mode == "loo":
        want, terms = O.predict_loo_factored(X, Y.astype(np.float64)), R.terms_loo(X, Y, np.arange(ns))
    else:
        want, terms = R.oracle_folds(X, Y, inp["fold"]), None       # k-fold has no fp32-input engine
    return inp, X, want, terms


@pytest.mark.parametrize("alpha_edge", [False, True], ids=["alpha=0.4", "alpha=lowest-kept"])
@pytest.mark.parametrize("mode", ["query", "loo", "kfold"])
@all_engines
def test_exactly_summable_inputs_bitwise(engine, mode, alpha_edge):
    """Weighted, all six plane products: blocks of sources with power-of-two degrees (dense_ref.exact_inputs), values
    0.5 + 2^-10 + l * 2^-19.  The plane engines (and k-fold, which always runs on them in fp32) equal float32(oracle)
    bit for bit, the fp64 engine equals the oracle bit for bit, the fp32-input engine rounds its 40-bit products and
    gets the general band.  predict("source") is not here: the element of a source's own targets adds the target path's
    0.5 to a feature path below 2^-7 with bits down to 2^-31, which is not representable; it is covered in tier 2."""
    _check_exact(engine, mode, alpha_edge, True)


@pytest.mark.parametrize("alpha_edge", [False, True], ids=["alpha=0.4", "alpha=lowest-kept"])
@pytest.mark.parametrize("mode", ["query", "loo", "kfold"])
@all_engines
def test_asymmetric_exactly_summable_inputs_bitwise(engine, mode, alpha_edge):
    """The same tier with Ss[i, j] != Ss[j, i] for every pair inside a block (exact_inputs(symmetric=False)): an operand
    read as Ss[f, s], or a column-major Ss taken for row-major, changes a bit in every non-zero score row
    (tests/test_dense_inputs_cpu.py)."""
    _check_exact(engine, mode, alpha_edge, False)


def _check_exact(engine, mode, alpha_edge, symmetric):
    inp, X, want, terms = _exact_case(mode, alpha_edge, symmetric)
    g = _graph(inp, True, engine)
    _check_degrees(g, X, inp["Y"])
    if mode == "query":
        got = g.predict("query")
    elif mode == "loo":
        got = g.predict_loo()
    else:
        got = g.predict_kfold(inp["fold"], 9)
    _tag(engine["tag_kfold"] if mode == "kfold" else engine["tag"])
    if engine["dtype"] == np.float64:
        np.testing.assert_array_equal(got, want)
    elif engine["planes"] or mode == "kfold":
        R.assert_bitwise(got, want, f"{engine['name']} {mode}")
    else:
        _check_band(engine, got, want, terms, f"exact inputs, {mode}, weighted", True,
                    worst=WORST if symmetric else WORST_ASYM)
    g.close()


# ----------------------------------------------------------------------------- tier 2: one term per score
@functools.lru_cache(maxsize=None)
def _single_case(symmetric=True):
    inp = R.single_feature_inputs(symmetric=symmetric)
    X, Xq = R.cut(inp["Ss"], inp["alpha"], False), R.cut(inp["Sq"], inp["alpha"], False)
    return inp, X, R.oracle_query(Xq, X, inp["Y"])


@all_engines
def test_single_term_scores_within_three_roundings(engine):
    """Unweighted, one feature per query row, one source per target: a score is fl(1/kf) (summed exactly from its
    three planes) times fl(1/ks).  Three roundings against the fp64 oracle: 4 * 2^-24 of the score, element-wise.  A
    kernel without the lo plane of the query side misses this on 73 % of the non-zero scores
    (tests/test_dense_inputs_cpu.py)."""
    _check_single(engine, True)


@all_engines
def test_asymmetric_single_term_scores_within_three_roundings(engine):
    """The same on an iid pattern: kf is a column count and ks a row count, and they differ for nearly every node."""
    _check_single(engine, False)


def _check_single(engine, symmetric):
    inp, X, want = _single_case(symmetric)
    g = _graph(inp, False, engine)
    _check_degrees(g, X, inp["Y"])
    got = g.predict("query")
    _tag(engine["tag"])
    if engine["dtype"] == np.float64:
        assert_close(got, want, np.float64)
    else:
        ratio = R.assert_band(got, want, R.band_single_term(want), f"{engine['name']} single term")
        (WORST if symmetric else WORST_ASYM)[engine["name"] + " (single term)"] = ratio
    g.close()


# ----------------------------------------------------------------------------- tiers 2 and 3: shapes, offsets, every mode
SHAPES = [(129, 256), (256, 260), (200, 130), (37, 321), (300, 2176)]
KFOLD_MAX_NS = 400       # k-fold references cost nfolds products of ns^2: small shapes only


@functools.lru_cache(maxsize=None)
def _random_case(nq, ns, weighted):
    """mode -> (inputs, thresholded Ss, references and terms).  Unweighted: the same inputs for every mode."""
    out = {}
    for mode in ("query", "loo", "kfold"):
        if mode == "kfold" and ns > KFOLD_MAX_NS:
            continue
        inp = R.random_inputs(nq, ns, weighted, mode)
        X, Xq, Y = R.cut(inp["Ss"], inp["alpha"], weighted), R.cut(inp["Sq"], inp["alpha"], weighted), inp["Y"]
        ref = {}
        Xcsr = sp.csr_matrix(X)
        if mode == "query":
            ref["query"] = (R.oracle_query(Xq, Xcsr, Y), R.terms(Xq, X, Y))
        for a, b in R.row_ranges(ns):
            rows = np.arange(a, b)
            if mode == "query":
                ref["source", a, b] = (R.oracle_source(X, Y, rows, Xcsr), R.terms_source(X, Y, rows))
            elif mode == "loo":
                ref["loo", a, b] = (O.predict_loo_dense_blocked(X, Y.astype(np.float64), queries=rows),
                                    R.terms_loo(X, Y, rows))
        if mode == "kfold":
            ref["kfold"] = (R.oracle_folds(X, Y, inp["fold"]), R.terms_folds(X, Y, inp["fold"]))
        out[mode] = (inp, X, ref)
    return out


@pytest.mark.parametrize("weighted", [False, True], ids=["unweighted", "weighted"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
@all_engines
def test_shapes_offsets_and_modes_within_their_bands(engine, shape, weighted):
    """Query rows, source rows and leave-one-out rows over ranges with begin % 4 in {0, 1, 2, 3}, lengths 3, 128, 129
    and one ending with the last row (one of them column-major), k-fold at the small shapes.  Between them: float4 loads
    of both operands of the fp32-input kernel taken (lda % 4 == 0, begin % 4 == 0, four rows left) and refused for each
    reason; the 16-byte pair loads of the fp64 kernel taken (full tile, even begin, even ld) and refused for each
    reason; K padded 260 -> 320 for the planes; M one past a tile; at ns = 2176 the last tile group is one block wide
    in every kernel (17 = 16 + 1 blocks of 128, 9 = 8 + 1 of 256) with two or three row blocks.
    Element-wise band (n + 2) * 2^-24 * sum|terms| (dense_ref.band_general; weighted inputs come per mode so that the
    feature scaling is exact and the band is the fp32-input engine's worst case, see dense_ref.random_inputs)."""
    nq, ns = shape
    w = "weighted" if weighted else "unweighted"
    g = None
    for mode, (inp, X, ref) in _random_case(nq, ns, weighted).items():
        if g is None or weighted:
            if g is not None:
                g.close()
            g = _graph(inp, weighted, engine)
            _check_degrees(g, X, inp["Y"])
        if mode == "query":
            got = g.predict("query")
            _tag(engine["tag"])
            _check_band(engine, got, *ref["query"], f"{shape} query, {w}", weighted)
        if mode == "kfold":
            got = g.predict_kfold(inp["fold"], inp["nfolds"])
            _tag(engine["tag_kfold"])
            _check_band(engine, got, *ref["kfold"], f"{shape} k-fold, {w}", weighted, planes=engine["dtype"] == np.float32)
            continue
        for i, (a, b) in enumerate(R.row_ranges(ns)):
            layout = "col" if i == 1 else "row"
            if mode == "query":
                got = g.predict("source", a, b, layout=layout)
                _tag(engine["tag"])
                _check_band(engine, got, *ref["source", a, b], f"{shape} source rows [{a},{b}), {w}", weighted)
            else:
                got = g.predict_loo(a, b, layout=layout)
                _tag(engine["tag"])
                _check_band(engine, got, *ref["loo", a, b], f"{shape} leave-one-out rows [{a},{b}), {w}", weighted)
    g.close()


# ----------------------------------------------------------------------------- an asymmetric Ss: degrees, bands, layout
ASYM_SHAPE = (129, 260)         # K padded 260 -> 320 for the planes, M one past a tile, three partial 128-blocks


@functools.lru_cache(maxsize=None)
def _asym_case(weighted):
    """mode -> (inputs, thresholded Ss, references and terms) on random_inputs(symmetric=False)."""
    nq, ns = ASYM_SHAPE
    out = {}
    for mode in ("query", "loo", "kfold"):
        inp = R.random_inputs(nq, ns, weighted, mode, symmetric=False)
        X, Xq, Y = R.cut(inp["Ss"], inp["alpha"], weighted), R.cut(inp["Sq"], inp["alpha"], weighted), inp["Y"]
        assert ((X != 0) & (X.T == 0)).sum() > ns and (np.count_nonzero(X, axis=0) != np.count_nonzero(X, axis=1)).any()
        Y64 = Y.astype(np.float64)
        ref = {}
        if mode == "query":
            ref["query"] = (R.oracle_query(Xq, X, Y), R.terms(Xq, X, Y))
        for a, b in R.row_ranges(ns):
            rows = np.arange(a, b)
            if mode == "query":
                ref["source", a, b] = (R.oracle_source(X, Y, rows), R.terms_source(X, Y, rows))
            elif mode == "loo":
                ref["loo", a, b] = (O.predict_loo_factored(X, Y64, queries=rows),
                                    O.predict_loo_factored(X, Y64, clean_flag=True, queries=rows), R.terms_loo(X, Y, rows))
        if mode == "kfold":
            ref["kfold"] = (R.oracle_folds(X, Y, inp["fold"]), R.terms_folds(X, Y, inp["fold"]))
        out[mode] = (inp, X, ref)
    return out


@pytest.mark.parametrize("weighted", [False, True], ids=["unweighted", "weighted"])
@all_engines
def test_asymmetric_degrees_at_every_cutoff(engine, weighted):
    """kf counts a column of the thresholded Ss and ks a row (plus the labels), at construction and after set_cutoff to
    a higher and to a lower alpha; on these inputs the two counts differ for most nodes."""
    inp, X, _ = _asym_case(weighted)["query"]
    g = _graph(inp, weighted, engine)
    _check_degrees(g, X, inp["Y"])
    for alpha in (inp["alpha"] + 0.5 * (1.0 - inp["alpha"]), 0.6 * inp["alpha"], inp["alpha"]):
        Xa = R.cut(inp["Ss"], alpha, weighted)
        assert (np.count_nonzero(Xa, axis=0) != np.count_nonzero(Xa, axis=1)).mean() > 0.25
        _check_degrees(g.set_cutoff(alpha, weighted), Xa, inp["Y"])
    g.close()


@pytest.mark.parametrize("weighted", [False, True], ids=["unweighted", "weighted"])
@all_engines
def test_asymmetric_inputs_every_mode_within_its_band(engine, weighted):
    """Query rows, source rows and leave-one-out rows (with and without clean) over dense_ref.row_ranges, the whole
    k-fold and a sub-range of its rows, on random_inputs(symmetric=False): an asymmetric pattern, row degrees unlike
    column degrees, a leave-one-out divisor ks - has that depends on the direction of the pair.  References:
    oracle_query, oracle_source, O.predict_loo_factored, oracle_folds; the band of the symmetric tier."""
    nq, ns = ASYM_SHAPE
    w = "asymmetric, " + ("weighted" if weighted else "unweighted")
    check = functools.partial(_check_band, engine, weighted=weighted, worst=WORST_ASYM)
    g = None
    for mode, (inp, X, ref) in _asym_case(weighted).items():
        if g is None or weighted:
            if g is not None:
                g.close()
            g = _graph(inp, weighted, engine)
            _check_degrees(g, X, inp["Y"])
        if mode == "query":
            got = g.predict("query")
            _tag(engine["tag"])
            check(got, *ref["query"], label=f"query, {w}")
        if mode == "kfold":
            fold, k = inp["fold"], inp["nfolds"]
            got = g.predict_kfold(fold, k)
            _tag(engine["tag_kfold"])
            check(got, *ref["kfold"], label=f"k-fold, {w}", planes=engine["dtype"] == np.float32)
            a, b = R.row_ranges(ns)[1]
            part = g.predict_kfold_rows(fold, k, a, b)
            _tag(engine["tag_kfold"])
            check(part, ref["kfold"][0][a:b], tuple(t[a:b] for t in ref["kfold"][1]), label=f"k-fold rows [{a},{b}), {w}",
                  planes=engine["dtype"] == np.float32)
            continue
        for i, (a, b) in enumerate(R.row_ranges(ns)):
            layout = "col" if i == 1 else "row"
            if mode == "query":
                got = g.predict("source", a, b, layout=layout)
                _tag(engine["tag"])
                check(got, *ref["source", a, b], label=f"source rows [{a},{b}), {w}")
            else:
                want, want_clean, terms = ref["loo", a, b]
                got = g.predict_loo(a, b, layout=layout)
                _tag(engine["tag"])
                check(got, want, terms, label=f"leave-one-out rows [{a},{b}), {w}")
                got = g.predict_loo(a, b, clean=True, layout=layout)
                _tag(engine["tag"])
                assert np.array_equal(got == -99.0, want_clean == -99.0) and (want_clean == -99.0).any()
                check(got, want_clean, terms, label=f"leave-one-out rows [{a},{b}) with clean, {w}")
    g.close()


@pytest.mark.parametrize("weighted", [False, True], ids=["unweighted", "weighted"])
@all_engines
def test_asymmetric_graph_is_the_same_from_every_layout(engine, weighted):
    """One asymmetric graph from a numpy array and from a CUDA tensor, each with ld_pad 0 and 3 (NaN under the last
    row): the query rows and the leave-one-out rows of the four are bitwise equal, and inside their band, so no path
    hands Ss over transposed."""
    import torch
    case = _asym_case(weighted)
    inp, X, ref = case["query"]
    a, b = R.row_ranges(ASYM_SHAPE[1])[1]
    Ycsr = sp.csr_matrix(inp["Y"])
    tdt = torch.float32 if engine["dtype"] == np.float32 else torch.float64
    Yd = (torch.from_numpy(Ycsr.indptr.astype(np.int64)).cuda(), torch.from_numpy(Ycsr.indices.astype(np.int32)).cuda(),
          torch.from_numpy(Ycsr.data).cuda().to(tdt), Ycsr.shape[1])
    first = None
    for device in (False, True):
        for ld_pad in (0, 3):
            if device:
                Sq, Ss, Y = torch.from_numpy(inp["Sq"]).cuda(), torch.from_numpy(inp["Ss"]).cuda(), Yd
            else:
                Sq, Ss, Y = inp["Sq"], inp["Ss"], Ycsr
            g = ss.DeviceGraph.from_similarity(Sq, Ss, Y, alpha=inp["alpha"], weighted=weighted, dtype=engine["dtype"],
                                               ld_pad=ld_pad)
            _check_degrees(g, X, inp["Y"])
            q = g.predict("query")
            _tag(engine["tag"])
            loo = g.predict_loo(a, b, clean=True)
            _tag(engine["tag"])
            g.close()
            if first is None:
                first = (q, loo)
                _check_band(engine, q, *ref["query"], "query, asymmetric, " + ("weighted" if weighted else "unweighted"),
                            weighted, worst=WORST_ASYM)
                assert not np.isnan(loo).any() and (loo == -99.0).any()
            else:
                assert q.tobytes() == first[0].tobytes(), (device, ld_pad)
                assert loo.tobytes() == first[1].tobytes(), (device, ld_pad)


# ----------------------------------------------------------------------------- tier 4: the input domain
@functools.lru_cache(maxsize=None)
def _domain_case(alpha, weighted):
    rng = np.random.default_rng(404)
    nq, ns, nt = 37, 130, 24
    Ss = R._sym((rng.random((ns, ns)) * 1.5 - 0.5).astype(np.float32))      # U(-0.5, 1): negatives on both sides of alpha
    Sq = (rng.random((nq, ns)) * 1.5 - 0.5).astype(np.float32)
    for S, sym in ((Ss, True), (Sq, False)):
        for val in (np.nan, 0.0, -0.0):
            i, j = rng.integers(0, S.shape[0], 60), rng.integers(0, ns, 60)
            S[i, j] = val
            if sym:
                S[j, i] = val
    Ss[5, 5] = np.nan          # a source whose own feature is no edge
    Ss[3, 7] = Ss[7, 3] = alpha
    Y = (rng.random((ns, nt)) < 0.08).astype(np.float32)
    inp = dict(Sq=Sq, Ss=Ss, Y=Y, alpha=float(np.float32(alpha)))
    X, Xq = R.cut(Ss, alpha, weighted), R.cut(Sq, alpha, weighted)
    assert not np.isnan(X).any() and not np.isnan(Xq).any()                  # O.cutoff: NaN >= alpha is false
    Y64 = Y.astype(np.float64)
    fold = (np.arange(ns) % 3).astype(np.int32)
    want = dict(query=R.oracle_query(Xq, X, Y), loo=O.predict_loo_factored(X, Y64, clean_flag=True),
                source=O.predict_factored(None, X, sp.csr_matrix(Y64), rows="source"), kfold=R.oracle_folds(X, Y, fold))
    return inp, X, fold, want


@pytest.mark.parametrize("weighted", [False, True], ids=["unweighted", "weighted"])
@pytest.mark.parametrize("alpha", [0.3, 0.0, -0.25])
@all_engines
def test_input_domain_follows_the_cutoff_rule(engine, alpha, weighted):
    """x >= alpha ? (weighted ? x : 1) : 0 and "an edge is a non-zero", whatever the engine: a NaN similarity is no
    edge anywhere (degrees, scores, the leave-one-out has-test); with alpha <= 0 and unweighted every finite entry is
    an edge, exact zeros and negatives included, and what the kernels pad beyond ns stays zero; weighted, an exact
    zero (of either sign) is no edge and negative weights keep their sign through the planes.  +-Inf and values near
    FLT_MAX are outside the supported domain (include/simspread_hip.h)."""
    inp, X, fold, want = _domain_case(alpha, weighted)
    g = _graph(inp, weighted, engine)
    _check_degrees(g, X, inp["Y"])
    dt = engine["dtype"]
    assert_close(g.predict("query"), want["query"], dt)
    _tag(engine["tag"])
    assert_close(g.predict_loo(clean=True), want["loo"], dt)
    _tag(engine["tag"])
    assert_close(g.predict("source"), want["source"], dt)
    _tag(engine["tag"])
    assert_close(g.predict_kfold(fold, 3), want["kfold"], dt)
    _tag(engine["tag_kfold"])
    g.close()
    # the same cutoff reached in place from another one (ss_graph_set_cutoff_*): same degrees, same scores
    g = _graph(dict(inp, alpha=0.7), not weighted, engine).set_cutoff(inp["alpha"], weighted)
    _check_degrees(g, X, inp["Y"])
    assert_close(g.predict("query"), want["query"], dt)
    _tag(engine["tag"])
    assert_close(g.predict_loo(clean=True), want["loo"], dt)
    g.close()
