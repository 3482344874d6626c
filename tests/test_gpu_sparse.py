"""The sparse regime element by element: both stages of predict / predict_loo / predict_kfold on CSR graphs, and every
route of the raw W*R product, under every kernel and switch the library has.

Exact:  exactly summable inputs (tests/sparse_ref.py; tests/test_sparse_inputs_cpu.py proves the property): every
        partial sum in any order is representable, so every kernel, chunking and summation order returns the oracle
        rounded to the precision, bit for bit.  Degrees are equal and the -99 of clean! sit where the oracle's do.
Bands:  ordinary inputs with arbitrary degrees; every score within gamma(k) of the fp64 oracle, k counted from the
        kernels (sparse_ref.band_graph_scores, band_spmm), never relative to a block maximum; structural zeros exact.

Operands are built once per handle and read their switches then: every switch setting gets a fresh handle.  Every call
asserts in ss.path_last() that the intended kernel ran.  The fixed-point stage-1 variants (FIX, FIX1, QFLAT, WIDE,
WIDE2) scale per row and are not exact on these inputs; test_gpu_parity.py keeps their oracle test."""
import functools

import numpy as np
import pytest
import scipy.sparse as sp

import simspread_jl_amd as ss
from oracle import simspread_oracle as O

import sparse_ref as S

pytestmark = pytest.mark.gpu

SWITCHES = ("SS_TRANSFER_CHUNK", "SS_TRANSFER_ORDER", "SS_TRANSFER_U", "SS_TRANSFER_DUAL", "SS_CHUNK_SCHED",
            "SS_TRANSFER_BYTES", "SS_TRANSFER_V", "SS_TRANSFER_FIX", "SS_TRANSFER_FIX1", "SS_TRANSFER_LD",
            "SS_TRANSFER_ALIGN", "SS_TRANSFER_NW", "SS_TRANSFER_WIDE", "SS_TRANSFER_WIDE2", "SS_TRANSFER_QFLAT",
            "SS_SELL_CHUNK", "SS_SELL_QT", "SS_SELL_SORT", "SS_SELL_LMAX", "SS_SELL_PLAIN", "SS_NARROW_CHUNK",
            "SS_CSELL", "SS_CSELL_ROW16", "SS_CSELL_ROW32", "SS_CSELL_B12", "SS_CSELL_CUT", "SS_COL", "SS_COL_CG",
            "SS_COL_FROM")
FIXED_POINT_TAGS = {"fixed_point", "wide", "wide2", "qflat"}

# stage 1: name -> (switches, number of chunks asked for (None: the library's choice), stage-1 tags of a call that is
#                   not leave-one-out, applies to leave-one-out, fp32 only)
STAGE1 = {
    "default": ({}, None, ("transfer",), True, False),
    "8 chunks": ({}, 8, ("transfer",), True, False),
    "16 chunks": ({}, 16, ("transfer",), True, False),                         # launch order by groups of 8 chunks
    "16 chunks, interleaved": ({"SS_TRANSFER_ORDER": "0"}, 16, ("transfer",), True, False),
    "U=4": ({"SS_TRANSFER_U": "4"}, 8, ("transfer",), True, False),
    "U=16": ({"SS_TRANSFER_U": "16"}, 8, ("transfer",), True, False),
    "dual": ({"SS_TRANSFER_DUAL": "1"}, 8, ("transfer",), True, False),
    "unscheduled": ({"SS_CHUNK_SCHED": "0"}, 8, ("transfer",), True, False),
    # rows of T held at once: the fold sweeps and the source rows of the band graph take two or three batches here; query
    # rows get their three batches in test_query_rows_exact_in_three_transfer_batches
    "transfer batches": ({"SS_TRANSFER_BYTES": str(1 << 20)}, None, ("transfer",), True, False),
    # the opt-in kernels that sum in floating point: query-block workgroups (query rows only), buffer loads (fp32)
    "block kernel": ({"SS_TRANSFER_V": "2", "SS_TRANSFER_FIX": "0"}, 8, ("transfer_block",), False, False),
    "buffer loads": ({"SS_TRANSFER_V": "1", "SS_TRANSFER_LD": "1"}, 8, ("transfer", "buffer_loads"), False, True),
}
STAGE1_TAGS = {"transfer", "transfer_loo", "transfer_block", "buffer_loads"}
# stage 2: name -> (switches, labels of the exact query inputs, tag)
STAGE2 = {
    "default": ({}, "random", "spmm_sell"),
    "SELL chunk 64": ({"SS_SELL_CHUNK": "64"}, "random", "spmm_sell"),
    "SELL chunk 128": ({"SS_SELL_CHUNK": "128"}, "random", "spmm_sell"),
    "QT=8": ({"SS_SELL_QT": "8"}, "random", "spmm_sell"),
    "sorted": ({"SS_SELL_SORT": "1", "SS_SELL_LMAX": "256"}, "hub", "spmm_sell_sorted"),
    # the length-sorted operand over several batches of T: the scratch rows, the packed rows and the row maps of the
    # stage-2 step together (the batches are counted in _assert_batches; 2^20 is the library's floor)
    "sorted, transfer batches": ({"SS_SELL_SORT": "1", "SS_SELL_LMAX": "256", "SS_TRANSFER_BYTES": str(1 << 20)}, "hub",
                                 "spmm_sell_sorted"),
}
DTYPES = [np.float32, np.float64]


def _params(switch_list):
    """(dtype, kind, name) for every switch of the list in both precisions, fp32-only kernels in fp32 only."""
    out = []
    for dt in DTYPES:
        for kind, name in switch_list:
            if kind == "stage1" and STAGE1[name][4] and dt is np.float64:
                continue
            out.append(pytest.param(dt, kind, name, id=f"{np.dtype(dt).name}-{name}"))
    return out


WEIGHTED = [True, False]
W_IDS = ["weighted", "pattern-only"]
WORST = {}       # (kernel or route, mode, precision) -> largest error / band seen (printed)


@pytest.fixture(scope="module", autouse=True)
def _init():
    ss.init(0)


@pytest.fixture
def switches(monkeypatch):
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)

    def set_(env):
        for k, v in env.items():
            monkeypatch.setenv(k, v)
    return set_


def _stage1_env(name, family):
    env, nch, tags, loo_ok, f32_only = STAGE1[name]
    env = dict(env)
    if nch is not None:
        env["SS_TRANSFER_CHUNK"] = str(S.CHUNK_ENV[family][nch])
    return env, tags


def _tags(stage1, stage2="spmm_sell", loo=False):
    """The last call went through exactly these stage-1 kernels and this stage-2 kernel, and through no fixed-point one."""
    want = {"transfer_loo"} if loo else set(stage1)
    path = set(ss.path_last())
    assert path & STAGE1_TAGS == want, (want, path)
    assert stage2 is None or path & {"spmm_sell", "spmm_sell_sorted"} == {stage2}, (stage2, path)
    assert not (FIXED_POINT_TAGS & path), path


def _batches(env, nrows, ns, dtype):
    """Transfer batches nrows rows take: rb = max(8, (bytes / (ns * itemsize)) & ~7) rows each, one without the switch."""
    if "SS_TRANSFER_BYTES" not in env:
        return 1
    rb = S.transfer_batch_rows(nrows, ns, np.dtype(dtype).itemsize, int(env["SS_TRANSFER_BYTES"]))
    return -(-nrows // rb)


def _graph(Xq, Xs, Ys, dtype):
    return ss.DeviceGraph.from_sparse(None if Xq is None else Xq.astype(dtype), Xs.astype(dtype), Ys.astype(dtype),
                                      dtype=dtype)


def _check_degrees(g, Xs, Ys):
    for got, want in zip(g.degrees(), O.degrees(Xs, Ys)):
        np.testing.assert_array_equal(got, want)


def _cleaned(want, mask):
    out = want.copy()
    out[np.broadcast_to(mask, out.shape)] = -99.0
    return out


# ----------------------------------------------------------------------------- exact inputs: query rows
@functools.lru_cache(maxsize=None)
def _query_case(elem, chunk, weighted, labels="random", nq=70):
    inp = S.exact_query_for(elem, chunk, weighted=weighted, labels=labels, nq=nq)
    want = S.oracle_query(inp["Xq"], inp["Xs"], inp["Ys"])
    want.setflags(write=False)
    return inp, want


RANGES = [(1, 2), (5, 8), (9, 13), (13, 18), (17, 26)]       # begin % 8 in {1, 5}, lengths 1, 3, 4, 5, 9


def _check_query_exact(g, inp, want, dtype, tags, stage2, label, ranges=True):
    _check_degrees(g, inp["Xs"], inp["Ys"])
    S.assert_bitwise(g.predict("query"), want, dtype, f"{label}, all rows")
    _tags(tags, stage2)
    got = g.predict("query", clean=True)
    S.assert_bitwise(got, _cleaned(want, S.clean_mask(inp["Ys"])), dtype, f"{label}, clean")
    assert (got == -99).any()
    if not ranges:
        return
    for a, b in RANGES:
        S.assert_bitwise(g.predict("query", a, b), want[a:b], dtype, f"{label}, rows [{a},{b})")
        _tags(tags, stage2)
    a, b = RANGES[-1]
    got = g.predict("query", a, b, layout="col")
    assert got.shape == (b - a, want.shape[1]) and got.flags.f_contiguous
    S.assert_bitwise(np.ascontiguousarray(got), want[a:b], dtype, f"{label}, column-major")


@pytest.mark.parametrize("weighted", WEIGHTED, ids=W_IDS)
@pytest.mark.parametrize("dtype,kind,name", _params([("stage1", n) for n in STAGE1]))
def test_query_rows_exact_under_every_stage1_switch(dtype, kind, name, weighted, switches):
    """predict("query") on the exact inputs planted for the chunk width in force: all rows, with clean!, five sub-ranges
    and a column-major one equal the oracle's bits."""
    env, tags = _stage1_env(name, "query")
    switches(env)
    chunk = int(env["SS_TRANSFER_CHUNK"]) if "SS_TRANSFER_CHUNK" in env else None
    inp, want = _query_case(np.dtype(dtype).itemsize, chunk, weighted)
    g = _graph(inp["Xq"], inp["Xs"], inp["Ys"], dtype)
    _check_query_exact(g, inp, want, dtype, tags, "spmm_sell", f"query, {name}")
    g.close()


@pytest.mark.parametrize("weighted", WEIGHTED, ids=W_IDS)
@pytest.mark.parametrize("dtype,kind,name", _params([("stage1", n) for n in STAGE1]))
def test_stage1_alone_exact_under_every_stage1_switch(dtype, kind, name, weighted, switches):
    """One private target per source: score column s is the transfer element T[q][s] itself, compared with
    O.transfer_factored.  A stage-2 defect can neither mask nor mimic a stage-1 one here."""
    env, tags = _stage1_env(name, "query")
    switches(env)
    chunk = int(env["SS_TRANSFER_CHUNK"]) if "SS_TRANSFER_CHUNK" in env else None
    inp, want = _query_case(np.dtype(dtype).itemsize, chunk, weighted, "private")
    ns = inp["Xs"].shape[0]
    T = S.oracle_transfer(inp["Xq"], inp["Xs"], inp["Ys"])
    g = _graph(inp["Xq"], inp["Xs"], inp["Ys"], dtype)
    got = g.predict("query")
    _tags(tags, None)    # (stage 2 only copies here; the builder's own skew test sorts these labels by length)
    S.assert_bitwise(np.ascontiguousarray(got[:, :ns]), T, dtype, f"T, {name}")
    S.assert_bitwise(got, want, dtype, f"T and the padding targets, {name}")
    g.close()


@pytest.mark.parametrize("name", list(STAGE2))
@pytest.mark.parametrize("weighted", WEIGHTED, ids=W_IDS)
@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f64"])
def test_query_rows_exact_under_every_stage2_switch(dtype, weighted, name, switches):
    """Several SELL chunks (F re-read per chunk), 32-byte tile rows, and the length-sorted operand with a target that
    nearly every source has (split at SS_SELL_LMAX = 256 into a dozen parts that unpermute adds)."""
    env, labels, tag = STAGE2[name]
    switches(env)
    inp, want = _query_case(np.dtype(dtype).itemsize, None, weighted, labels)
    g = _graph(inp["Xq"], inp["Xs"], inp["Ys"], dtype)
    _check_query_exact(g, inp, want, dtype, ("transfer",), tag, f"query, {name}")
    g.close()


@pytest.mark.parametrize("weighted", WEIGHTED, ids=W_IDS)
@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f64"])
def test_query_rows_exact_in_three_transfer_batches(dtype, weighted, switches):
    """SS_TRANSFER_BYTES = 2^20 at 3000 sources: 170 rows go through stage 1 and 2 in batches of 80 (fp32) or 40."""
    switches({"SS_TRANSFER_BYTES": str(1 << 20)})
    elem = np.dtype(dtype).itemsize
    inp, want = _query_case(elem, None, weighted, "random", 170)
    assert -(-170 // S.transfer_batch_rows(170, inp["Xs"].shape[0], elem, 1 << 20)) >= 3
    g = _graph(inp["Xq"], inp["Xs"], inp["Ys"], dtype)
    _check_query_exact(g, inp, want, dtype, ("transfer",), "spmm_sell", "query, three batches", ranges=False)
    S.assert_bitwise(g.predict("query", 77, 170), want[77:170], dtype, "query, rows [77,170)")
    g.close()


# ----------------------------------------------------------------------------- exact inputs: leave-one-out, k-fold
FOLD_SWITCHES = [("stage1", n) for n in STAGE1] + [("stage2", n) for n in STAGE2 if n != "default"]


def _fold_env(kind, name, family):
    if kind == "stage1":
        env, tags = _stage1_env(name, family)
        return env, tags, "spmm_sell"
    return dict(STAGE2[name][0]), ("transfer",), STAGE2[name][2]


@functools.lru_cache(maxsize=None)
def _loo_case(weighted):
    inp = S.exact_loo(weighted)
    want = S.oracle_loo(inp["X"], inp["Y"])
    want.setflags(write=False)
    return inp, want


@pytest.mark.parametrize("weighted", WEIGHTED, ids=W_IDS)
@pytest.mark.parametrize("dtype,kind,name", _params([s for s in FOLD_SWITCHES if s[0] == "stage2" or STAGE1[s[1]][3]]))
def test_leave_one_out_exact_under_every_switch(dtype, kind, name, weighted, switches):
    """predict_loo on blocks of 2^j + 1 sources: whole, with clean!, a sub-range and a column-major one.  Under
    SS_TRANSFER_BYTES = 2^20 the 488 rows take two batches of 264 in fp64 and one of 488 in fp32 (536 would fit); the
    band graph's 608 rows take at least two in both precisions, asserted there."""
    env, tags, stage2 = _fold_env(kind, name, "loo")
    switches(env)
    inp, want = _loo_case(weighted)
    X, Y = inp["X"], inp["Y"]
    g = _graph(None, X, Y, dtype)
    _check_degrees(g, X, Y)
    S.assert_bitwise(g.predict_loo(), want, dtype, f"leave-one-out, {name}")
    _tags(tags, stage2, loo=True)
    got = g.predict_loo(clean=True)
    mask = S.clean_mask(Y, np.arange(X.shape[0]))
    S.assert_bitwise(got, _cleaned(want, mask), dtype, f"leave-one-out, clean, {name}")
    np.testing.assert_array_equal(got == -99, mask)
    S.assert_bitwise(g.predict_loo(61, 70), want[61:70], dtype, f"leave-one-out rows [61,70), {name}")
    S.assert_bitwise(np.ascontiguousarray(g.predict_loo(125, 134, layout="col")), want[125:134], dtype,
                     f"leave-one-out rows [125,134), column-major, {name}")
    g.close()


@functools.lru_cache(maxsize=None)
def _kfold_case(weighted):
    inp = S.exact_kfold(weighted)
    want = S.oracle_kfold(inp["X"], inp["Y"], inp["fold"])
    want.setflags(write=False)
    return inp, want


@pytest.mark.parametrize("weighted", WEIGHTED, ids=W_IDS)
@pytest.mark.parametrize("dtype,kind,name", _params([s for s in FOLD_SWITCHES if s[1] != "block kernel"]))
def test_kfold_exact_under_every_switch(dtype, kind, name, weighted, switches):
    """predict_kfold and predict_kfold_rows (a sub-range, one column-major) on blocks of 36 = 9 folds x 4.  A fold has
    28 members and SS_TRANSFER_BYTES cannot go below 2^20, which holds 520 (fp64) or 1040 (fp32) rows of 252 sources:
    no fold of these inputs, nor of the band graph's five (122 members, 208 or 424 rows), takes a second batch.  Several
    batches are asserted for the leave-one-out sweep and the source rows of the band graph, and
    test_kfold_of_one_large_fold_in_several_sorted_batches gives the band graph a fold that needs them."""
    env, tags, stage2 = _fold_env(kind, name, "kfold")
    switches(env)
    inp, want = _kfold_case(weighted)
    X, Y, fold = inp["X"], inp["Y"], inp["fold"]
    g = _graph(None, X, Y, dtype)
    _check_degrees(g, X, Y)
    S.assert_bitwise(g.predict_kfold(fold, inp["nfolds"]), want, dtype, f"k-fold, {name}")
    _tags(tags, stage2)
    S.assert_bitwise(g.predict_kfold_rows(fold, inp["nfolds"]), want, dtype, f"k-fold rows, all, {name}")
    _tags(tags, stage2)
    S.assert_bitwise(g.predict_kfold_rows(fold, inp["nfolds"], 29, 70), want[29:70], dtype, f"k-fold rows [29,70), {name}")
    got = g.predict_kfold_rows(fold, inp["nfolds"], 5, 18, layout="col")
    S.assert_bitwise(np.ascontiguousarray(got), want[5:18], dtype, f"k-fold rows [5,18), column-major, {name}")
    got = g.predict_kfold(fold, inp["nfolds"], clean=True)
    assert ((got == -99) == np.broadcast_to(S.clean_mask(Y), got.shape)).all()      # 28 members never empty a target
    g.close()


# ----------------------------------------------------------------------------- raw W @ R
SPMM_B = (1, 2, 3, 4, 5, 8, 9, 16, 17, 32, 33, 64, 65)
SPMM_CHUNK = 500
# route -> (switches, the tag the route is named after)
ROUTES = {
    "narrow": ({"SS_CSELL_ROW16": "0", "SS_CSELL_B12": "0"}, "spmm_chunked_narrow"),
    "lane-per-row": ({}, "spmm_csell"),
    "lane-per-row, cut 3,1": ({"SS_CSELL_CUT": "3,1"}, "spmm_csell"),
    "lane-per-row, cut 1,6": ({"SS_CSELL_CUT": "1,6"}, "spmm_csell"),
    "2-D, one column group": ({"SS_CSELL": "0", "SS_COL_CG": "1"}, "spmm_colgroup"),
    "2-D, three column groups": ({"SS_CSELL": "0", "SS_COL_CG": "3"}, "spmm_colgroup"),
    "SELL": ({"SS_COL": "0", "SS_SELL_CHUNK": str(SPMM_CHUNK)}, "spmm_sell"),
}


def _route(B, dtype, binary, colmajor, env):
    """The routing of ss_spmm (api.hip) restated: which kernel serves this width."""
    elem = np.dtype(dtype).itemsize
    csell = env.get("SS_CSELL") != "0"
    if not colmajor:
        if B >= 5 and B * elem <= 256 and not (binary and B * elem > 128) and env.get("SS_COL") != "0":
            return "spmm_csell" if csell else "spmm_colgroup"
        if B <= 4:
            if elem == 8 and B == 2 and env.get("SS_CSELL_B12") != "0" and csell:
                return "spmm_csell"
            if B >= 3 and env.get("SS_CSELL_ROW16") != "0" and csell:
                return "spmm_csell"
            return "spmm_chunked_narrow"
    return "spmm_sell"


@functools.lru_cache(maxsize=None)
def _spmm_case(weighted, exact, dtype):
    W, R = S.spmm_operands(K=2700, weighted=weighted, exact=exact)
    R = R.astype(dtype).astype(np.float64)          # what the device is given (exact operands: unchanged)
    want = W @ R
    want.setflags(write=False)
    return W, R, want


def _spmm_all_widths(dtype, weighted, route, switches, exact):
    env, named = ROUTES[route]
    env = dict(env, SS_NARROW_CHUNK=str(SPMM_CHUNK))
    switches(env)
    W, R, want = _spmm_case(weighted, exact, dtype)
    nchunks = -(-W.shape[1] // SPMM_CHUNK)
    assert nchunks == 6
    w = ss.DeviceSpMat(W.astype(dtype), dtype=dtype)
    seen = set()
    for colmajor in (False, True):
        if colmajor and route not in ("SELL", "lane-per-row"):
            continue           # column-major operands always take the SELL kernel
        for B in SPMM_B:
            Rb = np.ascontiguousarray(R[:, :B])
            if colmajor:
                got = np.ascontiguousarray(w.spmm(np.ascontiguousarray(Rb.T).astype(dtype), colmajor=True).T)
            else:
                got = w.spmm(Rb.astype(dtype))
            path = ss.path_last()
            tag = _route(B, dtype, not weighted, colmajor, env)
            # (the SELL operand of this W is length-sorted by the builder's own skew test: spmm_sell_sorted)
            assert [t.replace("_sorted", "") for t in path if t.startswith("spmm_")] == [tag], (B, colmajor, path)
            seen.add(tag)
            label = f"W @ R, {route}, B = {B}{', column-major' if colmajor else ''}"
            if exact:
                S.assert_bitwise(got, want[:, :B], dtype, label)
            else:
                ratio = S.assert_band(got, want[:, :B], S.band_spmm(W, Rb, dtype, nchunks), label)
                key = (tag, "W @ R", np.dtype(dtype).name)
                WORST[key] = max(WORST.get(key, 0.0), ratio)
    assert named in seen, (route, seen)
    w.close()
    if not exact:
        print(f"[sparse] worst so far: {WORST}")


@pytest.mark.parametrize("route", list(ROUTES))
@pytest.mark.parametrize("weighted", WEIGHTED, ids=W_IDS)
@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f64"])
def test_spmm_exact_on_every_route(dtype, weighted, route, switches):
    """W (301 x 2700, empty rows, a full row, a last row with one entry in the last column; weights k/16 or ones) times
    R of small signed integers / 16, at thirteen widths, six column chunks: every route equals W @ R in fp64 bit for
    bit, hence all routes equal each other."""
    _spmm_all_widths(dtype, weighted, route, switches, exact=True)


@pytest.mark.parametrize("route", list(ROUTES))
@pytest.mark.parametrize("weighted", WEIGHTED, ids=W_IDS)
@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f64"])
def test_spmm_within_its_bands_on_every_route(dtype, weighted, route, switches):
    """The same W with standard-normal R: |got - want| <= gamma(n_row + nchunks + 1) (|W| |R|)_ij element by element."""
    _spmm_all_widths(dtype, weighted, route, switches, exact=False)


# ----------------------------------------------------------------------------- bands on ordinary graphs
@functools.lru_cache(maxsize=None)
def _band_case(weighted):
    g = S.band_graph(weighted)
    Xq, X, Y, fold = g["Xq"], g["X"], g["Y"], g["fold"]
    ref = dict(query=(S.oracle_query(Xq, X, Y), S.counts_query(Xq, X, Y)),
               source=(S.oracle_source(X, Y), S.counts_query(None, X, Y, source_rows=True)),
               loo=(S.oracle_loo(X, Y), S.counts_loo(X, Y)),
               kfold=(S.oracle_kfold(X, Y, fold), S.counts_kfold(X, Y, fold)))
    return g, ref


BAND_SWITCHES = [("stage1", n) for n in STAGE1] + [("stage2", n) for n in STAGE2 if n != "default"]


@pytest.mark.parametrize("weighted", WEIGHTED, ids=W_IDS)
@pytest.mark.parametrize("dtype,kind,name", _params(BAND_SWITCHES))
def test_every_score_within_its_band_under_every_switch(dtype, kind, name, weighted, switches):
    """Query rows, source rows (a sub-range too), leave-one-out and k-fold on a low-fill graph with arbitrary degrees:
    |got - oracle| <= gamma(k) * oracle for every score, structural zeros exact, -99 where the oracle has them."""
    env, tags, stage2 = _fold_env(kind, name, "band")
    switches(env)
    inp, ref = _band_case(weighted)
    Xq, X, Y, fold = inp["Xq"], inp["X"], inp["Y"], inp["fold"]
    ns = X.shape[0]
    kc = int(env.get("SS_SELL_CHUNK", ns))
    extra = dict(sell_chunks=-(-ns // min(kc, ns)), dual=env.get("SS_TRANSFER_DUAL") == "1",
                 parts=S.parts_of_targets(Y, 256) if stage2 == "spmm_sell_sorted" else 0)
    loo_ok = kind == "stage2" or STAGE1[name][3]
    query_only = kind == "stage1" and name == "block kernel"
    if "SS_TRANSFER_BYTES" in env:      # the source rows and the leave-one-out sweep really take several batches
        assert _batches(env, ns, ns, dtype) >= 2

    def check(got, mode, rows=slice(None)):
        want, (chain, addends) = ref[mode]
        band = S.band_graph_scores(want[rows], chain[rows], addends[rows], dtype, **extra)
        ratio = S.assert_band(got, want[rows], band, f"{mode}, {name}, {np.dtype(dtype).name}")
        key = (name, mode, np.dtype(dtype).name)
        WORST[key] = max(WORST.get(key, 0.0), ratio)

    g = _graph(Xq, X, Y, dtype)
    _check_degrees(g, X, Y)
    check(g.predict("query"), "query")
    _tags(tags, stage2)
    got = g.predict("query", clean=True)
    np.testing.assert_array_equal(got == -99, np.broadcast_to(S.clean_mask(Y), got.shape))
    if not query_only:       # (the block kernel serves query rows; source rows fall to the single-wave kernel)
        check(g.predict("source"), "source")
        _tags(tags, stage2)
        check(g.predict("source", 77, 205), "source", slice(77, 205))
    g.close()
    if not query_only:
        g = _graph(None, X, Y, dtype)
        if loo_ok:
            check(g.predict_loo(), "loo")
            _tags(tags, stage2, loo=True)
            got = g.predict_loo(clean=True)
            np.testing.assert_array_equal(got == -99, S.clean_mask(Y, np.arange(ns)))
        check(g.predict_kfold(fold, inp["nfolds"]), "kfold")
        _tags(tags, stage2)
        check(g.predict_kfold_rows(fold, inp["nfolds"], 13, 99), "kfold", slice(13, 99))
        g.close()
    print(f"[sparse] worst so far: {WORST}")


@functools.lru_cache(maxsize=None)
def _large_fold_case(weighted):
    inp, _ = _band_case(weighted)
    X, Y = inp["X"], inp["Y"]
    fold = (np.arange(X.shape[0]) % 8 == 0).astype(np.int32)       # fold 0: 532 of the 608 sources, fold 1: 76
    want, counts = S.oracle_kfold(X, Y, fold), S.counts_kfold(X, Y, fold)
    want.setflags(write=False)
    return X, Y, fold, want, counts


@pytest.mark.parametrize("weighted", WEIGHTED, ids=W_IDS)
@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f64"])
def test_kfold_of_one_large_fold_in_several_sorted_batches(dtype, weighted, switches):
    """Where the length-sorted operand, several batches of one fold and a row map meet: a fold of 532 members under
    SS_TRANSFER_BYTES = 2^20 (batches of 424 rows in fp32, 208 in fp64).  predict_kfold (row copies from the host's
    order) and predict_kfold_rows (device row map; all rows and a sub-range) stay within the oracle's bands, and equal
    bit for bit what a handle without the switch gives in one batch per fold: a row's sums do not depend on its batch."""
    X, Y, fold, want, (chain, addends) = _large_fold_case(weighted)
    ns = X.shape[0]
    env = dict(STAGE2["sorted, transfer batches"][0])
    assert _batches(env, int((fold == 0).sum()), ns, dtype) >= 2
    got = {}
    for batched in (False, True):
        switches(env if batched else STAGE2["sorted"][0])
        g = _graph(None, X, Y, dtype)
        got[batched] = (g.predict_kfold(fold, 2), g.predict_kfold_rows(fold, 2), g.predict_kfold_rows(fold, 2, 13, 599),
                        g.predict_kfold(fold, 2, clean=True))
        _tags(("transfer",), "spmm_sell_sorted")
        g.close()
    band = S.band_graph_scores(want, chain, addends, dtype, sell_chunks=1, parts=S.parts_of_targets(Y, 256))
    S.assert_band(got[True][0], want, band, f"k-fold, one large fold, {np.dtype(dtype).name}")
    for one, several, what in zip(got[False], got[True], ("k-fold", "k-fold rows", "k-fold rows [13,599)", "clean")):
        np.testing.assert_array_equal(several, one, err_msg=what)
    np.testing.assert_array_equal(got[True][1], got[True][0])
    np.testing.assert_array_equal(got[True][2], got[True][0][13:599])
    assert (got[True][3] == -99).any()       # (without 532 sources some targets have none left)
