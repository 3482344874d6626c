"""The stride contract of the C ABI: every score entry point writes (or reads) the window its pointer and leading
dimension describe and nothing else -- ss_predict_*, ss_predict_loo_*, ss_predict_kfold_*, ss_predict_kfold_rows_*,
ss_predict_queries_*, ss_spmm_* (ldr and ldf, two independent layouts) and the consumers ss_topl_f32,
ss_pool_add_rows_*, ss_target_topl_add_rows_*.  The mirror only ever passes the tight leading dimension and
allocator-aligned bases; here every call goes through ctypes on the handles of the mirror's objects.

Every block sits on a canvas of NaN sentinels (tests/stride_ref.py; tests/test_strides_cpu.py shows what its check
rejects): ld = width + pad with pad in {1, 3, 4} (and 2 where the width is 2 mod 4), so that ld % 4 != 0 where the
width is a multiple of four and the reverse, and the base at element 0 or 1 of the allocation, on or off 16-byte
alignment.  Row-major (ld = nt + pad) and column-major (ld = nrows + pad), host and device memory, both precisions.
After the call the window equals, bit for bit, the tight call of the mirror on the same handle, and every other element
still holds the sentinel.  The tight call itself is float32(oracle) / the fp64 oracle bit for bit on the exactly
summable inputs of tests/sparse_ref.py and tests/dense_ref.py; source rows are the exception -- their target path
divides by target degrees that are no powers of two, so no exact input exists for them (tests/test_gpu_sparse.py holds
them to their bands) and they are judged against the tight call alone.

Widths: the exact builders need nt - 1 >= the labels of a source, so the widths are the smallest a builder allows that
are a multiple of four, 1 mod 4 and neither: query rows 64, 65 and -- on graph_input_ref.tall_graph -- 3; leave-one-out
129, 130, 132; k-fold 33, 35, 36, and 65, 67, 68 for the length-sorted stage-2 operand, which needs more than 64
targets.  Switches are read when a handle's operands are built: every setting gets a fresh handle.  Every call asserts
its kernel tags in ss.path_last(), and every test asserts at its end that each kernel it is about ran with ld % 4 == 0
and != 0 and with aligned and misaligned bases; the states seen are printed ("[strides]")."""
import functools

import numpy as np
import pytest
import scipy.sparse as sp

import simspread_jl_amd as ss
from simspread_jl_amd import _lib
from oracle import simspread_oracle as O

import dense_ref as D
import graph_input_ref as G
import pooled_ref
import sparse_ref as S
import stride_ref as R
import target_topl_ref

pytestmark = pytest.mark.gpu

DTYPES = [np.float32, np.float64]
DT_IDS = ["f32", "f64"]
HOST, DEVICE = R.HOST, R.DEVICE
ROW, COL = _lib.SS_LAYOUT_ROWMAJOR, _lib.SS_LAYOUT_COLMAJOR
PADS = (1, 3, 4)
FRONTS = (0, 1)
BACK = 8                     # elements behind the block: an overrun of the last row lands on sentinels, not outside
EINVAL = -1
SWITCHES = ("SS_TRANSFER_CHUNK", "SS_TRANSFER_BYTES", "SS_TRANSFER_V", "SS_SELL_CHUNK", "SS_SELL_QT", "SS_SELL_SORT",
            "SS_SELL_LMAX", "SS_SELL_PLAIN", "SS_NARROW_CHUNK", "SS_CSELL", "SS_CSELL_ROW16", "SS_CSELL_ROW32",
            "SS_CSELL_B12", "SS_CSELL_CUT", "SS_COL", "SS_COL_CG", "SS_COL_FROM", "SS_DENSE_BF16", "SS_DENSE_RING",
            "SS_DENSE_TILE", "SS_TOPL_BOUND")


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


def _suf(dtype):
    return "f32" if np.dtype(dtype) == np.float32 else "f64"


def _fn(name, dtype):
    return getattr(ss._lib.lib(), f"{name}_{_suf(dtype)}")


def _sync():
    _lib.check(ss._lib.lib().ss_synchronize())


def _ok(rc):
    assert rc == 0, ss._lib.lib().ss_last_error().decode("utf-8", "replace")


def _cleaned(want, mask):
    out = np.array(want, dtype=np.float64)
    out[np.broadcast_to(mask, out.shape)] = -99.0
    return out


def _state(cv):
    return (cv.ld % 4 == 0, cv.aligned)


ALL_STATES = {(a, b) for a in (False, True) for b in (False, True)}


def _pads(width):
    """PADS, plus the pad that makes ld a multiple of four where none of them does (width % 4 == 2)."""
    return sorted(set(PADS) | {(-width) % 4 or 4})


def _stage2_tag():
    """The SELL kernel of the last call: spmm_sell, or spmm_sell_sorted where the builder's skew test (or SS_SELL_SORT)
    length-sorted the operand."""
    tags = [t for t in ss.path_last() if t in ("spmm_sell", "spmm_sell_sorted")]
    assert len(set(tags)) == 1, ss.path_last()
    return tags[0]


def _report(entry, seen):
    """seen: tag -> set of (ld % 4 == 0, base 16-byte aligned) of the device, row-major (direct) calls"""
    print()
    for tag in sorted(seen):
        states = ", ".join(f"ld%4{'==' if a else '!='}0/{'aligned' if b else 'misaligned'}" for a, b in sorted(seen[tag]))
        print(f"[strides] {entry}: {tag}: {states}")


# ----------------------------------------------------------------------------- producers: the sweep over canvases
def _sweep(entry, call, nrows, nt, dtype, tight, tags, cleans=(0, 1)):
    """call(ptr, ld, layout, mem, clean) -> rc runs the entry point; tight[clean]: the (nrows, nt) result of the tight
    mirror call.  Host and device, both layouts, every pad and base offset: the window is the tight result bit for bit and
    nothing else is written.  tags: kernels every call must name.  Returns tag -> states seen on the direct route (device
    memory, row-major: the caller's pointer and ld go straight into the kernels)."""
    seen = {}
    for clean in cleans:
        want_rm = np.ascontiguousarray(tight[clean], dtype=dtype)
        assert want_rm.shape == (nrows, nt)
        want_cm = np.ascontiguousarray(want_rm.T)
        for mem in (HOST, DEVICE):
            for layout in (ROW, COL):
                r, c = (nrows, nt) if layout == ROW else (nt, nrows)
                for pad in _pads(c):
                    for front in FRONTS:
                        cv = R.canvas(r, c, c + pad, front, BACK, dtype, mem)
                        if mem == DEVICE:
                            ss.use_torch_stream()
                        _ok(call(cv.ptr, cv.ld, layout, mem, clean))
                        path = set(ss.path_last())
                        assert set(tags) <= path, (entry, tags, path)
                        _sync()
                        label = (f"{entry}, {_suf(dtype)}, {'device' if mem else 'host'}, "
                                 f"{'column' if layout == COL else 'row'}-major, ld = {c} + {pad}, front {front}, clean {clean}")
                        R.check(cv, cv.host(), want_rm if layout == ROW else want_cm, label)
                        if mem == DEVICE and layout == ROW:
                            for t in path:
                                seen.setdefault(t, set()).add(_state(cv))
    for t in tags:
        assert seen.get(t) == ALL_STATES, (entry, t, seen.get(t))
    _report(f"{entry} {_suf(dtype)} nt={nt}", {t: seen[t] for t in tags})
    return seen


def _refuses_short_ld(call, nrows, nt, dtype):
    """ld one short of the width: SS_EINVAL and nothing written, both layouts, host and device."""
    for mem in (HOST, DEVICE):
        for layout in (ROW, COL):
            r, c = (nrows, nt) if layout == ROW else (nt, nrows)
            cv = R.canvas(r, c, c, 1, BACK, dtype, mem)
            if mem == DEVICE:
                ss.use_torch_stream()
            assert call(cv.ptr, c - 1, layout, mem, 0) == EINVAL
            _sync()
            R.check(cv, cv.host(), cv.window(cv.host()).copy(), "short ld")


# ----------------------------------------------------------------------------- ss_predict_*, ss_predict_queries_*: sparse
QUERY_NQ = 170
QUERY_ROWS = (3, 167)        # 164 rows: three stage-1 batches of 80 in fp32, five of 40 in fp64 (SS_TRANSFER_BYTES = 2^20)
SOURCE_ROWS = (77, 205)      # 128 rows: two and four batches
BATCH_ENV = {"SS_TRANSFER_BYTES": str(1 << 20)}


@functools.lru_cache(maxsize=None)
def _query_case(elem, nt):
    inp = S.exact_query_for(elem, None, nt=nt, nq=QUERY_NQ, weighted=True)
    want = S.oracle_query(inp["Xq"], inp["Xs"], inp["Ys"])
    want.setflags(write=False)
    return inp, want


def _sparse_graph(Xq, Xs, Ys, dtype):
    return ss.DeviceGraph.from_sparse(None if Xq is None else Xq.astype(dtype), Xs.astype(dtype), Ys.astype(dtype),
                                      dtype=dtype)


@pytest.mark.parametrize("nt", [64, 65])
@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
def test_predict_query_and_source_rows_sparse(dtype, nt, switches):
    """ss_predict_* on the exact query graph (3000 sources): a sub-range with row_begin > 0 that takes several stage-1
    batches, clean 0 and 1.  Query rows equal the oracle's bits; source rows the tight call."""
    switches(BATCH_ENV)
    elem = np.dtype(dtype).itemsize
    inp, want = _query_case(elem, nt)
    ns = inp["Xs"].shape[0]
    mask = S.clean_mask(inp["Ys"])
    g = _sparse_graph(inp["Xq"], inp["Xs"], inp["Ys"], dtype)
    fn = _fn("ss_predict", dtype)
    for kind, name, (lo, hi) in ((_lib.SS_ROWS_QUERY, "query", QUERY_ROWS), (_lib.SS_ROWS_SOURCE, "source", SOURCE_ROWS)):
        assert -(-(hi - lo) // S.transfer_batch_rows(hi - lo, ns, elem, 1 << 20)) >= 2
        tight = {c: g.predict(name, lo, hi, clean=bool(c)) for c in (0, 1)}
        assert ss.timing_last()["transfer_launches"] >= 2
        if name == "query":
            S.assert_bitwise(tight[0], want[lo:hi], dtype, "query rows, tight")
            S.assert_bitwise(tight[1], _cleaned(want[lo:hi], mask), dtype, "query rows, tight, clean")
        assert (tight[1] == -99).any() and not (tight[0] == -99).any()

        def call(ptr, ld, layout, mem, clean, kind=kind, lo=lo, hi=hi):
            return fn(g._h, kind, lo, hi, clean, ptr, ld, layout, mem)
        _sweep(f"ss_predict {name} rows", call, hi - lo, nt, dtype, tight, ("transfer", "spmm_sell"))
        _refuses_short_ld(call, hi - lo, nt, dtype)
    g.close()


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
def test_predict_query_rows_three_targets(dtype, switches):
    """A width below four: graph_input_ref.tall_graph (70 000 sources, 4 features, 3 targets, 5 queries), rows [1, 5)."""
    switches({})
    inp = G.tall_graph()
    want = S.oracle_query(inp["Xq"], inp["Xs"], inp["Ys"])
    g = _sparse_graph(inp["Xq"], inp["Xs"], inp["Ys"], dtype)
    lo, hi = 1, 5
    mask = S.clean_mask(inp["Ys"])
    tight = {c: g.predict("query", lo, hi, clean=bool(c)) for c in (0, 1)}
    S.assert_bitwise(tight[0], want[lo:hi], dtype, "tall graph, tight")
    S.assert_bitwise(tight[1], _cleaned(want[lo:hi], mask), dtype, "tall graph, tight, clean")
    assert (tight[1] == -99).any()
    stage2 = _stage2_tag()
    fn = _fn("ss_predict", dtype)
    _sweep("ss_predict query rows", lambda ptr, ld, layout, mem, clean: fn(g._h, _lib.SS_ROWS_QUERY, lo, hi, clean, ptr, ld,
                                                                            layout, mem),
           hi - lo, 3, dtype, tight, ("transfer", stage2))
    g.close()


@pytest.mark.parametrize("nt", [64, 65])
@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
def test_predict_queries_on_a_query_set(dtype, nt, switches):
    """ss_predict_queries_*: a CSR query set bound to the exact query graph built without queries; a sub-range."""
    switches(BATCH_ENV)
    inp, want = _query_case(np.dtype(dtype).itemsize, nt)
    g = _sparse_graph(None, inp["Xs"], inp["Ys"], dtype)
    q = ss.DeviceQueries.from_sparse(g, inp["Xq"].astype(dtype))
    lo, hi = QUERY_ROWS
    mask = S.clean_mask(inp["Ys"])
    tight = {c: g.predict(row_begin=lo, row_end=hi, clean=bool(c), queries=q) for c in (0, 1)}
    assert ss.timing_last()["transfer_launches"] >= 2
    S.assert_bitwise(tight[0], want[lo:hi], dtype, "query set, tight")
    S.assert_bitwise(tight[1], _cleaned(want[lo:hi], mask), dtype, "query set, tight, clean")
    fn = _fn("ss_predict_queries", dtype)

    def call(ptr, ld, layout, mem, clean):
        return fn(g._h, q._h, lo, hi, clean, ptr, ld, layout, mem)
    _sweep("ss_predict_queries", call, hi - lo, nt, dtype, tight, ("transfer", "spmm_sell"))
    _refuses_short_ld(call, hi - lo, nt, dtype)
    q.close()
    g.close()


# ----------------------------------------------------------------------------- dense similarity: ss_predict_*, ss_predict_loo_*
DENSE_TAG = {np.float32: "transfer_dense_bf16", np.float64: "transfer_dense_f64_mfma"}


@functools.lru_cache(maxsize=None)
def _dense_case(mode):
    inp = D.exact_inputs(mode)
    X, Xq, Y = D.cut(inp["Ss"], inp["alpha"], True), D.cut(inp["Sq"], inp["alpha"], True), inp["Y"]
    if mode == "query":
        want = {0: D.oracle_query(Xq, X, Y)}
        want[1] = _cleaned(want[0], S.clean_mask(sp.csr_matrix(Y)))
    else:
        Y64 = Y.astype(np.float64)
        want = {0: O.predict_loo_factored(X, Y64), 1: O.predict_loo_factored(X, Y64, clean_flag=True)}
    return inp, X, want


def _dense_graph(inp, dtype):
    return ss.DeviceGraph.from_similarity(inp["Sq"], inp["Ss"], sp.csr_matrix(inp["Y"]), alpha=inp["alpha"], weighted=True,
                                          dtype=dtype)


def _dense_tag(dtype):
    """The stage-1 engine of the last call: the bf16 plane kernels in fp32, the fp64 matrix instruction in fp64."""
    want = DENSE_TAG[dtype]
    tags = [t for t in ss.path_last() if t.startswith("transfer_dense")]
    assert tags and all(t.startswith(want) for t in tags), (want, tags)
    return tags[0]


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
def test_predict_rows_dense_similarity(dtype, switches):
    """from_similarity on dense_ref.exact_inputs (255 sources, 4559 targets: 3 mod 4): query rows [3, 129) equal the
    oracle's bits on the bf16 planes and in fp64; source rows [5, 70) equal the tight call.  (One stage-1 batch:
    SS_TRANSFER_BYTES cannot go below 2^20, which holds more than a thousand rows of 255 sources.)"""
    switches({})
    inp, X, want = _dense_case("query")
    nt = inp["Y"].shape[1]
    g = _dense_graph(inp, dtype)
    fn = _fn("ss_predict", dtype)
    for kind, name, (lo, hi) in ((_lib.SS_ROWS_QUERY, "query", (3, 129)), (_lib.SS_ROWS_SOURCE, "source", (5, 70))):
        tight = {c: g.predict(name, lo, hi, clean=bool(c)) for c in (0, 1)}
        tag, stage2 = _dense_tag(dtype), _stage2_tag()
        if name == "query":
            for c in (0, 1):
                S.assert_bitwise(tight[c], want[c][lo:hi], dtype, f"dense query rows, tight, clean {c}")

        def call(ptr, ld, layout, mem, clean, kind=kind, lo=lo, hi=hi):
            return fn(g._h, kind, lo, hi, clean, ptr, ld, layout, mem)
        _sweep(f"ss_predict dense {name} rows", call, hi - lo, nt, dtype, tight, (tag, stage2))
    g.close()


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
def test_predict_loo_dense_similarity(dtype, switches):
    """Leave-one-out on dense_ref.exact_inputs("loo") (164 sources, 2966 targets: 2 mod 4).  Every target has exactly
    one source, so with clean = 1 launch_loo_clean_fix writes a -99 into every row of the range, at the caller's ld."""
    switches({})
    inp, X, want = _dense_case("loo")
    nt = inp["Y"].shape[1]
    g = _dense_graph(inp, dtype)
    lo, hi = 9, 158
    tight = {c: g.predict_loo(lo, hi, clean=bool(c)) for c in (0, 1)}
    tag, stage2 = _dense_tag(dtype), _stage2_tag()
    for c in (0, 1):
        S.assert_bitwise(tight[c], want[c][lo:hi], dtype, f"dense leave-one-out, tight, clean {c}")
    assert ((tight[1] == -99).sum(axis=1) > 0).all()
    fn = _fn("ss_predict_loo", dtype)
    _sweep("ss_predict_loo dense", lambda ptr, ld, layout, mem, clean: fn(g._h, lo, hi, clean, ptr, ld, layout, mem),
           hi - lo, nt, dtype, tight, (tag, stage2))
    g.close()


# ----------------------------------------------------------------------------- ss_predict_loo_*: sparse
@functools.lru_cache(maxsize=None)
def _loo_case(nt):
    inp = S.exact_loo(True, nt=nt)
    want = S.oracle_loo(inp["X"], inp["Y"])
    want.setflags(write=False)
    return inp, want


@pytest.mark.parametrize("nt", [129, 130, 132])
@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
def test_predict_loo_sparse(dtype, nt, switches):
    """ss_predict_loo_* on the exact leave-one-out graph (488 sources), folds [61, 470): two stage-1 batches in fp64."""
    switches(BATCH_ENV)
    inp, want = _loo_case(nt)
    X, Y = inp["X"], inp["Y"]
    g = _sparse_graph(None, X, Y, dtype)
    lo, hi = 61, 470
    mask = S.clean_mask(Y, np.arange(lo, hi))
    tight = {c: g.predict_loo(lo, hi, clean=bool(c)) for c in (0, 1)}
    if dtype == np.float64:
        assert ss.timing_last()["transfer_launches"] >= 2
    S.assert_bitwise(tight[0], want[lo:hi], dtype, "leave-one-out, tight")
    S.assert_bitwise(tight[1], _cleaned(want[lo:hi], mask), dtype, "leave-one-out, tight, clean")
    assert (tight[1] == -99).any()
    fn = _fn("ss_predict_loo", dtype)

    def call(ptr, ld, layout, mem, clean):
        return fn(g._h, lo, hi, clean, ptr, ld, layout, mem)
    _sweep("ss_predict_loo", call, hi - lo, nt, dtype, tight, ("transfer_loo", "spmm_sell"))
    _refuses_short_ld(call, hi - lo, nt, dtype)
    g.close()


# ----------------------------------------------------------------------------- ss_predict_kfold_*, ss_predict_kfold_rows_*
@functools.lru_cache(maxsize=None)
def _kfold_case(nt):
    inp = S.exact_kfold(True, nt=nt)
    want = S.oracle_kfold(inp["X"], inp["Y"], inp["fold"])
    want.setflags(write=False)
    return inp, want


# (the stage-2 operand is length-sorted only when it has more than 64 rows, i.e. targets)
KFOLD_CASES = [("0", 33), ("0", 35), ("0", 36), ("1", 65), ("1", 67), ("1", 68)]


@pytest.mark.parametrize("sort,nt", KFOLD_CASES,
                         ids=[f"{'length-sorted' if s == '1' else 'unsorted'}-{n}" for s, n in KFOLD_CASES])
@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
def test_predict_kfold_and_kfold_rows(dtype, nt, sort, switches):
    """Exact k-fold graph (252 sources, nine folds whose members interleave): the whole sweep and rows [29, 70), which
    cross every fold, so each fold's rows go through a row map.  SS_SELL_SORT = 0: the map is fused into the SELL launch;
    1: unpermute to packed rows, then the scatter (device row map) or one copy per row (ss_predict_kfold_*) to ld."""
    switches({"SS_SELL_SORT": sort, "SS_SELL_LMAX": "256"})
    stage2 = "spmm_sell_sorted" if sort == "1" else "spmm_sell"
    inp, want = _kfold_case(nt)
    X, Y, fold, nfolds = inp["X"], inp["Y"], inp["fold"], inp["nfolds"]
    ns = X.shape[0]
    g = _sparse_graph(None, X, Y, dtype)
    mask = S.clean_mask(Y)
    lo, hi = 29, 70
    assert len(set(fold[lo:hi].tolist())) == nfolds
    import torch
    fold_dev = torch.from_numpy(fold).cuda()
    fptr = {HOST: fold.ctypes.data, DEVICE: fold_dev.data_ptr()}

    tight = {c: g.predict_kfold(fold, nfolds, clean=bool(c)) for c in (0, 1)}
    assert stage2 in ss.path_last()
    S.assert_bitwise(tight[0], want, dtype, "k-fold, tight")
    S.assert_bitwise(tight[1], _cleaned(want, mask), dtype, "k-fold, tight, clean")
    assert (tight[1] == -99).any()
    fn = _fn("ss_predict_kfold", dtype)
    _sweep(f"ss_predict_kfold {stage2}",
           lambda ptr, ld, layout, mem, clean: fn(g._h, fptr[mem], nfolds, clean, ptr, ld, layout, mem),
           ns, nt, dtype, tight, ("transfer", stage2))

    tight = {c: g.predict_kfold_rows(fold, nfolds, lo, hi, clean=bool(c)) for c in (0, 1)}
    S.assert_bitwise(tight[0], want[lo:hi], dtype, "k-fold rows, tight")
    S.assert_bitwise(tight[1], _cleaned(want[lo:hi], mask), dtype, "k-fold rows, tight, clean")
    fnr = _fn("ss_predict_kfold_rows", dtype)

    def call(ptr, ld, layout, mem, clean):
        return fnr(g._h, fptr[mem], nfolds, lo, hi, clean, ptr, ld, layout, mem)
    _sweep(f"ss_predict_kfold_rows {stage2}", call, hi - lo, nt, dtype, tight, ("transfer", stage2))
    _refuses_short_ld(call, hi - lo, nt, dtype)
    g.close()


# ----------------------------------------------------------------------------- ss_spmm_*
SPMM_B = (1, 2, 3, 4, 5, 8, 9, 16, 17, 32, 33, 64, 65)
SPMM_CHUNK = 500             # K = 1300: three column chunks, so a chunk after the first adds to what the first stored
SPMM_PADS = (0, 1, 4)


def _spmm_pads(width):
    """SPMM_PADS, plus the pad that makes the leading dimension a multiple of four where none of them does."""
    return sorted(set(SPMM_PADS) | {(-width) % 4})


SPMM_FRONTS = [(a, b) for a in FRONTS for b in FRONTS]
SPMM_ENV = {
    "default": {},
    "narrow": {"SS_CSELL_ROW16": "0", "SS_CSELL_B12": "0"},
    "column-group": {"SS_CSELL": "0"},
    "SELL": {"SS_COL": "0"},
}


def _route(B, dtype, rowmajor, env):
    """The routing of ss_spmm (wr_route in api.hip) restated for a weighted W: (tag, csell slot or None)."""
    elem = np.dtype(dtype).itemsize
    csell = env.get("SS_CSELL") != "0"
    if rowmajor:
        if B >= 5 and B * elem <= 256 and env.get("SS_COL") != "0":
            if not csell:
                return "spmm_colgroup", None
            if elem == 4 and B <= 8:
                return "spmm_csell", 3
            return "spmm_csell", 0 if B * elem <= 64 else (1 if B * elem <= 128 else 2)
        if B <= 4:
            if elem == 8 and B == 2 and env.get("SS_CSELL_B12") != "0" and csell:
                return "spmm_csell", 5
            if B >= 3 and env.get("SS_CSELL_ROW16") != "0" and csell:
                return "spmm_csell", 4
            return "spmm_chunked_narrow", None
    return "spmm_sell", None


@functools.lru_cache(maxsize=None)
def _spmm_case():
    W, Rm = S.spmm_operands(M=301, K=1300, weighted=True, exact=True)
    want = W @ Rm
    assert S.spmm_quanta_bound(W) < 2 ** 24
    want.setflags(write=False)
    return W, Rm, want


def _spmm_canvases(Rb, wantb, dtype, mem, r_layout, f_layout, pad, padf, front, frontf):
    K, B = Rb.shape
    M = wantb.shape[0]
    rr, rc = (K, B) if r_layout == ROW else (B, K)
    fr, fc = (M, B) if f_layout == ROW else (B, M)
    rcv = R.canvas(rr, rc, rc + pad, front, BACK, dtype, mem).put(Rb if r_layout == ROW else Rb.T)
    fcv = R.canvas(fr, fc, fc + padf, frontf, BACK, dtype, mem)
    return rcv, fcv


def _spmm_sweep(w, dtype, mem, B, r_layout, f_layout, env, seen):
    """One width, one pair of layouts: every (pad, pad') and base offset.  R's padding is the NaN sentinel, so a read of it
    poisons a score; F equals W @ R in fp64 bit for bit, its padding and all of R's canvas are untouched."""
    W, Rm, want = _spmm_case()
    Rb = np.ascontiguousarray(Rm[:, :B]).astype(dtype)
    wantb = np.ascontiguousarray(want[:, :B]).astype(dtype)
    tag, slot = _route(B, dtype, r_layout == ROW and f_layout == ROW, env)
    fn = _fn("ss_spmm", dtype)
    pw = 16 // np.dtype(dtype).itemsize
    pads = [(p, q) for p in _spmm_pads(B if r_layout == ROW else Rb.shape[0])
            for q in _spmm_pads(B if f_layout == ROW else wantb.shape[0]) if (p, q) != (0, 0)]
    for pad, padf in pads:
        for front, frontf in SPMM_FRONTS:
            rcv, fcv = _spmm_canvases(Rb, wantb, dtype, mem, r_layout, f_layout, pad, padf, front, frontf)
            if mem == DEVICE:
                ss.use_torch_stream()
            _ok(fn(w._h, rcv.ptr, B, rcv.ld, r_layout, fcv.ptr, fcv.ld, f_layout, mem))
            path = ss.path_last()
            assert [t.replace("_sorted", "") for t in path if t.startswith("spmm_")] == [tag], (B, r_layout, f_layout, path)
            _sync()
            label = (f"ss_spmm {_suf(dtype)}, {tag}, B = {B}, layouts {r_layout}{f_layout}, {'device' if mem else 'host'}, "
                     f"ldr = +{pad}, ldf = +{padf}, fronts {front}{frontf}")
            R.check(fcv, fcv.host(), wantb if f_layout == ROW else np.ascontiguousarray(wantb.T), label + ": F")
            R.check(rcv, rcv.host(), Rb if r_layout == ROW else np.ascontiguousarray(Rb.T), label + ": R")
            if mem == DEVICE:
                s = seen.setdefault((tag, slot), dict(B=set(), f=set(), r=set()))
                s["B"].add(B)
                if B % 4 == 0:        # where only ld and the base decide between 16-byte and scalar accesses
                    s["f"].add((fcv.ld % pw == 0, fcv.aligned))
                    s["r"].add((rcv.ld % pw == 0, rcv.aligned))


def _spmm_report(what, dtype, seen):
    print()
    for (tag, slot), s in sorted(seen.items(), key=str):
        if any(b % 4 == 0 for b in s["B"]):
            assert s["f"] == ALL_STATES and s["r"] == ALL_STATES, (tag, slot, s)
        print(f"[strides] ss_spmm {_suf(dtype)} {what}: {tag}{'' if slot is None else f' slot {slot}'}: B = {sorted(s['B'])}, "
              f"(ldf % PW == 0, F aligned) {sorted(s['f'])}, (ldr % PW == 0, R aligned) {sorted(s['r'])}")


@pytest.mark.parametrize("route", list(SPMM_ENV))
@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
def test_spmm_padded_operands_on_every_route(dtype, route, switches):
    """Device memory, row-major R and F, thirteen widths: ldr = B + pad, ldf = B + pad' with pad, pad' in {0, 1, 4} (not
    both 0; also the pad that makes the leading dimension a multiple of four, where none of these does) and each base
    at element 0 or 1 independently.  Every kernel the setting routes to must be seen, and at the
    widths that are multiples of four each must be seen with ldf % PW and ldr % PW zero and non-zero and with aligned and
    misaligned bases (PW = 16 bytes of the precision): both sides of every 16-byte / scalar switch."""
    env = dict(SPMM_ENV[route], SS_NARROW_CHUNK=str(SPMM_CHUNK), SS_SELL_CHUNK=str(SPMM_CHUNK))
    switches(env)
    W = _spmm_case()[0]
    w = ss.DeviceSpMat(W.astype(dtype), dtype=dtype)
    seen = {}
    for B in SPMM_B:
        _spmm_sweep(w, dtype, DEVICE, B, ROW, ROW, env, seen)
    w.close()
    f32 = dtype == np.float32
    want = {
        "default": {("spmm_chunked_narrow", None), ("spmm_csell", 0), ("spmm_csell", 1), ("spmm_csell", 2), ("spmm_csell", 4),
                    ("spmm_csell", 3 if f32 else 5), ("spmm_sell", None)},
        "narrow": {("spmm_chunked_narrow", None)},
        "column-group": {("spmm_colgroup", None), ("spmm_chunked_narrow", None)},
        "SELL": {("spmm_sell", None)},
    }[route]
    assert want <= set(seen), (route, want - set(seen))
    if route == "narrow":
        assert seen[("spmm_chunked_narrow", None)]["B"] >= {1, 2, 3, 4}
    if route == "column-group":
        assert seen[("spmm_colgroup", None)]["B"] >= ({5, 8, 9, 16, 17, 32, 33, 64} if f32 else {5, 8, 9, 16, 17, 32})
    if route == "SELL":
        assert seen[("spmm_sell", None)]["B"] >= set(b for b in SPMM_B if b >= 5)
    _spmm_report(route, dtype, seen)


@pytest.mark.parametrize("mem", [DEVICE, HOST], ids=["device", "host"])
@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
def test_spmm_padded_operands_in_every_layout_pair(dtype, mem, switches):
    """B = 4, 9, 64 with the four (r_layout, f_layout) pairs -- the mixed ones transpose one operand only -- on device
    canvases and on padded host operands.  A pair that is not row-major twice takes the SELL kernel."""
    env = dict(SS_NARROW_CHUNK=str(SPMM_CHUNK), SS_SELL_CHUNK=str(SPMM_CHUNK))
    switches(env)
    W = _spmm_case()[0]
    w = ss.DeviceSpMat(W.astype(dtype), dtype=dtype)
    for r_layout in (ROW, COL):
        for f_layout in (ROW, COL):
            seen = {}
            for B in (4, 9, 64):
                _spmm_sweep(w, dtype, mem, B, r_layout, f_layout, env, seen)
            if mem == DEVICE:
                if (r_layout, f_layout) != (ROW, ROW):
                    assert set(seen) == {("spmm_sell", None)}, seen.keys()
                _spmm_report(f"layouts r={r_layout} f={f_layout}", dtype, seen)
    w.close()


def test_spmm_refuses_short_leading_dimensions(switches):
    switches({})
    W, Rm, want = _spmm_case()
    M, K = W.shape
    B = 9
    for dtype in DTYPES:
        w = ss.DeviceSpMat(W.astype(dtype), dtype=dtype)
        Rb = np.ascontiguousarray(Rm[:, :B]).astype(dtype)
        fn = _fn("ss_spmm", dtype)
        for mem in (HOST, DEVICE):
            for r_layout, f_layout, dr, df in ((ROW, ROW, 1, 0), (ROW, ROW, 0, 1), (COL, COL, 1, 0), (COL, COL, 0, 1)):
                rcv, fcv = _spmm_canvases(Rb, want[:, :B], dtype, mem, r_layout, f_layout, 0, 0, 1, 1)
                if mem == DEVICE:
                    ss.use_torch_stream()
                assert fn(w._h, rcv.ptr, B, rcv.ld - dr, r_layout, fcv.ptr, fcv.ld - df, f_layout, mem) == EINVAL
                _sync()
                R.check(fcv, fcv.host(), fcv.window(fcv.host()).copy(), "short ld: F untouched")
        w.close()


# ----------------------------------------------------------------------------- consumers
NROWS = 40
FILLS = (np.inf, 1000.0)     # padding that would enter a top-L list or a pool if it were read: above every score


def _scores(nrows, ncols, dtype, seed):
    """Scores with many ties: k / 4 in [0, 8), a twentieth clean!'s -99; labels at about a tenth of the positions."""
    rng = np.random.default_rng(seed)
    Sc = (rng.integers(0, 32, (nrows, ncols)) / 4).astype(dtype)
    Sc[rng.random((nrows, ncols)) < 0.05] = dtype(-99.0)
    Y = sp.random(nrows, ncols, density=0.1, random_state=rng, format="csr")
    Y.data[:] = 1.0
    Y.sort_indices()
    return Sc, Y


class _Labels:
    """CSR positives (int64 ptr, int32 idx, base 0) in host or device memory."""

    def __init__(self, Y, mem):
        self.ptr = Y.indptr.astype(np.int64)
        self.idx = (Y.indices if Y.nnz else np.zeros(1)).astype(np.int32)
        if mem == DEVICE:
            import torch
            self.ptr, self.idx = torch.from_numpy(self.ptr).cuda(), torch.from_numpy(self.idx).cuda()
            self.p, self.i = self.ptr.data_ptr(), self.idx.data_ptr()
        else:
            self.p, self.i = self.ptr.ctypes.data, self.idx.ctypes.data


def _score_canvases(Sc, dtype):
    """Every (mem, fill, pad, front) canvas of a score block, with the block in its window."""
    nrows, ncols = Sc.shape
    for mem in (HOST, DEVICE):
        for fill in FILLS:
            for pad in PADS:
                for front in FRONTS:
                    yield mem, R.canvas(nrows, ncols, ncols + pad, front, BACK, dtype, mem, fill=fill).put(Sc)


@pytest.mark.parametrize("L", [1, 20])
@pytest.mark.parametrize("ncols", [7, 300, 5000])
def test_topl_reads_the_window_only(ncols, L, switches):
    """ss_topl_f32 on a padded score block whose padding holds +inf or 1000: the lists are the stable descending argsort
    of the window.  L = 20 of 7 columns is no list (L <= ncols): SS_EINVAL, idx and val untouched."""
    switches({})
    lib = ss._lib.lib()
    Sc, _ = _scores(NROWS, ncols, np.float32, 5 + ncols)
    order = np.argsort(-Sc.astype(np.float64), axis=1, kind="stable")[:, :min(L, ncols)]
    want_idx, want_val = order.astype(np.int32), np.take_along_axis(Sc, order, axis=1)
    import torch
    for mem, cv in _score_canvases(Sc, np.float32):
        if mem == DEVICE:
            idx = torch.full((NROWS, L), -7, dtype=torch.int32, device="cuda")
            val = torch.full((NROWS, L), -7.0, dtype=torch.float32, device="cuda")
            ss.use_torch_stream()
            rc = lib.ss_topl_f32(cv.ptr, NROWS, ncols, cv.ld, L, idx.data_ptr(), val.data_ptr(), mem)
            _sync()
            idx, val = idx.cpu().numpy(), val.cpu().numpy()
        else:
            idx, val = np.full((NROWS, L), -7, np.int32), np.full((NROWS, L), -7.0, np.float32)
            rc = lib.ss_topl_f32(cv.ptr, NROWS, ncols, cv.ld, L, idx.ctypes.data, val.ctypes.data, mem)
        label = f"top-{L} of {ncols}, {'device' if mem else 'host'}, ld {cv.ld}, front {cv.front}"
        if L > ncols:
            assert rc == EINVAL, label
            assert (idx == -7).all() and (val == -7.0).all(), label
        else:
            _ok(rc)
            np.testing.assert_array_equal(idx, want_idx, err_msg=label)
            np.testing.assert_array_equal(val.view(np.uint32), want_val.view(np.uint32), err_msg=label)
        R.check(cv, cv.host(), Sc, label)


def _same_bits(a, b, label):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    assert a.shape == b.shape and a.dtype == b.dtype, label
    assert np.array_equal(a.view(np.uint8), b.view(np.uint8)), label


@pytest.mark.parametrize("ncols", [7, 300])
@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
def test_pool_add_rows_reads_the_window_only(dtype, ncols, switches):
    """ss_pool_add_rows_* then export: the table of pooled_ref.table on the window, bitwise the table of the tight call."""
    switches({})
    Sc, Y = _scores(NROWS, ncols, dtype, 11 + ncols)
    want = pooled_ref.table(Y.toarray(), Sc)
    assert want[0].max() < 1000.0
    tight = ss.Pool(dtype).add_rows(Y, Sc)
    tight_table = tight.export()
    for a, b in zip(tight_table, want):
        _same_bits(a, b, "tight call against the reference")
    fn = _fn("ss_pool_add_rows", dtype)
    for mem, cv in _score_canvases(Sc, dtype):
        lab = _Labels(Y, mem)
        pool = ss.Pool(dtype)
        if mem == DEVICE:
            ss.use_torch_stream()
        _ok(fn(pool._h, lab.p, lab.i, 0, cv.ptr, NROWS, ncols, cv.ld, mem))
        _sync()
        label = f"pool, {_suf(dtype)}, {ncols} columns, {'device' if mem else 'host'}, ld {cv.ld}, front {cv.front}"
        assert pool.info()["n"] == NROWS * ncols and pool.info()["npos"] == Y.nnz, label
        for a, b in zip(pool.export(), tight_table):
            _same_bits(a, b, label)
        R.check(cv, cv.host(), Sc, label)
        pool.close()
    tight.close()


@pytest.mark.parametrize("ncols", [7, 300])
@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
def test_target_topl_add_rows_reads_the_window_only(dtype, ncols, switches):
    """ss_target_topl_add_rows_* with row_begin = 1000, then export: target_topl_ref.table on the window."""
    switches({})
    L, row_begin = 20, 1000
    Sc, Y = _scores(NROWS, ncols, dtype, 17 + ncols)
    rows = row_begin + np.arange(NROWS, dtype=np.int64)
    wv, wr, wl, wn = target_topl_ref.table(Y.toarray(), Sc, L, rows)
    fn = _fn("ss_target_topl_add_rows", dtype)
    for mem, cv in _score_canvases(Sc, dtype):
        lab = _Labels(Y, mem)
        h = ss.TargetTopL(ncols, L, dtype)
        if mem == DEVICE:
            ss.use_torch_stream()
        _ok(fn(h._h, lab.p, lab.i, 0, cv.ptr, NROWS, ncols, cv.ld, row_begin, mem))
        _sync()
        label = f"target top-L, {_suf(dtype)}, {ncols} targets, {'device' if mem else 'host'}, ld {cv.ld}, front {cv.front}"
        vals, rid, labels, npos, nadded = h.export()
        assert nadded == NROWS, label
        np.testing.assert_array_equal(rid, wr, err_msg=label)
        _same_bits(vals, wv, label)
        np.testing.assert_array_equal(labels, wl, err_msg=label)
        np.testing.assert_array_equal(npos, wn, err_msg=label)
        R.check(cv, cv.host(), Sc, label)
        h.close()
