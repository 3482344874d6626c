"""Slot lending in the wide stage-2 operand (DevSell, graph.hpp; sell_plan_kernel / sell_fill_sched_kernel, assemble.hip;
spmm_sell_kernel, kernels.hip): a slice ends below its longest rows when their excess fits the free slots of short rows.

ss_spmm on the SELL route (SS_COL=0, column-major operands), B = 4 and 7 (a ragged last tile), fp32 and fp64, weighted
and pattern-only.  Operands are exact (weights k/16, R = i/16 with small integers: every partial sum is a multiple of
2^-8 below 2^7), so the scores equal the fp64 host product bit for bit with lending on and off; the random-value cases
use the per-score band of sparse_ref.  The planning rule is restated below (plan) and the builder's storage, reported
under SS_SELL_STATS=1, must be the rule's."""
import re

import numpy as np
import pytest
import scipy.sparse as sp

import simspread_jl_amd as ss

import sparse_ref as S

pytestmark = pytest.mark.gpu

SWITCHES = ("SS_SELL_LEND", "SS_SELL_STATS", "SS_COL", "SS_SELL_CHUNK", "SS_SELL_QT", "SS_SELL_PLAIN", "SS_SELL_SORT",
            "SS_SELL_LMAX")
MAX_CHUNK = 160 * 1024 // 16 - 16          # sell_max_chunk: 16-byte tile rows in 160 KiB of LDS next to 16 zero rows
Q1_STEP, R_MAX = 8, 3                      # SELL_Q1_STEP, SELL_LEND_R (graph.hpp)
DTYPES = [np.float32, np.float64]
WIDTHS = (4, 7)


@pytest.fixture(scope="module", autouse=True)
def _init():
    ss.init(0)


@pytest.fixture(autouse=True)
def _env(monkeypatch):
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setenv("SS_COL", "0")
    monkeypatch.setenv("SS_SELL_STATS", "1")


# ----------------------------------------------------------------------------- the rule, restated
def plan(n):
    """(Q1, Q2) of one slice from the entries of its 64 lanes: the smallest Q2 below the longest row for which, with
    receivers = lanes of at most 4 Q1 entries (Q1 a multiple of Q1_STEP) offering 4 (Q2 - Q1) slots to one donor each,
    every row's excess over 4 Q2 fits at most R_MAX receivers and all needs fit the receivers; ties: the largest Q1."""
    n = np.asarray(n, dtype=np.int64)
    qmax = int((n.max() + 3) // 4)
    best = (qmax, qmax)
    for q1 in range(0, max(qmax - 1, 0), Q1_STEP):
        nrecv = int((n <= 4 * q1).sum())
        for q2 in range(q1 + 1, qmax):
            cap = 4 * (q2 - q1)
            need = -(-np.maximum(n - 4 * q2, 0) // cap)
            if need.max() <= R_MAX and need.sum() <= nrecv:
                if q2 <= best[1]:
                    best = (q1, q2)
                break
    return best


def plan_matrix(W, chunk=MAX_CHUNK):
    """Stored quads and the donor rows of W under the rule (rows in slices of 64, columns in chunks)."""
    W = sp.csr_matrix(W)
    M, K = W.shape
    quads, donors, lending = 0, np.zeros(M, bool), 0
    for k0 in range(0, K, chunk):
        n = np.diff(W[:, k0:k0 + chunk].tocsr().indptr)
        for r0 in range(0, M, 64):
            lanes = np.zeros(64, np.int64)
            lanes[:min(64, M - r0)] = n[r0:r0 + 64]
            q1, q2 = plan(lanes)
            quads += q2
            lending += q1 < q2
            donors[r0:r0 + 64] |= (lanes > 4 * q2)[:min(64, M - r0)]
    return quads, donors, lending


# ----------------------------------------------------------------------------- operands
def matrix(lengths, K, weighted, seed=5, exact=True, col0=0, width=None):
    """Row i has lengths[i] entries in distinct random columns of [col0, col0 + width)."""
    rng = np.random.default_rng(seed)
    width = K - col0 if width is None else width
    rows, cols = [], []
    for i, ln in enumerate(lengths):
        rows += [i] * ln
        cols += list(col0 + rng.choice(width, size=ln, replace=False))
    if not weighted:
        vals = np.ones(len(rows))
    elif exact:
        vals = rng.integers(8, 17, size=len(rows)) / 16.0
    else:
        vals = 0.5 + 0.5 * rng.random(len(rows))
    return sp.csr_matrix((vals, (rows, cols)), shape=(len(lengths), K))


def dense_R(K, exact, seed=9):
    rng = np.random.default_rng(seed)
    return rng.integers(-8, 9, size=(K, max(WIDTHS))) / 16.0 if exact else rng.standard_normal((K, max(WIDTHS)))


def product(W, R, dtype, lend, monkeypatch, capfd):
    """W @ R[:, :B] for every width on a freshly cut operand; the tags of the calls and the builder's report."""
    monkeypatch.setenv("SS_SELL_LEND", "1" if lend else "0")
    capfd.readouterr()
    w = ss.DeviceSpMat(sp.csr_matrix(W).astype(dtype), dtype=dtype)
    out, tags = {}, set()
    for B in WIDTHS:
        Rt = np.ascontiguousarray(R[:, :B].T).astype(dtype)
        out[B] = np.ascontiguousarray(w.spmm(Rt, colmajor=True).T)
        path = ss.path_last()
        assert "spmm_sell" in path, path
        tags |= set(path)
    w.close()
    m = re.search(r"sell_build: .* nnz (\d+) .* quads (\d+) slots_per_nnz ([0-9.]+) lend (\d)", capfd.readouterr().err)
    assert m, "no report from the builder under SS_SELL_STATS=1"
    return out, tags, dict(nnz=int(m.group(1)), quads=int(m.group(2)), lend=int(m.group(4)))


def check_exact(lengths, K, dtype, weighted, monkeypatch, capfd, lends, W=None):
    """Lending on and off equal the fp64 product bit for bit; two builds give the same bits; storage follows the rule."""
    W = matrix(lengths, K, weighted) if W is None else W
    R = dense_R(K, exact=True)
    on, tags_on, st_on = product(W, R, dtype, True, monkeypatch, capfd)
    again, _, st_again = product(W, R, dtype, True, monkeypatch, capfd)
    off, tags_off, st_off = product(W, R, dtype, False, monkeypatch, capfd)
    for B in WIDTHS:
        want = W @ R[:, :B]
        S.assert_bitwise(on[B], want, dtype, f"lending on, B = {B}")
        S.assert_bitwise(off[B], want, dtype, f"lending off, B = {B}")
        S.assert_bitwise(again[B], want, dtype, f"second build, B = {B}")
    quads, _, lending = plan_matrix(W)
    plain = sum(int((np.diff(W[r0:r0 + 64, k0:k0 + MAX_CHUNK].tocsr().indptr).max() + 3) // 4)
                for k0 in range(0, W.shape[1], MAX_CHUNK) for r0 in range(0, W.shape[0], 64))
    print(f"[sell_lend] quads: rule {quads}, built {st_on['quads']}, plain {st_off['quads']} ({plain}); nnz {W.nnz}")
    assert st_on["quads"] == st_again["quads"] == quads and st_off["quads"] == plain
    assert ("sell_lend" in tags_on) == lends == bool(lending) == bool(st_on["lend"])
    assert "sell_lend" not in tags_off and st_off["lend"] == 0
    return st_on, st_off


CASES = [(dt, w) for dt in DTYPES for w in (True, False)]
IDS = [f"{np.dtype(dt).name}-{'weighted' if w else 'pattern-only'}" for dt, w in CASES]


# ----------------------------------------------------------------------------- the cases
@pytest.mark.parametrize("dtype,weighted", CASES, ids=IDS)
def test_rows_of_equal_length_do_not_lend(dtype, weighted, monkeypatch, capfd):
    """Rows of 8 entries: full slices have nobody to lend (M = 64, 128: no tag, the plain storage).  With M = 130 the
    two full slices stay plain as well, but the last slice holds two rows and 62 lanes past the last row, and those
    lanes may receive (the rule that the ragged-slice test relies on): it ends after one quad instead of two, so this
    operand carries the tag -- the rule leaves no other outcome -- and stores exactly one quad less."""
    for M in (64, 128):
        on, off = check_exact([8] * M, 300, dtype, weighted, monkeypatch, capfd, lends=False)
        assert on["quads"] == off["quads"]
    on, off = check_exact([8] * 130, 300, dtype, weighted, monkeypatch, capfd, lends=True)
    assert (on["quads"], off["quads"]) == (5, 6)


@pytest.mark.parametrize("dtype,weighted", CASES, ids=IDS)
def test_one_long_row_lends_from_every_read_group(dtype, weighted, monkeypatch, capfd):
    """One row of 40 among 63 of 8: the receivers are rows of at most 32 entries, the slice ends at 9 quads, not 10."""
    for lane in (0, 15, 16, 31, 32, 63):
        lengths = [8] * 64
        lengths[lane] = 40
        on, off = check_exact(lengths, 300, dtype, weighted, monkeypatch, capfd, lends=True)
        assert on["quads"] < off["quads"]


@pytest.mark.parametrize("dtype,weighted", CASES, ids=IDS)
def test_a_row_that_needs_more_receivers_raises_the_level(dtype, weighted, monkeypatch, capfd):
    """One row of 200 among rows of 8: three receivers hold its excess only from Q2 = 19 on (Q1 = 8): 200 - 76 = 124
    entries in 3 x 44 slots; at Q2 = 18 they would be 128 in 3 x 40 -- four receivers."""
    lengths = [8] * 64
    lengths[21] = 200
    on, off = check_exact(lengths, 300, dtype, weighted, monkeypatch, capfd, lends=True)
    assert (on["quads"], off["quads"]) == (19, 50)


@pytest.mark.parametrize("dtype,weighted", CASES, ids=IDS)
def test_no_possible_receiver_keeps_the_plain_layout(dtype, weighted, monkeypatch, capfd):
    lengths = [12] * 64
    lengths[40] = 16
    on, off = check_exact(lengths, 300, dtype, weighted, monkeypatch, capfd, lends=False)
    assert on["quads"] == off["quads"] == 4


@pytest.mark.parametrize("dtype,weighted", CASES, ids=IDS)
def test_ragged_last_slice_lends_to_the_lanes_past_the_last_row(dtype, weighted, monkeypatch, capfd):
    """M = 65 and 127, empty rows among the others: the long last row of the last slice lends to empty rows and to the
    lanes behind it; the product has exactly M rows."""
    for M in (65, 127):
        lengths = [0 if i % 5 == 2 else 8 for i in range(M)]
        lengths[M - 1] = 60
        lengths[3] = 44
        on, off = check_exact(lengths, 300, dtype, weighted, monkeypatch, capfd, lends=True)
        assert on["quads"] < off["quads"]


@pytest.mark.parametrize("dtype,weighted", CASES, ids=IDS)
def test_random_lengths_store_few_slots_and_leave_other_rows_alone(dtype, weighted, monkeypatch, capfd):
    """3 x 64 rows of Poisson(100) entries, K = 2000, standard-normal R: at most 1.10 slots per non-zero (the rule gives
    that on these lengths: checked first, on the host), every score within its band, rows that are not donors bit for bit
    what the plain layout gives, two builds the same bits."""
    lengths = np.random.default_rng(17).poisson(100, 192)
    W = matrix(list(lengths), 2000, weighted, exact=False)
    quads, donors, lending = plan_matrix(W)
    print(f"[sell_lend] rule: {quads * 256 / W.nnz:.4f} slots per non-zero, {int(donors.sum())} donor rows")
    assert quads * 256 / W.nnz <= 1.10 and lending == 3 and 0 < donors.sum() < 192
    R = dense_R(2000, exact=False)
    on, tags, st = product(W, R, dtype, True, monkeypatch, capfd)
    again, _, _ = product(W, R, dtype, True, monkeypatch, capfd)
    off, _, st_off = product(W, R, dtype, False, monkeypatch, capfd)
    print(f"[sell_lend] built: {st['quads'] * 256 / st['nnz']:.4f} slots per non-zero, plain {st_off['quads'] * 256 / st_off['nnz']:.4f}")
    assert st["quads"] == quads and st["quads"] * 256 / st["nnz"] <= 1.10 and "sell_lend" in tags
    bits = np.uint32 if dtype == np.float32 else np.uint64
    for B in WIDTHS:
        Rb = R[:, :B].astype(dtype).astype(np.float64)
        want = W.astype(dtype).astype(np.float64) @ Rb
        S.assert_band(on[B], want, S.band_spmm(W, Rb, dtype, 1 + R_MAX), f"lending on, B = {B}")
        S.assert_band(off[B], want, S.band_spmm(W, Rb, dtype, 1), f"lending off, B = {B}")
        np.testing.assert_array_equal(on[B].view(bits), again[B].view(bits))
        np.testing.assert_array_equal(on[B][~donors].view(bits), off[B][~donors].view(bits))


@pytest.mark.parametrize("dtype,weighted", CASES, ids=IDS)
def test_two_chunks_lend_in_both_and_accumulate(dtype, weighted, monkeypatch, capfd):
    """K = largest chunk + 50, 70 rows: the first chunk lends in both slices (the second to the lanes past row 69), the
    50 columns of the second chunk too; its sums are added to the first chunk's in F."""
    K = MAX_CHUNK + 50
    first = [8] * 70
    first[9], first[66] = 120, 100
    second = [4] * 70
    second[30], second[9], second[69] = 40, 36, 44
    W = matrix(first, K, weighted, seed=1, width=MAX_CHUNK) + matrix(second, K, weighted, seed=2, col0=MAX_CHUNK)
    _, _, lending = plan_matrix(W)
    assert lending == 4
    check_exact(None, K, dtype, weighted, monkeypatch, capfd, lends=True, W=sp.csr_matrix(W))


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f64"])
def test_clean_and_kfold_rows_on_a_lending_operand(dtype, monkeypatch, capfd):
    """The store's epilogue on a graph whose W = Ys' lends: targets without an edge read -99 (clean_deg), k-fold rows go
    to their sources' rows (out_rows).  Against the plain layout: targets that are not donors bit for bit, donors within
    two chains' roundings of a sum of non-negative terms."""
    rng = np.random.default_rng(23)
    ns, nt, nfolds = 96, 130, 4
    X = sp.random(ns, ns, density=0.2, random_state=rng, format="csr")
    X.data = 0.5 + 0.5 * X.data
    X = sp.csr_matrix(X + X.T + sp.eye(ns))
    deg = [0 if t % 9 == 4 else 8 for t in range(nt)]
    deg[7], deg[70], deg[129] = 40, 60, 36
    Y = sp.csr_matrix(matrix(deg, ns, weighted=False, seed=4).T)
    _, donors, lending = plan_matrix(Y.T)
    assert lending == 3 and donors.sum() == 3
    fold = np.arange(ns) % nfolds
    res = {}
    for lend in (True, False):
        monkeypatch.setenv("SS_SELL_LEND", "1" if lend else "0")
        g = ss.DeviceGraph.from_sparse(None, X.astype(dtype), Y.astype(dtype), dtype=dtype)
        a = g.predict("source", clean=True)
        assert ("sell_lend" in ss.path_last()) == lend and "spmm_sell" in ss.path_last(), ss.path_last()
        b = g.predict_kfold_rows(np.asarray(fold), nfolds, 5, 90)
        assert ("sell_lend" in ss.path_last()) == lend, ss.path_last()
        res[lend] = (a, b)
        g.close()
    empty = np.asarray(deg) == 0
    u = S.U32 if dtype == np.float32 else S.U64
    bits = np.uint32 if dtype == np.float32 else np.uint64
    for on, off in zip(res[True], res[False]):
        np.testing.assert_array_equal(on[:, ~donors].view(bits), off[:, ~donors].view(bits))
        tol = 2 * S.gamma(60 + R_MAX + 1, u) * np.maximum(np.abs(on), np.abs(off))[:, donors]
        assert (np.abs(on.astype(np.float64) - off)[:, donors] <= tol).all()
    np.testing.assert_array_equal(res[True][0] == -99, np.broadcast_to(empty, res[True][0].shape))
    assert not (res[True][1] == -99).any()
