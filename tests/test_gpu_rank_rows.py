"""Per-row ranking metrics on the device (ss_rank_metrics_rows_*) and the leave-one-out sweep evaluated in place
(ss_evaluate_loo_*), against the literal oracle (oracle.auroc / auprc / bedroc / validity_ratio), the single-vector
device route (ss.rank_metrics, ss.topl) and the host reference of tests/rank_ref.py."""
import os

import numpy as np
import pytest
import scipy.sparse as sp

import simspread_jl_amd as ss
from oracle import simspread_oracle as O
from rank_ref import assert_rows_close, ref_row, ref_rows
from simspread_jl_amd import _lib

pytestmark = pytest.mark.gpu

ALPHA = 20.0


def _oracle_rows(Y, S, L):
    out = []
    for y, s in zip(Y, S):
        with np.errstate(invalid="ignore", divide="ignore"):
            head = [O.auroc(y, s), O.auprc(y, s), O.bedroc(y, s, alpha=ALPHA), O.validity_ratio(s)]
        out.append(head + list(ref_row(y, s, ALPHA, L)[4:]))
    return np.array(out)


def _cases(ncols, L, rng, dtype):
    """A batch of rows of one width covering the edge cases; returns dense labels and scores."""
    rows_y, rows_s = [], []

    def add(y, s):
        rows_y.append(np.asarray(y, np.uint8))
        rows_s.append(np.asarray(s, np.float64))

    cont = rng.random(ncols)
    few = rng.choice(np.array([0.0, 0.25, 0.5, 1.0]), ncols)
    add(np.zeros(ncols), cont)                                   # P = 0
    add(np.zeros(ncols), np.full(ncols, 0.5))                    # P = 0, one score: AuROC 0 (no (0,0) point)
    y1 = np.zeros(ncols); y1[rng.integers(ncols)] = 1
    add(y1, cont)                                                # P = 1
    add(np.ones(ncols), cont)                                    # P = ncols
    add(np.ones(ncols), few)                                     # P = ncols, ties
    y = (rng.random(ncols) < 0.3).astype(np.uint8); y[0] = 1
    add(y, np.zeros(ncols))                                      # all-zero row
    add(y, np.full(ncols, -99.0))                                # all -99 (clean!) row
    add(y, few)                                                  # heavy ties
    m = few.copy(); m[rng.random(ncols) < 0.3] = -99.0
    add(y, m)                                                    # ties and -99
    # a tie group straddling rank L: L - 1 top scores, then a group of 3 holding positives and negatives
    s = np.full(ncols, 0.1); s[:max(L - 1, 0)] = 2.0 + np.arange(max(L - 1, 0))
    grp = np.arange(max(L - 1, 0), min(L + 2, ncols)); s[grp] = 1.0
    ys = np.zeros(ncols); ys[grp[-1]] = 1; ys[-1] = 1
    add(ys, s)
    yf = np.zeros(ncols); yf[0] = 1; yf[-1] = 1
    add(yf, cont)                                                # positives in the first and last column
    add(yf, few)
    for _ in range(4):
        yr = (rng.random(ncols) < rng.random()).astype(np.uint8)
        add(yr, np.where(rng.random(ncols) < 0.5, 0.0, rng.random(ncols)))
    S = np.stack(rows_s).astype(dtype)
    return np.stack(rows_y), S


def _raw_call(dtype, ptr, idx, base, S, ld, L, out, mem, nrows=None, ncols=None):
    fn = getattr(_lib.lib(), "ss_rank_metrics_rows_" + ("f32" if dtype == np.float32 else "f64"))
    return fn(ptr, idx, base, S, nrows, ncols, ld, ALPHA, L, out, mem)


def _check_against_everything(Y, S, got, L, dtype, what):
    # the literal oracle on the same (fp64-widened) scores
    assert_rows_close(got, _oracle_rows(Y, S.astype(np.float64), L), 1e-9, 1e-12, what + " vs oracle")
    if dtype == np.float32:
        want4 = np.array([[d[k] for k in ("AuROC", "AuPRC", "BEDROC", "validity_ratio")]
                          for d in (ss.rank_metrics(y, s, ALPHA) for y, s in zip(Y, S))])
        assert_rows_close(got[:, :4], want4, 1e-12, 1e-14, what + " vs ss.rank_metrics")
        idx, _ = ss.topl(S, L)
        hits = np.take_along_axis(Y, idx.astype(np.int64), axis=1).sum(1)
    else:
        order = np.argsort(-S, axis=1, kind="stable")[:, :L]
        hits = np.take_along_axis(Y, order, axis=1).sum(1)
    P = Y.sum(1)
    with np.errstate(invalid="ignore", divide="ignore"):
        rec = np.where(P > 0, hits / np.maximum(P, 1), np.nan)
    np.testing.assert_array_equal(got[:, 4], rec)
    np.testing.assert_array_equal(got[:, 5], hits / L)


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("ncols, L, pad", [(2, 1, 0), (37, 5, 3), (300, 20, 0), (129, 64, 7)])
def test_case_matrix_host_device_torch(dtype, ncols, L, pad):
    import torch
    ss.init(0)
    rng = np.random.default_rng(1000 + ncols)
    Y, S = _cases(ncols, L, rng, dtype)
    nrows = S.shape[0]
    got = ss.rank_metrics_rows(Y, S, alpha=ALPHA, L=L)
    assert got.shape == (nrows, 6) and got.dtype == np.float64
    _check_against_everything(Y, S, got, L, dtype, f"{np.dtype(dtype).name} ncols={ncols}")
    assert "rank_rows_lds" in ss.path_last()
    # repeated call: bitwise identical
    np.testing.assert_array_equal(ss.rank_metrics_rows(sp.csr_matrix(Y), S, alpha=ALPHA, L=L), got)
    # torch: scores on the device, labels on the host and as a device CSR pair
    tS = torch.from_numpy(S).cuda()
    g1 = ss.rank_metrics_rows(Y, tS, alpha=ALPHA, L=L)
    assert g1.is_cuda and g1.dtype == torch.float64
    np.testing.assert_array_equal(g1.cpu().numpy(), got)
    m = sp.csr_matrix(Y)
    dptr = torch.from_numpy(m.indptr.astype(np.int64)).cuda()
    didx = torch.from_numpy(m.indices.astype(np.int32)).cuda()
    np.testing.assert_array_equal(ss.rank_metrics_rows((dptr, didx), tS, alpha=ALPHA, L=L).cpu().numpy(), got)
    # raw ABI: ld > ncols, a label slice of a larger CSR (yptr[0] != base), index_base 1; host and device memory
    ld = ncols + pad
    Sp = np.zeros((nrows, ld), dtype); Sp[:, :ncols] = S
    lead = np.array([[1] + [0] * (ncols - 1)] * 3, np.uint8)                 # 3 rows in front of the slice
    big = sp.csr_matrix(np.vstack([lead, Y]))
    for base in (0, 1):
        ptr = (big.indptr.astype(np.int64) + base)[3:]                         # rows 3.. of the big CSR
        idx = big.indices.astype(np.int32) + base
        assert ptr[0] != base
        out = np.full((nrows, 6), -7.0)
        assert _raw_call(dtype, ptr.ctypes.data, idx.ctypes.data, base, Sp.ctypes.data, ld, L, out.ctypes.data,
                         _lib.SS_MEM_HOST, nrows, ncols) == 0
        np.testing.assert_array_equal(out, got)
        tp, ti, tsp = (torch.from_numpy(a).cuda() for a in (ptr, idx, Sp))
        tout = torch.full((nrows, 6), -7.0, dtype=torch.float64, device="cuda")
        ss.use_torch_stream()
        assert _raw_call(dtype, tp.data_ptr(), ti.data_ptr(), base, tsp.data_ptr(), ld, L, tout.data_ptr(),
                         _lib.SS_MEM_DEVICE, nrows, ncols) == 0
        np.testing.assert_array_equal(tout.cpu().numpy(), got)
    # nrows == 0 is a no-op
    assert _raw_call(dtype, ptr.ctypes.data, idx.ctypes.data, 0, Sp.ctypes.data, ld, L, None, _lib.SS_MEM_HOST, 0,
                     ncols) == 0


def test_fp64_scores_below_fp32_resolution_are_not_ties():
    ss.init(0)
    n = 64
    rng = np.random.default_rng(5)
    s64 = 1.0 + rng.permutation(n) * 1e-12                      # distinct in fp64, one value in fp32
    y = np.zeros((1, n), np.uint8); y[0, np.argsort(-s64)[:8]] = 1   # the 8 best are the positives
    s64 = s64[None]
    got64 = ss.rank_metrics_rows(y, s64, alpha=ALPHA, L=8)
    assert_rows_close(got64, _oracle_rows(y, s64, 8), 1e-9, 1e-12, "fp64")
    assert got64[0, 0] == 1.0 and got64[0, 4] == 1.0
    got32 = ss.rank_metrics_rows(y, s64.astype(np.float32), alpha=ALPHA, L=8)
    assert_rows_close(got32, _oracle_rows(y, s64.astype(np.float32), 8), 1e-9, 1e-12, "fp32 rounded")
    assert got32[0, 0] != got64[0, 0] and got32[0, 2] != got64[0, 2]


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_large_positive_counts_take_the_global_path(dtype):
    import torch
    ss.init(0)
    n = 100_000
    rng = np.random.default_rng(9)
    S = np.empty((6, n))
    Y = np.zeros((6, n), np.uint8)
    S[0] = rng.random(n); Y[0] = 1                                          # P = ncols
    S[1] = rng.choice(np.array([0.0, 0.5, 1.0, -99.0]), n); Y[1] = 1         # P = ncols, four tie groups
    S[2] = np.round(rng.random(n), 3); Y[2, rng.random(n) < 0.3] = 1         # ~30k positives, heavy ties
    S[3] = np.where(rng.random(n) < 0.6, 0.0, rng.random(n)); Y[3, rng.choice(n, 2049, replace=False)] = 1  # just past LDS
    S[4] = rng.random(n); Y[4, rng.choice(n, 500, replace=False)] = 1        # LDS path rows in the same call
    S[5] = np.where(rng.random(n) < 0.9, 0.0, rng.random(n)); Y[5, rng.choice(n, 2048, replace=False)] = 1
    S = S.astype(dtype)
    got = ss.rank_metrics_rows(Y, S, alpha=ALPHA, L=20)
    path = ss.path_last()
    assert "rank_rows_lds" in path and "rank_rows_large" in path, path
    assert_rows_close(got, ref_rows(Y, S.astype(np.float64), ALPHA, 20), 1e-9, 1e-12, "large P vs host reference")
    if dtype == np.float32:
        want4 = np.array([[d[k] for k in ("AuROC", "AuPRC", "BEDROC", "validity_ratio")]
                          for d in (ss.rank_metrics(y, s, ALPHA) for y, s in zip(Y, S))])
        assert_rows_close(got[:, :4], want4, 1e-12, 1e-14, "large P vs ss.rank_metrics")
    # each row alone (some then take a different path set): the same bits
    for i in range(6):
        np.testing.assert_array_equal(ss.rank_metrics_rows(Y[i:i + 1], S[i:i + 1], alpha=ALPHA, L=20), got[i:i + 1])
    tS = torch.from_numpy(S).cuda()
    np.testing.assert_array_equal(ss.rank_metrics_rows(Y, tS, alpha=ALPHA, L=20).cpu().numpy(), got)


@pytest.mark.parametrize("mem", ["host", "device"])
@pytest.mark.parametrize("bad", ["range", "unsorted", "duplicate", "negative"])
def test_bad_labels_are_refused_and_nothing_is_written(mem, bad):
    import torch
    ss.init(0)
    rng = np.random.default_rng(3)
    S = rng.random((3, 10)).astype(np.float32)
    idx = {"range": [1, 3, 10, 2, 5], "unsorted": [1, 3, 2, 0, 5], "duplicate": [1, 3, 3, 2, 5],
           "negative": [1, 3, 4, -1, 5]}[bad]
    ptr = np.array([0, 3, 3, 5], np.int64)
    idx = np.array(idx, np.int32)
    if mem == "host":
        out = np.full((3, 6), -7.0)
        rc = _raw_call(np.float32, ptr.ctypes.data, idx.ctypes.data, 0, S.ctypes.data, 10, 2, out.ctypes.data,
                       _lib.SS_MEM_HOST, 3, 10)
        assert (out == -7.0).all()
    else:
        tp, ti, ts = (torch.from_numpy(a).cuda() for a in (ptr, idx, S))
        tout = torch.full((3, 6), -7.0, dtype=torch.float64, device="cuda")
        ss.use_torch_stream()
        rc = _raw_call(np.float32, tp.data_ptr(), ti.data_ptr(), 0, ts.data_ptr(), 10, 2, tout.data_ptr(),
                       _lib.SS_MEM_DEVICE, 3, 10)
        assert (tout.cpu().numpy() == -7.0).all()
    assert rc == -1, rc


def test_bad_shapes_are_refused():
    ss.init(0)
    S = np.zeros((1, 4), np.float32)
    ptr, idx = np.array([0, 1], np.int64), np.array([2], np.int32)
    out = np.zeros((1, 6))
    for ncols, L in ((1, 1), (4, 4), (4, 0), (1 << 31, 1)):
        assert _raw_call(np.float32, ptr.ctypes.data, idx.ctypes.data, 0, S.ctypes.data, max(ncols, 4), L,
                         out.ctypes.data, _lib.SS_MEM_HOST, 1, ncols) == -1, (ncols, L)
    assert _raw_call(np.float32, ptr.ctypes.data, idx.ctypes.data, 0, S.ctypes.data, 4, 4, out.ctypes.data,
                     _lib.SS_MEM_HOST, 1, 4) == -1
    assert b"Number of labels is less than length" in _lib.lib().ss_last_error()
    assert (out == 0).all()


# ------------------------------------------------------------------ evaluate_loo
def _square_graph(rng, n, nt, dtype, weighted=True):
    Xs = sp.random(n, n, density=0.08, random_state=rng, format="csr")
    Xs = Xs + Xs.T + sp.identity(n)
    Xs.data[:] = rng.uniform(0.5, 1.0, Xs.nnz) if weighted else 1.0
    Ys = sp.random(n, nt, density=0.15, random_state=rng, format="csr")
    Ys.data[:] = 1.0
    Ys.sort_indices()
    return sp.csr_matrix(Xs), sp.csr_matrix(Ys)


def _device_reference(g, i0, i1, clean, L):
    """predict_loo into a device buffer, then rank_metrics_rows on it against the graph's labels."""
    import torch
    dt = torch.float32 if g.dtype == np.float32 else torch.float64
    out = torch.empty((i1 - i0, g.nt), dtype=dt, device="cuda")
    g.predict_loo(i0, i1, clean=clean, out=out)
    return out


def _same_ties(a, b):
    """Rows whose scores have the same order and tie pattern in a and b (the oracle and the device may round a
    mathematically tied pair apart)."""
    keep = []
    for x, y in zip(a, b):
        ox, oy = np.argsort(-x, kind="stable"), np.argsort(-y, kind="stable")
        keep.append(np.array_equal(ox, oy) and np.array_equal(np.diff(x[ox]) == 0, np.diff(y[oy]) == 0))
    return np.array(keep)


def _evaluate_and_compare(g, Ylab, Xw, clean, L, want_scores=None):
    import torch
    n = g.ns
    scores = _device_reference(g, 0, n, clean, L)
    m = sp.csr_matrix(Ylab)
    m.eliminate_zeros()
    dptr = torch.from_numpy(m.indptr.astype(np.int64)).cuda()
    didx = torch.from_numpy(m.indices.astype(np.int32) if m.nnz else np.zeros(1, np.int32)).cuda()
    ref = ss.rank_metrics_rows((dptr, didx), scores, alpha=ALPHA, L=L).cpu().numpy()
    for br in (1, 7, 0):
        got = g.evaluate_loo(0, n, clean=clean, alpha=ALPHA, L=L, block_rows=br)
        np.testing.assert_array_equal(got, ref)
    sub = g.evaluate_loo(3, n - 2, clean=clean, alpha=ALPHA, L=L, block_rows=5)
    np.testing.assert_array_equal(sub, ref[3:n - 2])
    if Xw is not None:
        want_scores = O.predict_loo_factored(Xw, sp.csr_matrix(Ylab, dtype=np.float64), clean_flag=clean)
    if want_scores is not None:
        dev = scores.cpu().numpy().astype(np.float64)
        keep = _same_ties(dev, want_scores)
        assert keep.mean() > 0.5, keep.mean()
        Yd = sp.csr_matrix(Ylab).toarray() != 0
        assert_rows_close(ref[keep], _oracle_rows(Yd[keep], want_scores[keep], L),
                          1e-6 if g.dtype == np.float32 else 1e-9, 1e-9, "evaluate_loo vs oracle scores")
    return ref


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("clean", [False, True])
def test_evaluate_loo_csr_graph(dtype, clean):
    ss.init(0)
    rng = np.random.default_rng(21)
    Xs, Ys = _square_graph(rng, 60, 40, dtype)
    g = ss.DeviceGraph.from_sparse(None, Xs, Ys, dtype=dtype)
    _evaluate_and_compare(g, Ys, Xs.astype(dtype).astype(np.float64), clean, 5)
    assert "rank_rows_lds" in ss.path_last() and "transfer_loo" in ss.path_last()
    g.close()


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("clean", [False, True])
def test_evaluate_loo_dense_similarity_graph(dtype, clean):
    ss.init(0)
    rng = np.random.default_rng(22)
    n, nt, alpha = 80, 30, 0.6
    F = rng.random((n, 12))
    S = (np.minimum(F[:, None], F[None]).sum(-1) / np.maximum(F[:, None], F[None]).sum(-1)).astype(dtype)
    Y = sp.random(n, nt, density=0.2, random_state=rng, format="csr"); Y.data[:] = 1.0
    g = ss.DeviceGraph.from_similarity(None, S, Y, alpha=alpha, weighted=True, dtype=dtype)
    _evaluate_and_compare(g, Y, None, clean, 3)
    g.close()


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("clean", [False, True])
def test_evaluate_loo_fingerprint_graph(dtype, clean):
    ss.init(0)
    rng = np.random.default_rng(23)
    n, nt, bits = 90, 25, 128
    B = rng.random((n, bits)) < 0.3
    Y = sp.random(n, nt, density=0.2, random_state=rng, format="csr"); Y.data[:] = 1.0
    g = ss.DeviceGraph.from_fingerprints(None, ss.pack_fingerprints(B), Y, alpha=0.2, weighted=True, dtype=dtype)
    inter = B.astype(np.float64) @ B.T.astype(np.float64)
    cnt = B.sum(1).astype(np.float64)
    with np.errstate(invalid="ignore", divide="ignore"):
        T = np.where(cnt[:, None] + cnt[None] - inter == 0, 1.0, inter / (cnt[:, None] + cnt[None] - inter))
    T = T.astype(dtype).astype(np.float64)
    X = sp.csr_matrix(np.where(T >= float(dtype(0.2)), T, 0.0))
    _evaluate_and_compare(g, Y, X, clean, 4)
    g.close()


def _iris():
    here = os.path.join(os.path.dirname(__file__), "golden", "iris")

    def read(p):
        with open(os.path.join(here, p)) as f:
            lines = f.read().splitlines()
        return np.array([[float(v) for v in l.split()[1:]] for l in lines[1:]])
    F, Cm = read("iris.features"), read("iris.classes")
    S = np.minimum(F[:, None, :], F[None, :, :]).sum(-1) / np.maximum(F[:, None, :], F[None, :, :]).sum(-1)
    return S, Cm


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("weighted", [False, True])
def test_evaluate_loo_iris(dtype, weighted):
    ss.init(0)
    S, Cm = _iris()
    g = ss.DeviceGraph.from_dense(None, S.astype(dtype), Cm.astype(dtype), alpha=dtype(0.9), weighted=weighted,
                                  dtype=dtype)
    X = O.cutoff(S.astype(dtype).astype(np.float64), float(dtype(0.9)), weighted)
    for clean in (True, False):
        want = O.predict_loo_factored(X, Cm, clean_flag=clean)
        ref = _evaluate_and_compare(g, sp.csr_matrix(Cm), None, clean, 1, want_scores=want)
        assert ref.shape == (150, 6) and np.nanmean(ref[:, 0]) > 0.9          # iris is easy
    g.close()


# ------------------------------------------------------------------ at size
def _at_size_check(g, labels, lo, folds, sample_rng, what):
    """evaluate_loo over [lo, lo + folds) == predict_loo + rank_metrics_rows bit for bit; 32 folds against the
    single-vector device route and the host reference on the same scores."""
    import torch
    n = g.nt
    out = torch.empty((folds, n), dtype=torch.float32, device="cuda")
    g.predict_loo(lo, lo + folds, clean=True, out=out)
    ptr_all, idx_all = labels
    ptr = (ptr_all[lo:lo + folds + 1]).contiguous()
    ref = ss.rank_metrics_rows((ptr, idx_all), out, alpha=ALPHA, L=20).cpu().numpy()
    path_rows = ss.path_last()
    got = g.evaluate_loo(lo, lo + folds, clean=True, alpha=ALPHA, L=20, block_rows=0)
    path_eval = ss.path_last()
    np.testing.assert_array_equal(got, ref)
    pos = ptr.cpu().numpy()
    idx_h = idx_all.cpu().numpy()
    for i in sample_rng.choice(folds, 32, replace=False):
        y = np.zeros(n, np.uint8)
        y[idx_h[pos[i]:pos[i + 1]]] = 1
        s = out[i].cpu().numpy()
        d = ss.rank_metrics(y, s, ALPHA)
        assert_rows_close(got[i:i + 1, :4], np.array([[d["AuROC"], d["AuPRC"], d["BEDROC"], d["validity_ratio"]]]),
                          1e-12, 1e-14, f"{what} fold {lo + i}")
        assert_rows_close(got[i:i + 1], ref_row(y, s, ALPHA, 20)[None], 1e-9, 1e-12, f"{what} fold {lo + i} (host)")
    return path_rows, path_eval


def test_c3_block_evaluated_in_place():
    """C3: 100k x 100k at 1 %, a 2048-fold block."""
    import torch
    from tools.c3_loo import rand_csr, rand_sym_csr
    ss.init(0)
    ss.use_torch_stream()
    n, folds = 100_000, 2048
    gen = torch.Generator(device="cuda"); gen.manual_seed(20250222 + 3)
    xp, xi = rand_sym_csr(n, 0.01, gen)
    yp, yi = rand_csr(n, n, 0.01, gen)
    xv = (0.5 + 0.5 * torch.rand(xi.numel(), device="cuda", generator=gen)).float()
    g = ss.DeviceGraph.from_device_csr(0, n, n, n, None, (xp, xi, xv), (yp, yi, None), dtype=np.float32)
    path_rows, path_eval = _at_size_check(g, (yp, yi), 40_000, folds, np.random.default_rng(0), "C3")
    assert "rank_rows_lds" in path_eval and "transfer_loo" in path_eval, path_eval
    g.close()


def test_c5_block_with_hot_sources_evaluated_in_place():
    """C5: Zipf(1.2) source degrees capped at nt; the block holds hot sources (> 2048 positives)."""
    import torch
    from tools.c3_loo import rand_sym_csr
    from tools.c5_powerlaw import zipf_bipartite_spec
    ss.init(0)
    ss.use_torch_stream()
    n = 100_000
    gen = torch.Generator(device="cuda"); gen.manual_seed(20250222 + 5)
    xp, xi = rand_sym_csr(n, 0.01, gen)
    yp, yi = zipf_bipartite_spec(n, n, 1000, 1.2, gen)
    xv = (0.5 + 0.5 * torch.rand(xi.numel(), device="cuda", generator=gen)).float()
    g = ss.DeviceGraph.from_device_csr(0, n, n, n, None, (xp, xi, xv), (yp, yi, None), dtype=np.float32)
    deg = (yp[1:] - yp[:-1]).cpu().numpy()
    hot = int(np.argmax(deg))
    lo = max(0, min(hot - 100, n - 512))
    assert deg[lo:lo + 512].max() > 2048
    path_rows, path_eval = _at_size_check(g, (yp, yi), lo, 512, np.random.default_rng(1), "C5")
    assert "rank_rows_large" in path_eval and "rank_rows_lds" in path_eval, path_eval
    assert "rank_rows_large" in path_rows, path_rows
    g.close()
