"""k-fold cross-validation in row blocks (ss_predict_kfold_rows_*) and evaluated in place (ss_evaluate_kfold_*,
ss_evaluate_kfold_binary_*): bitwise against the one-call sweep ss_predict_kfold_* and the two-call route through
rank_metrics_rows / binary_metrics_rows, shard concatenation, the long metric paths, the oracle's fold loop through the
host mirror, leave-one-out as the ns-fold case, the argument checks and a C3-shaped graph."""
import time

import numpy as np
import pytest
import scipy.sparse as sp

import simspread_jl_amd as ss
from oracle import c_oracle
from rank_ref import assert_rows_close, ref_row
from simspread_jl_amd import _lib

pytestmark = pytest.mark.gpu

ALPHA = 20.0
N, NT = 97, 73          # NT > 64: SS_SELL_SORT=1 can sort the stage-2 operand (W = Ys' has NT rows)


def _labels(rng, n, nt, dens=0.15):
    Y = sp.random(n, nt, density=dens, random_state=rng, format="csr")
    Y.data[:] = 1.0
    Y.sort_indices()
    return sp.csr_matrix(Y)


def _graph(kind, dtype, rng, n=N, nt=NT):
    """A graph of each kind that serves k-fold (nq == 0, features named after the sources) and its labels."""
    Y = _labels(rng, n, nt)
    if kind == "csr":
        X = sp.random(n, n, density=0.08, random_state=rng, format="csr")
        X = X + X.T + sp.identity(n)
        X.data[:] = rng.uniform(0.5, 1.0, X.nnz)
        return ss.DeviceGraph.from_sparse(None, sp.csr_matrix(X), Y, dtype=dtype), Y
    if kind == "dense":
        F = rng.random((n, 12))
        S = (np.minimum(F[:, None], F[None]).sum(-1) / np.maximum(F[:, None], F[None]).sum(-1)).astype(dtype)
        return ss.DeviceGraph.from_similarity(None, S, Y, alpha=0.6, weighted=True, dtype=dtype), Y
    if kind == "fingerprint":
        B = rng.random((n, 128)) < 0.3
        return ss.DeviceGraph.from_fingerprints(None, ss.pack_fingerprints(B), Y, alpha=0.2, weighted=True,
                                                dtype=dtype), Y
    if kind == "features":
        F = rng.random((n, 9)).astype(dtype)
        return ss.DeviceGraph.from_features(None, F, Y, alpha=0.5, weighted=True, dtype=dtype), Y
    raise ValueError(kind)


def _assignments(rng, n):
    """(name, fold ids, nfolds): random with an empty fold, contiguous, one fold, one source per fold."""
    rnd = rng.integers(0, 4, n).astype(np.int32)
    rnd[rnd == 2] = 4                                  # fold 2 of 5 has no member
    return [("random+empty", rnd, 5),
            ("contiguous", (np.arange(n) * 5 // n).astype(np.int32), 5),
            ("one", np.zeros(n, np.int32), 1),
            ("singleton", np.arange(n, dtype=np.int32), n)]


def _ranges(n):
    """whole, one row, inside the first contiguous fold, across every fold, empty."""
    return [(0, n), (n // 2, n // 2 + 1), (2, n // 5 - 3), (3, n - 2), (10, 10)]


def _torch_dtype(dtype):
    import torch
    return torch.float32 if dtype == np.float32 else torch.float64


# ------------------------------------------------------------------ predict_kfold_rows == predict_kfold
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("kind", ["csr", "dense", "fingerprint", "features"])
@pytest.mark.parametrize("sort", ["0", "1"])
def test_predict_kfold_rows_bitwise(dtype, kind, sort, monkeypatch):
    import torch
    monkeypatch.setenv("SS_SELL_SORT", sort)
    ss.init(0)
    rng = np.random.default_rng(101)
    g, _ = _graph(kind, dtype, rng)
    n = g.ns
    for k, (name, fold, nfolds) in enumerate(_assignments(rng, n)):
        clean = k % 2 == 1
        whole = g.predict_kfold(fold, nfolds, clean=clean)
        if name == "one":
            assert (whole == 0.0).all()
            assert (g.predict_kfold_rows(fold, 1, 5, 30, clean=True) == -99.0).all()
        for lo, hi in _ranges(n):
            got = g.predict_kfold_rows(fold, nfolds, lo, hi, clean=clean)
            np.testing.assert_array_equal(got, whole[lo:hi], err_msg=f"{name} [{lo},{hi}) row")
            if hi > lo:
                assert ("spmm_sell_sorted" in ss.path_last()) == (sort == "1"), ss.path_last()
            col = g.predict_kfold_rows(fold, nfolds, lo, hi, clean=clean, layout="col")
            np.testing.assert_array_equal(col, whole[lo:hi], err_msg=f"{name} [{lo},{hi}) col")
        lo, hi = 3, n - 2
        dev = torch.full((hi - lo, g.nt), -7.0, dtype=_torch_dtype(dtype), device="cuda")
        g.predict_kfold_rows(torch.from_numpy(fold), nfolds, lo, hi, clean=clean, out=dev)
        np.testing.assert_array_equal(dev.cpu().numpy(), whole[lo:hi], err_msg=f"{name} device row")
        devc = torch.full((g.nt, hi - lo), -7.0, dtype=_torch_dtype(dtype), device="cuda")
        g.predict_kfold_rows(fold, nfolds, lo, hi, clean=clean, out=devc, layout="col")
        np.testing.assert_array_equal(devc.cpu().numpy().T, whole[lo:hi], err_msg=f"{name} device col")
    g.close()


def test_c5_shaped_labels_take_the_sorted_path_without_forcing():
    """Skewed labels (a few targets held by every source) make the library sort the stage-2 operand on its own: the
    path that copied member rows one by one in ss_predict_kfold_* and scatters them in one kernel here."""
    ss.init(0)
    rng = np.random.default_rng(5)
    n, nt = 3000, 256
    X = sp.random(n, n, density=0.01, random_state=rng, format="csr")
    X = sp.csr_matrix(X + X.T + sp.identity(n))
    Yd = rng.random((n, nt)) < 0.003
    Yd[:, :8] = True                                   # eight targets held by every source: a skewed W = Ys'
    Y = sp.csr_matrix(Yd.astype(np.float32))
    g = ss.DeviceGraph.from_sparse(None, X, Y, dtype=np.float32)
    fold = rng.integers(0, 10, n).astype(np.int32)
    whole = g.predict_kfold(fold, 10, clean=True)
    got = g.predict_kfold_rows(fold, 10, 37, 311, clean=True)
    assert "spmm_sell_sorted" in ss.path_last(), ss.path_last()
    np.testing.assert_array_equal(got, whole[37:311])
    g.close()


# ------------------------------------------------------------------ shards
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_shards_concatenate_to_the_whole_range(dtype):
    ss.init(0)
    rng = np.random.default_rng(7)
    g, Y = _graph("csr", dtype, rng)
    n = g.ns
    fold = rng.integers(0, 6, n).astype(np.int32)
    weights = np.diff(Y.indptr).astype(np.float64) + np.arange(n) * 0.5      # uneven shards
    shards = [ss.shard_range(n, r, 3, weights=weights) for r in range(3)]
    assert len({hi - lo for lo, hi in shards}) > 1, shards
    whole = [g.predict_kfold_rows(fold, 6, clean=True), g.evaluate_kfold(fold, 6, clean=True, L=5, block_rows=4),
             g.evaluate_kfold_binary(fold, 6, clean=True, block_rows=4)]
    parts = [[g.predict_kfold_rows(fold, 6, lo, hi, clean=True),
              g.evaluate_kfold(fold, 6, lo, hi, clean=True, L=5, block_rows=4),
              g.evaluate_kfold_binary(fold, 6, lo, hi, clean=True, block_rows=4)] for lo, hi in shards]
    for j in range(3):
        np.testing.assert_array_equal(np.concatenate([p[j] for p in parts]), whole[j])
    np.testing.assert_array_equal(whole[0], g.predict_kfold(fold, 6, clean=True))
    g.close()


# ------------------------------------------------------------------ evaluate == predict + metric rows
def _two_call(g, Y, fold, nfolds, clean, L):
    scores = g.predict_kfold(fold, nfolds, clean=clean)
    return scores, ss.rank_metrics_rows(Y, scores, alpha=ALPHA, L=L), ss.binary_metrics_rows(Y, scores)


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("kind", ["csr", "dense"])
@pytest.mark.parametrize("clean", [False, True])
def test_evaluate_kfold_bitwise(dtype, kind, clean):
    import torch
    ss.init(0)
    rng = np.random.default_rng(11)
    g, Y = _graph(kind, dtype, rng)
    n = g.ns
    fold = rng.integers(0, 5, n).astype(np.int32)
    _, rank, binary = _two_call(g, Y, fold, 5, clean, 5)
    for br in (1, 7, 0):
        np.testing.assert_array_equal(g.evaluate_kfold(fold, 5, clean=clean, L=5, block_rows=br), rank,
                                      err_msg=f"block_rows={br}")
        assert "rank_rows_lds" in ss.path_last(), ss.path_last()
        np.testing.assert_array_equal(g.evaluate_kfold_binary(fold, 5, clean=clean, block_rows=br), binary,
                                      err_msg=f"binary block_rows={br}")
        assert "binary_rows_lds" in ss.path_last(), ss.path_last()
    np.testing.assert_array_equal(g.evaluate_kfold(fold, 5, 4, n - 9, clean=clean, L=5, block_rows=7), rank[4:n - 9])
    np.testing.assert_array_equal(g.evaluate_kfold_binary(fold, 5, 4, n - 9, clean=clean, block_rows=7),
                                  binary[4:n - 9])
    # the header's statement: predict_kfold_rows into a device buffer + the metric rows on device labels
    scores = torch.empty((n, g.nt), dtype=_torch_dtype(dtype), device="cuda")
    g.predict_kfold_rows(fold, 5, clean=clean, out=scores)
    dptr = torch.from_numpy(Y.indptr.astype(np.int64)).cuda()
    didx = torch.from_numpy(Y.indices.astype(np.int32)).cuda()
    np.testing.assert_array_equal(ss.rank_metrics_rows((dptr, didx), scores, alpha=ALPHA, L=5).cpu().numpy(), rank)
    np.testing.assert_array_equal(ss.binary_metrics_rows((dptr, didx), scores).cpu().numpy(), binary)
    # empty range: no-op
    assert g.evaluate_kfold(fold, 5, 9, 9, L=5).shape == (0, 6)
    assert g.evaluate_kfold_binary(fold, 5, 9, 9).shape == (0, 18)
    g.close()


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_long_rows_take_the_global_metric_paths(dtype):
    """nt > 16384 (binary metrics: segmented sort in scratch) and rows of more than 2048 positives (ranking metrics:
    global-memory path) next to short rows (LDS paths), every block_rows bitwise."""
    ss.init(0)
    rng = np.random.default_rng(13)
    n, nt = 48, 17000
    X = sp.random(n, n, density=0.1, random_state=rng, format="csr")
    X = sp.csr_matrix(X + X.T + sp.identity(n))
    Yd = rng.random((n, nt)) < 0.002
    for r in (3, 20, 41):
        Yd[r, rng.choice(nt, 2600, replace=False)] = True
    Y = sp.csr_matrix(Yd.astype(np.float32))
    g = ss.DeviceGraph.from_sparse(None, X, Y, dtype=dtype)
    fold = rng.integers(0, 4, n).astype(np.int32)
    _, rank, binary = _two_call(g, Y, fold, 4, True, 20)
    for br in (1, 7, 0):
        np.testing.assert_array_equal(g.evaluate_kfold(fold, 4, clean=True, block_rows=br), rank)
        if br != 1:
            assert "rank_rows_large" in ss.path_last() and "rank_rows_lds" in ss.path_last(), ss.path_last()
        np.testing.assert_array_equal(g.evaluate_kfold_binary(fold, 4, clean=True, block_rows=br), binary)
        assert "binary_rows_large" in ss.path_last(), ss.path_last()
    g.close()


# ------------------------------------------------------------------ oracle, leave-one-out
def _same_ties(a, b):
    keep = []
    for x, y in zip(a, b):
        ox, oy = np.argsort(-x, kind="stable"), np.argsort(-y, kind="stable")
        keep.append(np.array_equal(ox, oy) and np.array_equal(np.diff(x[ox]) == 0, np.diff(y[oy]) == 0))
    return np.array(keep)


def test_against_the_oracle_fold_loop_through_the_host_mirror():
    """evaluate_kfold / evaluate_kfold_binary against the host mirror (ss.AuROC, ..., ss.maxperformance, ...) applied to
    the oracle's k-fold scores (c_oracle.predict_kfold), on the rows whose score order and ties agree."""
    ss.init(0)
    rng = np.random.default_rng(17)
    n, nt, k = 80, 50, 4
    X = sp.random(n, n, density=0.1, random_state=rng, format="csr")
    X = X + X.T + sp.identity(n)
    X.data[:] = rng.uniform(0.5, 1.0, X.nnz).astype(np.float32)
    X = sp.csr_matrix(X)
    Y = _labels(rng, n, nt, 0.2)
    fold = rng.integers(0, k, n).astype(np.int32)
    g = ss.DeviceGraph.from_sparse(None, X, Y, dtype=np.float32)
    want = c_oracle.predict_kfold(X.astype(np.float64), Y.astype(np.float64), fold, k, clean=True)
    dev = g.predict_kfold(fold, k, clean=True)
    keep = _same_ties(dev.astype(np.float64), want.astype(np.float32).astype(np.float64))
    assert keep.mean() > 0.5, keep.mean()
    rank = g.evaluate_kfold(fold, k, clean=True, L=5)
    binary = g.evaluate_kfold_binary(fold, k, clean=True).reshape(n, 6, 3)
    Yd = Y.toarray() != 0
    fns = [ss.f1score, ss.mcc, ss.accuracy, ss.balancedaccuracy, ss.recall, ss.precision]
    for i in np.flatnonzero(keep):
        y, s = Yd[i].astype(np.uint8), want[i].astype(np.float32)
        host = [ss.AuROC(y, s), ss.AuPRC(y, s), ss.BEDROC(y, s, alpha=ALPHA), ss.validity_ratio(s)]
        assert_rows_close(rank[i:i + 1], np.array([host + list(ref_row(y, s, ALPHA, 5)[4:])]), 1e-6, 1e-9,
                          f"rank row {i}")
        for m, f in enumerate(fns):
            mean, std = ss.meanstdperformance(y, s, f)
            assert_rows_close(binary[i, m][None], np.array([[ss.maxperformance(y, s, f), mean, std]]), 1e-9, 1e-12,
                              f"binary row {i} metric {m}")
    g.close()


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_one_source_per_fold_is_leave_one_out(dtype):
    ss.init(0)
    rng = np.random.default_rng(19)
    g, _ = _graph("csr", dtype, rng)
    n = g.ns
    fold = np.arange(n, dtype=np.int32)
    a, b = g.predict_kfold_rows(fold, n, clean=True), g.predict_loo(clean=True)
    tol = 1e-5 if dtype == np.float32 else 1e-12
    np.testing.assert_allclose(a, b, rtol=tol, atol=tol)
    keep = _same_ties(a.astype(np.float64), b.astype(np.float64))
    assert keep.mean() > 0.5, keep.mean()
    rtol = 1e-6 if dtype == np.float32 else 1e-9
    assert_rows_close(g.evaluate_kfold(fold, n, clean=True, L=5)[keep], g.evaluate_loo(clean=True, L=5)[keep], rtol,
                      1e-9, "rank")
    assert_rows_close(g.evaluate_kfold_binary(fold, n, clean=True)[keep], g.evaluate_loo_binary(clean=True)[keep],
                      rtol, 1e-9, "binary")
    g.close()


# ------------------------------------------------------------------ argument checks
def _raw(name, dtype, g, fold, nfolds, lo, hi, out, extra=()):
    fn = getattr(_lib.lib(), f"{name}_{'f32' if dtype == np.float32 else 'f64'}")
    if name == "ss_predict_kfold_rows":
        return fn(g._h, fold.ctypes.data, nfolds, lo, hi, 1, out.ctypes.data, out.shape[1], _lib.SS_LAYOUT_ROWMAJOR,
                  _lib.SS_MEM_HOST)
    return fn(g._h, fold.ctypes.data, nfolds, lo, hi, 1, *extra, out.ctypes.data, _lib.SS_MEM_HOST)


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_bad_arguments_are_refused_and_nothing_is_written(dtype):
    ss.init(0)
    rng = np.random.default_rng(23)
    g, _ = _graph("csr", dtype, rng)
    n = g.ns
    good = rng.integers(0, 3, n).astype(np.int32)
    bad_id = good.copy(); bad_id[n - 1] = 3                       # outside 0..2, and outside the asked range
    neg = good.copy(); neg[0] = -1
    calls = [("ss_predict_kfold_rows", (), 0),
             ("ss_evaluate_kfold", (ALPHA, 5, 0), 6),
             ("ss_evaluate_kfold_binary", (0,), 18)]
    for name, extra, width in calls:
        for fold, nfolds, lo, hi in [(bad_id, 3, 0, 10), (neg, 3, 20, 30), (good, 0, 0, 10), (good, 3, -1, 10),
                                     (good, 3, 10, n + 1), (good, 3, 10, 9)]:
            out = np.full((max(hi - lo, 1), width or g.nt), -12345.0, np.float64 if width else dtype)
            assert _raw(name, dtype, g, fold, nfolds, lo, hi, out, extra) == -1, (name, nfolds, lo, hi)
            assert _lib.lib().ss_last_error().decode(), name
            assert (out == -12345.0).all(), name
    # L >= nt
    out = np.full((10, 6), -12345.0)
    assert _raw("ss_evaluate_kfold", dtype, g, good, 3, 0, 10, out, (ALPHA, g.nt, 0)) == -1
    assert "Number of labels" in _lib.lib().ss_last_error().decode()
    assert (out == -12345.0).all()
    # a fold array of the wrong length stops in Python, before the library
    for call in (lambda f: g.predict_kfold_rows(f, 3), lambda f: g.evaluate_kfold(f, 3, L=5),
                 lambda f: g.evaluate_kfold_binary(f, 3)):
        with pytest.raises(ValueError):
            call(good[:-1])
    with pytest.raises(_lib.SimSpreadError, match="outside"):
        g.evaluate_kfold(bad_id, 3, 0, 10, L=5)
    g.close()
    # nq != 0
    Xq = sp.random(5, n, density=0.2, random_state=rng, format="csr")
    X = sp.csr_matrix(sp.identity(n))
    gq = ss.DeviceGraph.from_sparse(Xq, X, _labels(rng, n, NT), dtype=dtype)
    for name, extra, width in calls:
        out = np.full((10, width or gq.nt), -12345.0, np.float64 if width else dtype)
        assert _raw(name, dtype, gq, good, 3, 0, 10, out, extra) == -1, name
        assert "nq == 0" in _lib.lib().ss_last_error().decode()
        assert (out == -12345.0).all()
    gq.close()


# ------------------------------------------------------------------ at size
def test_c3_shaped_graph_two_blocks():
    """C3 shape (100k sources x 100k targets, 1 %), 10 contiguous folds: evaluate_kfold over a 2048-row range inside
    fold 0 and one across the fold 0 / fold 1 border == predict_kfold_rows + rank_metrics_rows, bit for bit."""
    import torch
    from tools.c3_loo import rand_csr, rand_sym_csr
    ss.init(0)
    ss.use_torch_stream()
    n, k, rows = 100_000, 10, 2048
    gen = torch.Generator(device="cuda"); gen.manual_seed(20250222 + 33)
    xp, xi = rand_sym_csr(n, 0.01, gen)
    yp, yi = rand_csr(n, n, 0.01, gen)
    xv = (0.5 + 0.5 * torch.rand(xi.numel(), device="cuda", generator=gen)).float()
    g = ss.DeviceGraph.from_device_csr(0, n, n, n, None, (xp, xi, xv), (yp, yi, None), dtype=np.float32)
    fold = (np.arange(n) * k // n).astype(np.int32)
    out = torch.empty((rows, n), dtype=torch.float32, device="cuda")
    for lo in (40, n // k - 1000):
        g.predict_kfold_rows(fold, k, lo, lo + rows, clean=True, out=out)
        ref = ss.rank_metrics_rows(((yp[lo:lo + rows + 1]).contiguous(), yi), out, alpha=ALPHA, L=20).cpu().numpy()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        got = g.evaluate_kfold(fold, k, lo, lo + rows, clean=True, alpha=ALPHA, L=20)
        dt = time.perf_counter() - t0
        print(f"C3 evaluate_kfold [{lo}, {lo + rows}) folds {sorted(set(fold[lo:lo + rows]))}: {dt * 1e3:.1f} ms wall, "
              f"device {ss.timing_last()['total_ms']:.1f} ms")
        np.testing.assert_array_equal(got, ref)
        assert np.isfinite(got[:, 0]).mean() > 0.99
    g.close()
