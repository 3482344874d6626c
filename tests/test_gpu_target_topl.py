"""Per-target top-L tables on the device (ss_target_topl_*): recallatL / precisionatL(y, yhat, grouping, L) with
grouping = target, and every target's screening list.  add_rows against the host reference (tests/target_topl_ref.py),
bitwise invariance under splits, orders, merges and export -> import, add_loo / add_kfold bitwise against predict into
a device buffer + add_rows, the long-candidate route, all-or-nothing errors, iris LOO against the host mirror, two ranks
meeting through dist.target_topl and one C3 block of 2048 folds checked on every target."""
import os
import socket
import sys

import numpy as np
import pytest
import scipy.sparse as sp

import simspread_jl_amd as ss
import target_topl_ref as R
from simspread_jl_amd import _lib

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _block(rng, nrows, ncols, dtype, levels=16, dens=0.05):
    S = (rng.integers(-2, levels, (nrows, ncols)) / 4).astype(dtype)
    S[rng.random((nrows, ncols)) < 0.05] = dtype(-99.0)
    S[rng.random((nrows, ncols)) < 0.05] = dtype(-0.0)
    S[rng.random((nrows, ncols)) < 0.05] = dtype(0.0)
    Y = sp.random(nrows, ncols, density=dens, random_state=rng, format="csr")
    Y.data[:] = 1.0
    Y.sort_indices()
    return S, Y


def _check_table(h, Y, S, L, rows=None, msg=""):
    vals, rid, lab, npos, nrows = h.export()
    wv, wr, wl, wn = R.table(Y.toarray() if sp.issparse(Y) else Y, S, L, rows)
    np.testing.assert_array_equal(rid, wr, err_msg=msg)
    np.testing.assert_array_equal(vals.view(np.uint8), wv.view(np.uint8), err_msg=msg)   # -0.0 kept as -0.0
    np.testing.assert_array_equal(lab, wl, err_msg=msg)
    np.testing.assert_array_equal(npos, wn, err_msg=msg)
    if S.shape[0] > L:
        m = h.metrics()
        want, hits = R.metrics(wl, wn, L)
        np.testing.assert_array_equal(m["hits"], hits)
        np.testing.assert_array_equal(m["npos"], wn)
        np.testing.assert_array_equal(np.array([m[f] for f in ss.TARGET_TOPL_FIELDS]), np.array(want))


def _export_equal(a, b):
    for x, y in zip(a.export(), b.export()):
        np.testing.assert_array_equal(np.asarray(x).view(np.uint8) if np.asarray(x).dtype.kind == "f" else x,
                                      np.asarray(y).view(np.uint8) if np.asarray(y).dtype.kind == "f" else y)


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("L", [1, 20, 1024])
def test_add_rows_against_the_reference(dtype, L):
    ss.init(0)
    rng = np.random.default_rng(1)
    for nrows, ncols, levels in ((L + 40, 300, 16), (2 * L + 300, 37, 5000), (3, 1000, 4)):
        S, Y = _block(rng, nrows, ncols, dtype, levels)
        h = ss.TargetTopL(ncols, L, dtype).add_rows(Y, S, row_begin=0)
        _check_table(h, Y, S, L, msg=f"{nrows}x{ncols}")
        assert h.info() == dict(nt=ncols, L=L, rows=nrows, npos=Y.nnz)
        h.close()


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_any_split_order_merge_and_export_is_bitwise_one_table(dtype):
    import torch
    ss.init(0)
    rng = np.random.default_rng(2)
    n, nt, L = 400, 150, 20
    S, Y = _block(rng, n, nt, dtype, 12)
    one = ss.TargetTopL(nt, L, dtype).add_rows(Y, S)
    _check_table(one, Y, S, L)
    Yd = Y.toarray()
    for trial in range(3):
        cuts = np.sort(rng.choice(np.arange(1, n), size=3 + trial, replace=False))
        parts = np.split(np.arange(n), cuts)
        rng.shuffle(parts)
        a, b = ss.TargetTopL(nt, L, dtype), ss.TargetTopL(nt, L, dtype)
        for k, rows in enumerate(parts):
            (a if k % 2 else b).add_rows(sp.csr_matrix(Yd[rows]), np.ascontiguousarray(S[rows]), row_begin=int(rows[0]))
        a.merge(b)
        _export_equal(a, one)
        c = ss.TargetTopL(nt, L, dtype).import_(*a.export())
        _export_equal(c, one)
        d = ss.TargetTopL(nt, L, dtype).add_rows(Y, torch.from_numpy(S).cuda())      # device scores
        _export_equal(d, one)


def _labels(rng, n, nt, dens=0.15):
    Y = sp.random(n, nt, density=dens, random_state=rng, format="csr")
    Y.data[:] = 1.0
    Y.sort_indices()
    return sp.csr_matrix(Y)


def _graph(kind, dtype, rng, n=97, nt=73):
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
    F = rng.random((n, 9)).astype(dtype)
    return ss.DeviceGraph.from_features(None, F, Y, alpha=0.5, weighted=True, dtype=dtype), Y


def _torch_dtype(dtype):
    import torch
    return torch.float32 if dtype == np.float32 else torch.float64


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("kind", ["csr", "dense", "fingerprint", "features"])
def test_add_loo_and_kfold_equal_predict_then_add_rows(dtype, kind):
    import torch
    ss.init(0)
    rng = np.random.default_rng(3)
    g, Y = _graph(kind, dtype, rng)
    n, nt, L = g.ns, g.nt, 20
    fold = rng.integers(0, 5, n).astype(np.int32)
    for clean in (False, True):
        out = torch.empty((n, nt), dtype=_torch_dtype(dtype), device="cuda")
        g.predict_loo(0, n, clean=clean, out=out)
        want = ss.TargetTopL(nt, L, dtype).add_rows(Y, out)
        _check_table(want, Y, out.cpu().numpy(), L, msg=f"loo {kind}")
        for br in (0, 1, 10, 64):
            h = ss.TargetTopL(nt, L, dtype).add_loo(g, 0, n, clean=clean, block_rows=br)
            _export_equal(h, want)
        a = ss.TargetTopL(nt, L, dtype).add_loo(g, 40, n, clean=clean, block_rows=13)
        a.merge(ss.TargetTopL(nt, L, dtype).add_loo(g, 0, 40, clean=clean, block_rows=7))
        _export_equal(a, want)

        kout = torch.empty((n, nt), dtype=_torch_dtype(dtype), device="cuda")
        g.predict_kfold_rows(fold, 5, 0, n, clean=clean, out=kout)
        kwant = ss.TargetTopL(nt, L, dtype).add_rows(Y, kout)
        for br in (0, 1, 17):
            h = ss.TargetTopL(nt, L, dtype).add_kfold(g, fold, 5, 0, n, clean=clean, block_rows=br)
            _export_equal(h, kwant)
        b = ss.TargetTopL(nt, L, dtype).add_kfold(g, fold, 5, 30, n, clean=clean).add_kfold(g, fold, 5, 0, 30,
                                                                                             clean=clean)
        _export_equal(b, kwant)
    g.close()


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_rising_scores_take_the_long_candidate_route(dtype):
    ss.init(0)
    rng = np.random.default_rng(4)
    n, nt = 6000, 40
    # scores that rise with the row: after the seed every later row beats every target's L-th entry
    S = (np.arange(n)[:, None] * 3 + rng.integers(0, 3, (n, nt))).astype(dtype) / 8
    Y = _labels(rng, n, nt, 0.05)
    for L in (20, 1024):
        h = ss.TargetTopL(nt, L, dtype).add_rows(Y, S)
        assert "target_topl_merge_large" in ss.path_last(), ss.path_last()
        _check_table(h, Y, S, L, msg=f"rising L={L}")
        # seeded already: the next block takes the filter and the long route again
        h.add_rows(Y[:3000], np.ascontiguousarray(S[:3000] + dtype(10000)), row_begin=n)
        assert "target_topl_merge_large" in ss.path_last() and "target_topl_filter" in ss.path_last()
        S2 = np.vstack([S, S[:3000] + dtype(10000)])
        Y2 = sp.vstack([Y, Y[:3000]]).tocsr()
        _check_table(h, Y2, S2, L, msg=f"rising twice L={L}")
    # ordinary scores keep to the LDS path
    S, Y = _block(rng, 3000, 500, dtype, 100000)
    h = ss.TargetTopL(500, 20, dtype).add_rows(Y, S)
    assert "target_topl_merge_lds" in ss.path_last() and "target_topl_merge_large" not in ss.path_last()
    _check_table(h, Y, S, 20)


def _snapshot(h):
    return [np.array(x, copy=True) for x in h.export()[:4]], h.info()


def _unchanged(h, snap):
    got = _snapshot(h)
    for x, y in zip(got[0], snap[0]):
        np.testing.assert_array_equal(x.view(np.uint8) if x.dtype.kind == "f" else x,
                                      y.view(np.uint8) if y.dtype.kind == "f" else y)
    assert got[1] == snap[1]


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_errors_leave_the_handle_as_it_was(dtype):
    ss.init(0)
    rng = np.random.default_rng(6)
    S, Y = _block(rng, 60, 200, dtype, 5000)
    h = ss.TargetTopL(200, 20, dtype).add_rows(Y, S)
    snap = _snapshot(h)
    for r in (3, 45):   # a NaN in the seed rows of a fresh handle is covered below; here in the filtered rows
        bad = S.copy()
        bad[r, 7] = np.nan
        with pytest.raises(ss.SimSpreadError, match="NaN"):
            h.add_rows(Y, bad, row_begin=100)
        _unchanged(h, snap)
    fresh = ss.TargetTopL(200, 20, dtype)
    bad = S.copy()
    bad[2, 5] = np.nan
    with pytest.raises(ss.SimSpreadError, match="NaN"):
        fresh.add_rows(Y, bad)
    assert fresh.info()["rows"] == 0
    suf, other = ("f32", "f64") if dtype == np.float32 else ("f64", "f32")
    row = np.ascontiguousarray(S[:1])
    ptr, idx = np.array([0, 2], np.int64), np.array([5, 3], np.int32)          # labels not sorted
    fn = getattr(_lib.lib(), f"ss_target_topl_add_rows_{suf}")
    assert fn(h._h, ptr.ctypes.data, idx.ctypes.data, 0, row.ctypes.data, 1, 200, 200, 500, _lib.SS_MEM_HOST) == -1
    _unchanged(h, snap)
    idx2 = np.array([3, 200], np.int32)                                        # out of range
    assert fn(h._h, ptr.ctypes.data, idx2.ctypes.data, 0, row.ctypes.data, 1, 200, 200, 500, _lib.SS_MEM_HOST) == -1
    _unchanged(h, snap)
    row2 = row.astype(np.float64 if dtype == np.float32 else np.float32)       # the other precision
    ok = np.array([0, 1], np.int64)
    assert getattr(_lib.lib(), f"ss_target_topl_add_rows_{other}")(
        h._h, ok.ctypes.data, idx.ctypes.data, 0, row2.ctypes.data, 1, 200, 200, 500, _lib.SS_MEM_HOST) == -1
    _unchanged(h, snap)
    wide = np.ascontiguousarray(np.zeros((1, 201), dtype))                     # ncols != nt
    assert fn(h._h, ok.ctypes.data, idx.ctypes.data, 0, wide.ctypes.data, 1, 201, 201, 500, _lib.SS_MEM_HOST) == -1
    _unchanged(h, snap)
    with pytest.raises(ss.SimSpreadError):
        h.merge(ss.TargetTopL(200, 20, np.float64 if dtype == np.float32 else np.float32))
    with pytest.raises(ss.SimSpreadError):
        h.merge(ss.TargetTopL(200, 21, dtype))
    _unchanged(h, snap)
    vals, rid, lab, npos, nr = h.export()
    with pytest.raises(ss.SimSpreadError, match="ordered"):
        h.import_(vals[:, ::-1], rid[:, ::-1], lab[:, ::-1], npos, nr)
    with pytest.raises(ss.SimSpreadError, match="npos"):
        h.import_(vals, rid, lab, np.zeros_like(npos) - 1, nr)
    _unchanged(h, snap)
    for L in (0, 1025):
        with pytest.raises(ss.SimSpreadError, match="L ="):
            ss.TargetTopL(200, L, dtype)
    small = ss.TargetTopL(200, 20, dtype).add_rows(Y[:20], np.ascontiguousarray(S[:20]))
    with pytest.raises(ss.SimSpreadError, match="more than L"):
        small.metrics()
    small.add_rows(Y[20:21], np.ascontiguousarray(S[20:21]), row_begin=20)
    assert np.isfinite(small.metrics()["precisionatL"])


def _iris():
    here = os.path.join(ROOT, "tests", "golden", "iris")

    def read(p):
        with open(os.path.join(here, p)) as f:
            lines = f.read().splitlines()
        return np.array([[float(v) for v in l.split()[1:]] for l in lines[1:]])
    return read("iris.features"), read("iris.classes")


def test_iris_loo_grouped_by_target_is_the_mirrors_number():
    ss.init(0)
    F, Cm = _iris()
    S = ss.jaccard_similarity(F).astype(np.float32)
    g = ss.DeviceGraph.from_dense(None, S, Cm.astype(np.float32), alpha=np.float32(0.9), weighted=True,
                                  dtype=np.float32)
    yhat = g.predict_loo(clean=True)
    n, nt = yhat.shape
    grouping = np.repeat(np.arange(nt), n)
    for L in (5, 20, 50):
        m = ss.TargetTopL(nt, L, np.float32).add_loo(g, clean=True).metrics()
        assert m["recallatL"] == ss.recallatL(Cm.ravel(order="F"), yhat.ravel(order="F"), grouping, L)
        assert m["precisionatL"] == ss.precisionatL(Cm.ravel(order="F"), yhat.ravel(order="F"), grouping, L)
        assert m["targets_with_positives"] == nt
    g.close()


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _rank_worker(rank, world, port, tmp):
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import torch.distributed as dist
    import simspread_jl_amd as ss_
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    ss_.init(0)
    g, _ = _graph("csr", np.float32, np.random.default_rng(8), n=211, nt=97)
    lo, hi = ss_.shard_range(g.ns, rank, world)
    h = ss_.TargetTopL(g.nt, 20, np.float32).add_loo(g, lo, hi, clean=True, block_rows=50)
    out = ss_.target_topl(h, root=0)
    assert (out is None) == (rank != 0)
    if rank == 0:
        vals, rows, labels, npos, n = out.export()
        np.savez(os.path.join(tmp, "topl.npz"), vals=vals, rows=rows, labels=labels, npos=npos, n=n)
    dist.barrier()
    dist.destroy_process_group()


def test_two_ranks_meet_in_dist_target_topl(tmp_path):
    import torch.multiprocessing as mp
    mp.spawn(_rank_worker, args=(2, _free_port(), str(tmp_path)), nprocs=2, join=True)
    ss.init(0)
    g, _ = _graph("csr", np.float32, np.random.default_rng(8), n=211, nt=97)
    vals, rows, labels, npos, n = ss.TargetTopL(g.nt, 20, np.float32).add_loo(g, clean=True).export()
    got = np.load(tmp_path / "topl.npz")
    np.testing.assert_array_equal(got["vals"], vals)
    np.testing.assert_array_equal(got["rows"], rows)
    np.testing.assert_array_equal(got["labels"], labels)
    np.testing.assert_array_equal(got["npos"], npos)
    assert int(got["n"]) == n == g.ns


def test_c3_block_of_2048_folds_on_every_target():
    import torch
    sys.path.insert(0, ROOT)
    from tools.c3_loo import rand_csr, rand_sym_csr
    ss.init(0)
    ss.use_torch_stream()
    n, folds, L = 100_000, 2048, 20
    gen = torch.Generator(device="cuda")
    gen.manual_seed(20250222 + 3)
    xp, xi = rand_sym_csr(n, 0.01, gen)
    yp, yi = rand_csr(n, n, 0.01, gen)
    xv = (0.5 + 0.5 * torch.rand(xi.numel(), device="cuda", generator=gen)).float()
    g = ss.DeviceGraph.from_device_csr(0, n, n, n, None, (xp, xi, xv), (yp, yi, None), dtype=np.float32)
    h = ss.TargetTopL(n, L, np.float32).add_loo(g, 0, folds, clean=True)
    vals, rows, labels, npos, nr = h.export()
    out = torch.empty((folds, n), dtype=torch.float32, device="cuda")
    g.predict_loo(0, folds, clean=True, out=out)
    # the reference on the device: per target a stable descending sort of the 2048 scores (ties by ascending row)
    keys = out.view(torch.int32)
    keys = torch.where(keys < 0, ~keys, keys | torch.tensor(-2 ** 31, dtype=torch.int32, device="cuda"))
    kk = (keys.to(torch.int64) & 0xFFFFFFFF)                                  # the isless key, as unsigned
    order = torch.sort(kk, dim=0, descending=True, stable=True).indices[:L]  # (L, n): rows ascending within ties
    np.testing.assert_array_equal(rows, order.t().cpu().numpy())
    want_vals = torch.gather(out, 0, order).t().cpu().numpy()
    np.testing.assert_array_equal(vals.view(np.uint32), want_vals.view(np.uint32))
    ptr = yp[:folds + 1].cpu().numpy()
    Yb = sp.csr_matrix((np.ones(int(ptr[-1])), yi[:int(ptr[-1])].cpu().numpy(), ptr), shape=(folds, n))
    np.testing.assert_array_equal(npos, np.asarray(Yb.sum(0)).ravel().astype(np.int64))
    lab = np.asarray(Yb[order.t().cpu().numpy().ravel(), np.repeat(np.arange(n), L)]).reshape(n, L)
    np.testing.assert_array_equal(labels, lab.astype(np.uint8))
    g.close()


def test_add_predict_screens_query_rows_block_by_block():
    import torch
    ss.init(0)
    rng = np.random.default_rng(9)
    nq, ns, nt = 150, 120, 60
    Xq = sp.random(nq, ns, density=0.1, random_state=rng, format="csr")
    Xq.data[:] = rng.uniform(0.5, 1.0, Xq.nnz)
    Xs = sp.random(ns, ns, density=0.1, random_state=rng, format="csr")
    Xs = sp.csr_matrix(Xs + Xs.T + sp.identity(ns))
    Xs.data[:] = rng.uniform(0.5, 1.0, Xs.nnz)
    Ys = _labels(rng, ns, nt)
    g = ss.DeviceGraph.from_sparse(Xq, Xs, Ys, dtype=np.float32)
    S = g.predict("query", 0, nq, clean=False)
    Yq = _labels(rng, nq, nt, 0.1)
    want = ss.TargetTopL(nt, 20, np.float32).add_rows(Yq, S)
    for br in (0, 7, 64):
        h = ss.TargetTopL(nt, 20, np.float32).add_predict(g, "query", 0, nq, y=Yq, block_rows=br)
        _export_equal(h, want)
    # unlabelled rows count as negatives; rows keep their query index
    h = ss.TargetTopL(nt, 20, np.float32).add_predict(g, "query", 30, nq, block_rows=16)
    _check_table(h, np.zeros((nq - 30, nt)), S[30:], 20, rows=np.arange(30, nq))
    assert h.metrics()["targets_with_positives"] == 0
    torch.cuda.synchronize()
    g.close()
