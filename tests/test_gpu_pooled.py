"""Pooled evaluation on the device (ss_pool_*): the reference's AuROC(vec(y), vec(yhat)), AuPRC and
maxperformance(vec(y), vec(yhat), f) of a whole matrix or sweep.  add_rows against the host reference
(tests/pooled_ref.py), bitwise invariance under row splits, orders, merges and export -> import, add_loo / add_kfold
bitwise against predict into a device buffer + add_rows, iris LOO in fp64, counts past 2^31, all-or-nothing errors
and two ranks meeting through dist.pooled_metrics."""
import os
import socket
import sys

import numpy as np
import pytest
import scipy.sparse as sp

import simspread_jl_amd as ss
import pooled_ref as R
from simspread_jl_amd import _lib

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _block(rng, nrows, ncols, dtype, levels=64, dens=0.05):
    S = (rng.integers(-2, levels, (nrows, ncols)) / 7).astype(dtype)
    S[rng.random((nrows, ncols)) < 0.05] = dtype(-99.0)
    S[rng.random((nrows, ncols)) < 0.05] = dtype(-0.0)
    Y = sp.random(nrows, ncols, density=dens, random_state=rng, format="csr")
    Y.data[:] = 1.0
    Y.sort_indices()
    return S, Y


def _ref(Y, S):
    Yd = Y.toarray() if sp.issparse(Y) else np.asarray(Y)
    return R.metrics(*R.table(Yd.ravel(), S.ravel()))


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_add_rows_against_the_reference(dtype):
    ss.init(0)
    rng = np.random.default_rng(1)
    for nrows, ncols, levels in ((40, 300, 64), (7, 5000, 4000), (1, 20000, 100000)):
        S, Y = _block(rng, nrows, ncols, dtype, levels)
        p = ss.Pool(dtype).add_rows(Y, S)
        assert ss.path_last() == ["pool_radix_u32" if dtype == np.float32 else "pool_radix_u64"], ss.path_last()
        want, scale = _ref(Y, S)
        R.assert_pooled_close(p.metrics_array(), want, scale, f"{nrows}x{ncols}")
        keys, npos, nneg = p.export()
        wk, wp, wn = R.table(Y.toarray().ravel(), S.ravel())
        np.testing.assert_array_equal(keys, wk)
        np.testing.assert_array_equal(npos, wp)
        np.testing.assert_array_equal(nneg, wn)
        assert p.info()["n"] == nrows * ncols and p.info()["npos"] == Y.nnz
        p.close()


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_any_split_order_merge_and_export_is_bitwise_one_table(dtype):
    import torch
    ss.init(0)
    rng = np.random.default_rng(2)
    S, Y = _block(rng, 60, 700, dtype, 300)
    one = ss.Pool(dtype).add_rows(Y, S).metrics_array()
    Yd = Y.toarray()
    for trial in range(3):
        perm = rng.permutation(60)
        cuts = np.sort(rng.choice(np.arange(1, 60), size=3 + trial, replace=False))
        a, b = ss.Pool(dtype), ss.Pool(dtype)
        for k, rows in enumerate(np.split(perm, cuts)):
            (a if k % 2 else b).add_rows(sp.csr_matrix(Yd[rows]), np.ascontiguousarray(S[rows]))
        a.merge(b)
        np.testing.assert_array_equal(a.metrics_array(), one)
        c = ss.Pool(dtype).import_(*a.export())
        np.testing.assert_array_equal(c.metrics_array(), one)
        # device scores and device labels
        d = ss.Pool(dtype).add_rows(Y, torch.from_numpy(S).cuda())
        np.testing.assert_array_equal(d.metrics_array(), one)
    # the same pairs shuffled across rows and columns: only the multiset matters
    flat = rng.permutation(S.size)
    S2 = S.ravel()[flat].reshape(140, 300)
    Y2 = sp.csr_matrix(Yd.ravel()[flat].reshape(140, 300))
    np.testing.assert_array_equal(ss.Pool(dtype).add_rows(Y2, S2).metrics_array(), one)


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
    B = rng.random((n, 128)) < 0.3
    return ss.DeviceGraph.from_fingerprints(None, ss.pack_fingerprints(B), Y, alpha=0.2, weighted=True, dtype=dtype), Y


def _torch_dtype(dtype):
    import torch
    return torch.float32 if dtype == np.float32 else torch.float64


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("kind", ["csr", "fingerprint"])
def test_add_loo_and_kfold_equal_predict_then_add_rows(dtype, kind):
    import torch
    ss.init(0)
    rng = np.random.default_rng(3)
    g, Y = _graph(kind, dtype, rng)
    n, nt = g.ns, g.nt
    Yd = Y.toarray()
    fold = rng.integers(0, 5, n).astype(np.int32)
    for clean in (False, True):
        out = torch.empty((n, nt), dtype=_torch_dtype(dtype), device="cuda")
        g.predict_loo(0, n, clean=clean, out=out)
        want = ss.Pool(dtype).add_rows(Y, out).metrics_array()
        ref, scale = R.metrics(*R.table(Yd.ravel(), out.cpu().numpy().ravel()))
        R.assert_pooled_close(want, ref, scale, f"loo {kind}")
        for br in (0, 1, 10, 64):
            p = ss.Pool(dtype).add_loo(g, 0, n, clean=clean, block_rows=br)
            assert any(t.startswith("pool_radix") for t in ss.path_last()), ss.path_last()
            np.testing.assert_array_equal(p.metrics_array(), want, err_msg=f"loo block_rows={br}")
        # shards in two pools, merged
        a = ss.Pool(dtype).add_loo(g, 0, 40, clean=clean, block_rows=7)
        a.merge(ss.Pool(dtype).add_loo(g, 40, n, clean=clean, block_rows=13))
        np.testing.assert_array_equal(a.metrics_array(), want)
        np.testing.assert_array_equal(np.array(list(g.evaluate_loo_pooled(clean=clean).values())), want)

        kout = torch.empty((n, nt), dtype=_torch_dtype(dtype), device="cuda")
        g.predict_kfold_rows(fold, 5, 0, n, clean=clean, out=kout)
        kwant = ss.Pool(dtype).add_rows(Y, kout).metrics_array()
        ref, scale = R.metrics(*R.table(Yd.ravel(), kout.cpu().numpy().ravel()))
        R.assert_pooled_close(kwant, ref, scale, f"kfold {kind}")
        for br in (0, 1, 17):
            p = ss.Pool(dtype).add_kfold(g, fold, 5, 0, n, clean=clean, block_rows=br)
            np.testing.assert_array_equal(p.metrics_array(), kwant, err_msg=f"kfold block_rows={br}")
        b = ss.Pool(dtype).add_kfold(g, fold, 5, 30, n, clean=clean).add_kfold(g, fold, 5, 0, 30, clean=clean)
        np.testing.assert_array_equal(b.metrics_array(), kwant)
        np.testing.assert_array_equal(np.array(list(g.evaluate_kfold_pooled(fold, 5, clean=clean).values())), kwant)
    g.close()


def _iris():
    here = os.path.join(ROOT, "tests", "golden", "iris")

    def read(p):
        with open(os.path.join(here, p)) as f:
            lines = f.read().splitlines()
        return np.array([[float(v) for v in l.split()[1:]] for l in lines[1:]])
    return read("iris.features"), read("iris.classes")


def test_iris_loo_fp64_is_the_tutorials_number_without_the_fp32_cast():
    ss.init(0)
    F, Cm = _iris()
    S = ss.jaccard_similarity(F)
    g = ss.DeviceGraph.from_dense(None, S, Cm, alpha=0.9, weighted=True, dtype=np.float64)
    yhat = g.predict_loo(clean=True)
    want, scale = R.metrics(*R.table(Cm.ravel(), yhat.ravel()))
    got = g.evaluate_loo_pooled(clean=True)
    R.assert_pooled_close(np.array(list(got.values())), want, scale, "iris")
    assert got["AuROC"] > 0.9
    g.close()


def test_counts_past_2_31():
    import torch
    ss.init(0)
    # a synthetic table with counts around 1e10: against the Python-integer mirror, mcc included
    rng = np.random.default_rng(4)
    keys = np.sort(rng.choice(np.arange(-500, 4000), 300, replace=False))[::-1].astype(np.float64) / 64
    npos = rng.integers(0, 3 * 10 ** 8, 300).astype(np.int64)
    nneg = rng.integers(1, 6 * 10 ** 9, 300).astype(np.int64)
    for dtype in (np.float32, np.float64):
        p = ss.Pool(dtype).import_(keys.astype(dtype), npos, nneg)
        want, scale = R.metrics(keys.astype(dtype), npos, nneg)
        R.assert_pooled_close(p.metrics_array(), want, scale, f"1e10 {dtype}")
        assert p.info()["n"] == int(npos.sum() + nneg.sum()) > 2 ** 31
    # one real 1 GiB fp32 block nine times: 2.4e9 pairs; every rate is the same ratio, so the three numbers are bitwise
    gen = torch.Generator(device="cuda")
    gen.manual_seed(5)
    nrows, ncols = 2048, 131072
    S = (torch.randint(0, 1 << 20, (nrows, ncols), device="cuda", generator=gen) - 1000).float() / (1 << 12)
    Ymask = torch.rand((nrows, ncols), device="cuda", generator=gen) < 0.01
    ptr = torch.zeros(nrows + 1, dtype=torch.int64, device="cuda")
    ptr[1:] = torch.cumsum(Ymask.sum(1), 0)
    idx = Ymask.nonzero()[:, 1].to(torch.int32).contiguous()
    del Ymask
    one = ss.Pool(np.float32).add_rows((ptr, idx), S).metrics_array()
    p = ss.Pool(np.float32)
    for _ in range(9):
        p.add_rows((ptr, idx), S)
    nine = p.metrics_array()
    assert p.info()["n"] == 9 * nrows * ncols > 2 ** 31
    np.testing.assert_array_equal(nine[:3], one[:3])
    assert np.isfinite(nine).all()


def _same(p, m, i):
    np.testing.assert_array_equal(p.metrics_array(), m)
    assert p.info() == i


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_errors_leave_the_pool_as_it_was(dtype):
    ss.init(0)
    rng = np.random.default_rng(6)
    S, Y = _block(rng, 20, 200, dtype, 5000)
    p = ss.Pool(dtype).add_rows(Y, S)
    m, i = p.metrics_array(), p.info()
    bad = S.copy()
    bad[3, 7] = np.nan
    with pytest.raises(ss.SimSpreadError, match="NaN"):
        p.add_rows(Y, bad)
    _same(p, m, i)
    # labels not sorted in a row: the library's own check (the Python layer would refuse them first)
    ptr = np.array([0, 2], np.int64)
    idx = np.array([5, 3], np.int32)
    fn = getattr(_lib.lib(), f"ss_pool_add_rows_{'f32' if dtype == np.float32 else 'f64'}")
    row = np.ascontiguousarray(S[:1])
    assert fn(p._h, ptr.ctypes.data, idx.ctypes.data, 0, row.ctypes.data, 1, 200, 200, _lib.SS_MEM_HOST) == -1
    _same(p, m, i)
    # the other precision
    other = getattr(_lib.lib(), f"ss_pool_add_rows_{'f64' if dtype == np.float32 else 'f32'}")
    row2 = row.astype(np.float64 if dtype == np.float32 else np.float32)
    ok = np.array([0, 1], np.int64)
    assert other(p._h, ok.ctypes.data, idx.ctypes.data, 0, row2.ctypes.data, 1, 200, 200, _lib.SS_MEM_HOST) == -1
    _same(p, m, i)
    with pytest.raises(ss.SimSpreadError):
        p.merge(ss.Pool(np.float64 if dtype == np.float32 else np.float32).add_rows(Y, S.astype(
            np.float64 if dtype == np.float32 else np.float32)))
    _same(p, m, i)
    # import of a table that is not strictly descending
    with pytest.raises(ss.SimSpreadError, match="descending"):
        p.import_(np.array([1.0, 2.0], dtype), np.array([1, 1]), np.array([0, 0]))
    _same(p, m, i)
    # capacity
    small = ss.Pool(dtype, max_entries=i["entries"] + 3).add_rows(Y, S)
    ms, is_ = small.metrics_array(), small.info()
    S3, Y3 = _block(rng, 20, 200, dtype, 100000)
    with pytest.raises(ss.SimSpreadError, match="max_entries"):
        small.add_rows(Y3, S3 + dtype(1000))
    _same(small, ms, is_)
    with pytest.raises(ss.SimSpreadError, match="empty"):
        ss.Pool(dtype).metrics_array()


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
    p = ss_.Pool(np.float32).add_loo(g, lo, hi, clean=True, block_rows=50)
    out = ss_.pooled_metrics(p, root=0)
    assert (out is None) == (rank != 0)
    if rank == 0:
        np.save(os.path.join(tmp, "pooled.npy"), np.array(list(out.values())))
    dist.barrier()
    dist.destroy_process_group()


def test_two_ranks_meet_in_dist_pooled_metrics(tmp_path):
    import torch.multiprocessing as mp
    mp.spawn(_rank_worker, args=(2, _free_port(), str(tmp_path)), nprocs=2, join=True)
    ss.init(0)
    g, _ = _graph("csr", np.float32, np.random.default_rng(8), n=211, nt=97)
    want = ss.Pool(np.float32).add_loo(g, clean=True).metrics_array()
    np.testing.assert_array_equal(np.load(tmp_path / "pooled.npy"), want)
