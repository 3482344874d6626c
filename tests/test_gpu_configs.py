"""BASELINE.json configs 3-5 at (or near) their full sizes, through the same C ABI: a block of folds is scored
on the GPU and every fold of it is checked against an fp64 CPU oracle (the C leave-one-out form for the sparse
configs, a blocked dense form for C4 at 20k; a strided sample covering every 256-row M-tile at 50k), entry by entry
(tests/block_compare.py)."""
import time

import numpy as np
import pytest
import scipy.sparse as sp

import simspread_jl_amd as ss
from block_compare import compare_block
from oracle import c_oracle
from oracle import simspread_oracle as O

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def _init():
    ss.init(0)
    ss.use_torch_stream()


def _host_csr(ptr, idx, val, shape):
    v = np.ones(idx.numel()) if val is None else val.cpu().numpy().astype(np.float64)
    return sp.csr_matrix((v, idx.cpu().numpy(), ptr.cpu().numpy()), shape=shape)


def _timed(label, fn, *a, **kw):
    t = time.perf_counter()
    r = fn(*a, **kw)
    print(f"[oracle] {label}: {time.perf_counter() - t:.1f} s host")
    return r


@pytest.fixture(scope="module")
def c3():
    """The C3 graph (100k x 100k, 1 %, nnz 1e8 each) on the device, and the C leave-one-out oracle prepared on it once
    for the fp32 and fp64 cases (X's values are drawn in fp32, so both precisions score the same graph)."""
    import torch
    from tools.c3_loo import rand_csr, rand_sym_csr
    n = 100_000
    gen = torch.Generator(device="cuda"); gen.manual_seed(20250222 + 3)
    xp, xi = rand_sym_csr(n, 0.01, gen)
    yp, yi = rand_csr(n, n, 0.01, gen)
    xv = (0.5 + 0.5 * torch.rand(xi.numel(), device="cuda", generator=gen)).float()
    X, Y = _host_csr(xp, xi, xv, (n, n)), _host_csr(yp, yi, None, (n, n))
    prep = _timed("C3 prepare", c_oracle.PreparedLoo, X, Y)
    del X, Y
    yield n, (xp, xi, xv), (yp, yi), prep
    prep.close()


def test_config3_100k_loo_block_vs_oracle(c3):
    """C3: 100k x 100k, 1 % (nnz 1e8 each), leave-one-out; one 512-fold block of the 100k folds, every fold."""
    import torch
    n, (xp, xi, xv), (yp, yi), prep = c3
    folds = 512
    g = ss.DeviceGraph.from_device_csr(0, n, n, n, None, (xp, xi, xv), (yp, yi, None), dtype=np.float32)
    assert g.nnz_xs > 9.9e7 and g.nnz_ys > 9.9e7
    lo = 50_000                                     # a block in the middle: what rank 4 of 8 would start with
    out = torch.empty((folds, n), dtype=torch.float32, device="cuda")
    g.predict_loo(lo, lo + folds, clean=True, out=out)
    want = _timed("C3 512 folds", prep.predict, lo, lo + folds, clean=True)
    compare_block(out.cpu().numpy(), want, np.float32, "C3 fp32 512 folds")
    # the same folds scored as part of a different block must give bit-identical rows (fold independence,
    # the property the 8-GPU sharding relies on)
    out2 = torch.empty((256, n), dtype=torch.float32, device="cuda")
    g.predict_loo(lo + 128, lo + 384, clean=True, out=out2)
    assert torch.equal(out2, out[128:384])


def test_config3_100k_loo_fp64(c3):
    """The C3 graph in fp64: transfer_loo + the SELL stage 2 at full size, a 128-fold block, every fold to 1e-12."""
    import torch
    n, (xp, xi, xv), (yp, yi), prep = c3
    folds, lo = 128, 70_000
    g = ss.DeviceGraph.from_device_csr(0, n, n, n, None, (xp, xi, xv.double()), (yp, yi, None), dtype=np.float64)
    out = torch.empty((folds, n), dtype=torch.float64, device="cuda")
    g.predict_loo(lo, lo + folds, clean=True, out=out)
    path = ss.path_last()
    assert "transfer_loo" in path and ("spmm_sell" in path or "spmm_sell_sorted" in path), path
    want = _timed("C3 128 folds", prep.predict, lo, lo + folds, clean=True)
    compare_block(out.cpu().numpy(), want, np.float64, "C3 fp64 128 folds")
    g.close()


def test_config5_power_law_block_vs_oracle():
    """C5 at its specified weight: Zipf(1.2) source degrees (mean 1000, capped at Nt) and target popularity,
    nnz(Y) ~ 1e8 AFTER de-duplication, 200k nodes, hot rows/columns at random positions."""
    import torch
    from tools.c3_loo import rand_sym_csr
    from tools.c5_powerlaw import zipf_bipartite_spec
    n, folds = 100_000, 256
    gen = torch.Generator(device="cuda"); gen.manual_seed(20250222 + 5)
    xp, xi = rand_sym_csr(n, 0.01, gen)
    yp, yi = zipf_bipartite_spec(n, n, 1000, 1.2, gen)
    assert 0.97e8 < yi.numel() < 1.03e8, yi.numel()        # the spec's weight, not a tenth of it
    xv = (0.5 + 0.5 * torch.rand(xi.numel(), device="cuda", generator=gen)).float()
    g = ss.DeviceGraph.from_device_csr(0, n, n, n, None, (xp, xi, xv), (yp, yi, None), dtype=np.float32)
    kf, ks, kt = g.degrees()
    rowdeg = (yp[1:] - yp[:-1]).cpu().numpy()
    assert kt.max() > 50_000 and rowdeg.max() > 90_000          # hot targets and (capped) hot sources
    assert np.median(rowdeg) < 400 and np.median(kt) < 1500     # ... and a long cold tail on both sides
    out = torch.empty((folds, n), dtype=torch.float32, device="cuda")
    g.predict_loo(0, folds, clean=True, out=out)
    assert "spmm_sell_sorted" in ss.path_last()                 # the skew-sorted, row-split stage-2 operand was chosen
    X, Y = _host_csr(xp, xi, xv, (n, n)), _host_csr(yp, yi, None, (n, n))
    # every fold of the block, the heaviest source inside it among them
    prep = _timed("C5 prepare", c_oracle.PreparedLoo, X, Y)
    del X, Y
    want = _timed("C5 256 folds", prep.predict, 0, folds, clean=True)
    prep.close()
    compare_block(out.cpu().numpy(), want, np.float32, "C5 fp32 256 folds")


def test_config4_dense_similarity_cutoff_sweep():
    """C4, small shape (12k sources, 512 folds -> the 128 x 128 bf16 kernel): raw similarity dense, cutoff sweep,
    MFMA stage 1, both weightings; S as SURVEY.md 8d states it (fill(S >= alpha) = 1 - alpha, measured)."""
    import torch
    from tools.c3_loo import rand_csr
    from tools.c4_dense import measured_fill, sym_uniform
    n, nt, folds = 12_000, 3_000, 512
    gen = torch.Generator(device="cuda"); gen.manual_seed(20250222 + 4)
    S = sym_uniform(n, gen)
    yp, yi = rand_csr(n, nt, 0.01, gen)
    Sh = S.cpu().numpy().astype(np.float64)
    Y = _host_csr(yp, yi, None, (n, nt))
    out = torch.empty((folds, nt), dtype=torch.float32, device="cuda")
    for alpha, weighted in ((0.1, True), (0.5, False), (0.9, True)):
        assert abs(measured_fill(S, alpha) - (1.0 - alpha)) < 2e-3
        g = ss.DeviceGraph.from_similarity(None, S, (yp, yi, None, nt), alpha=alpha, weighted=weighted)
        g.predict_loo(1000, 1000 + folds, clean=True, out=out)
        assert "transfer_dense_bf16_128" in ss.path_last()
        X = O.cutoff(Sh, float(np.float32(alpha)), weighted)
        want = O.predict_loo_dense_blocked(X, Y, clean_flag=True, queries=range(1000, 1000 + folds))
        compare_block(out.cpu().numpy(), want, np.float32, f"C4 12k bf16-128 alpha={alpha} weighted={weighted}")
        g.close()


@pytest.mark.parametrize("n", [20_000, 50_000])
def test_config4_ring_kernel_auto_selected(n):
    """C4 at production shapes: 4096 folds per alpha make (Mp/256) x (Np/256) >= 256 tiles, so the 256 x 256 ring
    kernel is chosen by size (NOT forced) and runs hundreds of K-tiles (20k: 313, 50k -- BASELINE configs[3] -- 782).
    90 % fill (alpha = 0.1, the named regime), both weightings, plus a sparse end of the sweep; against the fp64 oracle
    (the dense LOO form, blocked): every fold at 20k, at 50k a strided sample of 512 folds, 32 in each of the 16 256-row
    M-tiles, at every offset modulo 8 within a tile, the first and the last fold of the block among them."""
    import torch
    from tools.c3_loo import rand_csr
    from tools.c4_dense import measured_fill, sym_uniform
    nt, folds, lo = 10_000, 4096, 3000
    gen = torch.Generator(device="cuda"); gen.manual_seed(20250222 + 4)
    S = sym_uniform(n, gen)
    yp, yi = rand_csr(n, nt, 0.01, gen)
    Sh = S.cpu().numpy()
    Y = _host_csr(yp, yi, None, (n, nt))
    out = torch.empty((folds, nt), dtype=torch.float32, device="cuda")
    cases = ((0.1, True), (0.1, False), (0.9, True)) if n <= 20_000 else ((0.1, True), (0.1, False))
    for alpha, weighted in cases:
        assert abs(measured_fill(S, alpha) - (1.0 - alpha)) < 2e-3
        g = ss.DeviceGraph.from_similarity(None, S, (yp, yi, None, nt), alpha=alpha, weighted=weighted)
        g.predict_loo(lo, lo + folds, clean=True, out=out)
        assert "transfer_dense_bf16_ring" in ss.path_last(), ss.path_last()
        X = O.cutoff(Sh, np.float32(alpha), weighted)      # thresholded in fp32 like the device, summed in fp64
        rows = np.arange(folds) if n <= 20_000 else np.arange(0, folds, 8) + np.arange(folds // 8) % 8
        want = _timed(f"C4 {n} {len(rows)} folds", O.predict_loo_dense_blocked, X, Y, clean_flag=True, queries=lo + rows)
        del X
        compare_block(out[torch.from_numpy(rows).cuda()].cpu().numpy(), want, np.float32,
                      f"C4 {n} ring alpha={alpha} weighted={weighted} ({len(rows)} folds)")
        g.close()


def test_config4_fp64_dense_path_at_20k():
    """The fp64 dense-similarity kernel (dense_f64.hip, v_mfma_f64_16x16x4_f64) at the shape profiles/ quotes it on:
    20k sources x 4096 folds = 1250 K-steps of 16 per tile, routed by the constructor (not forced), both weightings at
    the 90 % fill of the named regime plus the sparse end; every fold against the fp64 oracle (blocked dense LOO form)."""
    import torch
    from tools.c3_loo import rand_csr
    from tools.c4_dense import measured_fill, sym_uniform
    n, nt, folds, lo = 20_000, 10_000, 4096, 3000
    gen = torch.Generator(device="cuda"); gen.manual_seed(20250222 + 4)
    S = sym_uniform(n, gen).double()
    yp, yi = rand_csr(n, nt, 0.01, gen)
    Sh = S.cpu().numpy()
    Y = _host_csr(yp, yi, None, (n, nt))
    out = torch.empty((folds, nt), dtype=torch.float64, device="cuda")
    for alpha, weighted in ((0.1, True), (0.1, False), (0.9, True)):
        assert abs(measured_fill(S, alpha) - (1.0 - alpha)) < 2e-3
        g = ss.DeviceGraph.from_similarity(None, S, (yp, yi, None, nt), alpha=alpha, weighted=weighted, dtype=np.float64)
        g.predict_loo(lo, lo + folds, clean=True, out=out)
        assert "transfer_dense_f64_mfma" in ss.path_last(), ss.path_last()
        X = O.cutoff(Sh, alpha, weighted)
        want = _timed("C4 fp64 4096 folds", O.predict_loo_dense_blocked, X, Y, clean_flag=True,
                      queries=range(lo, lo + folds))
        del X
        compare_block(out.cpu().numpy(), want, np.float64, f"C4 20k fp64 alpha={alpha} weighted={weighted}")
        g.close()


def test_kfold_10k_sources_vs_oracle():
    """10-fold cross-validation in one call at 10k sources (the shape tools/kfold_time.py times): symmetric ~5 % weighted
    similarity, 1 % labels, clean!, fp32; every row against the C oracle's query form run once per fold on the blocks
    construct(y, X, members) leaves (c_oracle.predict_kfold, pinned against the literal fold loop in test_oracle.py)."""
    n, k = 10_000, 10
    rng = np.random.default_rng(7)
    X = sp.random(n, n, density=0.025, format="csr", random_state=rng, dtype=np.float32)
    X = X + X.T; X.setdiag(1.0); X = sp.csr_matrix(X); X.data = (0.5 + 0.5 * rng.random(X.nnz)).astype(np.float32)
    Y = sp.random(n, n, density=0.01, format="csr", random_state=rng, dtype=np.float32); Y.data[:] = 1.0
    fold = rng.integers(0, k, n).astype(np.int32)
    g = ss.DeviceGraph.from_sparse(None, X, Y, dtype=np.float32)
    got = g.predict_kfold(fold, k, clean=True)
    g.close()
    want = _timed("k-fold 10k", c_oracle.predict_kfold, X.astype(np.float64), Y.astype(np.float64), fold, k, clean=True)
    compare_block(got, want, np.float32, "k-fold 10k x 10 folds")
