"""Timing of k-fold cross-validation in row blocks and evaluated in place, 10 folds (random assignment):

  C3 (100k x 100k, 1 %, built on the device as tools/c3_loo.py builds it), fp32 and fp64:
    kfold          ss_predict_kfold_* over all sources into a device row-major buffer (the no-copy path)
    kfold_rows     ss_predict_kfold_rows_* over all sources into the same buffer          target <= 1.05 x kfold
    evaluate       ss_evaluate_kfold_* over all sources (block_rows = 0)                  target <= 1.2 x kfold_rows
    evaluate_bin   ss_evaluate_kfold_binary_* over all sources (block_rows = 0)           target <= 3 x kfold_rows
  C5 (Zipf(1.2) labels: the stage-2 operand is length-sorted), fp32: kfold (one row copy per member) against kfold_rows
  (one scatter kernel per batch).
  10k (the graph of tools/kfold_time.py), fp32: today's route -- ss_predict_kfold_f32 to the host, then
  rank_metrics_rows / binary_metrics_rows on host arrays -- against evaluate_kfold / evaluate_kfold_binary.

Warm, median of REPS, host clock around work that ends in a device synchronise; the stage split of the last call from
ss_timing_last.

    python tools/kfold_eval_time.py [--reps 3] [--no-c5] [--no-10k] [--out profiles/kfold_eval_time.json]
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

K = 10


def _median_ms(fn, reps):
    import torch
    fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(ts))


def _split():
    import simspread_jl_amd as ss
    t = ss.timing_last()
    return {k: round(t[k], 3) for k in ("total_ms", "transfer_ms", "spmm_ms", "epilogue_ms")}


def _kfold_device(g, fold_dev, out):
    """ss_predict_kfold_* with a device row-major out (Python's predict_kfold writes to the host only)."""
    import simspread_jl_amd as ss
    from simspread_jl_amd import _lib
    ss.use_torch_stream()
    fn = getattr(_lib.lib(), f"ss_predict_kfold_{g._suf}")
    _lib.check(fn(g._h, fold_dev.data_ptr(), K, 1, out.data_ptr(), g.nt, _lib.SS_LAYOUT_ROWMAJOR, _lib.SS_MEM_DEVICE))


def measure_full(name, g, fold, reps, evaluate=True):
    import torch
    import simspread_jl_amd as ss
    n = g.ns
    dt = torch.float32 if g.dtype == np.float32 else torch.float64
    out = torch.empty((n, g.nt), dtype=dt, device="cuda")
    fold_dev = torch.from_numpy(fold).cuda()
    res = dict(config=name, dtype=str(g.dtype), ns=n, nt=g.nt, folds=K)
    res["kfold_ms"] = _median_ms(lambda: _kfold_device(g, fold_dev, out), reps)
    res["kfold_split"] = _split()
    res["kfold_path"] = ss.path_last()
    ref = out[:4096].clone()
    res["kfold_rows_ms"] = _median_ms(lambda: g.predict_kfold_rows(fold, K, clean=True, out=out), reps)
    res["kfold_rows_split"] = _split()
    res["kfold_rows_path"] = ss.path_last()
    res["rows_equal_kfold_first_4096"] = bool(torch.equal(ref, out[:4096]))
    res["rows_over_kfold"] = res["kfold_rows_ms"] / res["kfold_ms"]
    del out, ref
    torch.cuda.empty_cache()
    if evaluate:
        res["evaluate_ms"] = _median_ms(lambda: g.evaluate_kfold(fold, K, clean=True, L=20), reps)
        res["evaluate_split"] = _split()
        res["evaluate_path"] = ss.path_last()
        res["evaluate_binary_ms"] = _median_ms(lambda: g.evaluate_kfold_binary(fold, K, clean=True), reps)
        res["evaluate_binary_split"] = _split()
        res["evaluate_binary_path"] = ss.path_last()
        res["evaluate_over_rows"] = res["evaluate_ms"] / res["kfold_rows_ms"]
        res["evaluate_binary_over_rows"] = res["evaluate_binary_ms"] / res["kfold_rows_ms"]
        res["targets"] = {"rows_within_5pct": res["rows_over_kfold"] <= 1.05,
                          "evaluate_le_1.2x": res["evaluate_over_rows"] <= 1.2,
                          "evaluate_binary_le_3x": res["evaluate_binary_over_rows"] <= 3.0}
    return res


def measure_10k(reps):
    import scipy.sparse as sp
    import simspread_jl_amd as ss
    n = 10000
    rng = np.random.default_rng(7)
    X = sp.random(n, n, density=0.025, format="csr", random_state=rng, dtype=np.float32)
    X = X + X.T; X.setdiag(1.0); X = sp.csr_matrix(X); X.data = (0.5 + 0.5 * rng.random(X.nnz)).astype(np.float32)
    Y = sp.random(n, n, density=0.01, format="csr", random_state=rng, dtype=np.float32); Y.data[:] = 1.0
    Y.sort_indices()
    g = ss.DeviceGraph.from_sparse(None, X, Y, dtype=np.float32)
    fold = rng.integers(0, K, n).astype(np.int32)
    res = dict(config="10k", dtype="float32", ns=n, nt=n, folds=K)

    def host_route(binary):
        s = g.predict_kfold(fold, K, clean=True)
        return ss.binary_metrics_rows(Y, s) if binary else ss.rank_metrics_rows(Y, s, L=20)
    res["host_route_rank_ms"] = _median_ms(lambda: host_route(False), reps)
    res["evaluate_ms"] = _median_ms(lambda: g.evaluate_kfold(fold, K, clean=True, L=20), reps)
    res["host_route_binary_ms"] = _median_ms(lambda: host_route(True), reps)
    res["evaluate_binary_ms"] = _median_ms(lambda: g.evaluate_kfold_binary(fold, K, clean=True), reps)
    res["rank_equal"] = bool(np.array_equal(host_route(False), g.evaluate_kfold(fold, K, clean=True, L=20)))
    g.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--no-c5", action="store_true")
    ap.add_argument("--no-10k", action="store_true")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    import torch
    import simspread_jl_amd as ss
    from tools.c3_loo import rand_csr, rand_sym_csr
    ss.init(0)
    ss.use_torch_stream()
    n = 100_000
    fold = np.random.default_rng(3).integers(0, K, n).astype(np.int32)
    results = []
    gen = torch.Generator(device="cuda"); gen.manual_seed(20250222 + 3)
    xp, xi = rand_sym_csr(n, 0.01, gen)
    yp, yi = rand_csr(n, n, 0.01, gen)
    xv = (0.5 + 0.5 * torch.rand(xi.numel(), device="cuda", generator=gen)).float()
    for dt, xvt in ((np.float32, xv), (np.float64, xv.double())):
        g = ss.DeviceGraph.from_device_csr(0, n, n, n, None, (xp, xi, xvt), (yp, yi, None), dtype=dt)
        results.append(measure_full("C3", g, fold, a.reps))
        print(json.dumps(results[-1]), flush=True)
        g.close()
    del xp, xi, yp, yi, xv
    torch.cuda.empty_cache()
    if not a.no_c5:
        from tools.c5_powerlaw import zipf_bipartite_spec
        gen = torch.Generator(device="cuda"); gen.manual_seed(20250222 + 5)
        xp, xi = rand_sym_csr(n, 0.01, gen)
        yp, yi = zipf_bipartite_spec(n, n, 1000, 1.2, gen)
        xv = (0.5 + 0.5 * torch.rand(xi.numel(), device="cuda", generator=gen)).float()
        g = ss.DeviceGraph.from_device_csr(0, n, n, n, None, (xp, xi, xv), (yp, yi, None), dtype=np.float32)
        results.append(measure_full("C5", g, fold, a.reps, evaluate=False))
        print(json.dumps(results[-1]), flush=True)
        g.close()
        del xp, xi, yp, yi, xv
        torch.cuda.empty_cache()
    if not a.no_10k:
        results.append(measure_10k(a.reps))
        print(json.dumps(results[-1]), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(dict(source_hash=ss._lib.source_hash(), results=results), f, indent=1)


if __name__ == "__main__":
    main()
