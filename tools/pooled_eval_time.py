"""Timing of pooled evaluation (ss_pool_add_loo_*) on the C3 graph (100k x 100k, 1 %, built on the device as
tools/c3_loo.py builds it):

  block      one 2048-fold block (2.05e8 scores): predict_loo into a device buffer, evaluate_loo (per-row ranking
             metrics, for scale), pool.add_loo into an empty pool (predict + pooling) and the pooling share of it
             (ss_timing_last epilogue), and the table entries after the block
  sweep      the whole fp32 C3 leave-one-out sweep (1e10 scores): predict_loo block by block (predict only) against
             pool.add_loo over every fold followed by pool.metrics(); final table entries, levels stored, peak device
             memory (free memory sampled every 2 ms during the sweep)

Warm, median of REPS, host clock around work that ends in a device synchronise.  The HBM floor of the pooling is one
read of the block's scores (819 MB at 2048 x 100k fp32) at 6.3 TB/s.  The kernel split comes from a separate
`rocprofv3 --kernel-trace --stats` run of `--block-only`.

    python tools/pooled_eval_time.py [--folds 2048] [--reps 5] [--block-only] [--out profiles/pooled_eval_time.json]
"""
import argparse
import json
import os
import sys
import threading
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

HBM = 6.3e12


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


class _PeakSampler:
    """Lowest free device memory seen while running (the library's buffers are its own hipMallocs)."""

    def __init__(self):
        import torch
        self.base = torch.cuda.mem_get_info()[0]
        self.low = self.base
        self.stop = False
        self.t = threading.Thread(target=self._run, daemon=True)

    def _run(self):
        import torch
        while not self.stop:
            self.low = min(self.low, torch.cuda.mem_get_info()[0])
            time.sleep(0.002)

    def __enter__(self):
        self.t.start()
        return self

    def __exit__(self, *a):
        self.stop = True
        self.t.join()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--folds", type=int, default=2048)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--block-only", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    import simspread_jl_amd as ss
    from tools.c3_loo import rand_csr, rand_sym_csr
    ss.init(0)
    ss.use_torch_stream()
    n, folds = 100_000, a.folds
    gen = torch.Generator(device="cuda"); gen.manual_seed(20250222 + 3)
    xp, xi = rand_sym_csr(n, 0.01, gen)
    yp, yi = rand_csr(n, n, 0.01, gen)
    xv = (0.5 + 0.5 * torch.rand(xi.numel(), device="cuda", generator=gen)).float()
    g = ss.DeviceGraph.from_device_csr(0, n, n, n, None, (xp, xi, xv), (yp, yi, None), dtype=np.float32)
    res = dict(config="C3", folds=folds, ncols=n)
    out = torch.empty((folds, n), dtype=torch.float32, device="cuda")
    res["predict_loo_ms"] = _median_ms(lambda: g.predict_loo(0, folds, clean=True, out=out), a.reps)
    res["evaluate_loo_ms"] = _median_ms(lambda: g.evaluate_loo(0, folds, clean=True, L=20), a.reps)
    p = ss.Pool(np.float32)
    pool_ms, pool_share = [], []
    for _ in range(a.reps + 1):
        p.reset()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        p.add_loo(g, 0, folds, clean=True)
        torch.cuda.synchronize()
        pool_ms.append((time.perf_counter() - t0) * 1e3)
        pool_share.append(ss.timing_last()["epilogue_ms"])
    res["pool_add_loo_ms"] = float(np.median(pool_ms[1:]))
    res["pool_share_ms"] = float(np.median(pool_share[1:]))
    res["pool_path"] = ss.path_last()
    res["pool_share_over_predict"] = res["pool_share_ms"] / res["predict_loo_ms"]
    info = p.info()
    res["entries_after_block"] = info["entries"]
    res["pairs_after_block"] = info["n"]
    res["hbm_floor_pool_ms"] = folds * n * 4 / HBM * 1e3
    res["pool_add_rows_ms"] = _median_ms(lambda: ss.Pool(np.float32).add_rows((yp[:folds + 1].contiguous(), yi), out),
                                         a.reps)
    res["metrics_ms"] = _median_ms(lambda: p.metrics_array(), a.reps)
    res["block_metrics"] = p.metrics()
    print(json.dumps(res), flush=True)
    del out
    torch.cuda.empty_cache()
    sweep = None
    if not a.block_only:
        buf = torch.empty((folds, n), dtype=torch.float32, device="cuda")

        def predict_sweep():
            for i0 in range(0, n, folds):
                i1 = min(n, i0 + folds)
                g.predict_loo(i0, i1, clean=True, out=buf[:i1 - i0])
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        predict_sweep()
        torch.cuda.synchronize()
        pred_s = time.perf_counter() - t0
        del buf
        torch.cuda.empty_cache()
        p.reset()
        with _PeakSampler() as smp:
            t0 = time.perf_counter()
            p.add_loo(g, 0, n, clean=True, block_rows=folds)
            torch.cuda.synchronize()
            add_s = time.perf_counter() - t0
            held = p.info()["entries"]
            t1 = time.perf_counter()
            m = p.metrics()
            met_s = time.perf_counter() - t1
        share = ss.timing_last()
        sweep = dict(predict_only_s=pred_s, pool_add_loo_s=add_s, pool_metrics_s=met_s,
                     pooled_over_predict=(add_s + met_s) / pred_s, entries_before_metrics=held,
                     final_entries=p.info()["entries"], pairs=p.info()["n"], positives=p.info()["npos"],
                     peak_device_bytes_over_start=smp.base - smp.low, metrics=m)
        print(json.dumps(sweep), flush=True)
    p.close()
    g.close()
    if a.out:
        with open(a.out, "w") as f:
            json.dump(dict(source_hash=ss._lib.source_hash(), block=res, sweep=sweep), f, indent=1)


if __name__ == "__main__":
    main()
