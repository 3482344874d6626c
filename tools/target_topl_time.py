"""Timing of per-target top-L tables (ss_target_topl_add_loo_*) on the C3 graph (100k x 100k, 1 %, fp32, built on the
device as tools/c3_loo.py builds it):

  block      one 2048-fold block (2.05e8 scores): predict_loo into a device buffer, target_topl.add_loo into an empty
             handle (predict + top-L) and the top-L share of it (ss_timing_last epilogue, ms[3]), for L = 20 and 1024
  sweep      the whole fp32 C3 leave-one-out sweep (1e10 scores): predict_loo block by block (predict only) against
             add_loo over every fold followed by metrics(), L = 20

Warm, median of REPS, host clock around work that ends in a device synchronise.  The HBM floor of the top-L share is
one read of the block's scores (819 MB at 2048 x 100k fp32) at 6.3 TB/s.  The kernel split comes from a separate
`rocprofv3 --kernel-trace --stats` run of `--block-only`.

    python tools/target_topl_time.py [--folds 2048] [--reps 5] [--block-only] [--out profiles/target_topl_time.json]
"""
import argparse
import json
import os
import sys
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
    res = dict(config="C3", folds=folds, ncols=n, hbm_floor_topl_ms=folds * n * 4 / HBM * 1e3)
    out = torch.empty((folds, n), dtype=torch.float32, device="cuda")
    res["predict_loo_ms"] = _median_ms(lambda: g.predict_loo(0, folds, clean=True, out=out), a.reps)
    del out
    torch.cuda.empty_cache()
    for L in (20, 1024):
        h = ss.TargetTopL(n, L, np.float32)
        tot, share = [], []
        for _ in range(a.reps + 1):
            h.reset()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            h.add_loo(g, 0, folds, clean=True)
            torch.cuda.synchronize()
            tot.append((time.perf_counter() - t0) * 1e3)
            share.append(ss.timing_last()["epilogue_ms"])
        r = dict(add_loo_ms=float(np.median(tot[1:])), topl_share_ms=float(np.median(share[1:])),
                 path=ss.path_last())
        # a second block into the seeded table: the filter + merge path alone
        tot2, share2 = [], []
        for _ in range(a.reps):
            h.reset()
            h.add_loo(g, 0, folds, clean=True)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            h.add_loo(g, folds, 2 * folds, clean=True)
            torch.cuda.synchronize()
            tot2.append((time.perf_counter() - t0) * 1e3)
            share2.append(ss.timing_last()["epilogue_ms"])
        r.update(second_block_add_loo_ms=float(np.median(tot2)), second_block_topl_share_ms=float(np.median(share2)),
                 second_block_path=ss.path_last())
        r["topl_share_over_predict"] = r["topl_share_ms"] / res["predict_loo_ms"]
        res[f"L{L}"] = r
        h.close()
        torch.cuda.empty_cache()
    print(json.dumps(res), flush=True)
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
        h = ss.TargetTopL(n, 20, np.float32)
        t0 = time.perf_counter()
        h.add_loo(g, 0, n, clean=True, block_rows=folds)
        torch.cuda.synchronize()
        add_s = time.perf_counter() - t0
        share_s = ss.timing_last()["epilogue_ms"] / 1e3
        path = ss.path_last()
        t1 = time.perf_counter()
        m = h.metrics()
        met_s = time.perf_counter() - t1
        sweep = dict(L=20, predict_only_s=pred_s, add_loo_s=add_s, topl_share_s=share_s, metrics_s=met_s,
                     add_loo_over_predict=add_s / pred_s, path=path,
                     metrics={k: m[k] for k in ss.TARGET_TOPL_FIELDS}, rows=h.info()["rows"], positives=h.info()["npos"])
        print(json.dumps(sweep), flush=True)
        h.close()
    g.close()
    if a.out:
        with open(a.out, "w") as f:
            json.dump(dict(source_hash=ss._lib.source_hash(), block=res, sweep=sweep), f, indent=1)


if __name__ == "__main__":
    main()
