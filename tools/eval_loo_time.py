"""Timing of leave-one-out evaluation on the device on the C3 graph (100k x 100k, 1 %, built on the device as
tools/c3_loo.py builds it) and on a C5-shaped block (Zipf(1.2) source degrees capped at nt, hot sources in the block):

  predict_loo   one 2048-fold block into a device buffer (stage 1 + stage 2 only)
  rows_f32      ss_rank_metrics_rows_f32 on that block (labels = the graph's Ys rows)
  rows_f64      ss_rank_metrics_rows_f64 on the same scores widened to fp64
  evaluate_loo  ss_evaluate_loo_f32 over the same folds (block_rows = 0: one block)
  per_row       ss_rank_metrics_f32 called once per row on SAMPLE rows (today's alternative), extrapolated to the block

Warm, median of REPS, host clock around work that ends in a device synchronise.  The HBM floor of a metrics call is
the bytes of the block (fp32 819 MB, fp64 1.64 GB at 2048 x 100k) plus the labels, at 6.3 TB/s.

    python tools/eval_loo_time.py [--folds 2048] [--reps 5] [--sample 64] [--no-c5] [--out profiles/eval_loo_time.json]
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


def measure(name, g, yp, yi, lo, folds, reps, sample):
    import torch
    import simspread_jl_amd as ss
    n = g.nt
    out = torch.empty((folds, n), dtype=torch.float32, device="cuda")
    ptr = yp[lo:lo + folds + 1].contiguous()
    res = dict(config=name, folds=folds, ncols=n, first_fold=lo, nnz_labels=int((ptr[-1] - ptr[0]).item()))
    deg = (ptr[1:] - ptr[:-1]).cpu().numpy()
    res.update(positives_mean=float(deg.mean()), positives_max=int(deg.max()), rows_over_2048=int((deg > 2048).sum()))
    res["predict_loo_ms"] = _median_ms(lambda: g.predict_loo(lo, lo + folds, clean=True, out=out), reps)
    res["rows_f32_ms"] = _median_ms(lambda: ss.rank_metrics_rows((ptr, yi), out, L=20), reps)
    res["rows_f32_path"] = ss.path_last()
    out64 = out.double()
    res["rows_f64_ms"] = _median_ms(lambda: ss.rank_metrics_rows((ptr, yi), out64, L=20), reps)
    del out64
    res["evaluate_loo_ms"] = _median_ms(lambda: g.evaluate_loo(lo, lo + folds, clean=True, L=20), reps)
    res["evaluate_over_predict"] = res["evaluate_loo_ms"] / res["predict_loo_ms"]
    label_bytes = (folds + 1) * 8 + res["nnz_labels"] * 4
    res["hbm_floor_f32_ms"] = (folds * n * 4 + label_bytes) / HBM * 1e3
    res["hbm_floor_f64_ms"] = (folds * n * 8 + label_bytes) / HBM * 1e3
    if sample:
        rows = np.linspace(0, folds - 1, sample).astype(int)
        idx_h = yi.cpu().numpy()
        pos = ptr.cpu().numpy()
        ys = []
        for i in rows:
            y = torch.zeros(n, dtype=torch.uint8, device="cuda")
            y[torch.from_numpy(idx_h[pos[i]:pos[i + 1]].astype(np.int64)).cuda()] = 1
            ys.append(y)

        def per_row():
            for k, i in enumerate(rows):
                ss.rank_metrics(ys[k], out[i], 20.0)
        ms = _median_ms(per_row, max(1, reps // 2))
        res["per_row_calls_ms_each"] = ms / sample
        res["per_row_calls_ms_block_extrapolated"] = ms / sample * folds
    del out
    torch.cuda.empty_cache()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--folds", type=int, default=2048)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--sample", type=int, default=64)
    ap.add_argument("--no-c5", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    import simspread_jl_amd as ss
    from tools.c3_loo import rand_csr, rand_sym_csr
    ss.init(0)
    ss.use_torch_stream()
    n = 100_000
    results = []
    gen = torch.Generator(device="cuda"); gen.manual_seed(20250222 + 3)
    xp, xi = rand_sym_csr(n, 0.01, gen)
    yp, yi = rand_csr(n, n, 0.01, gen)
    xv = (0.5 + 0.5 * torch.rand(xi.numel(), device="cuda", generator=gen)).float()
    g = ss.DeviceGraph.from_device_csr(0, n, n, n, None, (xp, xi, xv), (yp, yi, None), dtype=np.float32)
    results.append(measure("C3", g, yp, yi, 0, a.folds, a.reps, a.sample))
    print(json.dumps(results[-1]), flush=True)
    g.close()
    del xp, xi, xv, yp, yi
    torch.cuda.empty_cache()
    if not a.no_c5:
        from tools.c5_powerlaw import zipf_bipartite_spec
        gen = torch.Generator(device="cuda"); gen.manual_seed(20250222 + 5)
        xp, xi = rand_sym_csr(n, 0.01, gen)
        yp, yi = zipf_bipartite_spec(n, n, 1000, 1.2, gen)
        xv = (0.5 + 0.5 * torch.rand(xi.numel(), device="cuda", generator=gen)).float()
        g = ss.DeviceGraph.from_device_csr(0, n, n, n, None, (xp, xi, xv), (yp, yi, None), dtype=np.float32)
        deg = (yp[1:] - yp[:-1]).cpu().numpy()
        # the 2048-fold window holding the most rows over the LDS path's 2048 positives
        c = np.concatenate([[0], np.cumsum(deg > 2048)])
        w = c[a.folds:] - c[:-a.folds]
        lo = int(np.argmax(w))
        results.append(measure("C5", g, yp, yi, lo, a.folds, a.reps, 0))
        print(json.dumps(results[-1]), flush=True)
        g.close()
    if a.out:
        with open(a.out, "w") as f:
            json.dump(dict(source_hash=ss._lib.source_hash(), results=results), f, indent=1)


if __name__ == "__main__":
    main()
