"""Timing of the per-row binary prediction metrics on the device on one C3 block (100k x 100k at 1 %, built on the
device as tools/c3_loo.py builds it; 2048 folds x 100k targets):

  predict_loo          one 2048-fold block into a device buffer
  binary_rows_f32      ss_binary_metrics_rows_f32 on that block (labels = the graph's Ys rows)
  binary_rows_f64      ss_binary_metrics_rows_f64 on the same scores widened to fp64
  evaluate_loo_binary  ss_evaluate_loo_binary_f32 over the same folds (block_rows = 0: one block)

Warm, median of REPS, host clock around work that ends in a device synchronise.  Bytes: the long path reads the block
and writes (score, label) pairs once (stage), the radix sort reads and writes the pairs once per digit pass
(ceil(bits / 8) passes assumed: 4 fp32, 8 fp64), and the finish reads the sorted pairs twice.  The HBM floor of those
bytes is taken at 6.3 TB/s, the HBM rate a float4 copy reaches on an MI355X.

    python tools/binary_rows_time.py [--folds 2048] [--reps 5] [--out profiles/binary_rows_time.json]
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


def sort_bytes(folds, n, score_bytes):
    """Bytes the long path moves per block: stage (read scores, write pairs), radix passes (read + write pairs each),
    finish (read the sorted pairs twice)."""
    pair = score_bytes + 1
    passes = score_bytes  # 8-bit digits
    elems = folds * n
    return dict(stage=elems * (score_bytes + pair + 1), sort=elems * 2 * pair * passes, finish=elems * 2 * pair)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--folds", type=int, default=2048)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    import simspread_jl_amd as ss
    from tools.c3_loo import rand_csr, rand_sym_csr
    ss.init(0)
    ss.use_torch_stream()
    n, folds, lo = 100_000, a.folds, 0
    gen = torch.Generator(device="cuda"); gen.manual_seed(20250222 + 3)
    xp, xi = rand_sym_csr(n, 0.01, gen)
    yp, yi = rand_csr(n, n, 0.01, gen)
    xv = (0.5 + 0.5 * torch.rand(xi.numel(), device="cuda", generator=gen)).float()
    g = ss.DeviceGraph.from_device_csr(0, n, n, n, None, (xp, xi, xv), (yp, yi, None), dtype=np.float32)
    out = torch.empty((folds, n), dtype=torch.float32, device="cuda")
    ptr = yp[lo:lo + folds + 1].contiguous()
    res = dict(config="C3", folds=folds, ncols=n, first_fold=lo, nnz_labels=int((ptr[-1] - ptr[0]).item()))
    res["predict_loo_ms"] = _median_ms(lambda: g.predict_loo(lo, lo + folds, clean=True, out=out), a.reps)
    res["binary_rows_f32_ms"] = _median_ms(lambda: ss.binary_metrics_rows((ptr, yi), out), a.reps)
    res["binary_rows_f32_path"] = ss.path_last()
    distinct = [int(torch.unique(out[i]).numel()) for i in range(0, folds, max(1, folds // 16))]
    res["distinct_scores_per_row_sampled"] = float(np.mean(distinct))
    out64 = out.double()
    res["binary_rows_f64_ms"] = _median_ms(lambda: ss.binary_metrics_rows((ptr, yi), out64), a.reps)
    del out64
    torch.cuda.empty_cache()
    res["evaluate_loo_binary_ms"] = _median_ms(lambda: g.evaluate_loo_binary(lo, lo + folds, clean=True), a.reps)
    res["evaluate_loo_binary_over_predict_loo"] = res["evaluate_loo_binary_ms"] / res["predict_loo_ms"]
    for tag, b in (("f32", 4), ("f64", 8)):
        by = sort_bytes(folds, n, b)
        tot = sum(by.values())
        res[f"bytes_{tag}"] = by
        res[f"hbm_floor_{tag}_ms"] = tot / HBM * 1e3
        res[f"hbm_share_{tag}"] = res[f"hbm_floor_{tag}_ms"] / res[f"binary_rows_{tag}_ms"]
    print(json.dumps(res), flush=True)
    g.close()
    if a.out:
        with open(a.out, "w") as f:
            json.dump(dict(source_hash=ss._lib.source_hash(), results=[res]), f, indent=1)


if __name__ == "__main__":
    main()
