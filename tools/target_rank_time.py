"""Times the four steps of a per-target evaluation (ss_target_rank_*: collect, seal, count, metrics) on one block of the
C3 shape: 2048 rows x 100k targets, fp32, 1 % labels, scores zero except for 1 % of the entries -- the sparse regime of
a leave-one-out block.  Scores and labels are made on the device; nothing but the result table leaves it.

    python tools/target_rank_time.py [out.json]      # needs an MI355X; default out: profiles/target_rank_time.json
"""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import simspread_jl_amd as ss  # noqa: E402


def main(out_path, nrows=2048, nt=100_000, reps=5):
    import torch
    ss.init(0)
    ss.use_torch_stream()
    gen = torch.Generator(device="cuda").manual_seed(1)
    S = torch.rand((nrows, nt), generator=gen, device="cuda")
    S = torch.where(torch.rand((nrows, nt), generator=gen, device="cuda") < 0.01, S, torch.zeros_like(S)).contiguous()
    Ymask = torch.rand((nrows, nt), generator=gen, device="cuda") < 0.01
    ptr = torch.cat([torch.zeros(1, dtype=torch.int64, device="cuda"), Ymask.sum(1).cumsum(0)]).contiguous()
    idx = Ymask.nonzero()[:, 1].to(torch.int32).contiguous()
    rows_of = Ymask.nonzero()[:, 0]
    del Ymask
    # the labels of the transposed block (nt x nrows), for the alternative below
    o = torch.sort(idx.to(torch.int64), stable=True).indices
    idxT = rows_of[o].to(torch.int32).contiguous()
    ptrT = torch.cat([torch.zeros(1, dtype=torch.int64, device="cuda"),
                      torch.bincount(idx.to(torch.int64), minlength=nt).cumsum(0)]).contiguous()

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3

    rows = []
    for _ in range(reps + 1):                            # the first repetition warms up
        h = ss.TargetRank(nt, np.float32)
        r = dict(collect_ms=timed(lambda: h.add_rows((ptr, idx), S)), seal_ms=timed(h.seal),
                 count_ms=timed(lambda: h.add_rows((ptr, idx), S)))
        r["count_kernel_ms"] = ss.timing_last()["epilogue_ms"]
        r["paths"] = ss.path_last()
        r["metrics_ms"] = timed(lambda: h.metrics(20.0, 20))
        if len(rows) == reps:                            # what the counts say about the work: searched negatives
            st, _, _, _ = h.export_positives()
            c, _ = h.export_counts()
            P = np.bincount(st, minlength=nt).astype(np.int64)
            off = np.cumsum(P) - P
            below = int(c[3 * (off + np.arange(nt)) + P].sum())
            neg = nrows * nt - int(P.sum())
            searched = dict(negatives=neg, below_every_positive=below, searched=neg - below,
                            searched_fraction=(neg - below) / neg)
        h.close()
        # the alternative without the handle: the block transposed on the device, then the per-row metrics on it
        keep = {}
        r["alt_transpose_ms"] = timed(lambda: keep.__setitem__("ST", S.t().contiguous()))
        r["alt_rank_rows_ms"] = timed(lambda: ss.rank_metrics_rows((ptrT, idxT), keep["ST"], alpha=20.0, L=20))
        del keep
        rows.append(r)
    rows = rows[1:]
    med = {k: float(np.median([r[k] for r in rows])) for k in rows[0] if k.endswith("_ms")}
    block_bytes = nrows * nt * 4
    res = dict(shape=dict(nrows=nrows, nt=nt, dtype="f32", label_density=0.01, nonzero_scores=0.01,
                          positives=int(idx.numel())),
               median_ms=med, paths=rows[0]["paths"], reps=reps, block_bytes=block_bytes, searched=searched,
               alternative="alt_*: transpose of the block on the device + ss.rank_metrics_rows on the nt x nrows result; "
                           "it holds a second copy of the block and so only serves row ranges whose transpose fits",
               count_GBps=block_bytes / med["count_kernel_ms"] / 1e6,
               note="wall times include staging checks and host synchronisation; count_kernel_ms is the device span "
                    "of the label check and the count kernel (ss_timing_last ms[3])",
               source_hash=ss._lib.source_hash())
    os.makedirs(os.path.dirname(out_path), exist_ok=True)
    with open(out_path, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "target_rank_time.json"))
