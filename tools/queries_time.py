"""Timing of prospective screening: a query batch bound to a resident graph against building the graph again around it,
and the support lists of its hits.

  * batch: ns x 2048-bit fingerprints (default 20 000), nt targets (2 000), a batch of nq queries (4 096), fp32, device
    inputs.  (a) the only route without query sets: DeviceGraph.from_fingerprints with the batch as its queries, then
    predict; (b) DeviceQueries.from_fingerprints on the resident graph, then predict(queries=...).  (b) does a strict
    subset of (a)'s work.  The scores of both are compared bitwise.
  * support: ss_support_f32 for 4 096 (row, target) pairs of that batch, M = 16, at targets held by 10, 1 000 and all ns
    sources: microseconds per pair of the whole call and of the support kernel alone (ss_timing_last), next to the byte
    model of DESIGN.md -- kt * (4 + 4 + 4) bytes per pair, 4 less per entry for pattern-only labels -- at the
    achievable HBM rate.

Median of REPS runs after one warm-up, host clock around work that ends in a device synchronise.

    python tools/queries_time.py [--ns 20000] [--nq 4096] [--nt 2000] [--reps 5] [--out profiles/query_sets_time.json]
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

HBM_RATE = 6.3e12   # bytes/s achievable on the MI355X (float4 copy: 6.29 TB/s of the 8 TB/s peak)
D = 2048
NPAIRS = 4096
M = 16


def clustered_fingerprints(n, clusters, seed, proto_seed=2026, density=0.1):
    """members of `clusters` prototypes with a per-row flip rate in [0.005, 0.06]: similarities inside a cluster spread
    over roughly 0.4 .. 0.9"""
    import simspread_jl_amd as ss
    proto = np.random.default_rng(proto_seed).random((clusters, D)) < density
    rng = np.random.default_rng(seed)
    member = rng.integers(0, clusters, n)
    flip = rng.uniform(0.005, 0.06, n).astype(np.float32)
    F = np.empty((n, D // 64), np.uint64)
    for r in range(0, n, 8192):
        m = member[r:r + 8192]
        F[r:r + 8192] = ss.pack_fingerprints(proto[m] ^ (rng.random((len(m), D), dtype=np.float32) < flip[r:r + 8192, None]))
    return F


def labels(ns, nt, seed):
    """target 0 held by every source, target 1 by 1 000 (or ns / 2), every other target by 10; pattern-only"""
    import scipy.sparse as sp
    rng = np.random.default_rng(seed)
    k1 = min(1000, ns // 2)
    rows = [np.arange(ns), rng.choice(ns, k1, replace=False)] + [rng.choice(ns, 10, replace=False) for _ in range(nt - 2)]
    cols = [np.full(len(r), t) for t, r in enumerate(rows)]
    Y = sp.csr_matrix((np.ones(sum(len(r) for r in rows), np.float32), (np.concatenate(rows), np.concatenate(cols))),
                      shape=(ns, nt))
    Y.sort_indices()
    return Y, k1


def timed(fn, reps):
    import torch
    fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(ts)), [round(t, 3) for t in ts]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ns", type=int, default=20_000)
    ap.add_argument("--nq", type=int, default=4096)
    ap.add_argument("--nt", type=int, default=2000)
    ap.add_argument("--alpha", type=float, default=0.5)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch  # before the library, as in the other timing tools: one HIP runtime for both
    import simspread_jl_amd as ss
    if not torch.cuda.is_available():
        raise SystemExit("queries_time: no GPU")
    ss.init(0)
    ss.use_torch_stream()
    ns, nq, nt, alpha = args.ns, args.nq, args.nt, args.alpha
    clusters = max(1, ns // 1000)
    Fs = torch.from_numpy(clustered_fingerprints(ns, clusters, 1).view(np.int64)).cuda()
    Fq = torch.from_numpy(clustered_fingerprints(nq, clusters, 2).view(np.int64)).cuda()
    Yh, k1 = labels(ns, nt, 3)
    Y = (torch.from_numpy(Yh.indptr.astype(np.int64)).cuda(), torch.from_numpy(Yh.indices.astype(np.int32)).cuda(), None,
         nt)
    out_a = torch.empty((nq, nt), dtype=torch.float32, device="cuda")
    out_b = torch.empty((nq, nt), dtype=torch.float32, device="cuda")

    def rebuild():
        g = ss.DeviceGraph.from_fingerprints(Fq, Fs, Y, alpha=alpha, weighted=True)
        g.predict("query", out=out_a)
        torch.cuda.synchronize()
        g.close()

    resident = ss.DeviceGraph.from_fingerprints(None, Fs, Y, alpha=alpha, weighted=True)

    def bind():
        q = ss.DeviceQueries.from_fingerprints(resident, Fq, Fs, alpha, weighted=True)
        resident.predict(out=out_b, queries=q)
        torch.cuda.synchronize()
        q.close()

    a_ms, a_all = timed(rebuild, args.reps)
    b_ms, b_all = timed(bind, args.reps)
    same = bool(torch.equal(out_a.view(torch.int32), out_b.view(torch.int32)))
    q = ss.DeviceQueries.from_fingerprints(resident, Fq, Fs, alpha, weighted=True)
    rec = {"what": "query batch on a resident graph against re-creating the graph around it; support lists; fp32",
           "ns": ns, "nq": nq, "nt": nt, "bits": D, "alpha": alpha, "reps": args.reps, "nnz_xs": resident.nnz_xs,
           "nnz_xq": q.nnz, "queries_without_neighbours": int((q.degrees() == 0).sum()),
           "hbm_rate_bytes_per_s": HBM_RATE, "source_hash": ss._lib.source_hash(),
           "batch": {"create_graph_and_predict_ms": a_ms, "create_graph_and_predict_all_ms": a_all,
                     "create_queries_and_predict_ms": b_ms, "create_queries_and_predict_all_ms": b_all,
                     "ratio_b_over_a": b_ms / a_ms, "scores_bitwise_equal": same},
           "support": []}
    print(json.dumps(rec["batch"]), flush=True)
    rng = np.random.default_rng(4)
    rows = torch.from_numpy(rng.integers(0, nq, NPAIRS).astype(np.int64)).cuda()
    for kt, tg in ((10, rng.integers(2, nt, NPAIRS)), (k1, np.full(NPAIRS, 1)), (ns, np.full(NPAIRS, 0))):
        targets = torch.from_numpy(tg.astype(np.int32)).cuda()
        kernel_ms, stage1_ms = [], []

        def run():
            resident.support(rows, targets, M=M, queries=q)
            t = ss.timing_last()
            kernel_ms.append(t["epilogue_ms"])
            stage1_ms.append(t["transfer_ms"])

        call_ms, call_all = timed(run, args.reps)
        kms = float(np.median(kernel_ms[1:]))
        nbytes = kt * (4 + 4) + M * 8 + 4          # pattern-only labels: index + gathered T entry per stored label
        r = {"kt": int(kt), "pairs": NPAIRS, "M": M, "call_ms": call_ms, "call_all_ms": call_all,
             "stage1_ms": float(np.median(stage1_ms[1:])), "kernel_ms": kms, "call_us_per_pair": call_ms * 1e3 / NPAIRS,
             "kernel_us_per_pair": kms * 1e3 / NPAIRS, "bytes_per_pair": nbytes,
             "hbm_floor_us_per_pair": nbytes / HBM_RATE * 1e6}
        rec["support"].append(r)
        print(json.dumps(r), flush=True)
    q.close()
    resident.close()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(rec, f, indent=1)
    print(json.dumps(rec)[:4000])


if __name__ == "__main__":
    main()
