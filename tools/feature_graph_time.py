"""Timing of the real-valued feature route: feature rows -> thresholded weighted Jaccard CSR (ss_similarity_jaccard_csr)
and -> graph (ss_graph_create_features), symmetric, d = 64, fp32, against the dense route it replaces (jaccard, then the
dense graph create with the cutoff) at 50k.  Warm, median of REPS calls, host clock around work that ends in a device
synchronise.  Clustered rows come in two orders: "sorted" (members of a cluster adjacent: most tiles keep nothing and the
fill pass skips them) and "shuffled" (every tile keeps something: the fill pass recomputes every pair).

    python tools/feature_graph_time.py [--sizes 50000,100000] [--reps 5] [--no-dense] [--out profiles/x.json]
    python tools/feature_graph_time.py --kernels <rocprofv3 kernel_stats.csv> [--n 100000] [--out ...]

The second form reads a `rocprofv3 --kernel-trace --stats` run of the first and sets each tile kernel's time against
its VALU floor (min, max and two adds per feature and pair, or three lane-ops with the adds packed, at 7.86e13
lane-ops/s)."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

VALU_RATE = 7.86e13   # lane-ops/s, MI355X_MICROARCH.md
D = 64
ALPHA = 0.85


def valu_floor_ms(n, d=D, sym=True, ops=4):
    pairs = n * (n + 1) / 2 if sym else n * n
    return pairs * d * ops / VALU_RATE * 1e3


def clustered(n, d, clusters, seed, shuffled, noise=0.05):
    rng = np.random.default_rng(seed)
    proto = rng.random((clusters, d)) + 0.05
    member = rng.integers(0, clusters, n)
    if not shuffled:
        member = np.sort(member)
    X = np.empty((n, d), np.float32)
    for r in range(0, n, 16384):
        m = member[r:r + 16384]
        X[r:r + 16384] = proto[m] * np.exp(rng.normal(0, noise, (len(m), d)))
    return X


def timed(fn, reps):
    import torch
    fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        r = fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
        del r
    return float(np.median(ts)), [round(t, 3) for t in ts]


def run(args):
    import torch
    import simspread_jl_amd as ss
    ss.init(0)
    ss.use_torch_stream()
    rec = {"what": f"feature route, symmetric, d = {D}, alpha {ALPHA}, fp32, weighted, clustered (n / 1000 clusters)",
           "reps": args.reps, "valu_rate_lane_ops_per_s": VALU_RATE, "source_hash": ss._lib.source_hash(), "sizes": {}}
    for n in args.sizes:
        for order in args.orders:
            X = clustered(n, D, clusters=max(1, n // 1000), seed=2026, shuffled=(order == "shuffled"))
            Xt = torch.from_numpy(X).cuda()
            Y = (torch.zeros(n + 1, dtype=torch.int64, device="cuda"), torch.zeros(1, dtype=torch.int32, device="cuda"),
                 None, 16)
            prod_ms, prod_all = timed(lambda: ss.jaccard_csr(Xt, alpha=ALPHA, weighted=True), args.reps)
            nnz = int(ss.jaccard_csr(Xt, alpha=ALPHA, weighted=True)[1].numel())
            graph_ms, graph_all = timed(lambda: ss.DeviceGraph.from_features(None, Xt, Y, alpha=ALPHA), args.reps)
            r = {"n": n, "order": order, "nnz": nnz, "fill": nnz / n / n, "producer_ms": prod_ms,
                 "producer_all_ms": prod_all, "graph_create_ms": graph_ms, "graph_create_all_ms": graph_all,
                 "valu_floor_one_pass_ms": valu_floor_ms(n), "valu_floor_one_pass_packed_ms": valu_floor_ms(n, ops=3)}
            if args.dense and n <= 50_000 and order == "shuffled":
                def dense():
                    S = ss.jaccard_similarity(Xt)
                    g = ss.DeviceGraph.from_dense(None, S, torch.zeros((n, 16), device="cuda"), alpha=ALPHA)
                    del S
                    return g
                dense_ms, dense_all = timed(dense, max(2, args.reps // 2))
                r.update(dense_route_ms=dense_ms, dense_route_all_ms=dense_all, speedup_vs_dense=dense_ms / graph_ms)
            rec["sizes"][f"{n}_{order}"] = r
            print(json.dumps(r), flush=True)
            del Xt
            torch.cuda.empty_cache()
    return rec


def kernels(args):
    import csv
    rows = list(csv.DictReader(open(args.kernels)))
    out = []
    for row in rows:
        name = row.get("Name") or row.get("KernelName") or ""
        calls = int(row.get("Calls", 1))
        avg_ms = float(row.get("AverageNs", 0)) / 1e6
        tot_ms = float(row.get("TotalDurationNs", 0)) / 1e6
        e = {"kernel": name[:160], "calls": calls, "avg_ms": avg_ms, "total_ms": tot_ms}
        if "jaccard_tile_kernel" in name:
            e["valu_floor_ms_at_n"] = {"n": args.n, "ms": valu_floor_ms(args.n), "packed_ms": valu_floor_ms(args.n, ops=3)}
        out.append(e)
    out.sort(key=lambda e: -e["total_ms"])
    return {"kernel_stats": os.path.basename(args.kernels), "n": args.n,
            "how": "rocprofv3 --kernel-trace --stats over tools/feature_graph_time.py --sizes N --reps 2 --no-dense",
            "source_hash": _source_hash(), "kernels": out}


def _source_hash():
    from simspread_jl_amd import _lib
    return _lib.source_hash()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="50000,100000")
    ap.add_argument("--orders", default="shuffled,sorted")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--no-dense", dest="dense", action="store_false")
    ap.add_argument("--kernels", default=None)
    ap.add_argument("--n", type=int, default=100_000)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    args.sizes = [int(s) for s in args.sizes.split(",") if s]
    args.orders = [s for s in args.orders.split(",") if s]
    rec = kernels(args) if args.kernels else run(args)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(rec, f, indent=1)
    print(json.dumps(rec)[:4000])


if __name__ == "__main__":
    main()
