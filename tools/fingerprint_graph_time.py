"""Timing of the fingerprint route: packed binary fingerprints -> thresholded Tanimoto CSR (ss_similarity_tanimoto_csr)
and -> graph (ss_graph_create_fingerprint), symmetric, 2048 bits, against the dense route it replaces (jaccard on the
unpacked rows, then the dense graph create with the cutoff) at 50k.  Warm, median of REPS calls, host clock around
work that ends in a device synchronise.

    python tools/fingerprint_graph_time.py [--sizes 50000,100000] [--reps 5] [--no-dense] [--out profiles/x.json]
    python tools/fingerprint_graph_time.py --kernels <rocprofv3 kernel_stats.csv> [--n 100000] [--out ...]

The second form reads a `rocprofv3 --kernel-trace --stats` run of the first and sets each kernel's time against its
VALU floor (v_and_b32 + v_bcnt_u32_b32 per 32-bit word and pair at 7.86e13 lane-ops/s)."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

VALU_RATE = 7.86e13   # lane-ops/s, MI355X_MICROARCH.md
D = 2048


def valu_floor_ms(n, d=D, sym=True):
    pairs = n * (n + 1) / 2 if sym else n * n
    return pairs * (d // 32) * 2 / VALU_RATE * 1e3


def clustered(n, d, clusters, seed, density=0.1, flip=0.015):
    import simspread_jl_amd as ss
    rng = np.random.default_rng(seed)
    proto = rng.random((clusters, d)) < density
    member = rng.integers(0, clusters, n)
    F = np.empty((n, d // 64), np.uint64)
    for r in range(0, n, 8192):
        m = member[r:r + 8192]
        F[r:r + 8192] = ss.pack_fingerprints(proto[m] ^ (rng.random((len(m), d), dtype=np.float32) < flip))
    return F


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
    rec = {"what": "fingerprint route, symmetric, 2048 bits, alpha 0.5, fp32, weighted", "reps": args.reps,
           "valu_rate_lane_ops_per_s": VALU_RATE, "source_hash": ss._lib.source_hash(), "sizes": {}}
    for n in args.sizes:
        F = clustered(n, D, clusters=max(1, n // 1000), seed=2026)
        Ft = torch.from_numpy(F.view(np.int64)).cuda()
        Y = (torch.zeros(n + 1, dtype=torch.int64, device="cuda"), torch.zeros(1, dtype=torch.int32, device="cuda"),
             None, 16)
        prod_ms, prod_all = timed(lambda: ss.tanimoto_csr(Ft, alpha=0.5, weighted=True), args.reps)
        nnz = int(ss.tanimoto_csr(Ft, alpha=0.5, weighted=True)[1].numel())
        graph_ms, graph_all = timed(lambda: ss.DeviceGraph.from_fingerprints(None, Ft, Y, alpha=0.5), args.reps)
        r = {"n": n, "nnz": nnz, "fill": nnz / n / n, "producer_ms": prod_ms, "producer_all_ms": prod_all,
             "graph_create_ms": graph_ms, "graph_create_all_ms": graph_all,
             "valu_floor_one_pass_ms": valu_floor_ms(n), "valu_floor_two_passes_ms": 2 * valu_floor_ms(n)}
        if args.dense and n <= 50_000:
            bits = torch.from_numpy(np.unpackbits(F.view(np.uint8), axis=1, bitorder="little").astype(np.float32)).cuda()

            def dense():
                S = ss.jaccard_similarity(bits)
                g = ss.DeviceGraph.from_dense(None, S, torch.zeros((n, 16), device="cuda"), alpha=0.5)
                del S
                return g
            dense_ms, dense_all = timed(dense, max(2, args.reps // 2))
            r.update(dense_route_ms=dense_ms, dense_route_all_ms=dense_all, speedup_vs_dense=dense_ms / graph_ms)
            del bits
        rec["sizes"][str(n)] = r
        print(json.dumps(r), flush=True)
        del Ft
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
        if "tanimoto_tile_kernel" in name:
            e["valu_floor_ms_at_n"] = {"n": args.n, "ms": valu_floor_ms(args.n)}
        out.append(e)
    out.sort(key=lambda e: -e["total_ms"])
    return {"kernel_stats": os.path.basename(args.kernels), "n": args.n,
            "how": "rocprofv3 --kernel-trace --stats over tools/fingerprint_graph_time.py --sizes N --reps 2 --no-dense",
            "source_hash": _source_hash(), "kernels": out}


def _source_hash():
    from simspread_jl_amd import _lib
    return _lib.source_hash()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="50000,100000")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--no-dense", dest="dense", action="store_false")
    ap.add_argument("--kernels", default=None)
    ap.add_argument("--n", type=int, default=100_000)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    args.sizes = [int(s) for s in args.sizes.split(",") if s]
    rec = kernels(args) if args.kernels else run(args)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(rec, f, indent=1)
    print(json.dumps(rec)[:4000])


if __name__ == "__main__":
    main()
