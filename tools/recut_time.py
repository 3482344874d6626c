"""Timing of a cutoff sweep: re-thresholding a resident graph against building it again at every cutoff.

  * fingerprint route, N x 2048 bits (default 50k), fp32: one weighted parent at the lowest cutoff of the grid; per
    cutoff the time of DeviceGraph.recut next to the time of DeviceGraph.from_fingerprints at the same cutoff, in the same
    run, and the recut's algorithmic bytes (two passes over Xs, XsT, Xq plus the output) over the achievable HBM rate;
  * dense-similarity route, M x M (default 20k), fp32: DeviceGraph.set_cutoff against DeviceGraph.from_similarity from
    device-resident similarities.

Warm, median of REPS calls, host clock around work that ends in a device synchronise.

    python tools/recut_time.py [--n 50000] [--dense-n 20000] [--reps 5] [--grid 0.3,0.4,...] [--out profiles/recut_time.json]
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


def spread_clusters(n, d, clusters, seed, density=0.1):
    """Cluster prototypes with a per-row flip rate in [0.005, 0.06]: similarities inside a cluster spread over roughly
    0.4 .. 0.9, so every cutoff of the grid keeps a different share of the parent's edges."""
    import simspread_jl_amd as ss
    rng = np.random.default_rng(seed)
    proto = rng.random((clusters, d)) < density
    member = rng.integers(0, clusters, n)
    flip = rng.uniform(0.005, 0.06, n).astype(np.float32)
    F = np.empty((n, d // 64), np.uint64)
    for r in range(0, n, 8192):
        m = member[r:r + 8192]
        F[r:r + 8192] = ss.pack_fingerprints(proto[m] ^ (rng.random((len(m), d), dtype=np.float32) < flip[r:r + 8192, None]))
    return F


def timed(fn, reps):
    import torch
    r = fn()
    torch.cuda.synchronize()
    if hasattr(r, "close"):
        r.close()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        r = fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
        if hasattr(r, "close"):
            r.close()
    return float(np.median(ts)), [round(t, 3) for t in ts]


def recut_bytes(blocks, elem=4):
    """Algorithmic bytes of one recut: per block (rows, nnz_in, nnz_out) the count pass reads the values and the row
    pointers, the fill pass the values, the indices and both pointer arrays, and writes indices and values."""
    total = 0
    for rows, nin, nout in blocks:
        total += nin * elem + (rows + 1) * 4 + rows * 4                  # count: val, ptr; counts written
        total += nin * (elem + 4) + (rows + 1) * (4 + 8) + nout * (elem + 4)   # fill: val, idx, ptr, optr; idx, val written
    return total


def fingerprint_sweep(args):
    import torch
    import simspread_jl_amd as ss
    n = args.n
    F = spread_clusters(n, D, clusters=max(1, n // 1000), seed=2026)
    Ft = torch.from_numpy(F.view(np.int64)).cuda()
    Y = (torch.zeros(n + 1, dtype=torch.int64, device="cuda"), torch.zeros(1, dtype=torch.int32, device="cuda"), None, 16)
    a0 = args.grid[0]
    parent = ss.DeviceGraph.from_fingerprints(None, Ft, Y, alpha=a0, weighted=True)
    rec = {"n": n, "bits": D, "parent_alpha": a0, "parent_nnz_xs": parent.nnz_xs, "parent_fill": parent.nnz_xs / n / n,
           "grid": []}
    for alpha in args.grid:
        child = parent.recut(alpha, True)
        nout = child.nnz_xs
        child.close()
        recut_ms, recut_all = timed(lambda: parent.recut(alpha, True), args.reps)
        fresh_ms, fresh_all = timed(lambda: ss.DeviceGraph.from_fingerprints(None, Ft, Y, alpha=alpha, weighted=True),
                                    args.reps)
        nbytes = recut_bytes([(n, parent.nnz_xs, nout), (n, parent.nnz_xs, nout), (0, 0, 0)])
        r = {"alpha": alpha, "nnz_xs": nout, "recut_ms": recut_ms, "recut_all_ms": recut_all, "create_ms": fresh_ms,
             "create_all_ms": fresh_all, "speedup": fresh_ms / recut_ms, "recut_bytes": nbytes,
             "recut_hbm_floor_ms": nbytes / HBM_RATE * 1e3}
        rec["grid"].append(r)
        print(json.dumps(r), flush=True)
    parent.close()
    return rec


def dense_sweep(args):
    import torch
    import simspread_jl_amd as ss
    m = args.dense_n
    g = torch.Generator(device="cuda").manual_seed(7)
    U = torch.rand((m, m), device="cuda", generator=g)
    S = (U + U.t()) / 2
    S.fill_diagonal_(1.0)
    del U
    Y = (torch.zeros(m + 1, dtype=torch.int64, device="cuda"), torch.zeros(1, dtype=torch.int32, device="cuda"), None, 16)
    graph = ss.DeviceGraph.from_similarity(None, S, Y, alpha=args.grid[0], weighted=True)
    rec = {"n": m, "grid": []}
    for alpha in args.grid:
        set_ms, set_all = timed(lambda: graph.set_cutoff(alpha, True) and None, args.reps)
        fresh_ms, fresh_all = timed(lambda: ss.DeviceGraph.from_similarity(None, S, Y, alpha=alpha, weighted=True),
                                    args.reps)
        r = {"alpha": alpha, "set_cutoff_ms": set_ms, "set_cutoff_all_ms": set_all, "create_ms": fresh_ms,
             "create_all_ms": fresh_all, "speedup": fresh_ms / set_ms,
             "degree_pass_bytes": 2 * m * m * 4, "degree_pass_hbm_floor_ms": 2 * m * m * 4 / HBM_RATE * 1e3}
        rec["grid"].append(r)
        print(json.dumps(r), flush=True)
    graph.close()
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=50_000)
    ap.add_argument("--dense-n", type=int, default=20_000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--grid", default="0.3,0.4,0.5,0.6,0.7,0.8,0.9")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    args.grid = [float(a) for a in args.grid.split(",") if a]
    import torch  # before the library, as in the other timing tools: one HIP runtime for both
    import simspread_jl_amd as ss
    if not torch.cuda.is_available():
        raise SystemExit("recut_time: no GPU")
    ss.init(0)
    ss.use_torch_stream()
    rec = {"what": "cutoff sweep: recut / set_cutoff of a resident graph against re-creating it, fp32, weighted",
           "reps": args.reps, "hbm_rate_bytes_per_s": HBM_RATE, "source_hash": ss._lib.source_hash()}
    if args.n > 0:
        rec["fingerprint"] = fingerprint_sweep(args)
    if args.dense_n > 0:
        rec["dense_similarity"] = dense_sweep(args)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(rec, f, indent=1)
    print(json.dumps(rec)[:4000])


if __name__ == "__main__":
    main()
