"""Timing of the neighbour floor (include/simspread_hip_neighbours.h) against the plain fingerprint producer, which is
the yardstick: its code is what the floor leaves unchanged, and both are measured in one process.

One shape: the clustered 100k x 2048-bit set of tests/test_gpu_fingerprint.py (100 clusters, seed 2026), symmetric,
k = 16, fp32, weighted.  On this set every fingerprint has about a thousand neighbours above alpha = 0.5, so the floor
keeps what the plain cut keeps and the two runs produce the same nnz: what differs is the work, not the output.

  kth     ss_similarity_tanimoto_kth_f32                                  the selection pass (full grid + lists)
  count   the size query of ss_similarity_tanimoto_floor_csr_f32 - kth    the count pass (full grid)
  fill    the full call - the size query                                  the fill pass (full grid)
  plain   the same two calls of ss_similarity_tanimoto_csr_f32            count and fill over the triangle
  graph   DeviceGraph.from_fingerprints with and without min_neighbours   the whole constructor

Warm, median of REPS calls, host clock around work that ends in a device synchronise; device inputs and outputs.

    python tools/neighbour_floor_time.py [--n 100000] [--k 16] [--reps 3] [--out profiles/neighbour_floor_time.json]"""
import argparse
import ctypes as C
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

D = 2048


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=100_000)
    ap.add_argument("--k", type=int, default=16)
    ap.add_argument("--alpha", type=float, default=0.5)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default="profiles/neighbour_floor_time.json")
    args = ap.parse_args()

    import torch
    import simspread_jl_amd as ss
    from simspread_jl_amd import _lib
    ss.init(0)
    ss.use_torch_stream()
    lib = _lib.lib()
    n, k, alpha = args.n, args.k, args.alpha
    F = clustered(n, D, clusters=100, seed=2026)
    Ft = torch.from_numpy(F.view(np.int64)).cuda()
    nw = Ft.shape[1]
    DEV = _lib.SS_MEM_DEVICE
    ptr = torch.empty(n + 1, dtype=torch.int64, device="cuda")
    nnz = C.c_int64(0)

    def floor_call(idx, val, cap):
        _lib.check(lib.ss_similarity_tanimoto_floor_csr_f32(Ft.data_ptr(), n, None, n, nw, C.c_float(alpha), k, 1,
                                                            ptr.data_ptr(), idx, val, cap, C.byref(nnz), DEV))

    def plain_call(idx, val, cap):
        _lib.check(lib.ss_similarity_tanimoto_csr_f32(Ft.data_ptr(), n, None, n, nw, C.c_float(alpha), 1, ptr.data_ptr(),
                                                      idx, val, cap, C.byref(nnz), DEV))

    floor_call(None, None, 0)
    nnz_floor = nnz.value
    plain_call(None, None, 0)
    nnz_plain = nnz.value
    cap = max(nnz_floor, nnz_plain, 1)
    idx = torch.empty(cap, dtype=torch.int32, device="cuda")
    val = torch.empty(cap, dtype=torch.float32, device="cuda")
    Y = (torch.zeros(n + 1, dtype=torch.int64, device="cuda"), torch.zeros(1, dtype=torch.int32, device="cuda"), None, 16)

    t = {}
    t["kth"] = timed(lambda: ss.tanimoto_kth(Ft, k=k), args.reps)
    t["floor_size_query"] = timed(lambda: floor_call(None, None, 0), args.reps)
    t["floor_full"] = timed(lambda: floor_call(idx.data_ptr(), val.data_ptr(), cap), args.reps)
    t["plain_size_query"] = timed(lambda: plain_call(None, None, 0), args.reps)
    t["plain_full"] = timed(lambda: plain_call(idx.data_ptr(), val.data_ptr(), cap), args.reps)
    t["floor_graph"] = timed(lambda: ss.DeviceGraph.from_fingerprints(None, Ft, Y, alpha=alpha, min_neighbours=k),
                             args.reps)
    t["plain_graph"] = timed(lambda: ss.DeviceGraph.from_fingerprints(None, Ft, Y, alpha=alpha), args.reps)
    tau = ss.tanimoto_kth(Ft, k=k)
    ms = {name: v[0] for name, v in t.items()}
    floor_count, floor_fill = ms["floor_size_query"] - ms["kth"], ms["floor_full"] - ms["floor_size_query"]
    plain_count, plain_fill = ms["plain_size_query"], ms["plain_full"] - ms["plain_size_query"]
    rec = {
        "what": f"neighbour floor against the plain fingerprint producer (the yardstick): clustered {n} x {D} bits, "
                f"symmetric, k = {k}, alpha = {alpha}, fp32, weighted, device in and out",
        "reps": args.reps, "source_hash": _lib.source_hash(), "n": n, "k": k, "alpha": alpha,
        "nnz_floor": nnz_floor, "nnz_plain": nnz_plain, "nnz_ratio": nnz_floor / max(nnz_plain, 1),
        "tau_min": float(tau.min()), "tau_max": float(tau.max()),
        "ms": {"kth": ms["kth"], "floor_count": floor_count, "floor_fill": floor_fill, "floor_producer": ms["floor_full"],
               "floor_graph_create": ms["floor_graph"], "plain_count": plain_count, "plain_fill": plain_fill,
               "plain_producer": ms["plain_full"], "plain_graph_create": ms["plain_graph"]},
        "ratio": {"kth_over_plain_count": ms["kth"] / plain_count, "count": floor_count / plain_count,
                  "fill": floor_fill / plain_fill, "producer": ms["floor_full"] / ms["plain_full"],
                  "graph_create": ms["floor_graph"] / ms["plain_graph"]},
        "all_ms": {name: v[1] for name, v in t.items()},
    }
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(rec, f, indent=1)
    print(json.dumps(rec))


if __name__ == "__main__":
    main()
