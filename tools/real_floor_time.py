"""Timing of the neighbour floor of the real-valued producers (include/simspread_hip_neighbours_real.h) against the plain
producers, which are the yardstick: their code is what the floor leaves unchanged, and both are measured in one process
on the same input.

Shapes: clustered n x 64 rows (n / 100 clusters, seed 2026), n = 20k and 50k, symmetric, k = 10, fp32, weighted; the
weighted-Jaccard producer on the non-negative rows, the inner-product producer (cosine) on the same rows centred.  By
pair work the symmetric floor case is three full-grid passes (selection, count, fill) against the plain producer's two
triangle passes, about three times the tiles.

  kth     ss_similarity_{jaccard,dot}_kth_f32                              the selection pass (full grid + lists)
  count   the size query of ss_similarity_*_floor_csr_f32 - kth            the count pass (full grid)
  fill    the full call - the size query                                   the fill pass (full grid, non-empty tiles)
  plain   the same two calls with k = 0: the plain producer                count and fill over the triangle

Warm, median of REPS calls, host clock around work that ends in a device synchronise; device inputs and outputs.

    python tools/real_floor_time.py [--n 20000 50000] [--k 10] [--reps 3] [--out profiles/real_floor_time.json]"""
import argparse
import ctypes as C
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

D = 64


def clustered(n, d, seed, noise=0.08):
    rng = np.random.default_rng(seed)
    clusters = max(1, n // 100)
    proto = rng.random((clusters, d)).astype(np.float32)
    X = proto[rng.integers(0, clusters, n)] * np.exp(rng.normal(0, noise, (n, d))).astype(np.float32)
    return np.ascontiguousarray(X, dtype=np.float32)


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


def measure(producer, X, k, alpha, reps):
    import torch
    import simspread_jl_amd as ss
    from simspread_jl_amd import _lib
    from simspread_jl_amd.engine import SIM_METRICS
    lib = _lib.lib()
    n, d = X.shape
    Xt = torch.from_numpy(X).cuda()
    Ft = Xt.t().contiguous()                       # column-major n x d, as the library reads it
    mid = () if producer == "jaccard" else (SIM_METRICS["cosine"],)
    csr = getattr(lib, f"ss_similarity_{producer}_floor_csr_f32")
    DEV = _lib.SS_MEM_DEVICE
    ptr = torch.empty(n + 1, dtype=torch.int64, device="cuda")
    nnz = C.c_int64(0)

    def call(kk, idx, val, cap):
        _lib.check(csr(Ft.data_ptr(), n, n, None, n, n, d, *mid, C.c_float(alpha), kk, 1, ptr.data_ptr(), idx, val, cap,
                       C.byref(nnz), DEV))

    def kth():
        return ss.jaccard_kth(Xt, k=k) if producer == "jaccard" else ss.dot_kth(Xt, metric="cosine", k=k)

    call(k, None, None, 0)
    nnz_floor = nnz.value
    call(0, None, None, 0)
    nnz_plain = nnz.value
    cap = max(nnz_floor, nnz_plain, 1)
    idx = torch.empty(cap, dtype=torch.int32, device="cuda")
    val = torch.empty(cap, dtype=torch.float32, device="cuda")
    t = {"kth": timed(kth, reps),
         "floor_size_query": timed(lambda: call(k, None, None, 0), reps),
         "floor_full": timed(lambda: call(k, idx.data_ptr(), val.data_ptr(), cap), reps),
         "plain_size_query": timed(lambda: call(0, None, None, 0), reps),
         "plain_full": timed(lambda: call(0, idx.data_ptr(), val.data_ptr(), cap), reps)}
    tau = kth()
    ms = {name: v[0] for name, v in t.items()}
    floor_count, floor_fill = ms["floor_size_query"] - ms["kth"], ms["floor_full"] - ms["floor_size_query"]
    plain_count, plain_fill = ms["plain_size_query"], ms["plain_full"] - ms["plain_size_query"]
    return {
        "producer": producer if producer == "jaccard" else "dot (cosine)", "n": n, "d": d, "k": k, "alpha": alpha,
        "nnz_floor": nnz_floor, "nnz_plain": nnz_plain,
        "tau_min": float(tau.min()), "tau_max": float(tau.max()),
        "ms": {"kth": ms["kth"], "floor_count": floor_count, "floor_fill": floor_fill, "floor_producer": ms["floor_full"],
               "plain_count": plain_count, "plain_fill": plain_fill, "plain_producer": ms["plain_full"]},
        "ratio": {"kth_over_plain_count": ms["kth"] / plain_count, "count": floor_count / plain_count,
                  "fill": floor_fill / plain_fill, "producer": ms["floor_full"] / ms["plain_full"]},
        "all_ms": {name: v[1] for name, v in t.items()},
    }


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, nargs="+", default=[20_000, 50_000])
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--alpha", type=float, default=0.8)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default="profiles/real_floor_time.json")
    args = ap.parse_args()

    import torch
    import simspread_jl_amd as ss
    from simspread_jl_amd import _lib
    torch.cuda.init()                              # torch's runtime first, then the library joins its device
    ss.init(0)
    ss.use_torch_stream()
    runs = []
    for n in args.n:
        X = clustered(n, D, seed=2026)
        runs.append(measure("jaccard", X, args.k, args.alpha, args.reps))
        runs.append(measure("dot", X - np.float32(0.5), args.k, args.alpha, args.reps))
    rec = {
        "what": "neighbour floor of the real-valued producers against the plain producers (k = 0) on the same input, in "
                f"one process: clustered n x {D} rows, symmetric, k = {args.k}, alpha = {args.alpha}, fp32, weighted, "
                "device in and out",
        "reps": args.reps, "source_hash": _lib.source_hash(), "runs": runs,
    }
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(rec, f, indent=1)
    print(json.dumps(rec))


if __name__ == "__main__":
    main()
