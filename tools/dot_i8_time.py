"""Timing of the int8 route of the inner-product producer (ss_similarity_dot_csr_i8, csrc/dot_tile_i8.hpp) against the
two routes that give the same graph from the same values: the 16-bit route on the bf16 copies (every int8 value is a
bf16 number) and the fp32 route on the widened copies, in one process.

The setting of DESIGN 4.19: n x d cosine, symmetric, weighted, clustered rows (n / 1000 clusters, shuffled) at about 1 %
fill.  The rows are quantised once (symmetric, per tensor: round(X * 127 / max|X|)); the int8 route reads them
row-major in place, the bf16 route their bf16 copies row-major, the fp32 route their fp32 copies column-major, as it
requires.  Per route: the count pass (the size query: row norms, count kernel, scans; the floating-point routes also
scan for NaN) and the fill pass (a full call minus the size query), warm, median of REPS calls with all values and their
spread (max - min), host clock around calls that end in a device synchronise.  The routes alternate inside every
repetition, so drift of the machine hits them alike.  The floor of one pass is pairs * d * 2 / peak of the route's
matrix instruction.

    python tools/dot_i8_time.py [--n 100000] [--dims 64,1024] [--reps 5] [--out profiles/dot_i8_time.json]"""
import argparse
import ctypes as C
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np

from dot_csr_time import ALPHA_COS, MFMA_F32_FLOPS, clustered
from dot_h16_time import MFMA_16BIT_FLOPS, Route, timed

MFMA_I8_OPS = 5.0e15          # v_mfma_i32_32x32x32_i8 dense peak, MI355X_MICROARCH.md: twice the 16-bit rate


def measure(routes, reps):
    import torch
    for r in routes:                      # warm every route and shape
        r.query()
        r.full()
    torch.cuda.synchronize()
    q = {r.name: [] for r in routes}
    f = {r.name: [] for r in routes}
    for _ in range(reps):
        for r in routes:                  # alternate the routes
            q[r.name].append(timed(r.query))
            f[r.name].append(timed(r.full))
    out = {}
    for r in routes:
        qa, fa = np.array(q[r.name]), np.array(f[r.name])
        qm, fm = float(np.median(qa)), float(np.median(fa))
        out[r.name] = {"nnz": r.nnz.value, "fill": r.nnz.value / r.n / r.n, "count_pass_ms": qm,
                       "count_pass_spread_ms": float(qa.max() - qa.min()),
                       "count_pass_all_ms": [round(t, 3) for t in q[r.name]], "total_ms": fm,
                       "total_spread_ms": float(fa.max() - fa.min()), "total_all_ms": [round(t, 3) for t in f[r.name]],
                       "fill_pass_ms": fm - qm, "fill_pass_spread_ms": float((fa - qa).max() - (fa - qa).min())}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=100_000)
    ap.add_argument("--dims", default="64,1024")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dims = [int(s) for s in args.dims.split(",") if s]
    import torch                       # before the library, as in the other tools: one HIP runtime for both
    torch.cuda.init()
    import simspread_jl_amd as ss
    from simspread_jl_amd import _lib
    lib = ss.init(0)
    n = args.n
    rec = {"source_hash": _lib.source_hash(),
           "what": f"n = {n}, cosine, symmetric, weighted, clustered (n / 1000 clusters, shuffled), quantised to int8 per "
                   "tensor; the int8 route, the bf16 route on the bf16 copies and the fp32 route on the widened copies, "
                   "alternating in one process",
           "reps": args.reps, "sizes": {}}
    pairs = n * (n + 1) / 2
    alpha = C.c_float(ALPHA_COS)
    for d in dims:
        X = torch.from_numpy(clustered(n, d, clusters=max(1, n // 1000), seed=2026)).cuda()
        Q = torch.round(X * (127.0 / float(X.abs().max()))).to(torch.int8).contiguous()   # the int8 rows, row-major n x d
        H = Q.to(torch.bfloat16).contiguous()                                             # exact
        W = Q.to(torch.float32).t().contiguous()                                          # exact, column-major n x d
        del X

        def i8(ptr, idx, val, cap, nnz):
            return lib.ss_similarity_dot_csr_i8(Q.data_ptr(), n, d, None, 0, 0, d, 0, alpha, 0, 1, ptr, idx, val, cap, nnz, 1)

        def bf16(ptr, idx, val, cap, nnz):
            return lib.ss_similarity_dot_csr_h16(H.data_ptr(), n, d, None, 0, 0, d, 0, 0, alpha, 1, ptr, idx, val, cap, nnz, 1)

        def f32(ptr, idx, val, cap, nnz):
            return lib.ss_similarity_dot_csr_f32(W.data_ptr(), n, n, None, 0, 0, d, 0, alpha, 1, ptr, idx, val, cap, nnz, 1)
        routes = [Route(lib, "fp32_widened", n, d, f32), Route(lib, "bf16", n, d, bf16), Route(lib, "i8", n, d, i8)]
        r = measure(routes, args.reps)
        a, b, c = r["fp32_widened"], r["bf16"], r["i8"]
        floors = {"fp32": pairs * d * 2 / MFMA_F32_FLOPS * 1e3, "bf16": pairs * d * 2 / MFMA_16BIT_FLOPS * 1e3,
                  "i8": pairs * d * 2 / MFMA_I8_OPS * 1e3}
        r["i8_over_bf16"] = {"count_pass": c["count_pass_ms"] / b["count_pass_ms"],
                             "fill_pass": c["fill_pass_ms"] / b["fill_pass_ms"], "total": c["total_ms"] / b["total_ms"]}
        r["i8_over_fp32"] = {"count_pass": c["count_pass_ms"] / a["count_pass_ms"],
                             "fill_pass": c["fill_pass_ms"] / a["fill_pass_ms"], "total": c["total_ms"] / a["total_ms"]}
        r["share_of_floor_count_pass"] = {"fp32": floors["fp32"] / a["count_pass_ms"], "bf16": floors["bf16"] / b["count_pass_ms"],
                                          "i8": floors["i8"] / c["count_pass_ms"]}
        # the three routes are exact on these values up to 2^24: the same graph, bit for bit
        r["same_csr_as_i8"] = {x.name: bool(torch.equal(x.ptr, routes[2].ptr) and torch.equal(x.idx, routes[2].idx)
                                            and torch.equal(x.val, routes[2].val)) for x in routes[:2]}
        r["resident_feature_bytes"] = {"fp32": 4 * n * d, "bf16": 2 * n * d, "i8": n * d}
        size = {"d": d, "alpha": ALPHA_COS, "mfma_floor_one_pass_ms": floors}
        size.update(r)
        rec["sizes"][f"dot_cosine_{n}x{d}"] = size
        print(json.dumps({f"{n}x{d}": r}), flush=True)
        del routes, Q, H, W
        torch.cuda.empty_cache()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(rec, f, indent=1)
    print(json.dumps(rec)[:6000])


if __name__ == "__main__":
    main()
