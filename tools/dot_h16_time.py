"""Timing of the 16-bit route of the inner-product producer (ss_similarity_dot_csr_h16, csrc/dot_tile_h16.hpp) against
the fp32 route (ss_similarity_dot_csr_f32) on the widened copies of the same rows, in one process.

The setting of DESIGN 4.13: n x d cosine, symmetric, weighted, clustered rows (n / 1000 clusters, shuffled: every tile
keeps something) at about 1 % fill.  The rows are rounded to bf16 and to fp16 once; each 16-bit route reads its patterns
row-major in place, the fp32 route reads the exact fp32 values of the same patterns (column-major, as it requires), so
the three produce the same graph up to summation order.  Per route: the count pass (the size query: NaN scan, row norms,
count kernel, scans) and the fill pass (a full call minus the size query), warm, median of REPS calls with all values,
host clock around calls that end in a device synchronise.  The routes alternate inside every repetition, so drift of
the machine hits them alike.  The floor of one pass is pairs * d * 2 / peak of the route's matrix instruction.

    python tools/dot_h16_time.py [--n 100000] [--dims 64,1024] [--reps 5] [--out profiles/dot_h16_time.json]"""
import argparse
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np

from dot_csr_time import ALPHA_COS, MFMA_F32_FLOPS, clustered

MFMA_16BIT_FLOPS = 2.5e15     # v_mfma_f32_32x32x16_{bf16,f16} dense peak, MI355X_MICROARCH.md


class Route:
    """One producer on device rows: query() is the size query, full() the whole call."""

    def __init__(self, lib, name, n, d, call):
        import torch
        self.name, self.n, self.d = name, n, d
        self.ptr = torch.empty(n + 1, dtype=torch.int64, device="cuda")
        self.nnz = C.c_int64(0)
        self._call = call
        self.query()
        self.idx = torch.empty(max(self.nnz.value, 1), dtype=torch.int32, device="cuda")
        self.val = torch.empty(max(self.nnz.value, 1), dtype=torch.float32, device="cuda")

    def query(self):
        assert self._call(self.ptr.data_ptr(), None, None, 0, C.byref(self.nnz)) == 0

    def full(self):
        assert self._call(self.ptr.data_ptr(), self.idx.data_ptr(), self.val.data_ptr(), self.nnz.value,
                          C.byref(self.nnz)) == 0


def timed(fn):
    import torch
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


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
        qm, fm = float(np.median(q[r.name])), float(np.median(f[r.name]))
        out[r.name] = {"nnz": r.nnz.value, "fill": r.nnz.value / r.n / r.n, "count_pass_ms": qm,
                       "count_pass_all_ms": [round(t, 3) for t in q[r.name]], "total_ms": fm,
                       "total_all_ms": [round(t, 3) for t in f[r.name]], "fill_pass_ms": fm - qm}
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
           "what": f"n = {n}, cosine, symmetric, weighted, clustered (n / 1000 clusters, shuffled); per storage the 16-bit "
                   "route on the patterns and the fp32 route on their widened copies, alternating in one process",
           "reps": args.reps, "sizes": {}}
    pairs = n * (n + 1) / 2
    for d in dims:
        X = torch.from_numpy(clustered(n, d, clusters=max(1, n // 1000), seed=2026)).cuda()
        size = {"d": d, "alpha": ALPHA_COS, "mfma_floor_one_pass_ms": {"fp32": pairs * d * 2 / MFMA_F32_FLOPS * 1e3,
                                                                       "h16": pairs * d * 2 / MFMA_16BIT_FLOPS * 1e3}}
        for storage, tdt, code in (("bf16", torch.bfloat16, 0), ("f16", torch.float16, 1)):
            H = X.to(tdt).contiguous()                    # the patterns, row-major n x d
            W = H.to(torch.float32).t().contiguous()      # their exact fp32 values, column-major n x d
            alpha = C.c_float(ALPHA_COS)

            def h16(ptr, idx, val, cap, nnz, H=H, code=code):
                return lib.ss_similarity_dot_csr_h16(H.data_ptr(), n, d, None, 0, 0, d, code, 0, alpha, 1, ptr, idx, val, cap,
                                                     nnz, 1)

            def f32(ptr, idx, val, cap, nnz, W=W):
                return lib.ss_similarity_dot_csr_f32(W.data_ptr(), n, n, None, 0, 0, d, 0, alpha, 1, ptr, idx, val, cap, nnz, 1)
            routes = [Route(lib, "fp32_widened", n, d, f32), Route(lib, storage, n, d, h16)]
            r = measure(routes, args.reps)
            a, b = r["fp32_widened"], r[storage]
            same = bool(torch.equal(routes[0].ptr, routes[1].ptr))
            r["h16_over_fp32"] = {"count_pass": b["count_pass_ms"] / a["count_pass_ms"],
                                  "fill_pass": b["fill_pass_ms"] / a["fill_pass_ms"], "total": b["total_ms"] / a["total_ms"]}
            r["share_of_floor"] = {"fp32_count_pass": size["mfma_floor_one_pass_ms"]["fp32"] / a["count_pass_ms"],
                                   "h16_count_pass": size["mfma_floor_one_pass_ms"]["h16"] / b["count_pass_ms"]}
            r["same_row_pointers"] = same
            size[storage] = r
            print(json.dumps({f"{n}x{d}_{storage}": r}), flush=True)
            del routes, H, W
            torch.cuda.empty_cache()
        rec["sizes"][f"dot_cosine_{n}x{d}"] = size
        del X
        torch.cuda.empty_cache()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(rec, f, indent=1)
    print(json.dumps(rec)[:6000])


if __name__ == "__main__":
    main()
