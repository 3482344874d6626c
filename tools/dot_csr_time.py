"""Accuracy and timing of the inner-product similarity route (ss_similarity_dot_csr_*, csrc/dot_csr.hip).

Accuracy: the largest |s_device - s64| over the case matrix of tests/test_gpu_dot_csr.py (symmetric and cross block,
non-negative and signed inputs, every pair kept: weighted at alpha = -2), per dtype and metric, next to the derived band
4 (d + 4) eps of tests/dot_ref.py; the largest ratio error / band over the cases is the number of interest.

Time: n x d fp32 cosine on clustered rows (n / 1000 clusters, shuffled: every tile keeps something) at about 1 % fill:
the count pass (the size query: NaN scan, row norms, count kernel, scans), the fill pass (a full call minus the size
query) and the total, warm, median of REPS calls, host clock around calls that end in a device synchronise.  The
comparator is ss_similarity_jaccard_csr_f32 on the same n x 64 rows, timed the same way in the same process.

    python tools/dot_csr_time.py [--n 100000] [--dims 64,1024] [--reps 5] [--no-accuracy] [--out profiles/dot_csr_time.json]"""
import argparse
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np

MFMA_F32_FLOPS = 157.3e12    # v_mfma_f32_32x32x2_f32 peak, MI355X_MICROARCH.md
ALPHA_COS, ALPHA_JAC = 0.97, 0.85


def clustered(n, d, clusters, seed, noise=0.05):
    rng = np.random.default_rng(seed)
    proto = rng.random((clusters, d)) + 0.05
    member = rng.permutation(np.arange(n) % clusters)
    X = np.empty((n, d), np.float32)
    for r in range(0, n, 16384):
        m = member[r:r + 16384]
        X[r:r + 16384] = proto[m] * np.exp(rng.normal(0, noise, (len(m), d)))
    return X


def median_ms(fn, reps):
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


def time_producer(lib, name, mid, Xt, n, d, alpha, reps):
    """Size query and full call of ss_similarity_<name>_csr_f32 on device rows (symmetric, weighted)."""
    import torch
    fn = getattr(lib, f"ss_similarity_{name}_csr_f32")
    Ft = Xt.t().contiguous()                      # column-major n x d
    ptr = torch.empty(n + 1, dtype=torch.int64, device="cuda")
    nnz = C.c_int64(0)
    head = (Ft.data_ptr(), n, n, None, 0, 0, d) + mid + (C.c_float(alpha), 1)

    def query():
        assert fn(*head, ptr.data_ptr(), None, None, 0, C.byref(nnz), 1) == 0
    query()
    idx = torch.empty(max(nnz.value, 1), dtype=torch.int32, device="cuda")
    val = torch.empty(max(nnz.value, 1), dtype=torch.float32, device="cuda")

    def full():
        assert fn(*head, ptr.data_ptr(), idx.data_ptr(), val.data_ptr(), nnz.value, C.byref(nnz), 1) == 0
    q_ms, q_all = median_ms(query, reps)
    f_ms, f_all = median_ms(full, reps)
    return {"nnz": nnz.value, "fill": nnz.value / n / n, "count_pass_ms": q_ms, "count_pass_all_ms": q_all,
            "total_ms": f_ms, "total_all_ms": f_all, "fill_pass_ms": f_ms - q_ms}


def timing(args):
    import torch
    import simspread_jl_amd as ss
    lib = ss.init(0)
    out = {"what": f"n = {args.n}, fp32, symmetric, weighted, clustered (n / 1000 clusters, shuffled), one count pass + one "
                   "fill pass per total", "reps": args.reps, "sizes": {}}
    for d in args.dims:
        X = clustered(args.n, d, clusters=max(1, args.n // 1000), seed=2026)
        Xt = torch.from_numpy(X).cuda()
        r = time_producer(lib, "dot", (0,), Xt, args.n, d, ALPHA_COS, args.reps)
        pairs = args.n * (args.n + 1) / 2
        r.update(metric="cosine", alpha=ALPHA_COS, d=d, mfma_floor_one_pass_ms=pairs * d * 2 / MFMA_F32_FLOPS * 1e3)
        out["sizes"][f"dot_cosine_{args.n}x{d}"] = r
        print(json.dumps(r), flush=True)
        if d == 64:
            j = time_producer(lib, "jaccard", (), Xt, args.n, d, ALPHA_JAC, args.reps)
            j.update(metric="jaccard", alpha=ALPHA_JAC, d=d)
            out["sizes"][f"jaccard_{args.n}x{d}"] = j
            print(json.dumps(j), flush=True)
            out["dot_over_jaccard_total"] = r["total_ms"] / j["total_ms"]
        del Xt
        torch.cuda.empty_cache()
    return out


def accuracy():
    import simspread_jl_amd as ss
    import dot_ref as R
    ss.init(0)
    out = {}
    for dt in (np.float32, np.float64):
        for metric in R.METRICS:
            worst = {"max_abs_err": 0.0, "max_err_over_band": 0.0}
            for n, d in R.CASES:
                band = R.band(dt, d)
                for signed in (False, True):
                    F, G = R.case_inputs(n, d, signed)
                    for Fb in (None, G):
                        M = ss.dot_csr(F, Fb, metric=metric, alpha=-2.0, weighted=True, dtype=dt)
                        s = R.ref_s64(F, F if Fb is None else G, metric, dt, sym=Fb is None)
                        rows = np.repeat(np.arange(M.shape[0]), np.diff(M.indptr))
                        err = float(np.abs(M.data.astype(np.float64) - s[rows, M.indices]).max(initial=0.0))
                        worst["max_abs_err"] = max(worst["max_abs_err"], err)
                        if err / band > worst["max_err_over_band"]:
                            worst.update(max_err_over_band=err / band, at={"n": n, "d": d, "signed": signed,
                                                                           "cross": Fb is not None, "err": err,
                                                                           "band": band})
            out[f"{np.dtype(dt).name}_{metric}"] = worst
            print(json.dumps({f"{np.dtype(dt).name}_{metric}": worst}), flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=100_000)
    ap.add_argument("--dims", default="64,1024")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--no-accuracy", dest="accuracy", action="store_false")
    ap.add_argument("--no-timing", dest="timing", action="store_false")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    args.dims = [int(s) for s in args.dims.split(",") if s]
    import torch                       # before the library, as in the other tools: one HIP runtime for both
    torch.cuda.init()
    from simspread_jl_amd import _lib
    rec = {"source_hash": _lib.source_hash()}
    if args.accuracy:
        rec["accuracy"] = accuracy()
    if args.timing:
        rec["time"] = timing(args)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(rec, f, indent=1)
    print(json.dumps(rec)[:4000])


if __name__ == "__main__":
    main()
