"""Timing of the cutoff profiles (ss_similarity_*_profile_*, csrc/cut_profile.hip) against the size query of the unchanged
producers (idx == NULL: one all-pairs count pass per alpha), in one process.

The setting of DESIGN 4.13: n rows, symmetric, weighted, clustered (n / 1000 clusters, shuffled: every tile keeps
something), about 1 % fill at the middle cut.  Three producers: 2048-bit fingerprints (Tanimoto, alpha 0.5), cosine fp32
d = 64 and cosine on bf16 rows d = 1024 (alpha 0.97).  NCUTS ascending cuts, evenly spaced, cut NCUTS / 2 the alpha of
4.13.  Per producer, warm, median of REPS with all values (the spread), host clock around calls that end in a device
synchronise; the three measurements alternate inside every repetition, so drift of the machine hits them alike:

    profile      one profile of the NCUTS cuts (totals and row degrees)
    query        one size query of the producer at the middle cut
    queries      NCUTS size queries, one per cut: what a sweep costs without a profile

The profile's totals are compared with the nnz of the NCUTS queries (they must be equal).

    python tools/cut_profile_time.py [--n 100000] [--ncuts 16] [--reps 5] [--out profiles/cut_profile_time.json]"""
import argparse
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np

from dot_csr_time import ALPHA_COS, clustered
from fingerprint_graph_time import clustered as clustered_bits

ALPHA_FP = 0.5


def timed(fn):
    import torch
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


class Case:
    """One producer on device rows: head() are the operands up to alpha / the cuts."""

    def __init__(self, lib, name, n, head, producer, profile, cuts):
        import torch
        self.lib, self.name, self.n, self.head, self.cuts = lib, name, n, head, cuts
        self.producer, self.profile_fn = getattr(lib, producer), getattr(lib, profile)
        self.ptr = torch.empty(n + 1, dtype=torch.int64, device="cuda")
        self.total = torch.zeros(len(cuts), dtype=torch.int64, device="cuda")
        self.rows = torch.zeros((n, len(cuts)), dtype=torch.int32, device="cuda")
        self.nnz = C.c_int64(0)
        self.query_nnz = []

    def query(self, alpha):
        rc = self.producer(*self.head, C.c_float(alpha), 1, self.ptr.data_ptr(), None, None, 0, C.byref(self.nnz), 1)
        assert rc in (0, -5), self.lib.ss_last_error()          # -5: nnz >= 2^31, *nnz is set all the same
        return self.nnz.value

    def middle(self):
        self.query(float(self.cuts[len(self.cuts) // 2]))

    def sweep(self):
        self.query_nnz = [self.query(float(c)) for c in self.cuts]

    def profile(self):
        rc = self.profile_fn(*self.head, self.cuts.ctypes.data, len(self.cuts), 1, self.total.data_ptr(),
                             self.rows.data_ptr(), 1)
        assert rc == 0, self.lib.ss_last_error()


def measure(case, reps):
    import torch
    for fn in (case.profile, case.middle, case.sweep):       # warm
        fn()
    torch.cuda.synchronize()
    t = {"profile": [], "query": [], "queries": []}
    for _ in range(reps):
        t["profile"].append(timed(case.profile))
        t["query"].append(timed(case.middle))
        t["queries"].append(timed(case.sweep))
    total = case.total.cpu().numpy()
    same_rows = bool(torch.equal(case.rows[:, -1].to(torch.int64), case.ptr[1:] - case.ptr[:-1]))   # the last query's ptr
    med = {k: float(np.median(v)) for k, v in t.items()}
    n = case.n
    return {"cuts": [round(float(c), 6) for c in case.cuts], "nnz": [int(x) for x in total],
            "fill_at_middle_cut": float(total[len(total) // 2]) / n / n,
            "profile_totals_equal_query_nnz": bool(np.array_equal(total, np.asarray(case.query_nnz, np.int64))),
            "profile_rows_equal_query_degrees_at_last_cut": same_rows,
            "profile_ms": med["profile"], "profile_all_ms": [round(x, 3) for x in t["profile"]],
            "query_ms": med["query"], "query_all_ms": [round(x, 3) for x in t["query"]],
            "queries_ms": med["queries"], "queries_all_ms": [round(x, 3) for x in t["queries"]],
            "profile_over_one_query": med["profile"] / med["query"],
            "queries_over_profile": med["queries"] / med["profile"]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=100_000)
    ap.add_argument("--ncuts", type=int, default=16)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch                       # before the library, as in the other tools: one HIP runtime for both
    torch.cuda.init()
    import simspread_jl_amd as ss
    from simspread_jl_amd import _lib
    lib = ss.init(0)
    n, nc = args.n, args.ncuts
    clusters = max(1, n // 1000)
    steps = np.arange(nc) - nc // 2
    rec = {"source_hash": _lib.source_hash(),
           "what": f"n = {n}, symmetric, weighted, clustered (n / 1000 clusters, shuffled); one profile of {nc} cuts, one "
                   f"size query at the middle cut and {nc} size queries, alternating in one process",
           "reps": args.reps, "cases": {}}

    def run(name, head, producer, profile, cuts):
        r = measure(Case(lib, name, n, head, producer, profile, cuts), args.reps)
        rec["cases"][name] = r
        print(json.dumps({name: r}), flush=True)
        torch.cuda.empty_cache()

    F = torch.from_numpy(clustered_bits(n, 2048, clusters=clusters, seed=2026).view(np.int64)).cuda()
    run("tanimoto_2048bit_f32", (F.data_ptr(), n, None, 0, 32), "ss_similarity_tanimoto_csr_f32",
        "ss_similarity_tanimoto_profile_f32", (ALPHA_FP + 0.025 * steps).astype(np.float32))
    del F
    cos_cuts = (ALPHA_COS + 0.0025 * steps).astype(np.float32)
    X = torch.from_numpy(clustered(n, 64, clusters=clusters, seed=2026)).cuda()
    W = X.to(torch.float32).t().contiguous()                  # column-major n x d
    run("cosine_f32_d64", (W.data_ptr(), n, n, None, 0, 0, 64, 0), "ss_similarity_dot_csr_f32",
        "ss_similarity_dot_profile_f32", cos_cuts)
    del X, W
    H = torch.from_numpy(clustered(n, 1024, clusters=clusters, seed=2026)).cuda().to(torch.bfloat16).contiguous()
    run("cosine_bf16_d1024", (H.data_ptr(), n, 1024, None, 0, 0, 1024, 0, 0), "ss_similarity_dot_csr_h16",
        "ss_similarity_dot_profile_h16", cos_cuts)
    del H
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(rec, f, indent=1)
    print(json.dumps(rec)[:6000])


if __name__ == "__main__":
    main()
