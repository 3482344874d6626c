"""Timing of the Butina clustering (include/simspread_hip_clusters.h) next to the fingerprint producer that feeds it,
which is the yardstick: nothing clustered before, and both are measured in one process.

One set: the clustered 100k x 2048-bit library of tools/neighbour_floor_time.py (100 prototypes, seed 2026), fp32, at
two cutoffs.  Per cutoff:

  producer   ss_similarity_tanimoto_csr_f32, unweighted, val == NULL: size query + fill     the pattern, device resident
  cluster    ss_cluster_butina_csr on that pattern (device in, device out), host clock
  split      ss_timing_last of that call: symmetrise (sort of 2 nnz keys, distinct, CSR), rounds, assign and label
  fused      ss_cluster_butina_fingerprint_f32, host clock                                   producer + cluster in one call
  rounds, clusters, the largest cluster, nnz

Warm, median of REPS calls, host clock around work that ends in a device synchronise.

    python tools/cluster_time.py [--n 100000] [--cutoffs 0.5 0.8] [--reps 3] [--out profiles/cluster_time.json]"""
import argparse
import ctypes as C
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

from tools.neighbour_floor_time import D, clustered, timed


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=100_000)
    ap.add_argument("--cutoffs", type=float, nargs="+", default=[0.5, 0.8])
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default="profiles/cluster_time.json")
    args = ap.parse_args()

    import torch
    import simspread_jl_amd as ss
    from simspread_jl_amd import _lib
    ss.init(0)
    ss.use_torch_stream()
    lib = _lib.lib()
    n = args.n
    F = clustered(n, D, clusters=100, seed=2026)
    Ft = torch.from_numpy(F.view(np.int64)).cuda()
    nw = Ft.shape[1]
    DEV = _lib.SS_MEM_DEVICE
    ptr = torch.empty(n + 1, dtype=torch.int64, device="cuda")
    centre, label, size = (torch.empty(n, dtype=torch.int32, device="cuda") for _ in range(3))
    nnz, nc, rounds = C.c_int64(0), C.c_int64(0), C.c_int64(0)
    outs = (centre.data_ptr(), label.data_ptr(), size.data_ptr(), C.byref(nc), C.byref(rounds), DEV)

    cases = []
    for cutoff in args.cutoffs:
        def produce(idx, cap):
            _lib.check(lib.ss_similarity_tanimoto_csr_f32(Ft.data_ptr(), n, None, n, nw, C.c_float(cutoff), 0,
                                                          ptr.data_ptr(), idx, None, cap, C.byref(nnz), DEV))

        produce(None, 0)
        idx = torch.empty(max(nnz.value, 1), dtype=torch.int32, device="cuda")

        def producer():
            produce(None, 0)
            produce(idx.data_ptr(), idx.numel())

        def cluster():
            _lib.check(lib.ss_cluster_butina_csr(n, ptr.data_ptr(), idx.data_ptr(), 0, *outs))

        def fused():
            _lib.check(lib.ss_cluster_butina_fingerprint_f32(Ft.data_ptr(), n, nw, C.c_float(cutoff), *outs))

        t = {"producer": timed(producer, args.reps), "cluster": timed(cluster, args.reps)}
        split = ss.timing_last()                          # of the last clustering call
        via_csr = (centre.clone(), label.clone(), nc.value, rounds.value)
        t["fused"] = timed(fused, args.reps)
        assert torch.equal(centre, via_csr[0]) and torch.equal(label, via_csr[1]) and nc.value == via_csr[2]
        ms = {k: v[0] for k, v in t.items()}
        cases.append({
            "cutoff": cutoff, "nnz": nnz.value, "mean_degree": nnz.value / n, "clusters": nc.value,
            "largest_cluster": int(size[:nc.value].max()), "singletons": int((size[:nc.value] == 1).sum()),
            "rounds": rounds.value,
            "ms": {"producer": ms["producer"], "cluster": ms["cluster"], "fused": ms["fused"],
                   "symmetrise": split["transfer_ms"], "rounds": split["spmm_ms"], "assign_label": split["epilogue_ms"],
                   "cluster_device_total": split["total_ms"]},
            "ratio": {"cluster_over_producer": ms["cluster"] / ms["producer"]},
            "all_ms": {k: v[1] for k, v in t.items()},
        })
        del idx
    rec = {
        "what": f"Butina clustering next to the fingerprint producer that feeds it (the yardstick): clustered {n} x {D} "
                "bits, fp32, unweighted pattern, device in and out",
        "reps": args.reps, "source_hash": _lib.source_hash(), "n": n, "cases": cases,
    }
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(rec, f, indent=1)
    print(json.dumps(rec))


if __name__ == "__main__":
    main()
