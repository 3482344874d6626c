"""simspread.jl_amd -- MI355X-native SimSpread resource-spreading engine.

The hot path ``featurize -> construct -> spread -> predict -> clean!`` of cvigilv/SimSpread.jl
(src/core.jl) behind the reference's own function names, computed by hand-written gfx950
kernels in ``libsimspread_hip.so`` (C ABI: include/simspread_hip.h).  No CPU fallback.
"""
from . import _lib
from ._lib import SimSpreadError, init, path_last, timing_hold, timing_last, use_torch_stream
from .core import (NamedMatrix, Network, clean, clean_, construct, cutoff, featurize, k, names, precisionatL, predict,
                   read_namedmatrix, recallatL, save, save_loo, split, split_clusters, spread, writedlm)
from .dist import (comm_destroy, comm_init, comm_unique_id, gather_scores, gather_topl, lib_gather_scores, pooled_metrics,
                   shard_range, target_rank, target_rank_positives, target_topl)
from .engine import (BINARY_ROWS_FIELDS, POOLED_FIELDS, RANK_ROWS_FIELDS, TARGET_RANK_FIELDS, TARGET_TOPL_FIELDS, DeviceGraph, DeviceQueries, DeviceSpMat,
                     CutoffProfile, Pool,
                     TargetRank, TargetTopL, ButinaClusters, binary_metrics_rows, butina_clusters, cluster_folds, cross_fold_edges,
                     cutoff_csr,
                     dot_csr, dot_kth, dot_kth_i8, dot_profile, jaccard_csr, jaccard_kth, jaccard_profile,
                     jaccard_similarity, pack_fingerprints, rank_metrics, rank_metrics_rows, tanimoto_csr, tanimoto_kth, tanimoto_profile,
                     quantize_i8, to_bf16_bits, topl)
from .metrics import (AuPRC, AuROC, BEDROC, ROCNums, accuracy, balancedaccuracy, f1score, maxperformance, mcc,
                      meanperformance, meanstdperformance, precision, recall, roc, validity_ratio)

__all__ = ["NamedMatrix", "Network", "DeviceGraph", "DeviceQueries", "DeviceSpMat", "SimSpreadError", "init", "timing_last", "timing_hold", "path_last", "use_torch_stream",
           "shard_range", "pooled_metrics", "Pool", "POOLED_FIELDS", "target_topl", "TargetTopL", "TARGET_TOPL_FIELDS", "gather_scores", "gather_topl", "comm_unique_id", "comm_init", "comm_destroy", "lib_gather_scores", "k", "cutoff", "featurize", "construct", "spread", "predict", "clean", "clean_", "names", "split", "save", "save_loo", "topl", "recallatL", "precisionatL",
           "read_namedmatrix", "writedlm", "rank_metrics", "rank_metrics_rows", "RANK_ROWS_FIELDS", "binary_metrics_rows", "BINARY_ROWS_FIELDS", "jaccard_similarity", "jaccard_csr", "dot_csr", "cutoff_csr", "pack_fingerprints", "tanimoto_csr", "tanimoto_kth", "jaccard_kth", "dot_kth", "AuROC", "AuPRC", "BEDROC", "validity_ratio", "roc", "ROCNums",
           "f1score", "mcc", "accuracy", "balancedaccuracy", "recall", "precision", "maxperformance", "meanperformance",
           "meanstdperformance", "ButinaClusters", "butina_clusters", "cluster_folds", "cross_fold_edges", "split_clusters", "TargetRank", "TARGET_RANK_FIELDS",
           "target_rank", "target_rank_positives", "to_bf16_bits", "CutoffProfile", "tanimoto_profile", "jaccard_profile",
           "dot_profile", "quantize_i8", "dot_kth_i8"]
