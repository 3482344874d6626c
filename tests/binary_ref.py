"""Host reference for the per-row binary prediction metrics (ss_binary_metrics_rows_*): the 18 numbers of one row in
fp64 by one descending sort -- every distinct score a threshold (positive when score >= threshold), the six metrics of
simspread_jl_amd.metrics evaluated on all thresholds at once with the mirror's operation order, then max, mean
(math.fsum) and the corrected std (two-pass fsum), as maxperformance / meanperformance / meanstdperformance summarise
them (src/performance.jl:420-520).  tests/test_binary_rows_cpu.py pins it against the mirror itself."""
import math

import numpy as np

METRICS = ("f1score", "mcc", "accuracy", "balancedaccuracy", "recall", "precision")
FIELDS = tuple(f"{m}_{s}" for m in METRICS for s in ("max", "mean", "std"))
EPS = 2.2250738585072014e-308   # floatmin(Float64), mcc's default eps


def _mcc_limit(a, b):
    a, b, e = a.astype(np.float64), b.astype(np.float64), EPS
    return (a * e - b * e) / np.sqrt((a + b) * (a + e) * (b + e) * (e + e))


def threshold_values(y, s):
    """(U, 6) float64: the six metrics at every distinct score of the row, highest threshold first.  `s` keeps its
    dtype, so fp32 scores tie as fp32 values do."""
    y = np.asarray(y).ravel() != 0
    s = np.asarray(s).ravel()
    n = s.size
    P = int(y.sum())
    N = n - P
    order = np.argsort(-s, kind="stable")
    ys, ss = y[order], s[order]
    ends = np.flatnonzero(np.r_[ss[1:] != ss[:-1], True])   # last position of every tie group (-0.0 == +0.0)
    tp = np.cumsum(ys, dtype=np.int64)[ends]
    fp = ends.astype(np.int64) + 1 - tp
    tn, fn = N - fp, P - tp
    p_pred, n_pred, p_act, n_act = tp + fp, fn + tn, tp + fn, fp + tn
    f = np.float64
    with np.errstate(invalid="ignore", divide="ignore", over="ignore", under="ignore"):
        d = tp.astype(f) + 0.5 * (fp + fn).astype(f)
        f1 = np.where(d == 0, np.nan, tp / d)
        main = (tp * tn - fp * fn).astype(f) / np.sqrt((p_pred * n_pred).astype(f) * (p_act * n_act).astype(f))
        mcc = np.select([p_pred == 0, n_pred == 0, p_act == 0, n_act == 0],
                        [_mcc_limit(tn, fn), _mcc_limit(tp, fp), _mcc_limit(tn, fp), _mcc_limit(tp, fn)], main)
        acc = (tp + tn) / ((tp + tn) + (fp + fn))
        tpr = np.where(p_act != 0, tp / np.where(p_act != 0, p_act, 1), np.nan)
        tnr = np.where(n_act != 0, tn / np.where(n_act != 0, n_act, 1), np.nan)
        bal = (tpr + tnr) / 2
        rec = np.where(p_act == 0, np.nan, tp / np.where(p_act != 0, p_act, 1))
        prec = np.where(p_pred == 0, np.nan, tp / np.where(p_pred != 0, p_pred, 1))
    return np.stack([f1, mcc, acc, bal, rec, prec], axis=1).astype(np.float64)


def _stats(v):
    U = v.size
    if np.isnan(v).any():
        return [math.nan] * 3
    mx = float(v.max())
    if np.isfinite(v).all():
        mean = math.fsum(v) / U
        std = math.sqrt(math.fsum((v - mean) ** 2) / (U - 1)) if U > 1 else math.nan
    else:                                      # +-Inf from mcc's limit forms: IEEE sums, as the device's
        with np.errstate(invalid="ignore"):
            mean = float(np.sum(v)) / U
            std = float(np.sqrt(np.sum((v - mean) ** 2) / (U - 1))) if U > 1 else math.nan
    return [mx, mean, std]


def ref_row(y, s, with_scale=False):
    """The 18 numbers of one row, in BINARY_ROWS_FIELDS order (and, with_scale, the 6 values mean|m| that scale the
    tolerances of mean and std)."""
    vals = threshold_values(y, s)
    out = np.array([x for k in range(6) for x in _stats(vals[:, k])])
    if not with_scale:
        return out
    with np.errstate(invalid="ignore"):
        return out, np.abs(vals).mean(axis=0)


def ref_rows(Y, S, with_scale=False):
    """Y: dense 0/1 (or scipy) labels, S: scores, both (nrows, ncols)."""
    import scipy.sparse as sp
    if sp.issparse(Y):
        Y = Y.toarray()
    rows = [ref_row(Y[i], S[i], True) for i in range(S.shape[0])]
    out = np.stack([r[0] for r in rows]) if rows else np.zeros((0, 18))
    if not with_scale:
        return out
    return out, (np.stack([r[1] for r in rows]) if rows else np.zeros((0, 6)))


def assert_binary_close(got, want, scale, what=""):
    """max bitwise; mean within 1e-12 mean|m| and std within 1e-10 max(std, mean|m|) (scale: (nrows, 6) mean|m| from
    ref_rows(..., with_scale=True)); NaN and +-Inf exactly where the reference has them."""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    assert got.shape == want.shape, (got.shape, want.shape)
    g3, w3 = got.reshape(-1, 6, 3), want.reshape(-1, 6, 3)
    sc = np.asarray(scale, np.float64).reshape(-1, 6)
    sc = np.where(np.isfinite(sc), sc, 0.0)
    nan_g, nan_w = np.isnan(g3), np.isnan(w3)
    bad = np.argwhere(nan_g != nan_w)
    assert bad.size == 0, f"{what}: NaN pattern differs at {bad[:5].tolist()}: got {g3[tuple(bad[0])]}, want {w3[tuple(bad[0])]}"
    inf_w = np.isinf(w3)
    assert np.array_equal(g3[inf_w], w3[inf_w]), f"{what}: inf entries differ"
    ok = ~nan_w & ~inf_w
    neq = np.argwhere(ok[..., 0] & (g3[..., 0] != w3[..., 0]))
    assert neq.size == 0, (f"{what}: max differs at {neq[:5].tolist()}: got {g3[tuple(neq[0]) + (0,)]!r} "
                           f"want {w3[tuple(neq[0]) + (0,)]!r}")
    std_w = np.where(ok[..., 2], np.abs(w3[..., 2]), 0.0)
    for s, tol, floor in ((1, 1e-12, sc), (2, 1e-10, np.maximum(std_w, sc))):
        with np.errstate(invalid="ignore"):
            err = np.where(ok[..., s], np.abs(g3[..., s] - w3[..., s]) - tol * floor, -1.0)
        if err.size and err.max() > 0:
            k = tuple(np.argwhere(err > 0)[0])
            raise AssertionError(f"{what}: {('max', 'mean', 'std')[s]} at {list(k)} got {g3[k + (s,)]!r} "
                                 f"want {w3[k + (s,)]!r}")
