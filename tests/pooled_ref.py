"""Host reference for pooled evaluation (ss_pool_*): a table of the distinct scores (descending, -0.0 == +0.0) with the
count of positives and of negatives at each, the merge of tables, and the 21 pooled numbers of a table in fp64 --
AuROC and AuPRC by the trapezoid over every distinct score without a (0,0) point (src/performance.jl:49-89, as
launch_rank_metrics forms it), the validity ratio, then max / mean / std over every threshold of the six binary metrics
evaluated by the host mirror itself (simspread_jl_amd.metrics, Python integers), summarised as
maxperformance / meanstdperformance do.  tests/test_pooled_cpu.py pins it against the mirror on plain vectors."""
import math

import numpy as np

from simspread_jl_amd import metrics as M

FIELDS = ("AuROC", "AuPRC", "validity_ratio") + tuple(
    f"{m}_{s}" for m in ("f1score", "mcc", "accuracy", "balancedaccuracy", "recall", "precision")
    for s in ("max", "mean", "std"))
EPS = 2.2250738585072014e-308   # floatmin(Float64), mcc's default eps


def _mcc(c):
    """metrics.mcc, with its limit forms in IEEE arithmetic (+-Inf / NaN where Python raises ZeroDivisionError, as on
    the device and in tests/binary_ref.py); the main form is the mirror's own Python-integer expression."""
    tn, fp, fn, tp = c.tn, c.fp, c.fn, c.tp
    p_pred, n_pred, p_act, n_act = tp + fp, fn + tn, tp + fn, fp + tn
    for cond, a, b in ((p_pred == 0, tn, fn), (n_pred == 0, tp, fp), (p_act == 0, tn, fp), (n_act == 0, tp, fn)):
        if cond:
            a, b, e = np.float64(a), np.float64(b), np.float64(EPS)
            with np.errstate(all="ignore"):
                return float((a * e - b * e) / np.sqrt((a + b) * (a + e) * (b + e) * (e + e)))
    return M.mcc(c)


_FNS = (M.f1score, _mcc, M.accuracy, M.balancedaccuracy, M.recall, M.precision)


def table(y, s):
    """(keys descending in s's dtype, npos int64, nneg int64) of the pairs (s[i], y[i] != 0)."""
    y = np.asarray(y).ravel() != 0
    s = np.asarray(s).ravel()
    s = np.where(s == 0, s.dtype.type(0), s)              # -0.0 -> +0.0
    keys, inv = np.unique(s, return_inverse=True)        # ascending
    npos = np.bincount(inv, weights=y, minlength=keys.size).astype(np.int64)
    nall = np.bincount(inv, minlength=keys.size).astype(np.int64)
    return keys[::-1].copy(), npos[::-1].copy(), (nall - npos)[::-1].copy()


def merge(*tables):
    """Union of the keys, counts added (exact integers)."""
    keys = np.concatenate([t[0] for t in tables])
    npos = np.concatenate([np.asarray(t[1], np.int64) for t in tables])
    nneg = np.concatenate([np.asarray(t[2], np.int64) for t in tables])
    u, inv = np.unique(keys, return_inverse=True)
    p = np.zeros(u.size, np.int64)
    q = np.zeros(u.size, np.int64)
    np.add.at(p, inv, npos)
    np.add.at(q, inv, nneg)
    return u[::-1].copy(), p[::-1].copy(), q[::-1].copy()


def _stats(v):
    v = np.asarray(v, np.float64)
    if np.isnan(v).any():
        return [math.nan] * 3
    mx = float(v.max())
    if np.isfinite(v).all():
        mean = math.fsum(v) / v.size
        std = math.sqrt(math.fsum((v - mean) ** 2) / (v.size - 1)) if v.size > 1 else math.nan
    else:
        with np.errstate(invalid="ignore"):
            mean = float(np.sum(v)) / v.size
            std = float(np.sqrt(np.sum((v - mean) ** 2) / (v.size - 1))) if v.size > 1 else math.nan
    return [mx, mean, std]


def metrics(keys, npos, nneg):
    """The 21 pooled numbers of a table (FIELDS order)."""
    keys = np.asarray(keys)
    tp = [int(v) for v in np.cumsum(np.asarray(npos, dtype=object))]   # Python integers: exact past 2^63
    fp = [int(v) for v in np.cumsum(np.asarray(nneg, dtype=object))]
    P, N = tp[-1], fp[-1]
    E = len(tp)
    Pd, Nd = float(P), float(N)
    roc, prc = [], []
    with np.errstate(invalid="ignore", divide="ignore"):
        for k in range(1, E):
            tp1, fp1, tp0, fp0 = float(tp[k]), float(fp[k]), float(tp[k - 1]), float(fp[k - 1])
            a = np.float64(fp1) / Nd - np.float64(fp0) / Nd
            b = np.float64(tp1) / Pd + np.float64(tp0) / Pd
            roc.append(a * b * 0.5)
            c = np.float64(tp1) / Pd - np.float64(tp0) / Pd
            d = np.float64(tp1) / (tp1 + fp1) + np.float64(tp0) / (tp0 + fp0)
            prc.append(c * d * 0.5)
    auroc = abs(math.fsum(roc)) if not any(map(math.isnan, roc)) else math.nan
    auprc = abs(math.fsum(prc)) if not any(map(math.isnan, prc)) else math.nan
    zero = int(np.sum((np.asarray(npos) + np.asarray(nneg))[keys == 0]))
    validity = (P + N - zero) / (P + N)
    vals = np.empty((E, 6))
    for k in range(E):
        c = M.ROCNums(P, N, tp[k], N - fp[k], fp[k], P - tp[k])
        for m, f in enumerate(_FNS):
            vals[k, m] = f(c)
    out = [auroc, auprc, validity]
    for m in range(6):
        out += _stats(vals[:, m])
    return np.array(out, np.float64), np.abs(vals).mean(axis=0)


def assert_pooled_close(got, want, scale, what=""):
    """AuROC, AuPRC, validity within 1e-12 relative; per metric max bitwise, mean and std within 1e-12 relative to
    max(|value|, mean|m|) (scale: the second value metrics() returns); NaN exactly where the reference has it."""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    assert got.shape == want.shape == (21,), (got.shape, want.shape)
    nan_g, nan_w = np.isnan(got), np.isnan(want)
    assert np.array_equal(nan_g, nan_w), f"{what}: NaN pattern got {got} want {want}"
    for i in range(3):
        if not nan_w[i]:
            assert abs(got[i] - want[i]) <= 1e-12 * max(abs(want[i]), 1e-300), f"{what}: {FIELDS[i]} {got[i]!r} {want[i]!r}"
    for m in range(6):
        mx, mean, std = 3 + 3 * m, 4 + 3 * m, 5 + 3 * m
        if not nan_w[mx]:
            assert got[mx] == want[mx], f"{what}: {FIELDS[mx]} {got[mx]!r} {want[mx]!r}"
        sc = scale[m] if np.isfinite(scale[m]) else 0.0
        for i in (mean, std):
            if not nan_w[i] and np.isfinite(want[i]):
                assert abs(got[i] - want[i]) <= 1e-12 * max(abs(want[i]), sc, 1e-300), \
                    f"{what}: {FIELDS[i]} {got[i]!r} {want[i]!r}"
            elif not nan_w[i]:
                assert got[i] == want[i], f"{what}: {FIELDS[i]}"
