"""Host reference for per-target top-L tables (ss_target_topl_*): per target a stable lexsort by (isless key
descending, row ascending), the first L entries with their labels, hits and npos, and the four means in target order
(sums divided by the count, as Julia's mean over an iterator).  tests/test_target_topl_cpu.py pins it against a
literal restatement of recallatL / precisionatL(y, yhat, grouping, L) (src/performance.jl:308-409) on vec(.)."""
import math

import numpy as np


def isless_key(s):
    """uint64 keys whose ascending order is Julia's isless on the scores (+0.0 after -0.0); NaN is not allowed."""
    s = np.asarray(s)
    if s.dtype == np.float32:
        u = s.view(np.uint32).astype(np.uint64)
        return np.where(u >> np.uint64(31), ~u & np.uint64(0xFFFFFFFF), u | np.uint64(0x80000000))
    u = np.ascontiguousarray(s, dtype=np.float64).view(np.uint64)
    return np.where(u >> np.uint64(63), ~u, u | np.uint64(1 << 63))


def table(Y, S, L, rows=None):
    """(vals, rows, labels) as (nt, fill) arrays and npos (nt,) of score matrix S (n, nt) with 0/1 labels Y (n, nt);
    rows: the row ids (default 0..n-1)."""
    S = np.asarray(S)
    Y = np.asarray(Y) != 0
    n, nt = S.shape
    rows = np.arange(n, dtype=np.int64) if rows is None else np.asarray(rows, dtype=np.int64)
    fill = min(L, n)
    vals = np.empty((nt, fill), S.dtype)
    rid = np.empty((nt, fill), np.int64)
    lab = np.empty((nt, fill), np.uint8)
    for t in range(nt):
        k = isless_key(S[:, t])
        order = np.lexsort((rows, ~k))[:fill]      # key descending, then row ascending
        vals[t], rid[t], lab[t] = S[order, t], rows[order], Y[order, t]
    return vals, rid, lab, Y.sum(0).astype(np.int64)


def metrics(labels, npos, L):
    """(recallatL, precisionatL, recall over the targets with positives, their number), hits."""
    hits = np.asarray(labels, np.int64).sum(1)
    rec = prec = rec_pos = 0.0
    with_pos = 0
    for h, p in zip(hits.tolist(), np.asarray(npos).tolist()):
        r = h / p if p > 0 else math.nan
        rec += r
        prec += h / L
        if p > 0:
            rec_pos += r
            with_pos += 1
    nt = len(hits)
    return (rec / nt, prec / nt, rec_pos / with_pos if with_pos else math.nan, float(with_pos)), hits


def julia_grouped(y, yhat, grouping, L):
    """recallatL(y, yhat, grouping, L) and precisionatL(...) restated line by line: groups in first-seen order
    (unique), a stable sortperm(yhat_g, rev=true) under isless, `length(y) > L` asserted, mean over the groups."""
    y, yhat, grouping = (np.asarray(v).ravel() for v in (y, yhat, grouping))
    rec, prec = [], []
    for gname in dict.fromkeys(grouping.tolist()):
        sel = grouping == gname
        yg, sg = y[sel], yhat[sel]
        assert len(yg) > L, "Number of labels is less than length (L > y)"
        # isless descending; ties (equal values and equal signs) keep their order (stable)
        order = sorted(range(len(sg)), key=lambda i: (-float(sg[i]), bool(np.signbit(sg[i])), i))
        ys = yg[order]
        xi, xil = ys.sum(), ys[:L].sum()
        rec.append(xil / xi if xi > 0 else math.nan)
        prec.append(xil / L)
    mean = lambda v: sum(v[1:], v[0]) / len(v)   # noqa: E731  (Julia's mean: left-to-right sum / count)
    return float(mean(rec)), float(mean(prec))
