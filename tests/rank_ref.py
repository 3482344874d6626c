"""Host reference for the per-row ranking metrics (ss_rank_metrics_rows_*): the six numbers of one row in fp64, by one
stable descending sort -- the reference's definitions (src/performance.jl:22-89,308-385,558-560) in O(n log n), so that
rows of 100k columns can be checked.  tests/test_rank_rows_cpu.py pins it against oracle.auroc / auprc / bedroc /
validity_ratio, which evaluate a confusion matrix per unique score literally."""
import numpy as np

FIELDS = ("AuROC", "AuPRC", "BEDROC", "validity_ratio", "recallatL", "precisionatL")


def ref_row(y, s, alpha=20.0, L=20):
    y = np.asarray(y).ravel() != 0
    s = np.asarray(s, dtype=np.float64).ravel()
    n = s.size
    P = int(y.sum())
    N = n - P
    order = np.argsort(-s, kind="stable")          # sortperm(yhat, rev=true): ties by position
    ys, ss = y[order], s[order]
    ends = np.flatnonzero(np.r_[ss[1:] != ss[:-1], True])   # last position of every tie group (= unique thresholds)
    ctp = np.cumsum(ys)
    tp = ctp[ends].astype(np.float64)
    fp = (ends + 1) - tp
    with np.errstate(invalid="ignore", divide="ignore"):
        tpr, fpr, prec = tp / P, fp / N, tp / (tp + fp)
        auroc = abs(float(np.sum((fpr[1:] - fpr[:-1]) * (tpr[1:] + tpr[:-1]) / 2.0)))
        auprc = abs(float(np.sum((tpr[1:] - tpr[:-1]) * (prec[1:] + prec[:-1]) / 2.0)))
        r = np.flatnonzero(ys) + 1
        Ra = P / n
        rand_sum = Ra * (1 - np.exp(-alpha)) / (np.exp(alpha / n) - 1)
        fac = Ra * np.sinh(alpha / 2) / (np.cosh(alpha / 2) - np.cosh(alpha / 2 - alpha * Ra))
        cte = 1 / (1 - np.exp(alpha * (1 - Ra)))
        bedroc = float(np.sum(np.exp(-alpha * r / n)) * fac / rand_sum + cte)
    hits = int(ys[:L].sum())
    return np.array([auroc, auprc, bedroc, np.count_nonzero(s) / n, hits / P if P else np.nan, hits / L])


def ref_rows(Y, S, alpha=20.0, L=20):
    """Y: dense 0/1 (or scipy) labels, S: scores, both (nrows, ncols)."""
    import scipy.sparse as sp
    if sp.issparse(Y):
        Y = Y.toarray()
    return np.stack([ref_row(Y[i], S[i], alpha, L) for i in range(S.shape[0])]) if S.shape[0] else np.zeros((0, 6))


def assert_rows_close(got, want, rtol, atol, what=""):
    """Element-wise |got - want| <= atol + rtol |want|, NaN exactly where want is NaN (inf where want is inf)."""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    assert got.shape == want.shape, (got.shape, want.shape)
    nan_g, nan_w = np.isnan(got), np.isnan(want)
    bad = np.argwhere(nan_g != nan_w)
    assert bad.size == 0, f"{what}: NaN pattern differs at {bad[:5].tolist()}: got {got[tuple(bad[0])]}, want {want[tuple(bad[0])]}"
    inf_w = np.isinf(want)
    assert np.array_equal(got[inf_w], want[inf_w]), f"{what}: inf entries differ"
    m = ~nan_w & ~inf_w
    err = np.abs(got[m] - want[m]) - (atol + rtol * np.abs(want[m]))
    if err.size and err.max() > 0:
        k = np.argwhere(m)[int(np.argmax(err))]
        raise AssertionError(f"{what}: entry {k.tolist()} got {got[tuple(k)]!r} want {want[tuple(k)]!r}")
