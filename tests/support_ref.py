"""Host restatement of the support lists of ss_support_* (include/simspread_hip.h) in numpy.

A score is ``Yhat[r,t] = sum_s T[r,s] * Ys[s,t]`` with ``T[r,:]`` the transfer row (stage-1 output, 1/ks included; for a
leave-one-out fold the degree-corrected row).  The support of the pair (r, t) is the set of sources s with a stored
``Ys[s,t]`` and ``c_s = T[r,s] * Ys[s,t] != 0``, ordered by c_s descending, ties by ascending s.  ``transfer_rows`` gives
the rows of T in fp64; ``support_lists`` turns any rows of T (fp64 here, or the device's own bits in the graph's dtype) into
the lists, multiplying in the dtype of T."""
import numpy as np
import scipy.sparse as sp


def _inv_count(d):
    d = np.asarray(d, dtype=np.float64)
    out = np.zeros_like(d)
    out[d > 0] = 1.0 / d[d > 0]
    return out


def _clean_csr(m):
    m = sp.csr_matrix(m, dtype=np.float64)
    m.eliminate_zeros()
    m.sort_indices()
    return m


def transfer_rows(Xq, Xs, Ys, rows, loo=False):
    """Rows ``rows`` of the transfer block as a dense (len(rows), ns) fp64 array: query rows of Xq, or with loo the
    leave-one-out folds of the square Xs (feature j named after source j)."""
    Xs, Ys = _clean_csr(Xs), _clean_csr(Ys)
    ns = Xs.shape[0]
    kf = np.asarray((Xs != 0).sum(axis=0)).ravel().astype(np.float64)
    ks = (np.asarray((Xs != 0).sum(axis=1)).ravel() + np.asarray((Ys != 0).sum(axis=1)).ravel()).astype(np.float64)
    out = np.zeros((len(rows), ns))
    if not loo:
        Xq = _clean_csr(Xq)
        T = (Xq[np.asarray(rows, dtype=np.int64)] @ sp.diags(_inv_count(kf))) @ Xs.T @ sp.diags(_inv_count(ks))
        return np.asarray(T.todense())
    assert Xs.shape[1] == ns
    Xc = Xs.tocsc()
    for o, i in enumerate(rows):
        lo, hi = Xs.indptr[i], Xs.indptr[i + 1]
        fidx, fval = Xs.indices[lo:hi], Xs.data[lo:hi]
        u = np.zeros(ns)
        u[fidx] = fval * _inv_count(kf[fidx] - 1.0)   # the query leaves every feature column it touched
        u[i] = 0.0                                    # its own feature column is dropped
        ksi = ks.copy()
        ksi[Xc.indices[Xc.indptr[i]:Xc.indptr[i + 1]]] -= 1.0
        z = (Xs @ u) * _inv_count(ksi)
        z[i] = 0.0
        out[o] = z
    return out


def support_lists(T, slot, Ys, targets, M):
    """The lists of the pairs (T[slot[p]], targets[p]): ``(src (n, M) int32, contrib (n, M) T.dtype, nsupp (n,) int32)``.
    The products are taken in T's dtype (Ys is cast to it), one rounding each; unused slots hold -1 / 0."""
    dt = T.dtype
    Yc = sp.csc_matrix(_clean_csr(Ys))
    Yc.sort_indices()
    n = len(targets)
    src = np.full((n, M), -1, np.int32)
    contrib = np.zeros((n, M), dt)
    nsupp = np.zeros(n, np.int32)
    for p in range(n):
        t = int(targets[p])
        s = Yc.indices[Yc.indptr[t]:Yc.indptr[t + 1]]
        c = T[slot[p], s] * Yc.data[Yc.indptr[t]:Yc.indptr[t + 1]].astype(dt)
        keep = c != 0
        s, c = s[keep], c[keep]
        order = np.argsort(-c, kind="stable")          # s ascending inside a tie: the rows of a CSC column are sorted
        s, c = s[order], c[order]
        nsupp[p] = len(s)
        m = min(M, len(s))
        src[p, :m] = s[:m]
        contrib[p, :m] = c[:m]
    return src, contrib, nsupp


def support_ref(Xq, Xs, Ys, rows, targets, M, loo=False):
    """ss_support_* in fp64 from the graph's blocks."""
    rows = np.asarray(rows, dtype=np.int64)
    uniq, slot = np.unique(rows, return_inverse=True)
    return support_lists(transfer_rows(Xq, Xs, Ys, uniq, loo=loo), slot, Ys, targets, M)
