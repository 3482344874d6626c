"""ctypes view of oracle/liboracle.so (C restatement, fp64, OpenMP) -- TEST INFRASTRUCTURE ONLY."""
import ctypes as C
import os

import numpy as np
import scipy.sparse as sp

_here = os.path.dirname(os.path.abspath(__file__))
_lib = None


def lib():
    global _lib
    if _lib is None:
        _lib = C.CDLL(os.path.join(_here, "liboracle.so"))
        _lib.oracle_predict_query.restype = C.c_int
        _lib.oracle_predict_query.argtypes = [C.c_int64] * 4 + [C.c_void_p] * 9 + [C.c_int64, C.c_int64, C.c_void_p, C.c_int]
        _lib.oracle_max_threads.restype = C.c_int
        _lib.oracle_prepare.restype = C.c_void_p
        _lib.oracle_prepare.argtypes = [C.c_int64] * 4 + [C.c_void_p] * 6
        _lib.oracle_predict_rows.restype = C.c_int
        _lib.oracle_predict_rows.argtypes = [C.c_void_p] * 4 + [C.c_int64, C.c_int64, C.c_void_p, C.c_int]
        _lib.oracle_release.restype = None
        _lib.oracle_release.argtypes = [C.c_void_p]
        if hasattr(_lib, "oracle_predict_loo_rows"):
            _lib.oracle_predict_loo_rows.restype = C.c_int
            _lib.oracle_predict_loo_rows.argtypes = ([C.c_void_p] * 7 + [C.c_int64, C.c_int64, C.c_int, C.c_void_p,
                                                     C.c_int])
    return _lib


def _need(sym):
    if not hasattr(lib(), sym):
        raise RuntimeError(f"{os.path.join(_here, 'liboracle.so')} predates {sym}: rebuild the oracle (make -C oracle)")


def _parts(m):
    m = sp.csr_matrix(m, dtype=np.float64, copy=True)   # own copies: the caller may edit its matrix in place later
    m.sum_duplicates()
    return (np.ascontiguousarray(m.indptr, np.int64), np.ascontiguousarray(m.indices, np.int32),
            np.ascontiguousarray(m.data, np.float64))


def predict_query(Xq, Xs, Ys, r0=0, r1=None, threads=0):
    nq, nf = Xq.shape
    ns, nt = Ys.shape
    r1 = nq if r1 is None else r1
    q, s, y = _parts(Xq), _parts(Xs), _parts(Ys)
    out = np.zeros((r1 - r0, nt))
    rc = lib().oracle_predict_query(nq, ns, nf, nt, q[0].ctypes.data, q[1].ctypes.data, q[2].ctypes.data,
                                    s[0].ctypes.data, s[1].ctypes.data, s[2].ctypes.data, y[0].ctypes.data,
                                    y[1].ctypes.data, y[2].ctypes.data, r0, r1, out.ctypes.data, threads)
    assert rc == 0
    return out


class Prepared:
    """The graph-dependent part (transposes, reciprocal degrees) built once; predict() then times the prediction
    only -- what bench.py's cpu_baseline measures beside a GPU path whose operands are already resident."""

    def __init__(self, Xq, Xs, Ys):
        self.nq, self.nf = Xq.shape
        self.ns, self.nt = Ys.shape
        self._q = _parts(Xq)
        s, y = _parts(Xs), _parts(Ys)
        self._h = lib().oracle_prepare(self.nq, self.ns, self.nf, self.nt, s[0].ctypes.data, s[1].ctypes.data,
                                       s[2].ctypes.data, y[0].ctypes.data, y[1].ctypes.data, y[2].ctypes.data)
        assert self._h

    def predict(self, r0=0, r1=None, threads=0, out=None):
        r1 = self.nq if r1 is None else r1
        if out is None:
            out = np.empty((r1 - r0, self.nt))
        q = self._q
        rc = lib().oracle_predict_rows(self._h, q[0].ctypes.data, q[1].ctypes.data, q[2].ctypes.data, r0, r1,
                                       out.ctypes.data, threads)
        assert rc == 0
        return out

    def close(self):
        if self._h:
            lib().oracle_release(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class PreparedLoo:
    """Leave-one-out form (oracle_predict_loo_rows): ``X`` the square featurized similarity (column j = the feature named
    after source j), ``Y`` the source x target labels.  Row i of predict(i0, i1) equals row i of
    simspread_oracle.predict_loo_factored(X, Y, clean); one prepared graph serves any number of row blocks."""

    def __init__(self, X, Y):
        _need("oracle_predict_loo_rows")
        self.n = X.shape[0]
        if X.shape != (self.n, self.n) or Y.shape[0] != self.n:
            raise ValueError("X must be square with one row per source of Y")
        self.nt = Y.shape[1]
        self._x, self._y = _parts(X), _parts(Y)
        x, y = self._x, self._y
        self._h = lib().oracle_prepare(0, self.n, self.n, self.nt, x[0].ctypes.data, x[1].ctypes.data, x[2].ctypes.data,
                                       y[0].ctypes.data, y[1].ctypes.data, y[2].ctypes.data)
        assert self._h

    def predict(self, i0=0, i1=None, clean=False, threads=0, out=None):
        i1 = self.n if i1 is None else i1
        if not 0 <= i0 <= i1 <= self.n:
            raise ValueError(f"row block [{i0}, {i1}) outside [0, {self.n})")
        if out is None:
            out = np.empty((i1 - i0, self.nt))
        assert out.shape == (i1 - i0, self.nt) and out.dtype == np.float64 and out.flags.c_contiguous
        x, y = self._x, self._y
        rc = lib().oracle_predict_loo_rows(self._h, x[0].ctypes.data, x[1].ctypes.data, x[2].ctypes.data,
                                           y[0].ctypes.data, y[1].ctypes.data, y[2].ctypes.data, i0, i1,
                                           1 if clean else 0, out.ctypes.data, threads)
        assert rc == 0, rc
        return out

    close = Prepared.close
    __del__ = Prepared.__del__


def predict_loo(X, Y, i0=0, i1=None, clean=False, threads=0):
    p = PreparedLoo(X, Y)
    try:
        return p.predict(i0, i1, clean, threads)
    finally:
        p.close()


def predict_kfold(X, Y, fold, nfolds=None, clean=False, threads=0):
    """k-fold scores, one query-form call per fold: for fold phi with members M and the rest T (sources and, by name,
    features), construct(y, X, M) (src/core.jl:148-201) leaves the bipartite blocks Xq = X[M][:, T], Xs = X[T][:, T],
    Ys = Y[T]; predict (:402-423) scores M against every target; clean! (:478-484) puts -99 where no source of T has the
    target.  Row i of the result is source i's score row in its own fold (tests/test_oracle.py pins this against the
    literal construct_queries loop)."""
    X = sp.csr_matrix(X, dtype=np.float64)
    Y = sp.csr_matrix(Y, dtype=np.float64)
    fold = np.asarray(fold)
    nfolds = int(fold.max()) + 1 if nfolds is None else nfolds
    out = np.zeros((X.shape[0], Y.shape[1]))
    for phi in range(nfolds):
        members, train = np.flatnonzero(fold == phi), np.flatnonzero(fold != phi)
        if members.size == 0:
            continue
        Xt = X[train]
        Ys = Y[train]
        rows = predict_query(X[members][:, train], Xt[:, train], Ys, threads=threads)
        if clean:
            Ys.eliminate_zeros()
            rows[:, np.diff(Ys.tocsc().indptr) == 0] = -99.0
        out[members] = rows
    return out


def max_threads():
    return lib().oracle_max_threads()
