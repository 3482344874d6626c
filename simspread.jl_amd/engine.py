"""Device handles over the C ABI: the tri-partite graph (`DeviceGraph`) and the raw W*R
operand (`DeviceSpMat`).  Inputs are numpy / scipy.sparse (host) or torch CUDA tensors
(device, passed by ``data_ptr()``); outputs are numpy arrays or, when ``out`` is a torch CUDA
tensor, written in place on the device.  Everything computes on the GPU through
libsimspread_hip.so -- nothing here falls back to the CPU.
"""
from __future__ import annotations

import ctypes as C
from typing import Optional

import numpy as np

from . import _lib as L
from . import _lib as L_


def _suffix(dtype) -> str:
    dt = np.dtype(dtype)
    if dt == np.float32:
        return "f32"
    if dt == np.float64:
        return "f64"
    raise TypeError(f"dtype {dt} not supported (float32 / float64)")


def _is_torch(x) -> bool:
    if type(x).__module__.startswith("torch"):
        L.use_torch_stream()  # order the library's kernels after the ones that produced this tensor
        return True
    return False


def _csr_parts(m, dtype, shape=None):
    """(ptr int64, idx int32, val dtype) numpy arrays of a scipy.sparse matrix, sorted indices."""
    import scipy.sparse as sp
    if m is None:
        rows = shape[0]
        return np.zeros(rows + 1, np.int64), np.zeros(0, np.int32), np.zeros(0, dtype)
    m = sp.csr_matrix(m)
    if shape is not None and m.shape != tuple(shape):
        raise ValueError(f"block has shape {m.shape}, expected {tuple(shape)}")
    if not m.has_sorted_indices:
        m = m.sorted_indices()
    m.sum_duplicates()
    return (np.ascontiguousarray(m.indptr, dtype=np.int64), np.ascontiguousarray(m.indices, dtype=np.int32),
            np.ascontiguousarray(m.data, dtype=dtype))


def _ptr(a):
    return None if a is None else a.ctypes.data


class DeviceGraph:
    """``construct(...)`` on the device: blocks Xq (nq x nf), Xs (ns x nf), Ys (ns x nt) as CSR plus
    transposes and count degrees (reference: src/core.jl:148-201,217-276,308-337,365-371)."""

    def __init__(self, handle, dtype, general=False):
        self._h = handle
        self.dtype = np.dtype(dtype)
        self._suf = _suffix(dtype)
        self.general = general
        info = (C.c_int64 * 7)()
        L.check(L.load().ss_graph_info(self._h, info))
        self.nq, self.ns, self.nf, self.nt, self.nnz_xq, self.nnz_xs, self.nnz_ys = [int(v) for v in info]

    # ---------------------------------------------------------------- constructors
    @classmethod
    def from_sparse(cls, Xq, Xs, Ys, dtype=np.float32):
        """Host CSR blocks (scipy.sparse or anything csr_matrix accepts).  Xq may be None (3-layer graph)."""
        import scipy.sparse as sp
        lib = L.lib()
        Xs = sp.csr_matrix(Xs)
        Ys = sp.csr_matrix(Ys)
        ns, nf = Xs.shape
        nt = Ys.shape[1]
        if Ys.shape[0] != ns:
            raise AssertionError("Labels and features have different number of source nodes")
        nq = 0 if Xq is None else sp.csr_matrix(Xq).shape[0]
        if Xq is not None and sp.csr_matrix(Xq).shape[1] != nf:
            raise AssertionError("Number of features between test and training sets doesn't match")
        q = _csr_parts(Xq, dtype, (nq, nf))
        s = _csr_parts(Xs, dtype, (ns, nf))
        y = _csr_parts(Ys, dtype, (ns, nt))
        h = C.c_void_p()
        fn = getattr(lib, f"ss_graph_create_csr_{_suffix(dtype)}")
        L.check(fn(nq, ns, nf, nt, _ptr(q[0]), _ptr(q[1]), _ptr(q[2]), _ptr(s[0]), _ptr(s[1]), _ptr(s[2]),
                   _ptr(y[0]), _ptr(y[1]), _ptr(y[2]), 0, L.SS_MEM_HOST, C.byref(h)))
        return cls(h, dtype)

    @classmethod
    def from_device_csr(cls, nq, ns, nf, nt, xq, xs, ys, dtype=np.float32):
        """CSR blocks that already live on the GPU: each of xq, xs, ys is a (ptr int64, idx int32, val)
        triple of torch CUDA tensors (xq may be None; a val of None means all ones)."""
        lib = L.lib()
        import torch

        def parts(t, rows):
            if t is None:
                z = torch.zeros(rows + 1, dtype=torch.int64, device="cuda")
                return z, None, None, (z,)
            ptr, idx, val = t
            _is_torch(ptr)
            want = torch.float32 if np.dtype(dtype) == np.float32 else torch.float64
            if ptr.dtype != torch.int64 or idx.dtype != torch.int32 or (val is not None and val.dtype != want):
                raise TypeError("device CSR needs int64 pointers, int32 indices and values of the graph precision")
            return ptr, idx, val, (ptr, idx, val)

        dp = lambda t: None if t is None else t.data_ptr()
        q = parts(xq, nq)
        s_ = parts(xs, ns)
        y = parts(ys, ns)
        h = C.c_void_p()
        fn = getattr(lib, f"ss_graph_create_csr_{_suffix(dtype)}")
        L.check(fn(nq, ns, nf, nt, dp(q[0]), dp(q[1]), dp(q[2]), dp(s_[0]), dp(s_[1]), dp(s_[2]),
                   dp(y[0]), dp(y[1]), dp(y[2]), 0, L.SS_MEM_DEVICE, C.byref(h)))
        return cls(h, dtype)

    @classmethod
    def from_dense(cls, Sq, Ss, Y, alpha: Optional[float] = None, weighted: bool = True, dtype=np.float32,
                   ld_pad: int = 0):
        """Dense blocks; with ``alpha`` the featurize cutoff (src/core.jl:106-112) is applied on the
        device while the CSR operands are assembled.  Arrays may be numpy (any order) or torch CUDA
        tensors; they are read as column-major (a C-order array is passed as its transpose... no copy
        is made for Fortran-order inputs).  ld_pad > 0: every block is handed over with a leading dimension of
        rows + ld_pad, the padding rows filled with NaN (a view into a larger column-major array)."""
        lib = L.lib()
        dt = np.dtype(dtype)

        def prep(a, rows_expected=None):
            # returns (pointer, ld, rows, cols, mem, keepalive) for a column-major view
            if a is None:
                return None, 1, 0, None, L.SS_MEM_HOST, None
            if _is_torch(a):
                import torch
                want = torch.float32 if dt == np.float32 else torch.float64
                t = a.to(want)
                # column-major rows x cols == row-major cols x rows: need t.T contiguous
                tt = _padded_colmajor(t, ld_pad)
                return tt.data_ptr(), max(t.shape[0] + ld_pad, 1), t.shape[0], t.shape[1], L.SS_MEM_DEVICE, tt
            arr = np.asarray(a, dtype=dt)
            if arr.ndim != 2:
                raise ValueError("dense blocks must be matrices")
            rows, cols = arr.shape
            arr = _padded_colmajor(arr, ld_pad)
            return arr.ctypes.data, max(rows + ld_pad, 1), rows, cols, L.SS_MEM_HOST, arr

        pq, ldq, nq, nfq, memq, kq = prep(Sq)
        ps, lds, ns, nf, mems, ks_ = prep(Ss)
        py, ldy, nsy, nt, memy, ky = prep(Y)
        if nsy != ns:
            raise AssertionError("Labels and features have different number of source nodes")
        if Sq is not None and nfq != nf:
            raise AssertionError("Number of features between test and training sets doesn't match")
        mems_used = {m for m, a in ((memq, Sq), (mems, Ss), (memy, Y)) if a is not None}
        if len(mems_used) != 1:
            raise ValueError("dense blocks must all live on the host or all on the device")
        mem = mems_used.pop()
        h = C.c_void_p()
        fn = getattr(lib, f"ss_graph_create_dense_{_suffix(dtype)}")
        ctype = C.c_float if dt == np.float32 else C.c_double
        L.check(fn(nq, ns, nf, nt, pq, ldq, ps, lds, py, ldy, 0 if alpha is None else 1,
                   ctype(0.0 if alpha is None else alpha), 1 if weighted else 0, mem, C.byref(h)))
        del kq, ks_, ky
        return cls(h, dtype)

    @classmethod
    def from_similarity(cls, Sq, Ss, Y, alpha: float, weighted: bool = True, dtype=np.float32, index_base: int = 0,
                        ld_pad: int = 0):
        """Dense-similarity regime: raw similarities Sq (nq x ns, may be None) and Ss (ns x ns) stay dense on the
        device, the cutoff is applied inside the MFMA stage-1 product; Y (ns x nt) is sparse.  Ss need not be
        symmetric: element (s, f) is source s (row) against feature f (column).  dtype float32: bf16
        matrix cores on exact bf16 planes (the reference's GPU=true precision); float64: the fp64 matrix instruction
        (the reference's default precision).  Inputs: numpy arrays / scipy matrix on the host, or torch CUDA tensors
        for Sq, Ss with Y = (ptr, idx, val, nt) device CSR.  Serves predict (query / source rows), predict_loo and
        predict_kfold.  index_base and a host (ptr, idx, val, nt) tuple as for ``from_fingerprints``; ld_pad as for
        ``from_dense``."""
        import scipy.sparse as sp
        lib = L.lib()
        dev = _is_torch(Ss)
        keep = []
        dt = np.dtype(dtype).type
        if dt not in (np.float32, np.float64):
            raise TypeError("dtype must be float32 or float64")

        def dense_cm(a):
            if a is None:
                return None, 1, 0
            if dev:
                import torch
                # row-major transpose == column-major original
                t = _padded_colmajor(a.to(torch.float32 if dt == np.float32 else torch.float64), ld_pad)
                keep.append(t)
                return t.data_ptr(), max(a.shape[0] + ld_pad, 1), a.shape[0]
            rows = np.shape(a)[0]
            arr = _padded_colmajor(np.asarray(a, dtype=dt), ld_pad)
            keep.append(arr)
            return arr.ctypes.data, max(rows + ld_pad, 1), rows

        pq, ldq, nq = dense_cm(Sq)
        ps, lds, ns = dense_cm(Ss)
        if dev:
            import torch
            yp, yi, yv = Y[0], Y[1], Y[2]
            nt = int(Y[3])
            # the ABI reads raw pointers: a tensor of another type would be reinterpreted silently -- convert (and keep
            # the converted tensors alive until the constructor has copied them)
            want = torch.float32 if dt == np.float32 else torch.float64
            if not (yp.is_cuda and yi.is_cuda and (yv is None or yv.is_cuda)):
                raise TypeError("device input: Y = (ptr, idx, val, nt) must be CUDA tensors")
            yp = yp.to(torch.int64).contiguous()
            yi = yi.to(torch.int32).contiguous()
            yv = None if yv is None else yv.to(want).contiguous()
            if yp.numel() != ns + 1:
                raise AssertionError("Labels and features have different number of source nodes")
            keep.extend([yp, yi, yv])
            yptr, yidx, yval = yp.data_ptr(), yi.data_ptr(), (None if yv is None else yv.data_ptr())
            mem = L.SS_MEM_DEVICE
        else:
            yptr, yidx, yval, nt, mem = _source_labels(Y, ns, dt, False, keep, index_base)
        h = C.c_void_p()
        if dt == np.float32:
            L.check(lib.ss_graph_create_similarity_f32(nq, ns, nt, pq, ldq, ps, lds, yptr, yidx, yval, index_base,
                                                       C.c_float(alpha), 1 if weighted else 0, mem, C.byref(h)))
        else:
            L.check(lib.ss_graph_create_similarity_f64(nq, ns, nt, pq, ldq, ps, lds, yptr, yidx, yval, index_base,
                                                       C.c_double(alpha), 1 if weighted else 0, mem, C.byref(h)))
        if dev:
            L.check(lib.ss_synchronize())
        del keep
        return cls(h, dt)

    @classmethod
    def from_fingerprints(cls, Fq, Fs, Y, alpha: float, weighted: bool = True, dtype=np.float32, index_base: int = 0,
                          min_neighbours: int = 0):
        """``construct(y, X)`` with ``X = featurize(Tanimoto(F), alpha, weighted)`` for packed binary fingerprints (see
        ``pack_fingerprints``): Xq = cut(T(Fq, Fs)), Xs = cut(T(Fs, Fs)), features named after the sources, produced as
        CSR on the device (the dense similarity never exists).  Fq may be None (3-layer graph: predict_loo /
        predict_kfold).  Fq, Fs: uint64 numpy arrays (n, nwords) with Y a scipy matrix (ns x nt), or int64 torch CUDA
        tensors with Y = (ptr, idx, val, nt) device CSR.  index_base (0 or 1) is the base of the label CSR handed to the
        library: a scipy matrix is converted, a (ptr, idx, val, nt) tuple (numpy arrays on the host) is taken as it
        is.  min_neighbours = k > 0 (at most 64) adds the neighbour floor of ``tanimoto_csr``: every source and every
        query also keeps its k nearest sources (ties included), whatever alpha says; alpha = inf gives the pure k-nearest
        graph.  The graph is an ordinary CSR graph afterwards; in a leave-one-out fold the held-out source's own column
        is dropped as always, so pass k + 1 for k neighbours in every fold."""
        lib = L.lib()
        dt = np.dtype(dtype).type
        if dt not in (np.float32, np.float64):
            raise TypeError("dtype must be float32 or float64")
        dev = _is_torch(Fs)
        keep = []
        fq, nq, nwq = _fingerprints(Fq, dev, keep)
        fs, ns, nwords = _fingerprints(Fs, dev, keep)
        if Fq is not None and nwq != nwords:
            raise ValueError("Fq and Fs have different fingerprint widths")
        yptr, yidx, yval, nt, mem = _source_labels(Y, ns, dt, dev, keep, index_base)
        h = C.c_void_p()
        ctype = C.c_float if dt == np.float32 else C.c_double
        if min_neighbours:
            fn = getattr(lib, f"ss_graph_create_fingerprint_floor_{_suffix(dt)}")
            L.check(fn(nq, ns, nt, nwords, fq, fs, yptr, yidx, yval, index_base, ctype(alpha), int(min_neighbours),
                       1 if weighted else 0, mem, C.byref(h)))
        else:
            fn = getattr(lib, f"ss_graph_create_fingerprint_{_suffix(dt)}")
            L.check(fn(nq, ns, nt, nwords, fq, fs, yptr, yidx, yval, index_base, ctype(alpha), 1 if weighted else 0, mem,
                       C.byref(h)))
        if dev:
            L.check(lib.ss_synchronize())
        del keep
        return cls(h, dt)

    @classmethod
    def from_features(cls, Fq, Fs, Y, alpha: float, weighted: bool = True, dtype=np.float32, index_base: int = 0,
                      min_neighbours: int = 0):
        """``construct(y, X)`` with ``X = featurize(1 .- pairwise(Jaccard(), F, dims=1), alpha, weighted)`` for
        real-valued feature rows (the reference's tutorial, docs/src/tutorial/fishers-flowers.jl:66,95-96): Xq =
        cut(J(Fq, Fs)), Xs = cut(J(Fs, Fs)) with J the weighted Jaccard similarity of ``jaccard_csr``, features named
        after the sources, produced as CSR on the device (the dense similarity never exists).  Fq may be None (3-layer
        graph: predict_loo / predict_kfold / evaluate_loo).  Fq, Fs: (n, d) numpy arrays with Y a scipy matrix (ns x
        nt), or float CUDA tensors of the graph's dtype with Y = (ptr, idx, val, nt) device CSR.  index_base as for
        ``from_fingerprints``.  min_neighbours = k > 0 (at most 64) adds the neighbour floor of ``jaccard_csr``: every
        source and every query also keeps its k nearest sources (ties included), whatever alpha says; everything said of
        it at ``from_fingerprints`` holds here."""
        dt = _feature_dtype(dtype)
        dev = _is_torch(Fs)
        keep = []
        fq, nq, dq, ldq = _features(Fq, dt, dev, keep)
        fs, ns, d, lds = _features(Fs, dt, dev, keep)
        if Fq is not None and dq != d:
            raise ValueError("Fq and Fs have different numbers of features")
        yptr, yidx, yval, nt, mem = _source_labels(Y, ns, dt, dev, keep, index_base)
        lib = L.lib()
        h = C.c_void_p()
        ctype = C.c_float if dt == np.float32 else C.c_double
        if min_neighbours:
            fn = getattr(lib, f"ss_graph_create_features_floor_{_suffix(dt)}")
            L.check(fn(nq, ns, nt, d, fq, ldq, fs, lds, yptr, yidx, yval, index_base, ctype(alpha), int(min_neighbours),
                       1 if weighted else 0, mem, C.byref(h)))
        else:
            fn = getattr(lib, f"ss_graph_create_features_{_suffix(dt)}")
            L.check(fn(nq, ns, nt, d, fq, ldq, fs, lds, yptr, yidx, yval, index_base, ctype(alpha), 1 if weighted else 0,
                       mem, C.byref(h)))
        if dev:
            L.check(lib.ss_synchronize())
        del keep
        return cls(h, dt)

    @classmethod
    def from_vectors(cls, Fq, Fs, Y, alpha: float, metric="cosine", weighted: bool = True, dtype=np.float32,
                     index_base: int = 0, min_neighbours: int = 0, storage=None):
        """``construct(y, X)`` with ``X = featurize(S(F), alpha, weighted)``, S the inner-product similarity ``metric``
        ("cosine", "tanimoto", "dice") of ``dot_csr`` between real-valued rows (embeddings, continuous descriptors): Xq =
        cut(S(Fq, Fs)), Xs = cut(S(Fs, Fs)), features named after the sources, produced as CSR on the device (the dense
        similarity never exists).  Fq may be None (3-layer graph: predict_loo / predict_kfold / evaluate_loo).  Inputs
        as ``from_features``, min_neighbours included: the k nearest are the k largest positive similarities, so negative
        ones (signed embeddings) never count among them.

        storage "bf16" / "f16": the 16-bit route of ``dot_csr`` (inputs as there: torch.bfloat16 / torch.float16 CUDA
        tensors read in place, numpy float16, raw uint16 patterns, or real arrays rounded on the host).  The graph is an
        ordinary float32 graph afterwards.  Here 16-bit CUDA tensors must name their storage: without it they are
        refused as tensors of the wrong dtype, as before; numpy float16 arrays select "f16" as in ``dot_csr``.

        storage "i8": the exact int8 route of ``dot_csr`` (inputs as there), min_neighbours allowed; taken only when
        named.  The graph is an ordinary float32 graph afterwards."""
        if _i8_storage(storage, (Fs, Fq), dtype, min_neighbours):
            m = _sim_metric(metric)
            dev = _is_torch(Fs)
            keep = []
            fq, nq, dq, ldq = _features_i8(Fq, dev, keep)
            fs, ns, d, lds = _features_i8(Fs, dev, keep)
            if Fq is None:
                ldq = max(d, 1)
            elif dq != d:
                raise ValueError("Fq and Fs have different numbers of features")
            yptr, yidx, yval, nt, mem = _source_labels(Y, ns, np.float32, dev, keep, index_base)
            lib = L.lib()
            h = C.c_void_p()
            L.check(lib.ss_graph_create_vectors_i8(nq, ns, nt, d, m, fq, ldq, fs, lds, yptr, yidx, yval, index_base,
                                                   C.c_float(alpha), int(min_neighbours), 1 if weighted else 0, mem,
                                                   C.byref(h)))
            if dev:
                L.check(lib.ss_synchronize())
            del keep
            return cls(h, np.float32)
        code = _h16_storage(storage, (Fs, Fq), dtype, min_neighbours, auto_tensor=False)
        if code is not None:
            m = _sim_metric(metric)
            dev = _is_torch(Fs)
            keep = []
            fq, nq, dq, ldq = _features_h16(Fq, code, dev, keep)
            fs, ns, d, lds = _features_h16(Fs, code, dev, keep)
            if Fq is None:
                ldq = max(d, 1)
            elif dq != d:
                raise ValueError("Fq and Fs have different numbers of features")
            yptr, yidx, yval, nt, mem = _source_labels(Y, ns, np.float32, dev, keep, index_base)
            lib = L.lib()
            h = C.c_void_p()
            L.check(lib.ss_graph_create_vectors_h16(nq, ns, nt, d, code, m, fq, ldq, fs, lds, yptr, yidx, yval, index_base,
                                                    C.c_float(alpha), 1 if weighted else 0, mem, C.byref(h)))
            if dev:
                L.check(lib.ss_synchronize())
            del keep
            return cls(h, np.float32)
        dt = _feature_dtype(dtype)
        m = _sim_metric(metric)
        dev = _is_torch(Fs)
        keep = []
        fq, nq, dq, ldq = _features(Fq, dt, dev, keep)
        fs, ns, d, lds = _features(Fs, dt, dev, keep)
        if Fq is not None and dq != d:
            raise ValueError("Fq and Fs have different numbers of features")
        yptr, yidx, yval, nt, mem = _source_labels(Y, ns, dt, dev, keep, index_base)
        lib = L.lib()
        h = C.c_void_p()
        ctype = C.c_float if dt == np.float32 else C.c_double
        if min_neighbours:
            fn = getattr(lib, f"ss_graph_create_vectors_floor_{_suffix(dt)}")
            L.check(fn(nq, ns, nt, d, m, fq, ldq, fs, lds, yptr, yidx, yval, index_base, ctype(alpha), int(min_neighbours),
                       1 if weighted else 0, mem, C.byref(h)))
        else:
            fn = getattr(lib, f"ss_graph_create_vectors_{_suffix(dt)}")
            L.check(fn(nq, ns, nt, d, m, fq, ldq, fs, lds, yptr, yidx, yval, index_base, ctype(alpha),
                       1 if weighted else 0, mem,
                       C.byref(h)))
        if dev:
            L.check(lib.ss_synchronize())
        del keep
        return cls(h, dt)

    @classmethod
    def general(cls, A_rows, B, B_cols_T, dtype=np.float64):
        """predict for caller-built A, B (src/core.jl:402-425): A_rows = A[rows, :], B, B_cols_T = B[:, cols]'."""
        import scipy.sparse as sp
        lib = L.lib()
        A_rows, B, Wt = sp.csr_matrix(A_rows), sp.csr_matrix(B), sp.csr_matrix(B_cols_T)
        n = B.shape[0]
        if B.shape[1] != n or A_rows.shape[1] != n or Wt.shape[1] != n:
            raise ValueError("general graph: inconsistent shapes")
        l, b, w = _csr_parts(A_rows, dtype), _csr_parts(B, dtype), _csr_parts(Wt, dtype)
        h = C.c_void_p()
        fn = getattr(lib, f"ss_graph_create_general_{_suffix(dtype)}")
        L.check(fn(n, A_rows.shape[0], Wt.shape[0], _ptr(l[0]), _ptr(l[1]), _ptr(l[2]), _ptr(b[0]), _ptr(b[1]),
                   _ptr(b[2]), _ptr(w[0]), _ptr(w[1]), _ptr(w[2]), 0, L.SS_MEM_HOST, C.byref(h)))
        return cls(h, dtype, general=True)

    # ---------------------------------------------------------------- queries
    def degrees(self):
        """(kf, ks, kt): count degrees of the query-free graph B (src/graphs.jl:9-11, src/core.jl:366)."""
        kf, ks, kt = (np.zeros(n, np.int64) for n in (self.nf, self.ns, self.nt))
        L.check(L.lib().ss_graph_degrees(self._h, _ptr(kf), _ptr(ks), _ptr(kt)))
        return kf, ks, kt

    def _run(self, fn_name, head_args, nrows, clean, out, layout):
        lib = L.lib()
        colmajor = (layout == "col")
        lay = L.SS_LAYOUT_COLMAJOR if colmajor else L.SS_LAYOUT_ROWMAJOR
        shape = (self.nt, nrows) if colmajor else (nrows, self.nt)  # as a C-order buffer
        if out is None:
            out = np.empty(shape, dtype=self.dtype)
        if _is_torch(out):
            if tuple(out.shape) != shape or not out.is_contiguous() or not out.is_cuda:
                raise ValueError(f"out must be a contiguous CUDA tensor of shape {shape}")
            if np.dtype(str(out.dtype).replace("torch.", "")) != self.dtype:
                raise TypeError("out dtype does not match the graph precision")
            ptr, mem = out.data_ptr(), L.SS_MEM_DEVICE
        else:
            if out.shape != shape or out.dtype != self.dtype or not out.flags.c_contiguous:
                raise ValueError(f"out must be a C-contiguous {self.dtype} array of shape {shape}")
            ptr, mem = out.ctypes.data, L.SS_MEM_HOST
        fn = getattr(lib, f"{fn_name}_{self._suf}")
        L.check(fn(self._h, *head_args, 1 if clean else 0, ptr, shape[1], lay, mem))
        if colmajor and not _is_torch(out):
            return out.T  # (nrows, nt) view, Fortran order -- what a Julia caller sees
        return out

    def predict(self, rows: str = "query", row_begin: int = 0, row_end: Optional[int] = None, clean: bool = False,
                out=None, layout: str = "row", queries: Optional["DeviceQueries"] = None):
        """Scores of rows [row_begin,row_end) of the query (or source) nodes against all targets
        (predict, src/core.jl:402-425,446-466; clean! fused, src/core.jl:478-484).  queries: a ``DeviceQueries`` bound
        to this graph whose rows are scored instead of the graph's own query block (ss_predict_queries_*): bitwise what
        the graph built with those queries gives."""
        if queries is not None:
            if rows != "query":
                raise ValueError("a query set has query rows only")
            row_end = queries.nq if row_end is None else row_end
            return self._run("ss_predict_queries", (queries._h, row_begin, row_end), row_end - row_begin, clean, out,
                             layout)
        kind = {"query": L.SS_ROWS_QUERY, "source": L.SS_ROWS_SOURCE}[rows]
        limit = self.nq if rows == "query" else self.ns
        row_end = limit if row_end is None else row_end
        return self._run("ss_predict", (kind, row_begin, row_end), row_end - row_begin, clean, out, layout)

    def predict_loo(self, i_begin: int = 0, i_end: Optional[int] = None, clean: bool = False, out=None,
                    layout: str = "row"):
        """Leave-one-out: row i = predict(construct(y, X, [source_i]), y[[source_i], :])."""
        i_end = self.ns if i_end is None else i_end
        return self._run("ss_predict_loo", (i_begin, i_end), i_end - i_begin, clean, out, layout)

    def predict_kfold(self, fold_of_source, nfolds: Optional[int] = None, clean: bool = False):
        """All folds of a k-fold cross-validation in one call: row i = the scores of source i when its fold is
        held out (construct(y, X, members) + predict (+ clean!) for every fold).  Returns (ns, nt) numpy."""
        fold = np.ascontiguousarray(fold_of_source, dtype=np.int32)
        if fold.shape != (self.ns,):
            raise ValueError("fold_of_source must have one entry per source")
        nfolds = int(fold.max()) + 1 if nfolds is None else nfolds
        out = np.empty((self.ns, self.nt), dtype=self.dtype)
        fn = getattr(L.lib(), f"ss_predict_kfold_{self._suf}")
        L.check(fn(self._h, fold.ctypes.data, nfolds, 1 if clean else 0, out.ctypes.data, self.nt,
                   L.SS_LAYOUT_ROWMAJOR, L.SS_MEM_HOST))
        return out

    def evaluate_loo(self, i_begin: int = 0, i_end: Optional[int] = None, clean: bool = False, alpha: float = 20.0,
                     L: int = 20, block_rows: int = 0):
        """The leave-one-out folds [i_begin, i_end) ranked against the graph's own labels without the scores leaving the
        device: row i - i_begin = rank_metrics_rows(Ys[i, :], predict_loo(i)).  Returns (n, 6) float64 numpy, columns
        RANK_ROWS_FIELDS.  block_rows: folds per device block (0: the library's choice, about 1 GiB of scores)."""
        i_end = self.ns if i_end is None else i_end
        n = max(i_end - i_begin, 0)
        _check_L(self.nt, L)
        out = np.empty((n, len(RANK_ROWS_FIELDS)), np.float64)
        fn = getattr(L_.lib(), f"ss_evaluate_loo_{self._suf}")
        L_.check(fn(self._h, i_begin, i_end, 1 if clean else 0, float(alpha), int(L), int(block_rows), out.ctypes.data,
                    L_.SS_MEM_HOST))
        return out

    def evaluate_loo_binary(self, i_begin: int = 0, i_end: Optional[int] = None, clean: bool = False,
                            block_rows: int = 0):
        """The leave-one-out folds [i_begin, i_end) judged by the binary prediction metrics against the graph's own
        labels without the scores leaving the device: row i - i_begin = binary_metrics_rows(Ys[i, :], predict_loo(i)).
        Returns (n, 18) float64 numpy, columns BINARY_ROWS_FIELDS.  block_rows: folds per device block (0: the
        library's choice, about 1 GiB of scores)."""
        i_end = self.ns if i_end is None else i_end
        n = max(i_end - i_begin, 0)
        out = np.empty((n, len(BINARY_ROWS_FIELDS)), np.float64)
        fn = getattr(L_.lib(), f"ss_evaluate_loo_binary_{self._suf}")
        L_.check(fn(self._h, i_begin, i_end, 1 if clean else 0, int(block_rows), out.ctypes.data, L_.SS_MEM_HOST))
        return out

    def _folds(self, fold_of_source, nfolds):
        """(int32 numpy fold ids, nfolds) of a k-fold assignment; shape and dtype are checked here, the ids themselves by
        the library (an id outside 0..nfolds-1 is SS_EINVAL there, before anything is written)."""
        if type(fold_of_source).__module__.startswith("torch"):
            fold_of_source = fold_of_source.detach().cpu().numpy()
        a = np.asarray(fold_of_source)
        if a.shape != (self.ns,):
            raise ValueError(f"fold_of_source has shape {a.shape}, expected one entry per source ({self.ns},)")
        if a.dtype.kind not in "iu":
            raise ValueError(f"fold_of_source must hold integer fold ids, not {a.dtype}")
        if a.size and (int(a.min()) < -(1 << 31) or int(a.max()) >= (1 << 31)):
            raise ValueError("fold ids must fit in int32")
        fold = np.ascontiguousarray(a, dtype=np.int32)
        nfolds = (int(fold.max()) + 1 if fold.size else 1) if nfolds is None else int(nfolds)
        return fold, nfolds

    def predict_kfold_rows(self, fold_of_source, nfolds: Optional[int] = None, i_begin: int = 0,
                           i_end: Optional[int] = None, clean: bool = False, out=None, layout: str = "row"):
        """Rows [i_begin, i_end) (source order) of predict_kfold: row i - i_begin is bitwise row i of the whole sweep,
        so a k-fold run shards across ranks by row range like predict_loo.  `out` as for predict_loo (numpy, or a CUDA
        tensor filled in place; layout "row" or "col")."""
        fold, nfolds = self._folds(fold_of_source, nfolds)
        i_end = self.ns if i_end is None else i_end
        keep = fold
        if _is_torch(out):
            import torch
            keep = torch.from_numpy(fold).to(out.device)
        ptr = keep.data_ptr() if _is_torch(keep) else keep.ctypes.data
        return self._run("ss_predict_kfold_rows", (ptr, nfolds, i_begin, i_end), max(i_end - i_begin, 0), clean, out,
                         layout)

    def evaluate_kfold(self, fold_of_source, nfolds: Optional[int] = None, i_begin: int = 0,
                       i_end: Optional[int] = None, clean: bool = False, alpha: float = 20.0, L: int = 20,
                       block_rows: int = 0):
        """The k-fold rows [i_begin, i_end) ranked against the graph's own labels without the scores leaving the
        device: row i - i_begin = rank_metrics_rows(Ys[i, :], predict_kfold_rows(i)).  Returns (n, 6) float64 numpy,
        columns RANK_ROWS_FIELDS.  block_rows: members per device block (0: the library's choice, about 1 GiB of
        scores)."""
        fold, nfolds = self._folds(fold_of_source, nfolds)
        i_end = self.ns if i_end is None else i_end
        n = max(i_end - i_begin, 0)
        _check_L(self.nt, L)
        out = np.empty((n, len(RANK_ROWS_FIELDS)), np.float64)
        fn = getattr(L_.lib(), f"ss_evaluate_kfold_{self._suf}")
        L_.check(fn(self._h, fold.ctypes.data, nfolds, i_begin, i_end, 1 if clean else 0, float(alpha), int(L),
                    int(block_rows), out.ctypes.data, L_.SS_MEM_HOST))
        return out

    def evaluate_kfold_binary(self, fold_of_source, nfolds: Optional[int] = None, i_begin: int = 0,
                              i_end: Optional[int] = None, clean: bool = False, block_rows: int = 0):
        """The k-fold rows [i_begin, i_end) judged by the binary prediction metrics against the graph's own labels
        without the scores leaving the device: row i - i_begin = binary_metrics_rows(Ys[i, :], predict_kfold_rows(i)).
        Returns (n, 18) float64 numpy, columns BINARY_ROWS_FIELDS.  block_rows as for evaluate_kfold."""
        fold, nfolds = self._folds(fold_of_source, nfolds)
        i_end = self.ns if i_end is None else i_end
        n = max(i_end - i_begin, 0)
        out = np.empty((n, len(BINARY_ROWS_FIELDS)), np.float64)
        fn = getattr(L_.lib(), f"ss_evaluate_kfold_binary_{self._suf}")
        L_.check(fn(self._h, fold.ctypes.data, nfolds, i_begin, i_end, 1 if clean else 0, int(block_rows),
                    out.ctypes.data, L_.SS_MEM_HOST))
        return out

    def evaluate_loo_pooled(self, i_begin: int = 0, i_end: Optional[int] = None, clean: bool = False,
                            block_rows: int = 0) -> dict:
        """The leave-one-out folds [i_begin, i_end) judged pooled, as the reference's AuROC(vec(y), vec(yhat)) and
        maxperformance(vec(y), vec(yhat), f) judge a whole matrix: Pool(...).add_loo(self, ...).metrics()."""
        p = Pool(self.dtype)
        try:
            return p.add_loo(self, i_begin, i_end, clean=clean, block_rows=block_rows).metrics()
        finally:
            p.close()

    def evaluate_kfold_pooled(self, fold_of_source, nfolds: Optional[int] = None, i_begin: int = 0,
                              i_end: Optional[int] = None, clean: bool = False, block_rows: int = 0) -> dict:
        """The k-fold rows [i_begin, i_end) judged pooled: Pool(...).add_kfold(self, ...).metrics()."""
        p = Pool(self.dtype)
        try:
            return p.add_kfold(self, fold_of_source, nfolds, i_begin, i_end, clean=clean,
                               block_rows=block_rows).metrics()
        finally:
            p.close()

    def evaluate_loo_targets(self, i_begin: int = 0, i_end: Optional[int] = None, clean: bool = False,
                             alpha: float = 20.0, L: int = 20, block_rows: int = 0) -> np.ndarray:
        """The leave-one-out folds [i_begin, i_end) judged per target: row t = rank_metrics_rows of column t of
        predict_loo against column t of the labels, ties by fold index.  Two sweeps (TargetRank: collect, seal, count);
        no score leaves the device.  Returns (nt, 6) float64 numpy, columns TARGET_RANK_FIELDS."""
        h = TargetRank(self.nt, self.dtype)
        try:
            h.add_loo(self, i_begin, i_end, clean=clean, block_rows=block_rows).seal()
            return h.add_loo(self, i_begin, i_end, clean=clean, block_rows=block_rows).metrics(alpha, L)
        finally:
            h.close()

    def evaluate_kfold_targets(self, fold_of_source, nfolds: Optional[int] = None, i_begin: int = 0,
                               i_end: Optional[int] = None, clean: bool = False, alpha: float = 20.0, L: int = 20,
                               block_rows: int = 0) -> np.ndarray:
        """The k-fold rows [i_begin, i_end) judged per target, as evaluate_loo_targets judges the leave-one-out folds."""
        h = TargetRank(self.nt, self.dtype)
        try:
            h.add_kfold(self, fold_of_source, nfolds, i_begin, i_end, clean=clean, block_rows=block_rows).seal()
            return h.add_kfold(self, fold_of_source, nfolds, i_begin, i_end, clean=clean,
                               block_rows=block_rows).metrics(alpha, L)
        finally:
            h.close()

    def support(self, rows, targets, M: int = 16, queries: Optional["DeviceQueries"] = None, loo: bool = False):
        """Which sources carry the scores of the (row, target) pairs ``zip(rows, targets)`` (ss_support_*): returns
        ``(src, contrib, nsupp)`` with src, contrib of shape (npairs, M) -- the sources s with the largest contributions
        ``T[r,s] * Ys[s,t]`` in descending order (ties by ascending s; unused slots -1 / 0) -- and nsupp[p] the number of
        sources that contribute at all.  rows are query rows of ``queries`` (a ``DeviceQueries`` of this graph), of the
        graph's own query block, or with ``loo=True`` leave-one-out folds.  numpy in, numpy out; CUDA tensors (int64
        rows, int32 targets) in, CUDA tensors out."""
        lib = L.lib()
        kind = L.SS_ROWS_LOO if loo else L.SS_ROWS_QUERY
        qh = None if queries is None else queries._h
        fn = getattr(lib, f"ss_support_{self._suf}")
        M = int(M)
        if _is_torch(rows):
            import torch
            r = rows.to(torch.int64).contiguous()
            t = targets.to(torch.int32).contiguous()
            if r.ndim != 1 or r.shape != t.shape or not (r.is_cuda and t.is_cuda):
                raise ValueError("rows and targets must be 1-D CUDA tensors of one length")
            n = int(r.numel())
            m = max(M, 1)
            src = torch.empty((n, m), dtype=torch.int32, device=r.device)
            con = torch.empty((n, m), dtype=torch.float32 if self._suf == "f32" else torch.float64, device=r.device)
            cnt = torch.empty(n, dtype=torch.int32, device=r.device)
            L.check(fn(self._h, qh, kind, n, r.data_ptr(), t.data_ptr(), M, src.data_ptr(), con.data_ptr(),
                       cnt.data_ptr(), L.SS_MEM_DEVICE))
            return src, con, cnt
        r = np.ascontiguousarray(rows, dtype=np.int64)
        t = np.ascontiguousarray(targets, dtype=np.int32)
        if r.ndim != 1 or r.shape != t.shape:
            raise ValueError("rows and targets must be 1-D arrays of one length")
        n = r.shape[0]
        m = max(M, 1)
        src = np.empty((n, m), np.int32)
        con = np.empty((n, m), self.dtype)
        cnt = np.empty(n, np.int32)
        L.check(fn(self._h, qh, kind, n, _ptr(r), _ptr(t), M, _ptr(src), _ptr(con), _ptr(cnt), L.SS_MEM_HOST))
        return src, con, cnt

    # ---------------------------------------------------------------- cutoff sweeps
    def _ctype(self):
        return C.c_float if self.dtype == np.float32 else C.c_double

    def recut(self, alpha: float, weighted: bool = True) -> "DeviceGraph":
        """A new, independent graph equal to this one with Xq, Xs replaced by ``featurize(X, alpha, weighted)`` of the
        blocks resident on the device (two streaming passes; no producer, no sort, nothing re-read from the caller).
        For a parent built weighted at a cutoff a0 > 0 and alpha >= a0 the child is bitwise the graph the parent's own
        constructor builds at (alpha, weighted): build one parent at the lowest cutoff of a sweep and cut the rest from
        it.  The parent stays usable and may be closed first.  Dense-similarity graphs use ``set_cutoff``."""
        h = C.c_void_p()
        fn = getattr(L.lib(), f"ss_graph_recut_{self._suf}")
        L.check(fn(self._h, self._ctype()(alpha), 1 if weighted else 0, C.byref(h)))
        return DeviceGraph(h, self.dtype)

    def set_cutoff(self, alpha: float, weighted: bool = True) -> "DeviceGraph":
        """Dense-similarity graphs (``from_similarity``): move the cutoff in place.  The raw similarities stay resident,
        only (alpha, weighted), the degrees and the cached operand planes change; afterwards the graph behaves bitwise
        like a fresh ``from_similarity`` at (alpha, weighted).  alpha may go down as well as up.  Returns self."""
        fn = getattr(L.lib(), f"ss_graph_set_cutoff_{self._suf}")
        L.check(fn(self._h, self._ctype()(alpha), 1 if weighted else 0))
        return self

    def close(self):
        if self._h is not None and self._h.value:
            L.load().ss_graph_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class DeviceQueries:
    """A block of query rows bound to one resident ``DeviceGraph`` (ss_queries_*): screen new batches on the graph that
    was built and cross-validated once.  ``g.predict(queries=q)`` gives bitwise the scores of the graph built with these
    queries; creating, using and closing query sets leaves every result of the graph itself unchanged.  The
    constructors mirror the graph's: ``from_sparse`` takes the (nq, nf) block itself, the others cut the cross block of
    raw query data against the sources ``Fs`` -- pass the Fs, alpha, weighted (and metric) the graph was built with."""

    def __init__(self, handle, graph: DeviceGraph):
        self._h = handle
        self.dtype = graph.dtype
        info = (C.c_int64 * 3)()
        L.check(L.load().ss_queries_info(self._h, info))
        self.nq, self.nf, self.nnz = [int(v) for v in info]

    @classmethod
    def from_sparse(cls, graph: DeviceGraph, Xq, index_base: int = 0):
        """Xq: a scipy matrix (nq, nf) (converted to ``index_base``), or a (ptr int64, idx int32, val, nq) CSR tuple of
        numpy arrays or CUDA tensors that already has that base (val None: all ones)."""
        lib = L.lib()
        dt = graph.dtype.type
        keep = []
        if isinstance(Xq, tuple):
            ptr, idx, val, nq = Xq
            if _is_torch(ptr):
                import torch
                want = torch.float32 if dt == np.float32 else torch.float64
                ptr, idx = ptr.to(torch.int64).contiguous(), idx.to(torch.int32).contiguous()
                val = None if val is None else val.to(want).contiguous()
                keep.extend([ptr, idx, val])
                args = (ptr.data_ptr(), idx.data_ptr(), None if val is None else val.data_ptr())
                mem = L.SS_MEM_DEVICE
            else:
                parts = (np.ascontiguousarray(ptr, dtype=np.int64), np.ascontiguousarray(idx, dtype=np.int32),
                         None if val is None else np.ascontiguousarray(val, dtype=dt))
                keep.append(parts)
                args = (_ptr(parts[0]), _ptr(parts[1]), _ptr(parts[2]))
                mem = L.SS_MEM_HOST
        else:
            import scipy.sparse as sp
            Xq = sp.csr_matrix(Xq)
            if Xq.shape[1] != graph.nf:
                raise AssertionError("Number of features between test and training sets doesn't match")
            nq = Xq.shape[0]
            parts = _csr_parts(Xq, dt)
            if index_base:
                parts = (parts[0] + index_base, parts[1] + np.int32(index_base), parts[2])
            keep.append(parts)
            args = (_ptr(parts[0]), _ptr(parts[1]), _ptr(parts[2]))
            mem = L.SS_MEM_HOST
        h = C.c_void_p()
        fn = getattr(lib, f"ss_queries_create_csr_{_suffix(dt)}")
        L.check(fn(graph._h, int(nq), *args, int(index_base), mem, C.byref(h)))
        if mem == L.SS_MEM_DEVICE:
            L.check(lib.ss_synchronize())
        del keep
        return cls(h, graph)

    @classmethod
    def from_fingerprints(cls, graph: DeviceGraph, Fq, Fs, alpha: float, weighted: bool = True, min_neighbours: int = 0):
        """Xq = cut(Tanimoto(Fq, Fs)) as ``DeviceGraph.from_fingerprints`` stores it; inputs as there.  min_neighbours =
        k > 0: every query also keeps its k nearest sources (ties included), so ``degrees()`` is at least k for a query
        with k positive similarities; the graph may be a plain or a floor graph."""
        lib = L.lib()
        dt = graph.dtype.type
        dev = _is_torch(Fs)
        keep = []
        fq, nq, nwq = _fingerprints(Fq, dev, keep)
        fs, ns, nwords = _fingerprints(Fs, dev, keep)
        if Fq is not None and nwq != nwords:
            raise ValueError("Fq and Fs have different fingerprint widths")
        h = C.c_void_p()
        mem = L.SS_MEM_DEVICE if dev else L.SS_MEM_HOST
        if min_neighbours:
            fn = getattr(lib, f"ss_queries_create_fingerprint_floor_{_suffix(dt)}")
            L.check(fn(graph._h, nq, ns, nwords, fq, fs, graph._ctype()(alpha), int(min_neighbours), 1 if weighted else 0,
                       mem, C.byref(h)))
        else:
            fn = getattr(lib, f"ss_queries_create_fingerprint_{_suffix(dt)}")
            L.check(fn(graph._h, nq, ns, nwords, fq, fs, graph._ctype()(alpha), 1 if weighted else 0, mem, C.byref(h)))
        if dev:
            L.check(lib.ss_synchronize())
        del keep
        return cls(h, graph)

    @classmethod
    def _from_rows(cls, name, graph, Fq, Fs, mid, alpha, weighted, min_neighbours=0):
        lib = L.lib()
        dt = graph.dtype.type
        dev = _is_torch(Fs)
        keep = []
        fq, nq, dq, ldq = _features(Fq, dt, dev, keep)
        fs, ns, d, lds = _features(Fs, dt, dev, keep)
        if Fq is not None and dq != d:
            raise ValueError("Fq and Fs have different numbers of features")
        h = C.c_void_p()
        floor = (int(min_neighbours),) if min_neighbours else ()       # the floor entry points take k after alpha
        fn = getattr(lib, f"ss_queries_create_{name}{'_floor' if floor else ''}_{_suffix(dt)}")
        L.check(fn(graph._h, nq, ns, d, *mid, fq, ldq, fs, lds, graph._ctype()(alpha), *floor, 1 if weighted else 0,
                   L.SS_MEM_DEVICE if dev else L.SS_MEM_HOST, C.byref(h)))
        if dev:
            L.check(lib.ss_synchronize())
        del keep
        return cls(h, graph)

    @classmethod
    def from_features(cls, graph: DeviceGraph, Fq, Fs, alpha: float, weighted: bool = True, min_neighbours: int = 0):
        """Xq = cut(J(Fq, Fs)), the weighted Jaccard block of ``DeviceGraph.from_features``; inputs as there.
        min_neighbours = k > 0: every query also keeps its k nearest sources, as ``from_fingerprints``."""
        return cls._from_rows("features", graph, Fq, Fs, (), alpha, weighted, min_neighbours)

    @classmethod
    def from_vectors(cls, graph: DeviceGraph, Fq, Fs, alpha: float, metric="cosine", weighted: bool = True,
                     min_neighbours: int = 0, storage=None):
        """Xq = cut(S(Fq, Fs)), the inner-product block of ``DeviceGraph.from_vectors``; inputs as there.
        min_neighbours = k > 0: every query also keeps its k nearest sources, as ``from_fingerprints``.
        storage "bf16" / "f16" (or 16-bit CUDA tensors, by their dtype; numpy float16 as in ``dot_csr``): the 16-bit route of ``dot_csr``,
        on a float32 graph built by any constructor.  storage "i8": the exact int8 route, min_neighbours allowed."""
        if _i8_storage(storage, (Fs, Fq), graph.dtype, min_neighbours):
            m = _sim_metric(metric)
            dev = _is_torch(Fs)
            keep = []
            fq, nq, dq, ldq = _features_i8(Fq, dev, keep)
            fs, ns, d, lds = _features_i8(Fs, dev, keep)
            if Fq is None:
                ldq = max(d, 1)
            elif dq != d:
                raise ValueError("Fq and Fs have different numbers of features")
            lib = L.lib()
            h = C.c_void_p()
            L.check(lib.ss_queries_create_vectors_i8(graph._h, nq, ns, d, m, fq, ldq, fs, lds, C.c_float(alpha),
                                                     int(min_neighbours), 1 if weighted else 0,
                                                     L.SS_MEM_DEVICE if dev else L.SS_MEM_HOST, C.byref(h)))
            if dev:
                L.check(lib.ss_synchronize())
            del keep
            return cls(h, graph)
        code = _h16_storage(storage, (Fs, Fq), graph.dtype, min_neighbours)
        if code is not None:
            m = _sim_metric(metric)
            dev = _is_torch(Fs)
            keep = []
            fq, nq, dq, ldq = _features_h16(Fq, code, dev, keep)
            fs, ns, d, lds = _features_h16(Fs, code, dev, keep)
            if Fq is None:
                ldq = max(d, 1)
            elif dq != d:
                raise ValueError("Fq and Fs have different numbers of features")
            lib = L.lib()
            h = C.c_void_p()
            L.check(lib.ss_queries_create_vectors_h16(graph._h, nq, ns, d, code, m, fq, ldq, fs, lds, C.c_float(alpha),
                                                      1 if weighted else 0, L.SS_MEM_DEVICE if dev else L.SS_MEM_HOST,
                                                      C.byref(h)))
            if dev:
                L.check(lib.ss_synchronize())
            del keep
            return cls(h, graph)
        return cls._from_rows("vectors", graph, Fq, Fs, (_sim_metric(metric),), alpha, weighted, min_neighbours)

    def degrees(self) -> np.ndarray:
        """Stored entries of every query row: 0 = no source is similar enough (outside the applicability domain)."""
        kq = np.zeros(self.nq, np.int64)
        L.check(L.lib().ss_queries_degrees(self._h, _ptr(kq), L.SS_MEM_HOST))
        return kq

    def close(self):
        if self._h is not None and self._h.value:
            L.load().ss_queries_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def _padded_colmajor(a, ld_pad):
    """The column-major copy of a matrix (numpy array or CUDA tensor) the dense entry points read, with ld_pad rows of
    NaN under the last row: a Fortran-order numpy array, or the row-major transpose as a tensor."""
    if type(a).__module__.startswith("torch"):
        import torch
        if ld_pad <= 0:
            return a.t().contiguous()
        t = torch.full((a.shape[1], a.shape[0] + ld_pad), float("nan"), dtype=a.dtype, device=a.device)
        t[:, :a.shape[0]] = a.t()
        return t
    if ld_pad <= 0:
        return np.asfortranarray(a)
    buf = np.full((a.shape[0] + ld_pad, a.shape[1]), np.nan, dtype=a.dtype, order="F")
    buf[:a.shape[0]] = a
    return buf


def _source_labels(Y, ns, dt, dev, keep, index_base=0):
    """(ptr, idx, val, nt, mem) of the source labels of a graph built from raw data: a scipy matrix (ns x nt) on the
    host, or (ptr, idx, val, nt) device CSR tensors (converted to the ABI's types and kept alive in ``keep``).  A CSR
    tuple (device tensors, or numpy arrays on the host) is taken as it is and must already have the base index_base; a
    scipy matrix is shifted to it."""
    if dev:
        import torch
        want = torch.float32 if dt == np.float32 else torch.float64
        yp, yi, yv, nt = Y[0].to(torch.int64).contiguous(), Y[1].to(torch.int32).contiguous(), Y[2], int(Y[3])
        yv = None if yv is None else yv.to(want).contiguous()
        if yp.numel() != ns + 1:
            raise AssertionError("Labels and features have different number of source nodes")
        keep.extend([yp, yi, yv])
        return yp.data_ptr(), yi.data_ptr(), (None if yv is None else yv.data_ptr()), nt, L.SS_MEM_DEVICE
    if isinstance(Y, tuple):
        parts = (np.ascontiguousarray(Y[0], dtype=np.int64), np.ascontiguousarray(Y[1], dtype=np.int32),
                 None if Y[2] is None else np.ascontiguousarray(Y[2], dtype=dt))
        if parts[0].shape != (ns + 1,):
            raise AssertionError("Labels and features have different number of source nodes")
        keep.append(parts)
        return _ptr(parts[0]), _ptr(parts[1]), _ptr(parts[2]), int(Y[3]), L.SS_MEM_HOST
    import scipy.sparse as sp
    Y = sp.csr_matrix(Y)
    if Y.shape[0] != ns:
        raise AssertionError("Labels and features have different number of source nodes")
    parts = _csr_parts(Y, dt)
    if index_base:
        parts = (parts[0] + index_base, parts[1] + np.int32(index_base), parts[2])
    keep.append(parts)
    return _ptr(parts[0]), _ptr(parts[1]), _ptr(parts[2]), Y.shape[1], L.SS_MEM_HOST


class DeviceSpMat:
    """The sparse operand W of F = W*R on the device (CSR; cut into LDS-tile form on first wide use)."""

    def __init__(self, W, dtype=np.float32):
        import scipy.sparse as sp
        lib = L.lib()
        W = sp.csr_matrix(W)
        self.shape = W.shape
        self.dtype = np.dtype(dtype)
        self._suf = _suffix(dtype)
        p, i, v = _csr_parts(W, dtype)
        self.nnz = int(len(i))
        self._h = C.c_void_p()
        fn = getattr(lib, f"ss_spmat_create_csr_{self._suf}")
        L.check(fn(W.shape[0], W.shape[1], _ptr(p), _ptr(i), _ptr(v), 0, L.SS_MEM_HOST, C.byref(self._h)))

    @classmethod
    def from_device_csr(cls, rows: int, cols: int, ptr, idx, val, dtype=np.float32):
        """W given as CSR torch CUDA tensors (ptr int64, idx int32, val of the precision; val None means all ones)."""
        import torch
        self = cls.__new__(cls)
        self.shape = (int(rows), int(cols))
        self.dtype = np.dtype(dtype)
        self._suf = _suffix(dtype)
        want = torch.float32 if self.dtype == np.float32 else torch.float64
        _is_torch(ptr)
        if ptr.dtype != torch.int64 or idx.dtype != torch.int32 or (val is not None and val.dtype != want):
            raise TypeError("device CSR needs int64 pointers, int32 indices and values of the matrix precision")
        self.nnz = int(idx.numel())
        self._keep = (ptr, idx, val)
        self._h = C.c_void_p()
        fn = getattr(L.lib(), f"ss_spmat_create_csr_{self._suf}")
        L.check(fn(rows, cols, ptr.data_ptr(), idx.data_ptr(), None if val is None else val.data_ptr(), 0,
                   L.SS_MEM_DEVICE, C.byref(self._h)))
        return self

    def cost(self, B: int):
        b, f = C.c_double(), C.c_double()
        L.check(L.load().ss_spmat_cost(self._h, B, C.byref(b), C.byref(f)))
        return b.value, f.value

    def spmm(self, R, out=None, colmajor: bool = False):
        """F = W @ R.  R: (K, B).  colmajor=False: R, F are C-order (K,B)/(M,B) arrays.
        colmajor=True: R is given as its transpose, a C-order (B, K) array, and F comes back as (B, M)."""
        lib = L.lib()
        M, K = self.shape
        torch_in = _is_torch(R)
        if not torch_in:
            R = np.ascontiguousarray(R, dtype=self.dtype)
        elif not R.is_contiguous():
            R = R.contiguous()
        if R.ndim == 1:
            R = R.reshape(-1, 1) if not colmajor else R.reshape(1, -1)
        if colmajor:
            B, k_in = R.shape
        else:
            k_in, B = R.shape
        if k_in != K:
            raise ValueError(f"R has {k_in} rows, W has {K} columns")
        shape = (B, M) if colmajor else (M, B)
        if out is None:
            if torch_in:
                import torch
                out = torch.empty(shape, dtype=R.dtype, device=R.device)
            else:
                out = np.empty(shape, dtype=self.dtype)
        lay = L.SS_LAYOUT_COLMAJOR if colmajor else L.SS_LAYOUT_ROWMAJOR
        if torch_in:
            rp, fp, mem = R.data_ptr(), out.data_ptr(), L.SS_MEM_DEVICE
        else:
            rp, fp, mem = R.ctypes.data, out.ctypes.data, L.SS_MEM_HOST
        fn = getattr(lib, f"ss_spmm_{self._suf}")
        L.check(fn(self._h, rp, B, R.shape[1], lay, fp, shape[1], lay, mem))
        return out

    def close(self):
        if self._h is not None and self._h.value:
            L.load().ss_spmat_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def topl(scores, L: int):
    """The L best columns of every row of a score block, in the order ``sortperm(yhat, rev=true)`` gives (score
    descending, ties by ascending column).  `scores`: C-order float32 numpy array or contiguous torch CUDA tensor
    (nrows, ncols).  Returns (idx int32 (nrows, L), val float32 (nrows, L)) of the same kind as the input."""
    lib = L_.lib()
    if _is_torch(scores):
        import torch
        if scores.dtype != torch.float32 or not scores.is_contiguous():
            raise TypeError("scores must be a contiguous float32 tensor")
        nrows, ncols = scores.shape
        idx = torch.empty((nrows, L), dtype=torch.int32, device=scores.device)
        val = torch.empty((nrows, L), dtype=torch.float32, device=scores.device)
        L_.check(lib.ss_topl_f32(scores.data_ptr(), nrows, ncols, ncols, L, idx.data_ptr(), val.data_ptr(), L_.SS_MEM_DEVICE))
        return idx, val
    a = np.ascontiguousarray(scores, dtype=np.float32)
    nrows, ncols = a.shape
    idx = np.empty((nrows, L), np.int32)
    val = np.empty((nrows, L), np.float32)
    L_.check(lib.ss_topl_f32(a.ctypes.data, nrows, ncols, ncols, L, idx.ctypes.data, val.ctypes.data, L_.SS_MEM_HOST))
    return idx, val


def rank_metrics(y, yhat, alpha: float = 20.0) -> dict:
    """AuROC, AuPRC, BEDROC(alpha) and the validity ratio of one score vector, computed on the device
    (src/performance.jl:22-89,558-560).  `y`: labels (non-zero = positive), `yhat`: float32 scores; numpy arrays
    or contiguous torch CUDA tensors (uint8 / float32) of the same length."""
    lib = L_.lib()
    out = (C.c_double * 4)()
    if _is_torch(yhat):
        import torch
        yl = y if (_is_torch(y) and y.dtype == torch.uint8) else (y != 0).to(torch.uint8)
        yl = yl.contiguous().reshape(-1)
        sc = yhat.contiguous().reshape(-1)
        if sc.dtype != torch.float32 or yl.numel() != sc.numel():
            raise TypeError("yhat must be float32 and as long as y")
        L_.check(lib.ss_rank_metrics_f32(yl.data_ptr(), sc.data_ptr(), sc.numel(), float(alpha), out, L_.SS_MEM_DEVICE))
    else:
        sc = np.ascontiguousarray(np.asarray(yhat).ravel(), dtype=np.float32)
        yl = np.ascontiguousarray((np.asarray(y).ravel() != 0).astype(np.uint8))
        if yl.size != sc.size:
            raise AssertionError("The number of scores must be equal to the number of labels")
        L_.check(lib.ss_rank_metrics_f32(yl.ctypes.data, sc.ctypes.data, sc.size, float(alpha), out, L_.SS_MEM_HOST))
    return {"AuROC": out[0], "AuPRC": out[1], "BEDROC": out[2], "validity_ratio": out[3]}


RANK_ROWS_FIELDS = ("AuROC", "AuPRC", "BEDROC", "validity_ratio", "recallatL", "precisionatL")


def _check_L(ncols: int, L: int):
    # the reference's assertions (src/performance.jl:309-312)
    if L < 1:
        raise AssertionError("Please use a list length greater than 0 (L > 0)")
    if ncols <= L:
        raise AssertionError("Number of labels is less than length (L > y)")


def _label_csr(y, nrows: int, ncols: int):
    """(ptr int64, idx int32) host arrays of a label matrix: scipy sparse (stored zeros dropped), a dense 0/1 array or a
    host (ptr, idx) pair.  Every remaining entry is a positive; the order of the indices is kept as given."""
    import scipy.sparse as sp
    if isinstance(y, tuple):
        ptr, idx = (np.ascontiguousarray(np.asarray(v), dtype=t) for v, t in zip(y, (np.int64, np.int32)))
        if ptr.shape != (nrows + 1,):
            raise ValueError(f"label row pointers have shape {ptr.shape}, expected {(nrows + 1,)}")
        return ptr, idx
    if sp.issparse(y):
        m = sp.csr_matrix(y, copy=True)
        if m.shape != (nrows, ncols):
            raise ValueError(f"labels have shape {m.shape}, scores {(nrows, ncols)}")
        m.eliminate_zeros()
        return np.ascontiguousarray(m.indptr, dtype=np.int64), np.ascontiguousarray(m.indices, dtype=np.int32)
    a = np.asarray(y)
    if a.shape != (nrows, ncols):
        raise ValueError(f"labels have shape {a.shape}, scores {(nrows, ncols)}")
    nzr, nzc = np.nonzero(a)
    ptr = np.zeros(nrows + 1, np.int64)
    np.cumsum(np.bincount(nzr, minlength=nrows), out=ptr[1:])
    return ptr, np.ascontiguousarray(nzc, dtype=np.int32)


def _check_label_order(ptr, idx, ncols: int):
    """Column indices sorted, unique and in range within every row (the library checks it again on the device)."""
    ptr = np.asarray(ptr, dtype=np.int64)
    if ptr[0] < 0 or np.any(np.diff(ptr) < 0) or ptr[-1] > np.size(idx):
        raise ValueError("label row pointers are not a 0-based CSR row pointer array")
    idx = np.asarray(idx, dtype=np.int64)[ptr[0]:ptr[-1]]    # rows of a larger CSR may start past its first entry
    ptr = ptr - ptr[0]
    if idx.size == 0:
        return
    if idx.min() < 0 or idx.max() >= ncols:
        raise ValueError("label column index out of range")
    starts = np.zeros(idx.size, bool)
    starts[ptr[:-1][np.diff(ptr) > 0]] = True
    if np.any(np.diff(idx)[~starts[1:]] <= 0):
        raise ValueError("label column indices must be sorted and unique within every row")


def rank_metrics_rows(y, yhat, alpha: float = 20.0, L: int = 20):
    """Ranking metrics of every row of a score block on the device: AuROC, AuPRC, BEDROC(alpha), validity ratio
    (src/performance.jl:22-89,558-560), recall@L and precision@L (src/performance.jl:308-385), one row each, columns in
    RANK_ROWS_FIELDS.  `yhat`: (nrows, ncols) float32/float64, a C-order numpy array or a contiguous CUDA tensor.
    `y`: the positives -- a scipy sparse matrix or dense 0/1 array of the same shape, or a 0-based CSR (ptr int64,
    idx int32) pair, host arrays or CUDA tensors, indices sorted and unique in every row; ptr may be a slice of a larger
    CSR's row pointers (ptr[0] > 0).  Returns (nrows, 6) float64
    of the same kind as `yhat`.  Bad shapes, L >= ncols and bad label indices raise before the device is touched."""
    torch_in = type(yhat).__module__.startswith("torch")
    if torch_in:
        import torch
        if yhat.dim() != 2 or not yhat.is_contiguous() or not yhat.is_cuda:
            raise ValueError("yhat must be a contiguous 2-D CUDA tensor")
        suf = {torch.float32: "f32", torch.float64: "f64"}.get(yhat.dtype)
        if suf is None:
            raise TypeError("yhat must be float32 or float64")
        nrows, ncols = (int(v) for v in yhat.shape)
    else:
        a = np.asarray(yhat)
        if a.ndim != 2:
            raise ValueError("yhat must be 2-D (rows x columns)")
        suf = _suffix(a.dtype)
        a = np.ascontiguousarray(a)
        nrows, ncols = a.shape
    _check_L(ncols, L)
    dev_labels = isinstance(y, tuple) and type(y[0]).__module__.startswith("torch")
    if dev_labels:
        import torch
        ptr_t, idx_t = y
        if ptr_t.dtype != torch.int64 or idx_t.dtype != torch.int32 or not (ptr_t.is_cuda and idx_t.is_cuda):
            raise TypeError("device labels are a (ptr int64, idx int32) pair of CUDA tensors")
        if ptr_t.numel() != nrows + 1:
            raise ValueError(f"label row pointers have {ptr_t.numel()} entries, expected {nrows + 1}")
        # the indices stay on the device: the library checks them there before it writes anything
    else:
        hp, hi = _label_csr(y, nrows, ncols)
        _check_label_order(hp, hi, ncols)
    lib = L_.lib()
    fn = getattr(lib, f"ss_rank_metrics_rows_{suf}")
    if torch_in:
        import torch
        _is_torch(yhat)  # order the library after the kernels that produced the scores
        if dev_labels:
            ptr_d, idx_d = ptr_t.contiguous(), idx_t.contiguous()
        else:
            ptr_d = torch.from_numpy(hp).to(yhat.device)
            idx_d = torch.from_numpy(hi if hi.size else np.zeros(1, np.int32)).to(yhat.device)
        out = torch.empty((nrows, 6), dtype=torch.float64, device=yhat.device)
        L_.check(fn(ptr_d.data_ptr(), idx_d.data_ptr(), 0, yhat.data_ptr(), nrows, ncols, ncols, float(alpha), int(L),
                    out.data_ptr(), L_.SS_MEM_DEVICE))
        return out
    if dev_labels:
        raise TypeError("device labels need device scores (a CUDA tensor yhat)")
    out = np.empty((nrows, 6), np.float64)
    L_.check(fn(hp.ctypes.data, hi.ctypes.data, 0, a.ctypes.data, nrows, ncols, ncols, float(alpha), int(L),
                out.ctypes.data, L_.SS_MEM_HOST))
    return out


BINARY_METRICS = ("f1score", "mcc", "accuracy", "balancedaccuracy", "recall", "precision")
BINARY_ROWS_FIELDS = tuple(f"{m}_{s}" for m in BINARY_METRICS for s in ("max", "mean", "std"))


def binary_metrics_rows(y, yhat):
    """Binary prediction metrics of every row of a score block over all of the row's thresholds, on the device: for
    f1score, mcc, accuracy, balancedaccuracy, recall and precision (src/performance.jl:102-296) the max, mean and
    corrected std over the row's distinct scores (positive when score >= threshold), as maxperformance /
    meanperformance / meanstdperformance (src/performance.jl:420-520) give them.  Columns in BINARY_ROWS_FIELDS.
    `y` and `yhat` take the kinds rank_metrics_rows takes; a 1-D `y` / `yhat` is one row (the reference's pooled
    maxperformance(vec(y), vec(yhat), f1score) on a flattened block) and gives an (18,) result.  Returns
    (nrows, 18) float64 of the same kind as `yhat`.  Bad shapes and bad label indices raise before the device is
    touched."""
    torch_in = type(yhat).__module__.startswith("torch")
    if torch_in:
        import torch
        one = yhat.dim() == 1
        if one:
            yhat = yhat.reshape(1, -1)
        if yhat.dim() != 2 or not yhat.is_contiguous() or not yhat.is_cuda:
            raise ValueError("yhat must be a contiguous 1-D or 2-D CUDA tensor")
        suf = {torch.float32: "f32", torch.float64: "f64"}.get(yhat.dtype)
        if suf is None:
            raise TypeError("yhat must be float32 or float64")
        nrows, ncols = (int(v) for v in yhat.shape)
    else:
        a = np.asarray(yhat)
        one = a.ndim == 1
        if one:
            a = a.reshape(1, -1)
        if a.ndim != 2:
            raise ValueError("yhat must be 1-D (one row) or 2-D (rows x columns)")
        suf = _suffix(a.dtype)
        a = np.ascontiguousarray(a)
        nrows, ncols = a.shape
    if not 1 <= ncols < (1 << 31):
        raise ValueError(f"rows of {ncols} scores: the row length must lie in [1, 2^31)")
    if one and not isinstance(y, tuple) and not hasattr(y, "tocsr"):
        y = np.asarray(y)
        if y.ndim != 1:
            raise ValueError("a 1-D yhat takes 1-D labels")
        y = y.reshape(1, -1)
    dev_labels = isinstance(y, tuple) and type(y[0]).__module__.startswith("torch")
    if dev_labels:
        import torch
        ptr_t, idx_t = y
        if ptr_t.dtype != torch.int64 or idx_t.dtype != torch.int32 or not (ptr_t.is_cuda and idx_t.is_cuda):
            raise TypeError("device labels are a (ptr int64, idx int32) pair of CUDA tensors")
        if ptr_t.numel() != nrows + 1:
            raise ValueError(f"label row pointers have {ptr_t.numel()} entries, expected {nrows + 1}")
        # the indices stay on the device: the library checks them there before it writes anything
    else:
        hp, hi = _label_csr(y, nrows, ncols)
        _check_label_order(hp, hi, ncols)
    if dev_labels and not torch_in:
        raise TypeError("device labels need device scores (a CUDA tensor yhat)")
    nf = len(BINARY_ROWS_FIELDS)
    fn = getattr(L_.lib(), f"ss_binary_metrics_rows_{suf}")
    if torch_in:
        _is_torch(yhat)  # order the library after the kernels that produced the scores
        if dev_labels:
            ptr_d, idx_d = ptr_t.contiguous(), idx_t.contiguous()
        else:
            ptr_d = torch.from_numpy(hp).to(yhat.device)
            idx_d = torch.from_numpy(hi if hi.size else np.zeros(1, np.int32)).to(yhat.device)
        out = torch.empty((nrows, nf), dtype=torch.float64, device=yhat.device)
        L_.check(fn(ptr_d.data_ptr(), idx_d.data_ptr(), 0, yhat.data_ptr(), nrows, ncols, ncols, out.data_ptr(),
                    L_.SS_MEM_DEVICE))
        return out[0] if one else out
    out = np.empty((nrows, nf), np.float64)
    L_.check(fn(hp.ctypes.data, hi.ctypes.data, 0, a.ctypes.data, nrows, ncols, ncols, out.ctypes.data,
                L_.SS_MEM_HOST))
    return out[0] if one else out


POOLED_FIELDS = ("AuROC", "AuPRC", "validity_ratio") + BINARY_ROWS_FIELDS


class Pool:
    """Pooled evaluation on the device: a table of the distinct scores with int64 counts of positives and negatives,
    so that AuROC(vec(y), vec(yhat)), AuPRC and maxperformance(vec(y), vec(yhat), f) of a whole score matrix or
    cross-validation sweep follow without the scores leaving the device (ss_pool_*).  Adds are all or nothing.
    `metrics()` returns POOLED_FIELDS: AuROC, AuPRC, validity ratio, then max / mean / std of the six binary metrics as
    binary_metrics_rows defines them for one row.  BEDROC and recall@L / precision@L are not pooled (see the header)."""

    def __init__(self, dtype=np.float32, max_entries: int = 0):
        self.dtype = np.dtype(dtype)
        self._suf = _suffix(dtype)
        h = C.c_void_p()
        L.check(getattr(L.lib(), f"ss_pool_create_{self._suf}")(int(max_entries), C.byref(h)))
        self._h = h

    def info(self) -> dict:
        """pairs pooled, positives among them, table entries stored, max_entries"""
        buf = (C.c_int64 * 4)()
        L.check(L.lib().ss_pool_info(self._h, buf))
        return dict(n=int(buf[0]), npos=int(buf[1]), entries=int(buf[2]), max_entries=int(buf[3]))

    def reset(self):
        L.check(L.lib().ss_pool_reset(self._h))
        return self

    def add_rows(self, y, yhat):
        """Pool every (score, label) pair of a score block: `y` and `yhat` as binary_metrics_rows takes them (numpy or
        a contiguous CUDA tensor; labels scipy / dense 0/1 / a 0-based (ptr int64, idx int32) CSR pair)."""
        torch_in = type(yhat).__module__.startswith("torch")
        if torch_in:
            import torch
            if yhat.dim() == 1:
                yhat = yhat.reshape(1, -1)
            if yhat.dim() != 2 or not yhat.is_contiguous() or not yhat.is_cuda:
                raise ValueError("yhat must be a contiguous 1-D or 2-D CUDA tensor")
            if {torch.float32: "f32", torch.float64: "f64"}.get(yhat.dtype) != self._suf:
                raise TypeError("yhat dtype does not match the pool precision")
            nrows, ncols = (int(v) for v in yhat.shape)
        else:
            a = np.asarray(yhat)
            if a.ndim == 1:
                a = a.reshape(1, -1)
            if a.ndim != 2:
                raise ValueError("yhat must be 1-D or 2-D")
            if a.dtype != self.dtype:
                raise TypeError("yhat dtype does not match the pool precision")
            a = np.ascontiguousarray(a)
            nrows, ncols = a.shape
        if not isinstance(y, tuple) and not hasattr(y, "tocsr"):
            y = np.asarray(y).reshape(nrows, ncols)
        dev_labels = isinstance(y, tuple) and type(y[0]).__module__.startswith("torch")
        fn = getattr(L.lib(), f"ss_pool_add_rows_{self._suf}")
        if dev_labels:
            if not torch_in:
                raise TypeError("device labels need device scores (a CUDA tensor yhat)")
            ptr_d, idx_d = y[0].contiguous(), y[1].contiguous()
        else:
            hp, hi = _label_csr(y, nrows, ncols)
            _check_label_order(hp, hi, ncols)
        if torch_in:
            import torch
            _is_torch(yhat)
            if not dev_labels:
                ptr_d = torch.from_numpy(hp).to(yhat.device)
                idx_d = torch.from_numpy(hi if hi.size else np.zeros(1, np.int32)).to(yhat.device)
            L.check(fn(self._h, ptr_d.data_ptr(), idx_d.data_ptr(), 0, yhat.data_ptr(), nrows, ncols, ncols,
                       L.SS_MEM_DEVICE))
        else:
            L.check(fn(self._h, hp.ctypes.data, hi.ctypes.data, 0, a.ctypes.data, nrows, ncols, ncols, L.SS_MEM_HOST))
        return self

    def add_loo(self, g: "DeviceGraph", i_begin: int = 0, i_end: Optional[int] = None, clean: bool = False,
                block_rows: int = 0):
        """Pool the leave-one-out folds [i_begin, i_end) of `g` against its own labels (ss_pool_add_loo_*)."""
        i_end = g.ns if i_end is None else i_end
        fn = getattr(L.lib(), f"ss_pool_add_loo_{self._suf}")
        L.check(fn(self._h, g._h, int(i_begin), int(i_end), 1 if clean else 0, int(block_rows)))
        return self

    def add_kfold(self, g: "DeviceGraph", fold_of_source, nfolds: Optional[int] = None, i_begin: int = 0,
                  i_end: Optional[int] = None, clean: bool = False, block_rows: int = 0):
        """Pool the k-fold rows [i_begin, i_end) of `g` against its own labels (ss_pool_add_kfold_*)."""
        fold, nfolds = g._folds(fold_of_source, nfolds)
        i_end = g.ns if i_end is None else i_end
        fn = getattr(L.lib(), f"ss_pool_add_kfold_{self._suf}")
        L.check(fn(self._h, g._h, fold.ctypes.data, nfolds, int(i_begin), int(i_end), 1 if clean else 0,
                   int(block_rows), L.SS_MEM_HOST))
        return self

    def merge(self, other: "Pool"):
        """Add every pair of `other` (unchanged) to this pool."""
        L.check(L.lib().ss_pool_merge(self._h, other._h))
        return self

    def export(self):
        """(scores descending, npos int64, nneg int64) numpy arrays of the table."""
        fn = getattr(L.lib(), f"ss_pool_export_{self._suf}")
        n = C.c_int64()
        L.check(fn(self._h, None, None, None, 0, C.byref(n), L.SS_MEM_HOST))
        keys = np.empty(n.value, self.dtype)
        npos, nneg = np.empty(n.value, np.int64), np.empty(n.value, np.int64)
        L.check(fn(self._h, keys.ctypes.data, npos.ctypes.data, nneg.ctypes.data, n.value, C.byref(n), L.SS_MEM_HOST))
        return keys, npos, nneg

    def import_(self, keys, npos, nneg):
        """Add a table such as export() returns (scores strictly descending, counts >= 0)."""
        k = np.ascontiguousarray(keys, dtype=self.dtype)
        p = np.ascontiguousarray(npos, dtype=np.int64)
        q = np.ascontiguousarray(nneg, dtype=np.int64)
        if not k.shape == p.shape == q.shape or k.ndim != 1:
            raise ValueError("keys, npos and nneg must be 1-D arrays of one length")
        fn = getattr(L.lib(), f"ss_pool_import_{self._suf}")
        L.check(fn(self._h, k.ctypes.data, p.ctypes.data, q.ctypes.data, k.size, L.SS_MEM_HOST))
        return self

    def metrics_array(self) -> np.ndarray:
        """The 21 pooled numbers, in POOLED_FIELDS order."""
        out = np.empty(len(POOLED_FIELDS), np.float64)
        L.check(L.lib().ss_pool_metrics(self._h, out.ctypes.data))
        return out

    def metrics(self) -> dict:
        return dict(zip(POOLED_FIELDS, (float(v) for v in self.metrics_array())))

    def close(self):
        if self._h is not None and self._h.value:
            L.load().ss_pool_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


TARGET_TOPL_FIELDS = ("recallatL", "precisionatL", "recall_with_positives", "targets_with_positives")


class TargetTopL:
    """Per target the L best rows seen so far, on the device (ss_target_topl_*): recallatL(y, yhat, grouping, L) and
    precisionatL with grouping = the target of every entry of vec(yhat) (src/performance.jl:308-409), and each target's
    screening list -- its L best rows under (score descending, row ascending), the order Julia's stable sortperm gives
    inside a target group.  Row ids are int64 >= 0 and must be distinct across adds; adds are all or nothing, and the
    table is one and the same whatever the blocks, their order, merges or export -> import."""

    def __init__(self, nt: int, L: int = 20, dtype=np.float32):
        self.dtype = np.dtype(dtype)
        self._suf = _suffix(dtype)
        h = C.c_void_p()
        L_.check(getattr(L_.lib(), f"ss_target_topl_create_{self._suf}")(int(nt), int(L), C.byref(h)))
        self._h = h

    def info(self) -> dict:
        """nt, L, rows added, positives among them"""
        buf = (C.c_int64 * 4)()
        L_.check(L_.lib().ss_target_topl_info(self._h, buf))
        return dict(nt=int(buf[0]), L=int(buf[1]), rows=int(buf[2]), npos=int(buf[3]))

    def reset(self):
        L_.check(L_.lib().ss_target_topl_reset(self._h))
        return self

    def add_rows(self, y, yhat, row_begin: int = 0):
        """Add the rows of a score block (nrows, nt): row r gets the id row_begin + r.  `y` and `yhat` as Pool.add_rows
        takes them (numpy or a contiguous CUDA tensor; labels scipy / dense 0/1 / a 0-based (ptr int64, idx int32) CSR
        pair, on the host or, with device scores, on the device)."""
        torch_in = _is_torch(yhat)
        if torch_in:
            import torch
            if yhat.dim() == 1:
                yhat = yhat.reshape(1, -1)
            if yhat.dim() != 2 or not yhat.is_contiguous() or not yhat.is_cuda:
                raise ValueError("yhat must be a contiguous 1-D or 2-D CUDA tensor")
            if {torch.float32: "f32", torch.float64: "f64"}.get(yhat.dtype) != self._suf:
                raise TypeError("yhat dtype does not match the table precision")
            nrows, ncols = (int(v) for v in yhat.shape)
        else:
            a = np.asarray(yhat)
            if a.ndim == 1:
                a = a.reshape(1, -1)
            if a.ndim != 2:
                raise ValueError("yhat must be 1-D or 2-D")
            if a.dtype != self.dtype:
                raise TypeError("yhat dtype does not match the table precision")
            a = np.ascontiguousarray(a)
            nrows, ncols = a.shape
        if not isinstance(y, tuple) and not hasattr(y, "tocsr"):
            y = np.asarray(y).reshape(nrows, ncols)
        dev_labels = isinstance(y, tuple) and _is_torch(y[0])
        fn = getattr(L_.lib(), f"ss_target_topl_add_rows_{self._suf}")
        if dev_labels:
            if not torch_in:
                raise TypeError("device labels need device scores (a CUDA tensor yhat)")
            ptr_d, idx_d = y[0].contiguous(), y[1].contiguous()
        else:
            hp, hi = _label_csr(y, nrows, ncols)
            _check_label_order(hp, hi, ncols)
        if torch_in:
            import torch
            if not dev_labels:
                ptr_d = torch.from_numpy(hp).to(yhat.device)
                idx_d = torch.from_numpy(hi if hi.size else np.zeros(1, np.int32)).to(yhat.device)
            L_.check(fn(self._h, ptr_d.data_ptr(), idx_d.data_ptr(), 0, yhat.data_ptr(), nrows, ncols, ncols,
                        int(row_begin), L_.SS_MEM_DEVICE))
        else:
            L_.check(fn(self._h, hp.ctypes.data, hi.ctypes.data, 0, a.ctypes.data, nrows, ncols, ncols, int(row_begin),
                        L_.SS_MEM_HOST))
        return self

    def add_loo(self, g: "DeviceGraph", i_begin: int = 0, i_end: Optional[int] = None, clean: bool = False,
                block_rows: int = 0):
        """Add the leave-one-out folds [i_begin, i_end) of `g` against its own labels, fold i as row i
        (ss_target_topl_add_loo_*)."""
        i_end = g.ns if i_end is None else i_end
        fn = getattr(L_.lib(), f"ss_target_topl_add_loo_{self._suf}")
        L_.check(fn(self._h, g._h, int(i_begin), int(i_end), 1 if clean else 0, int(block_rows)))
        return self

    def add_kfold(self, g: "DeviceGraph", fold_of_source, nfolds: Optional[int] = None, i_begin: int = 0,
                  i_end: Optional[int] = None, clean: bool = False, block_rows: int = 0):
        """Add the k-fold rows [i_begin, i_end) of `g` against its own labels, source i as row i
        (ss_target_topl_add_kfold_*)."""
        fold, nfolds = g._folds(fold_of_source, nfolds)
        i_end = g.ns if i_end is None else i_end
        fn = getattr(L_.lib(), f"ss_target_topl_add_kfold_{self._suf}")
        L_.check(fn(self._h, g._h, fold.ctypes.data, nfolds, int(i_begin), int(i_end), 1 if clean else 0,
                    int(block_rows), L_.SS_MEM_HOST))
        return self

    def add_predict(self, g: "DeviceGraph", rows: str = "query", begin: int = 0, end: Optional[int] = None,
                    clean: bool = False, y=None, block_rows: int = 0, queries: Optional["DeviceQueries"] = None):
        """Virtual screening: the scores of rows [begin, end) of the query (or source) nodes, predicted block by block
        into a device buffer (DeviceGraph.predict(..., out=tensor)) and added with row ids begin..end-1.  `y`: labels
        of those rows (scipy / dense 0/1, shape (end - begin, nt)) or None -- unlabelled rows count as negatives.
        block_rows: rows per block (0: about 1 GiB of scores).  queries: a ``DeviceQueries`` of `g` whose rows are
        screened instead of the graph's own."""
        import scipy.sparse as sp
        import torch
        limit = queries.nq if queries is not None else (g.nq if rows == "query" else g.ns)
        end = limit if end is None else end
        n = end - begin
        if n <= 0:
            return self
        nt = g.nt
        if y is None:
            Y = sp.csr_matrix((n, nt), dtype=np.float64)
        else:
            Y = sp.csr_matrix(y)
            if Y.shape != (n, nt):
                raise ValueError(f"labels have shape {Y.shape}, expected {(n, nt)}")
        rb = int(block_rows) if block_rows > 0 else max(1, (1 << 30) // (nt * self.dtype.itemsize))
        rb = min(rb, n)
        buf = torch.empty((rb, nt), dtype=torch.float32 if self._suf == "f32" else torch.float64, device="cuda")
        for r0 in range(0, n, rb):
            nb = min(rb, n - r0)
            out = buf[:nb]
            g.predict(rows, begin + r0, begin + r0 + nb, clean=clean, out=out, queries=queries)
            self.add_rows(Y[r0:r0 + nb], out, row_begin=begin + r0)
        return self

    def merge(self, other: "TargetTopL"):
        """Add every row of `other` (unchanged) to this table."""
        L_.check(L_.lib().ss_target_topl_merge(self._h, other._h))
        return self

    def export(self):
        """(scores, rows int64, labels uint8) as (nt, fill) numpy arrays, npos (nt,) int64 and the rows added."""
        i = self.info()
        fill = min(i["L"], i["rows"])
        vals = np.empty((i["nt"], fill), self.dtype)
        rows = np.empty((i["nt"], fill), np.int64)
        labels = np.empty((i["nt"], fill), np.uint8)
        npos = np.empty(i["nt"], np.int64)
        n = C.c_int64()
        fn = getattr(L_.lib(), f"ss_target_topl_export_{self._suf}")
        L_.check(fn(self._h, vals.ctypes.data, rows.ctypes.data, labels.ctypes.data, npos.ctypes.data, C.byref(n),
                    L_.SS_MEM_HOST))
        return vals, rows, labels, npos, int(n.value)

    def import_(self, vals, rows, labels, npos, rows_added: int):
        """Add a table such as export() returns (another rank's, for instance)."""
        i = self.info()
        fill = min(i["L"], int(rows_added))
        v = np.ascontiguousarray(vals, dtype=self.dtype)
        r = np.ascontiguousarray(rows, dtype=np.int64)
        lab = np.ascontiguousarray(labels, dtype=np.uint8)
        p = np.ascontiguousarray(npos, dtype=np.int64)
        if rows_added > 0 and not (v.shape == r.shape == lab.shape == (i["nt"], fill) and p.shape == (i["nt"],)):
            raise ValueError(f"the table must be (nt, fill) = {(i['nt'], fill)} arrays and npos (nt,)")
        fn = getattr(L_.lib(), f"ss_target_topl_import_{self._suf}")
        L_.check(fn(self._h, v.ctypes.data, r.ctypes.data, lab.ctypes.data, p.ctypes.data, int(rows_added),
                    L_.SS_MEM_HOST))
        return self

    def table(self):
        """(rows, scores, labels) of every target's list as (nt, fill) numpy arrays: row [t] is target t's screening
        result, best first."""
        vals, rows, labels, _, _ = self.export()
        return rows, vals, labels

    def metrics(self) -> dict:
        """TARGET_TOPL_FIELDS (recallatL and precisionatL exactly as the reference's grouped means with grouping =
        target; then, beyond the reference, mean recall over the targets that have positives and their number) plus
        the per-target arrays `hits` and `npos`."""
        nt = self.info()["nt"]
        hits, npos = np.empty(nt, np.int64), np.empty(nt, np.int64)
        out = np.empty(4, np.float64)
        L_.check(L_.lib().ss_target_topl_metrics(self._h, hits.ctypes.data, npos.ctypes.data, out.ctypes.data,
                                                 L_.SS_MEM_HOST))
        d = dict(zip(TARGET_TOPL_FIELDS, (float(v) for v in out)))
        d["targets_with_positives"] = int(out[3])
        d["hits"], d["npos"] = hits, npos
        return d

    def close(self):
        if self._h is not None and self._h.value:
            L_.load().ss_target_topl_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


TARGET_RANK_FIELDS = RANK_ROWS_FIELDS


class TargetRank:
    """Per target the six ranking metrics of a whole sweep -- AuROC, AuPRC, BEDROC, validity ratio, recall@L,
    precision@L of (Y[:, t], S[:, t]) as rank_metrics_rows gives them for a vector, ties by ascending row id -- on the
    device and without the score matrix (ss_target_rank_*).  It costs two sweeps: every row is added once to collect
    the positives' scores, then, after seal(), once more to count the negatives against them; the second pass is
    checked to repeat the first.  Row ids are >= 0, < 2^31 and distinct; adds are all or nothing; positives, counts
    and metrics are one and the same whatever the blocks, their order, merges or export -> import."""

    def __init__(self, nt: int, dtype=np.float32):
        self.dtype = np.dtype(dtype)
        self._suf = _suffix(dtype)
        h = C.c_void_p()
        L_.check(getattr(L_.lib(), f"ss_target_rank_create_{self._suf}")(int(nt), C.byref(h)))
        self._h = h

    def info(self) -> dict:
        """nt, phase ("collect" or "count"), rows and positives collected, rows counted"""
        buf = (C.c_int64 * 6)()
        L_.check(L_.lib().ss_target_rank_info(self._h, buf))
        return dict(nt=int(buf[0]), phase="count" if buf[1] else "collect", rows=int(buf[2]), npos=int(buf[3]),
                    rows_counted=int(buf[4]))

    def reset(self):
        L_.check(L_.lib().ss_target_rank_reset(self._h))
        return self

    def add_rows(self, y, yhat, row_begin: int = 0):
        """Add the rows of a score block (nrows, nt), row r under the id row_begin + r: collected before seal(),
        counted after it.  `y` and `yhat` as TargetTopL.add_rows takes them."""
        torch_in = _is_torch(yhat)
        if torch_in:
            import torch
            if yhat.dim() == 1:
                yhat = yhat.reshape(1, -1)
            if yhat.dim() != 2 or not yhat.is_contiguous() or not yhat.is_cuda:
                raise ValueError("yhat must be a contiguous 1-D or 2-D CUDA tensor")
            if {torch.float32: "f32", torch.float64: "f64"}.get(yhat.dtype) != self._suf:
                raise TypeError("yhat dtype does not match the handle's precision")
            nrows, ncols = (int(v) for v in yhat.shape)
        else:
            a = np.asarray(yhat)
            if a.ndim == 1:
                a = a.reshape(1, -1)
            if a.ndim != 2:
                raise ValueError("yhat must be 1-D or 2-D")
            if a.dtype != self.dtype:
                raise TypeError("yhat dtype does not match the handle's precision")
            a = np.ascontiguousarray(a)
            nrows, ncols = a.shape
        if not isinstance(y, tuple) and not hasattr(y, "tocsr"):
            y = np.asarray(y).reshape(nrows, ncols)
        dev_labels = isinstance(y, tuple) and _is_torch(y[0])
        fn = getattr(L_.lib(), f"ss_target_rank_add_rows_{self._suf}")
        if dev_labels:
            if not torch_in:
                raise TypeError("device labels need device scores (a CUDA tensor yhat)")
            ptr_d, idx_d = y[0].contiguous(), y[1].contiguous()
        else:
            hp, hi = _label_csr(y, nrows, ncols)
            _check_label_order(hp, hi, ncols)
        if torch_in:
            import torch
            if not dev_labels:
                ptr_d = torch.from_numpy(hp).to(yhat.device)
                idx_d = torch.from_numpy(hi if hi.size else np.zeros(1, np.int32)).to(yhat.device)
            L_.check(fn(self._h, ptr_d.data_ptr(), idx_d.data_ptr(), 0, yhat.data_ptr(), nrows, ncols, ncols,
                        int(row_begin), L_.SS_MEM_DEVICE))
        else:
            L_.check(fn(self._h, hp.ctypes.data, hi.ctypes.data, 0, a.ctypes.data, nrows, ncols, ncols, int(row_begin),
                        L_.SS_MEM_HOST))
        return self

    def add_loo(self, g: "DeviceGraph", i_begin: int = 0, i_end: Optional[int] = None, clean: bool = False,
                block_rows: int = 0):
        """Add the leave-one-out folds [i_begin, i_end) of `g` against its own labels, fold i as row i
        (ss_target_rank_add_loo_*)."""
        i_end = g.ns if i_end is None else i_end
        fn = getattr(L_.lib(), f"ss_target_rank_add_loo_{self._suf}")
        L_.check(fn(self._h, g._h, int(i_begin), int(i_end), 1 if clean else 0, int(block_rows)))
        return self

    def add_kfold(self, g: "DeviceGraph", fold_of_source, nfolds: Optional[int] = None, i_begin: int = 0,
                  i_end: Optional[int] = None, clean: bool = False, block_rows: int = 0):
        """Add the k-fold rows [i_begin, i_end) of `g` against its own labels, source i as row i
        (ss_target_rank_add_kfold_*)."""
        fold, nfolds = g._folds(fold_of_source, nfolds)
        i_end = g.ns if i_end is None else i_end
        fn = getattr(L_.lib(), f"ss_target_rank_add_kfold_{self._suf}")
        L_.check(fn(self._h, g._h, fold.ctypes.data, nfolds, int(i_begin), int(i_end), 1 if clean else 0,
                    int(block_rows), L_.SS_MEM_HOST))
        return self

    def seal(self):
        """End the collect phase: sort the positives; from now on adds count."""
        L_.check(L_.lib().ss_target_rank_seal(self._h))
        return self

    def merge(self, other: "TargetRank"):
        """Collect phase: add `other`'s positives and rows.  Count phase: add its counts (the same sealed positives)."""
        L_.check(L_.lib().ss_target_rank_merge(self._h, other._h))
        return self

    def export_positives(self):
        """(targets int32, rows int64, scores) of the positives and the rows collected: in collection order before
        seal(), sorted by (target, score descending, row ascending) after it."""
        n = self.info()["npos"]
        t, r, v = np.empty(n, np.int32), np.empty(n, np.int64), np.empty(n, self.dtype)
        rows = C.c_int64()
        fn = getattr(L_.lib(), f"ss_target_rank_export_positives_{self._suf}")
        L_.check(fn(self._h, t.ctypes.data, r.ctypes.data, v.ctypes.data, C.byref(rows), L_.SS_MEM_HOST))
        return t, r, v, int(rows.value)

    def import_positives(self, targets, rows, scores, rows_added: int):
        """Collect phase: add positives such as export_positives() returns (another rank's)."""
        t = np.ascontiguousarray(targets, dtype=np.int32)
        r = np.ascontiguousarray(rows, dtype=np.int64)
        v = np.ascontiguousarray(scores, dtype=self.dtype)
        if not (t.ndim == 1 and t.shape == r.shape == v.shape):
            raise ValueError("targets, rows and scores must be 1-D arrays of one length")
        fn = getattr(L_.lib(), f"ss_target_rank_import_positives_{self._suf}")
        L_.check(fn(self._h, t.ctypes.data, r.ctypes.data, v.ctypes.data, t.size, int(rows_added), L_.SS_MEM_HOST))
        return self

    def export_counts(self):
        """Count phase: the int64 count table (3 npos + 6 nt entries, layout in include/simspread_hip_target_rank.h)
        and the rows counted."""
        i = self.info()
        c = np.empty(3 * i["npos"] + 6 * i["nt"], np.int64)
        rows = C.c_int64()
        L_.check(L_.lib().ss_target_rank_export_counts(self._h, c.ctypes.data, C.byref(rows), L_.SS_MEM_HOST))
        return c, int(rows.value)

    def import_counts(self, counts, rows_counted: int):
        """Count phase: add a count table such as export_counts() returns, taken against the same sealed positives."""
        c = np.ascontiguousarray(counts, dtype=np.int64)
        L_.check(L_.lib().ss_target_rank_import_counts(self._h, c.ctypes.data, c.size, int(rows_counted),
                                                       L_.SS_MEM_HOST))
        return self

    def metrics(self, alpha: float = 20.0, L: int = 20) -> np.ndarray:
        """(nt, 6) float64, columns TARGET_RANK_FIELDS; every collected row must have been counted and L < rows."""
        out = np.empty((self.info()["nt"], len(TARGET_RANK_FIELDS)), np.float64)
        L_.check(L_.lib().ss_target_rank_metrics(self._h, float(alpha), int(L), out.ctypes.data, L_.SS_MEM_HOST))
        return out

    def close(self):
        if self._h is not None and self._h.value:
            L_.load().ss_target_rank_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def jaccard_similarity(X, dtype=np.float64):
    """Weighted Jaccard (Ruzicka) similarity between the rows of a feature matrix, on the device: the similarity
    producer of the reference's tutorial (`1 .- pairwise(Jaccard(), X, dims=1)`, docs/src/tutorial/fishers-flowers.jl:66).
    X: (n, d) numpy array or torch CUDA tensor; returns (n, n) of the same kind."""
    lib = L_.lib()
    if _is_torch(X):
        import torch
        if X.dtype not in (torch.float32, torch.float64):
            raise TypeError("X must be float32 or float64")
        suf = "f32" if X.dtype == torch.float32 else "f64"
        n, d = X.shape
        Xc = X.t().contiguous()                    # column-major n x d
        S = torch.empty((n, n), dtype=X.dtype, device=X.device)
        L_.check(getattr(lib, f"ss_similarity_jaccard_{suf}")(Xc.data_ptr(), n, d, n, S.data_ptr(), n, L_.SS_MEM_DEVICE))
        return S                                   # symmetric: row- and column-major coincide
    dt = np.dtype(dtype)
    suf = "f32" if dt == np.float32 else "f64"
    Xf = np.asfortranarray(np.asarray(X, dtype=dt))
    n, d = Xf.shape
    S = np.empty((n, n), dtype=dt, order="F")
    L_.check(getattr(lib, f"ss_similarity_jaccard_{suf}")(Xf.ctypes.data, n, d, max(n, 1), S.ctypes.data, max(n, 1), L_.SS_MEM_HOST))
    return np.ascontiguousarray(S)


def pack_fingerprints(bits):
    """Pack binary fingerprints (bool or 0/1 array of shape (n, d)) into the library's layout: (n, ceil(d/64)) uint64,
    bit k of a fingerprint = bit k % 64 of word k // 64 (little-endian), bits past d zero.  This is Julia's
    ``BitVector.chunks`` layout, one fingerprint per row."""
    b = np.asarray(bits)
    if b.ndim != 2:
        raise ValueError("bits must be an (n, d) matrix")
    n, d = b.shape
    nwords = max((d + 63) // 64, 1)
    packed = np.packbits(b != 0, axis=1, bitorder="little")          # (n, ceil(d/8)) bytes
    out = np.zeros((n, nwords * 8), dtype=np.uint8)
    out[:, :packed.shape[1]] = packed
    return out.view("<u8").astype(np.uint64, copy=False).reshape(n, nwords)


def _fingerprints(F, dev, keep):
    """(pointer, rows, nwords) of packed fingerprints: uint64 numpy rows or an int64 torch CUDA tensor."""
    if F is None:
        return None, 0, 0
    if dev:
        import torch
        if not (type(F).__module__.startswith("torch") and F.is_cuda and F.dtype == torch.int64 and F.ndim == 2):
            raise TypeError("device fingerprints must be (n, nwords) int64 CUDA tensors")
        t = F.contiguous()
        keep.append(t)
        return t.data_ptr(), t.shape[0], t.shape[1]
    a = np.asarray(F)
    if a.ndim != 2 or a.dtype.kind not in "ui" or a.dtype.itemsize != 8:
        raise TypeError("fingerprints must be an (n, nwords) uint64 array (see pack_fingerprints)")
    a = np.ascontiguousarray(a).view(np.uint64)
    keep.append(a)
    return a.ctypes.data, a.shape[0], a.shape[1]


def tanimoto_kth(Fa, Fb=None, k=None, dtype=np.float32):
    """tau[i] = the k-th largest of the positive Tanimoto similarities of fingerprint Fa[i] against the rows of Fb
    (multiplicity counted; Fb None: Fb = Fa, the diagonal included), +0 where a row has fewer than k: the per-row cut of
    ``tanimoto_csr(..., min_neighbours=k)``, computed on the device without the dense similarity.  1 <= k <= 64.  Host
    input (uint64 numpy) returns a numpy vector, device input (int64 torch CUDA tensors) a CUDA tensor."""
    if k is None:
        raise TypeError("tanimoto_kth needs k")
    lib = L_.lib()
    dt = np.dtype(dtype).type
    fn = getattr(lib, f"ss_similarity_tanimoto_kth_{_suffix(dt)}")
    dev = _is_torch(Fa)
    keep = []
    pa, na, nw = _fingerprints(Fa, dev, keep)
    pb, nb, nwb = _fingerprints(Fb, dev, keep)
    if Fb is None:
        nb, nwb = na, nw
    if nwb != nw:
        raise ValueError("Fa and Fb have different fingerprint widths")
    if dev:
        import torch
        tau = torch.empty(na, dtype=torch.float32 if dt == np.float32 else torch.float64, device=Fa.device)
        L_.check(fn(pa, na, pb, nb, nw, int(k), tau.data_ptr(), L_.SS_MEM_DEVICE))
        return tau
    tau = np.empty(na, dt)
    L_.check(fn(pa, na, pb, nb, nw, int(k), tau.ctypes.data, L_.SS_MEM_HOST))
    del keep
    return tau


def tanimoto_csr(Fa, Fb=None, alpha=None, weighted: bool = True, dtype=np.float32, min_neighbours: int = 0):
    """``featurize(1 .- pairwise(Jaccard(), F, dims=1), alpha, weighted)`` for packed binary fingerprints (see
    ``pack_fingerprints``), produced as CSR on the device without the dense similarity: entry (i, j) = Tanimoto(Fa[i],
    Fb[j]) when it is >= alpha (1 when not weighted).  Fb None: Fb = Fa.  Host input (uint64 numpy) returns a
    scipy.sparse.csr_matrix; device input (int64 torch CUDA tensors) returns (ptr int64, idx int32, val) tensors.
    min_neighbours = k > 0 (at most 64) adds the neighbour floor: row i also keeps every positive similarity >= tau_i,
    the k-th largest of its positive similarities (``tanimoto_kth``), i.e. at least its k nearest columns whatever alpha
    says (alpha = inf: exactly those).  Ties at tau_i are all kept, a row with fewer than k positive similarities keeps
    all of them, and the result is in general not symmetric ((i, j) is decided by tau_i, (j, i) by tau_j)."""
    if alpha is None:
        raise TypeError("tanimoto_csr needs alpha")
    lib = L_.lib()
    dt = np.dtype(dtype).type
    suf = _suffix(dt)
    ctype = C.c_float if dt == np.float32 else C.c_double
    if min_neighbours:
        floor = getattr(lib, f"ss_similarity_tanimoto_floor_csr_{suf}")

        def fn(pa, na, pb, nb, nw, a, w, *rest):
            return floor(pa, na, pb, nb, nw, a, int(min_neighbours), w, *rest)
    else:
        fn = getattr(lib, f"ss_similarity_tanimoto_csr_{suf}")
    dev = _is_torch(Fa)
    keep = []
    pa, na, nw = _fingerprints(Fa, dev, keep)
    pb, nb, nwb = _fingerprints(Fb, dev, keep)
    if Fb is None:
        nb, nwb = na, nw
    if nwb != nw:
        raise ValueError("Fa and Fb have different fingerprint widths")
    nnz = C.c_int64(0)
    w = 1 if weighted else 0
    if dev:
        import torch
        ptr = torch.empty(na + 1, dtype=torch.int64, device=Fa.device)
        L_.check(fn(pa, na, pb, nb, nw, ctype(alpha), w, ptr.data_ptr(), None, None, 0, C.byref(nnz), L_.SS_MEM_DEVICE))
        idx = torch.empty(max(nnz.value, 1), dtype=torch.int32, device=Fa.device)
        val = torch.empty(max(nnz.value, 1), dtype=torch.float32 if dt == np.float32 else torch.float64, device=Fa.device)
        L_.check(fn(pa, na, pb, nb, nw, ctype(alpha), w, ptr.data_ptr(), idx.data_ptr(), val.data_ptr(), nnz.value,
                    C.byref(nnz), L_.SS_MEM_DEVICE))
        return ptr, idx[:nnz.value], val[:nnz.value]
    import scipy.sparse as sp
    ptr = np.zeros(na + 1, np.int64)
    L_.check(fn(pa, na, pb, nb, nw, ctype(alpha), w, ptr.ctypes.data, None, None, 0, C.byref(nnz), L_.SS_MEM_HOST))
    idx = np.empty(max(nnz.value, 1), np.int32)
    val = np.empty(max(nnz.value, 1), dt)
    L_.check(fn(pa, na, pb, nb, nw, ctype(alpha), w, ptr.ctypes.data, idx.ctypes.data, val.ctypes.data, nnz.value,
                C.byref(nnz), L_.SS_MEM_HOST))
    del keep
    return sp.csr_matrix((val[:nnz.value], idx[:nnz.value], ptr), shape=(na, nb))


def _feature_dtype(dtype):
    dt = np.dtype(dtype).type
    if dt not in (np.float32, np.float64):
        raise TypeError("dtype must be float32 or float64")
    return dt


def _features(F, dt, dev, keep):
    """(pointer, rows, d, ld) of real-valued feature rows in the library's column-major layout: an (n, d) numpy array
    (any real dtype, converted to dt) or an (n, d) CUDA tensor of dtype dt (X.t().contiguous(), no copy when X is
    already column-major)."""
    if F is None:
        return None, 0, 0, 1
    if dev:
        import torch
        want = torch.float32 if dt == np.float32 else torch.float64
        if not (type(F).__module__.startswith("torch") and F.is_cuda and F.ndim == 2):
            raise TypeError("device features must be (n, d) CUDA tensors")
        if F.dtype != want:
            raise TypeError(f"device features must be {want} (the graph's dtype), got {F.dtype}")
        t = F.t().contiguous()                    # column-major n x d
        keep.append(t)
        return t.data_ptr(), F.shape[0], F.shape[1], max(F.shape[0], 1)
    if type(F).__module__.startswith("torch"):
        raise TypeError("features must all live on the host (numpy) or all on the device (CUDA tensors)")
    a = np.asarray(F)
    if a.ndim != 2:
        raise ValueError("features must be an (n, d) matrix")
    if a.dtype.kind not in "fiu":
        raise TypeError(f"features must be real numbers, got {a.dtype}")
    a = np.asfortranarray(a, dtype=dt)
    keep.append(a)
    return a.ctypes.data, a.shape[0], a.shape[1], max(a.shape[0], 1)


SIM_METRICS = {"cosine": 0, "tanimoto": 1, "dice": 2}       # SS_SIM_* of include/simspread_hip.h


def _sim_metric(metric):
    if metric not in SIM_METRICS:
        raise ValueError(f"metric must be one of {sorted(SIM_METRICS)}, got {metric!r}")
    return SIM_METRICS[metric]


H16_STORAGES = {"bf16": L.SS_H16_BF16, "f16": L.SS_H16_F16}     # SS_H16_* of include/simspread_hip_half.h


def to_bf16_bits(x) -> np.ndarray:
    """The bfloat16 bit patterns (uint16, same shape) of real numbers, rounded to nearest, ties to even; a NaN stays a
    NaN (quiet bit set), what lies above the largest bfloat16 becomes inf, +-0 and subnormals are kept.  fp32 input gives what
    ``torch.Tensor.to(torch.bfloat16)`` gives; fp64 input is rounded once, not through fp32."""
    a = np.asarray(x)
    if a.dtype.kind not in "fiu":
        raise TypeError(f"to_bf16_bits needs real numbers, got {a.dtype}")
    if a.dtype == np.float64:
        # fp64 -> fp32 rounded to odd (truncate, the last bit set when inexact), so that the second rounding is the only one
        with np.errstate(over="ignore", invalid="ignore"):
            f = a.astype(np.float32)
        u = f.view(np.uint32).astype(np.uint64)
        fin = np.isfinite(f) & np.isfinite(a)
        back = f.astype(np.float64)
        inexact = fin & (back != a)
        away = inexact & (np.abs(back) > np.abs(a))          # fp32 rounded away from zero: step back to the truncation
        u = np.where(away, u - 1, u)
        u = np.where(inexact, u | 1, u)
    else:
        u = np.ascontiguousarray(a, dtype=np.float32).view(np.uint32).astype(np.uint64)
    nan = (u & 0x7FFFFFFF) > 0x7F800000
    r = (u + 0x7FFF + ((u >> 16) & 1)) >> 16
    return np.where(nan, (u >> 16) | 0x0040, r).astype(np.uint16).reshape(a.shape)     # quiet, sign and payload kept


def _module_is_torch(x) -> bool:
    return type(x).__module__.startswith("torch")


def _h16_storage(storage, inputs, dtype, min_neighbours=0, auto_tensor=True):
    """The storage code (SS_H16_*) of the 16-bit route, or None for the fp32 / fp64 route.  Needs no device.  storage
    None: chosen by the inputs.  A 16-bit torch tensor (auto_tensor) selects its dtype's storage.  numpy float16 arrays
    select "f16" only where that changes no call that worked without it: every given input is float16, the graph
    precision is float32 and there is no neighbour floor; otherwise they are widened exactly, as they always were."""
    if storage is not None and storage not in H16_STORAGES:
        raise ValueError(f"storage must be None or one of {sorted(H16_STORAGES)} (\"i8\": dot_csr and the from_vectors "
                         f"constructors), got {storage!r}")
    given = [F for F in inputs if F is not None]
    if storage is None:
        half = {"torch.bfloat16": "bf16", "torch.float16": "f16"}
        tensors = [half[str(F.dtype)] for F in given if _module_is_torch(F) and str(F.dtype) in half]
        if tensors and auto_tensor:
            storage = tensors[0]            # a tensor of another dtype next to it is refused by _features_h16
        elif (given and not min_neighbours and np.dtype(dtype) == np.float32
              and all(getattr(F, "dtype", None) == np.float16 and not _module_is_torch(F) for F in given)):
            storage = "f16"
    if storage is None:
        return None
    if np.dtype(dtype) != np.float32:
        raise TypeError("16-bit storage builds float32 graphs: dtype must be float32")
    if min_neighbours:
        raise NotImplementedError("the neighbour floor (min_neighbours > 0) has no 16-bit route: widen the features")
    if len({_module_is_torch(F) for F in given}) > 1:
        raise TypeError("features must all live on the host (numpy) or all on the device (CUDA tensors)")
    return H16_STORAGES[storage]


def _features_h16(F, code, dev, keep):
    """(pointer, rows, d, ld) of 16-bit feature rows in the row-major layout of include/simspread_hip_half.h.  Device: an
    (n, d) CUDA tensor of the storage's dtype, used in place when its rows are contiguous (ld = stride(0)).  Host: numpy
    float16 for "f16" or uint16 (raw bit patterns) as they are, any other real array rounded to the storage."""
    if F is None:
        return None, 0, 0, 1
    if dev:
        import torch
        want = torch.bfloat16 if code == L.SS_H16_BF16 else torch.float16
        if not (_module_is_torch(F) and F.is_cuda and F.ndim == 2):
            raise TypeError("device features must be (n, d) CUDA tensors")
        if F.dtype != want:
            raise TypeError(f"device features of this storage must be {want}, got {F.dtype}")
        n, d = F.shape
        rows_ok = d <= 1 or F.stride(1) == 1                  # the d elements of a row are consecutive
        ld_ok = n <= 1 or F.stride(0) >= d                    # rows do not overlap
        if not (rows_ok and ld_ok):
            F = F.contiguous()
        keep.append(F)
        ld = F.stride(0) if n > 1 else d
        return F.data_ptr(), n, d, max(ld, d, 1)
    if _module_is_torch(F):
        raise TypeError("features must all live on the host (numpy) or all on the device (CUDA tensors)")
    a = np.asarray(F)
    if a.ndim != 2:
        raise ValueError("features must be an (n, d) matrix")
    if a.dtype.kind not in "fiu":
        raise TypeError(f"features must be real numbers, got {a.dtype}")
    if a.dtype == np.uint16:
        bits = a                                                      # raw patterns
    elif code == L.SS_H16_F16:
        with np.errstate(over="ignore"):
            bits = a.astype(np.float16, copy=False).view(np.uint16)   # numpy rounds to nearest even, straight from fp64
    else:
        bits = to_bf16_bits(a)
    bits = np.ascontiguousarray(bits)
    keep.append(bits)
    return bits.ctypes.data, a.shape[0], a.shape[1], max(a.shape[1], 1)


def _pair_csr_h16(Fa, Fb, code, m, alpha, weighted):
    """ss_similarity_dot_csr_h16 under the size protocol of ``_feature_pair_csr``."""
    dev = _is_torch(Fa)
    keep = []
    pa, na, d, lda = _features_h16(Fa, code, dev, keep)
    pb, nb, db, ldb = _features_h16(Fb, code, dev, keep)
    if Fb is None:
        nb, db, ldb = na, d, lda
    if db != d:
        raise ValueError("Fa and Fb have different numbers of features")
    fn = L_.lib().ss_similarity_dot_csr_h16
    nnz = C.c_int64(0)
    head = (pa, na, lda, pb, nb, ldb, d, code, m, C.c_float(alpha), 1 if weighted else 0)
    if dev:
        import torch
        ptr = torch.empty(na + 1, dtype=torch.int64, device=Fa.device)
        L_.check(fn(*head, ptr.data_ptr(), None, None, 0, C.byref(nnz), L_.SS_MEM_DEVICE))
        idx = torch.empty(max(nnz.value, 1), dtype=torch.int32, device=Fa.device)
        val = torch.empty(max(nnz.value, 1), dtype=torch.float32, device=Fa.device)
        L_.check(fn(*head, ptr.data_ptr(), idx.data_ptr(), val.data_ptr(), nnz.value, C.byref(nnz), L_.SS_MEM_DEVICE))
        del keep
        return ptr, idx[:nnz.value], val[:nnz.value]
    import scipy.sparse as sp
    ptr = np.zeros(na + 1, np.int64)
    L_.check(fn(*head, ptr.ctypes.data, None, None, 0, C.byref(nnz), L_.SS_MEM_HOST))
    idx = np.empty(max(nnz.value, 1), np.int32)
    val = np.empty(max(nnz.value, 1), np.float32)
    L_.check(fn(*head, ptr.ctypes.data, idx.ctypes.data, val.ctypes.data, nnz.value, C.byref(nnz), L_.SS_MEM_HOST))
    del keep
    return sp.csr_matrix((val[:nnz.value], idx[:nnz.value], ptr), shape=(na, nb))


NEIGHBOUR_K_MAX = 64


def quantize_i8(X):
    """Symmetric per-tensor quantisation of real numbers for ``storage="i8"``: ``(Q, scale)`` with
    ``Q = round(X * 127 / max|X|)`` (int8, same shape; round to nearest, ties to even) and ``scale = max|X| / 127``, so
    that ``X ~ Q * scale``.  An all-zero (or empty) X gives zeros and scale 1.  Cosine, Tanimoto and Dice are all
    invariant under a common scale of both sides, so the similarities of ``Q`` are those of ``Q * scale``: quantise
    every block that meets another one (sources and queries) with ONE scale, i.e. in one call.  A non-finite value
    raises ValueError."""
    a = np.asarray(X)
    if a.dtype.kind not in "fiub":
        raise TypeError(f"quantize_i8 needs real numbers, got {a.dtype}")
    a = a.astype(np.float64)
    if not np.isfinite(a).all():
        raise ValueError("quantize_i8: X holds a NaN or an infinity")
    top = float(np.abs(a).max(initial=0.0))
    if top == 0.0:
        return np.zeros(a.shape, np.int8), 1.0
    q = np.rint(a * (127.0 / top))
    return np.clip(q, -127, 127).astype(np.int8), top / 127.0


def _i8_storage(storage, inputs, dtype, min_neighbours=0, k_min=0) -> bool:
    """True when the call names the int8 route (storage == "i8"; it is never chosen by the inputs).  Needs no device.
    Checks what the route asks of the other arguments: a float32 graph, k in range, one memory kind."""
    if not (isinstance(storage, str) and storage == "i8"):
        return False
    if np.dtype(dtype) != np.float32:
        raise TypeError("int8 storage builds float32 graphs: dtype must be float32")
    k = int(min_neighbours)
    if k != min_neighbours or not k_min <= k <= NEIGHBOUR_K_MAX:
        raise ValueError(f"k / min_neighbours = {min_neighbours!r} outside {k_min}..{NEIGHBOUR_K_MAX}")
    given = [F for F in inputs if F is not None]
    if len({_module_is_torch(F) for F in given}) > 1:
        raise TypeError("features must all live on the host (numpy) or all on the device (CUDA tensors)")
    return True


def _features_i8(F, dev, keep):
    """(pointer, rows, d, ld) of int8 feature rows in the row-major layout of include/simspread_hip_int8.h.  Device: an
    (n, d) torch.int8 CUDA tensor, used in place when its rows are contiguous (ld = stride(0)).  Host: numpy int8 as it
    is.  Anything else must hold integers in -128 .. 127 and is converted exactly; there is no rounding: ValueError."""
    if F is None:
        return None, 0, 0, 1
    if dev:
        import torch
        if not (_module_is_torch(F) and F.is_cuda and F.ndim == 2):
            raise TypeError("device features must be (n, d) CUDA tensors")
        if F.dtype != torch.int8:
            if F.dtype == torch.bool or F.is_complex():
                raise ValueError(f"int8 storage needs integers in -128..127, got {F.dtype}")
            G = F.to(torch.int8)
            if F.numel() and not bool(((G.to(F.dtype) == F) & (F >= -128) & (F <= 127)).all()):
                raise ValueError("int8 storage needs integers in -128..127 (quantize_i8 rounds real numbers)")
            F = G
        n, d = F.shape
        rows_ok = d <= 1 or F.stride(1) == 1                  # the d bytes of a row are consecutive
        ld_ok = n <= 1 or F.stride(0) >= d                    # rows do not overlap
        if not (rows_ok and ld_ok):
            F = F.contiguous()
        keep.append(F)
        ld = F.stride(0) if n > 1 else d
        return F.data_ptr(), n, d, max(ld, d, 1)
    if _module_is_torch(F):
        raise TypeError("features must all live on the host (numpy) or all on the device (CUDA tensors)")
    a = np.asarray(F)
    if a.ndim != 2:
        raise ValueError("features must be an (n, d) matrix")
    if a.dtype != np.int8:
        if a.dtype.kind not in "fiu":
            raise ValueError(f"int8 storage needs integers in -128..127, got {a.dtype}")
        ok = a <= 127                                            # a NaN fails every comparison
        if a.dtype.kind != "u":
            ok = ok & (a >= -128)
        if a.dtype.kind == "f":
            with np.errstate(invalid="ignore"):
                ok = ok & (a == np.trunc(a))
        if not np.all(ok):
            raise ValueError("int8 storage needs integers in -128..127 (quantize_i8 rounds real numbers)")
        a = a.astype(np.int8)
    a = np.ascontiguousarray(a)
    keep.append(a)
    return a.ctypes.data, a.shape[0], a.shape[1], max(a.shape[1], 1)


def _pair_i8_operands(Fa, Fb):
    dev = _is_torch(Fa)
    keep = []
    pa, na, d, lda = _features_i8(Fa, dev, keep)
    pb, nb, db, ldb = _features_i8(Fb, dev, keep)
    if Fb is None:
        nb, db, ldb = na, d, lda
    if db != d:
        raise ValueError("Fa and Fb have different numbers of features")
    return dev, keep, (pa, na, lda, pb, nb, ldb, d), na, nb


def _pair_csr_i8(Fa, Fb, m, alpha, k, weighted):
    """ss_similarity_dot_csr_i8 under the size protocol of ``_feature_pair_csr``."""
    dev, keep, ops, na, nb = _pair_i8_operands(Fa, Fb)
    fn = L_.lib().ss_similarity_dot_csr_i8
    nnz = C.c_int64(0)
    head = ops + (m, C.c_float(alpha), int(k), 1 if weighted else 0)
    if dev:
        import torch
        ptr = torch.empty(na + 1, dtype=torch.int64, device=Fa.device)
        L_.check(fn(*head, ptr.data_ptr(), None, None, 0, C.byref(nnz), L_.SS_MEM_DEVICE))
        idx = torch.empty(max(nnz.value, 1), dtype=torch.int32, device=Fa.device)
        val = torch.empty(max(nnz.value, 1), dtype=torch.float32, device=Fa.device)
        L_.check(fn(*head, ptr.data_ptr(), idx.data_ptr(), val.data_ptr(), nnz.value, C.byref(nnz), L_.SS_MEM_DEVICE))
        del keep
        return ptr, idx[:nnz.value], val[:nnz.value]
    import scipy.sparse as sp
    ptr = np.zeros(na + 1, np.int64)
    L_.check(fn(*head, ptr.ctypes.data, None, None, 0, C.byref(nnz), L_.SS_MEM_HOST))
    idx = np.empty(max(nnz.value, 1), np.int32)
    val = np.empty(max(nnz.value, 1), np.float32)
    L_.check(fn(*head, ptr.ctypes.data, idx.ctypes.data, val.ctypes.data, nnz.value, C.byref(nnz), L_.SS_MEM_HOST))
    del keep
    return sp.csr_matrix((val[:nnz.value], idx[:nnz.value], ptr), shape=(na, nb))


def _kth_i8(Fa, Fb, m, k):
    """tau of ss_similarity_dot_kth_i8, as ``_feature_kth``."""
    dev, keep, ops, na, nb = _pair_i8_operands(Fa, Fb)
    fn = L_.lib().ss_similarity_dot_kth_i8
    head = ops + (m, int(k))
    if dev:
        import torch
        tau = torch.empty(na, dtype=torch.float32, device=Fa.device)
        L_.check(fn(*head, tau.data_ptr(), L_.SS_MEM_DEVICE))
        del keep
        return tau
    tau = np.empty(na, np.float32)
    L_.check(fn(*head, tau.ctypes.data, L_.SS_MEM_HOST))
    del keep
    return tau


def _feature_pair_csr(name, Fa, Fb, mid, alpha, weighted, dtype, min_neighbours=0):
    """The size protocol shared by the feature-row producers ss_similarity_<name>_csr_* and, with min_neighbours = k > 0,
    ss_similarity_<name>_floor_csr_* (k after alpha): `mid` are the arguments between d and alpha."""
    dt = _feature_dtype(dtype)
    dev = _is_torch(Fa)
    keep = []
    pa, na, d, lda = _features(Fa, dt, dev, keep)
    pb, nb, db, ldb = _features(Fb, dt, dev, keep)
    if Fb is None:
        nb, db, ldb = na, d, lda
    if db != d:
        raise ValueError("Fa and Fb have different numbers of features")
    floor = (int(min_neighbours),) if min_neighbours else ()
    fn = getattr(L_.lib(), f"ss_similarity_{name}{'_floor' if floor else ''}_csr_{_suffix(dt)}")
    ctype = C.c_float if dt == np.float32 else C.c_double
    nnz = C.c_int64(0)
    head = (pa, na, lda, pb, nb, ldb, d) + tuple(mid) + (ctype(alpha),) + floor + (1 if weighted else 0,)
    if dev:
        import torch
        ptr = torch.empty(na + 1, dtype=torch.int64, device=Fa.device)
        L_.check(fn(*head, ptr.data_ptr(), None, None, 0, C.byref(nnz), L_.SS_MEM_DEVICE))
        idx = torch.empty(max(nnz.value, 1), dtype=torch.int32, device=Fa.device)
        val = torch.empty(max(nnz.value, 1), dtype=torch.float32 if dt == np.float32 else torch.float64, device=Fa.device)
        L_.check(fn(*head, ptr.data_ptr(), idx.data_ptr(), val.data_ptr(), nnz.value, C.byref(nnz), L_.SS_MEM_DEVICE))
        del keep
        return ptr, idx[:nnz.value], val[:nnz.value]
    import scipy.sparse as sp
    ptr = np.zeros(na + 1, np.int64)
    L_.check(fn(*head, ptr.ctypes.data, None, None, 0, C.byref(nnz), L_.SS_MEM_HOST))
    idx = np.empty(max(nnz.value, 1), np.int32)
    val = np.empty(max(nnz.value, 1), dt)
    L_.check(fn(*head, ptr.ctypes.data, idx.ctypes.data, val.ctypes.data, nnz.value, C.byref(nnz), L_.SS_MEM_HOST))
    del keep
    return sp.csr_matrix((val[:nnz.value], idx[:nnz.value], ptr), shape=(na, nb))


def _feature_kth(name, Fa, Fb, mid, k, dtype):
    """tau of ss_similarity_<name>_kth_*: `mid` are the arguments between d and k."""
    if k is None:
        raise TypeError(f"{name}_kth needs k")
    dt = _feature_dtype(dtype)
    dev = _is_torch(Fa)
    keep = []
    pa, na, d, lda = _features(Fa, dt, dev, keep)
    pb, nb, db, ldb = _features(Fb, dt, dev, keep)
    if Fb is None:
        nb, db, ldb = na, d, lda
    if db != d:
        raise ValueError("Fa and Fb have different numbers of features")
    fn = getattr(L_.lib(), f"ss_similarity_{name}_kth_{_suffix(dt)}")
    head = (pa, na, lda, pb, nb, ldb, d) + tuple(mid) + (int(k),)
    if dev:
        import torch
        tau = torch.empty(na, dtype=torch.float32 if dt == np.float32 else torch.float64, device=Fa.device)
        L_.check(fn(*head, tau.data_ptr(), L_.SS_MEM_DEVICE))
        del keep
        return tau
    tau = np.empty(na, dt)
    L_.check(fn(*head, tau.ctypes.data, L_.SS_MEM_HOST))
    del keep
    return tau


def jaccard_kth(Fa, Fb=None, k=None, dtype=np.float32):
    """tau[i] = the k-th largest of the positive weighted-Jaccard similarities of row Fa[i] against the rows of Fb
    (multiplicity counted; Fb None: Fb = Fa, the diagonal included), +0 where a row has fewer than k: the per-row cut of
    ``jaccard_csr(..., min_neighbours=k)``, computed on the device without the dense similarity.  1 <= k <= 64.  Inputs
    as ``jaccard_csr``; host input returns a numpy vector, device input a CUDA tensor."""
    return _feature_kth("jaccard", Fa, Fb, (), k, dtype)


def dot_kth(Fa, Fb=None, metric="cosine", k=None, dtype=np.float32):
    """tau[i] of ``dot_csr(..., metric=metric, min_neighbours=k)``: the k-th largest of the positive similarities of row
    Fa[i] against the rows of Fb (Fb None: Fb = Fa, the diagonal, exactly 1, included), +0 where a row has fewer than k.
    Negative similarities never count.  1 <= k <= 64.  Inputs and outputs as ``jaccard_kth``.  The int8 route has its
    own entry, ``dot_kth_i8``."""
    return _feature_kth("dot", Fa, Fb, (_sim_metric(metric),), k, dtype)


def dot_kth_i8(Fa, Fb=None, metric="cosine", k=None):
    """``dot_kth`` on the exact int8 route: tau[i] of ``dot_csr(..., metric=metric, min_neighbours=k, storage="i8")``,
    float32, bit for bit the k-th largest positive value of the rule.  1 <= k <= 64.  Inputs as ``dot_csr`` with
    ``storage="i8"``; host input returns a numpy vector, device input a CUDA tensor."""
    if k is None:
        raise TypeError("dot_kth_i8 needs k")
    _i8_storage("i8", (Fa, Fb), np.float32, k, k_min=1)
    return _kth_i8(Fa, Fb, _sim_metric(metric), k)


def jaccard_csr(Fa, Fb=None, alpha=None, weighted: bool = True, dtype=np.float32, min_neighbours: int = 0):
    """``featurize(1 .- pairwise(Jaccard(), X, dims=1), alpha, weighted)`` for real-valued feature rows, produced as CSR
    on the device without the dense similarity: entry (i, j) = J(Fa[i], Fb[j]) = sum(min) / sum(max) (1 when both rows
    are all zero) when it is >= alpha (1 when not weighted), bitwise what ``jaccard_similarity`` followed by the cutoff
    gives.  Fb None: Fb = Fa.  Host input ((n, d) numpy) returns a scipy.sparse.csr_matrix; device input ((n, d) CUDA
    tensors of dtype) returns (ptr int64, idx int32, val) tensors.  A NaN feature or alpha raises SimSpreadError.
    min_neighbours = k > 0 (at most 64) adds the neighbour floor, as ``tanimoto_csr``: row i also keeps every positive
    similarity >= tau_i (``jaccard_kth``), i.e. at least its k nearest columns whatever alpha says (alpha = inf: exactly
    those); ties at tau_i are all kept, a row with fewer than k positive similarities keeps all of them, and the result
    is in general not symmetric."""
    if alpha is None:
        raise TypeError("jaccard_csr needs alpha")
    return _feature_pair_csr("jaccard", Fa, Fb, (), alpha, weighted, dtype, min_neighbours)


def dot_csr(Fa, Fb=None, metric="cosine", alpha=None, weighted: bool = True, dtype=np.float32, min_neighbours: int = 0,
            storage=None):
    """``featurize(S, alpha, weighted)`` with S an inner-product similarity of real-valued rows (embeddings, continuous
    descriptors), produced as CSR on the device without the dense similarity; the Gram blocks run on the matrix cores in
    full ``dtype`` precision.  metric: "cosine" g / (|a| |b|), "tanimoto" g / (|a|^2 + |b|^2 - g), "dice" 2g / (|a|^2 +
    |b|^2), g = a.b; two all-zero rows have s = 1, a zero row against a non-zero one s = 0.  Entry (i, j) = s when it
    is >= alpha (1 when not weighted).  Fb None: Fb = Fa (the diagonal is exactly 1 and the matrix bitwise symmetric).
    Inputs and outputs as ``jaccard_csr``.  A NaN feature or alpha raises SimSpreadError.  min_neighbours = k > 0 (at
    most 64) adds the neighbour floor as there (``dot_kth``): negative similarities never count among the k, the
    diagonal of Fb = Fa stays exactly 1 and counts, and the floor matrix is not symmetric.

    storage "bf16" / "f16" takes the 16-bit route (include/simspread_hip_half.h): the rows are bfloat16 / half values,
    the Gram blocks run on the 16-bit matrix instructions with fp32 accumulation -- every product is exact, so the result
    is a valid output of the fp32 rule on the widened inputs up to the order of the sums, and bitwise the fp32 result
    when all partial sums are exact.  CUDA tensors of torch.bfloat16 / torch.float16 select it by their dtype and are
    read in place, row-major, when ``stride(1) == 1`` (no copy, no widening); numpy float16 arrays select "f16" when
    every input is float16, dtype is float32 and min_neighbours is 0 (otherwise they are widened exactly, as before); with
    an explicit storage numpy uint16 arrays are raw bit patterns and other real arrays are rounded on the host (nearest
    even; ``to_bf16_bits``).  dtype must be float32; min_neighbours > 0 raises NotImplementedError.

    storage "i8" takes the exact int8 route (include/simspread_hip_int8.h), only when named: the rows are signed 8-bit
    integers, the Gram blocks run on the integer matrix instruction and g, |a|^2, |b|^2 are exact integers (d <=
    131071), each converted to float32 once, so the CSR is bitwise defined for every input, at a quarter of the bytes
    of float32 rows.  min_neighbours is allowed.  Inputs: numpy int8 as it is; torch.int8 CUDA tensors, read in place,
    row-major, when ``stride(1) == 1``; any other array whose values are integers in -128 .. 127, converted exactly --
    anything else raises ValueError (``quantize_i8`` rounds real numbers).  dtype must be float32."""
    if alpha is None:
        raise TypeError("dot_csr needs alpha")
    if _i8_storage(storage, (Fa, Fb), dtype, min_neighbours):
        return _pair_csr_i8(Fa, Fb, _sim_metric(metric), alpha, min_neighbours, weighted)
    code = _h16_storage(storage, (Fa, Fb), dtype, min_neighbours)
    if code is not None:
        return _pair_csr_h16(Fa, Fb, code, _sim_metric(metric), alpha, weighted)
    return _feature_pair_csr("dot", Fa, Fb, (_sim_metric(metric),), alpha, weighted, dtype, min_neighbours)


PROFILE_CUTS_MAX = 32


def _profile_cuts(cuts, dt) -> np.ndarray:
    """The cuts of a profile as a contiguous vector of dt: 1..32 of them, nondecreasing, no NaN (ValueError otherwise).
    Needs no device.  They are compared after the conversion to dt, as the library compares them."""
    if cuts is None or cuts is Ellipsis:
        raise TypeError("a cutoff profile needs cuts")
    c = np.atleast_1d(np.asarray(cuts, dtype=np.float64))
    if c.ndim != 1:
        raise ValueError("cuts must be a vector")
    if not 1 <= c.size <= PROFILE_CUTS_MAX:
        raise ValueError(f"a profile takes 1..{PROFILE_CUTS_MAX} cuts, got {c.size}")
    if np.isnan(c).any():
        raise ValueError("a cut is NaN")
    with np.errstate(over="ignore"):
        c = np.ascontiguousarray(c.astype(dt))
    if (c[1:] < c[:-1]).any():
        raise ValueError("cuts must be sorted (nondecreasing)")
    return c


class CutoffProfile:
    """What ``tanimoto_profile`` / ``jaccard_profile`` / ``dot_profile`` return: for every cut b, the size and the row
    degrees of the graph the matching ``*_csr`` producer builds at ``alpha = cuts[b]``, from one pass over the pairs.

    cuts      (ncuts,) the cuts, in the graph's dtype, ascending
    nnz       (ncuts,) int64: the producer's nnz at each cut (exact also at and above 2^31, where the producer refuses)
    degrees   (na, ncuts) int32: row i's entries at each cut, ``ptr[i + 1] - ptr[i]`` of the producer; numpy for host
              input, a CUDA tensor for device input
    shape     (na, nb)
    symmetric Fb was None: the graph is Fa against itself and holds its diagonal, whose similarity is 1

    The members below work on the host in numpy (device degrees are copied once per call)."""

    def __init__(self, cuts, nnz, degrees, shape, symmetric=False):
        self.cuts = np.asarray(cuts)
        self.nnz = np.asarray(nnz, dtype=np.int64)
        self.degrees = degrees
        self.shape = (int(shape[0]), int(shape[1]))
        self.symmetric = bool(symmetric)

    def __repr__(self):
        return f"CutoffProfile(shape={self.shape}, cuts={self.cuts.tolist()}, nnz={self.nnz.tolist()})"

    def _host_degrees(self) -> np.ndarray:
        d = self.degrees
        if _module_is_torch(d):
            d = d.cpu().numpy()
        return np.asarray(d).reshape(self.shape[0], self.cuts.size)

    def fill(self) -> np.ndarray:
        """nnz / (na * nb) per cut: the share of the pairs that are entries (0 for an empty shape)."""
        pairs = self.shape[0] * self.shape[1]
        if pairs == 0:
            return np.zeros(self.cuts.size)
        return self.nnz / float(pairs)

    def coverage(self, min_degree: int = 1, exclude_self: bool = False) -> np.ndarray:
        """Per cut, the share of rows with at least min_degree entries (0 when there are no rows): with the defaults the
        rows that still have a neighbour, the quantity that trades against accuracy when alpha rises.  exclude_self
        (symmetric profiles only) does not count a row's own diagonal entry: its similarity is 1, so it is an entry of
        the graph exactly at the cuts <= 1, and there 1 is subtracted from every non-zero degree first."""
        if exclude_self and not self.symmetric:
            raise ValueError("exclude_self needs a symmetric profile (Fb=None)")
        deg = self._host_degrees().astype(np.int64)
        if deg.shape[0] == 0:
            return np.zeros(self.cuts.size)
        if exclude_self:
            deg = np.maximum(deg - (self.cuts <= 1).astype(np.int64)[None, :], 0)
        return (deg >= int(min_degree)).mean(axis=0)

    def alpha_for_nnz(self, budget):
        """The smallest cut whose nnz <= budget (the lowest alpha whose graph fits), None when none does."""
        ok = np.flatnonzero(self.nnz <= budget)
        return self.cuts[ok[0]].item() if ok.size else None

    def alpha_for_mean_degree(self, k):
        """The smallest cut whose mean row degree nnz / na <= k, None when none has."""
        ok = np.flatnonzero(self.nnz <= k * self.shape[0])
        return self.cuts[ok[0]].item() if ok.size else None


def _profile_call(fn, head, na, nb, cuts, weighted, dev, device, symmetric):
    """One ss_similarity_*_profile_* call: `head` are the operands up to the cuts."""
    nc = cuts.size
    tail = (cuts.ctypes.data, nc, 1 if weighted else 0)
    if dev:
        import torch
        total = torch.zeros(nc, dtype=torch.int64, device=device)
        deg = torch.zeros((na, nc), dtype=torch.int32, device=device)
        L_.check(fn(*head, *tail, total.data_ptr(), deg.data_ptr(), L_.SS_MEM_DEVICE))
        return CutoffProfile(cuts, total.cpu().numpy(), deg, (na, nb), symmetric)
    total = np.zeros(nc, np.int64)
    deg = np.zeros((na, nc), np.int32)
    L_.check(fn(*head, *tail, total.ctypes.data, deg.ctypes.data, L_.SS_MEM_HOST))
    return CutoffProfile(cuts, total, deg, (na, nb), symmetric)


def tanimoto_profile(Fa, Fb=None, cuts=None, weighted: bool = True, dtype=np.float32):
    """The cutoff profile of ``tanimoto_csr``: for up to 32 ascending cuts, the nnz and the row degrees of
    ``tanimoto_csr(Fa, Fb, alpha=cut, weighted=weighted, dtype=dtype)`` at every cut, bit for bit, from ONE pass over
    the pairs and without building a graph (the similarity of a pair does not depend on alpha).  Inputs as
    ``tanimoto_csr``; returns a ``CutoffProfile``.  Cuts that are unsorted, NaN, none or more than 32 raise ValueError
    (checked here, no device needed); equal cuts and +-inf are fine.  There is no 2^31 refusal: the profile answers at
    cuts where the producer would refuse."""
    dt = _feature_dtype(dtype)
    c = _profile_cuts(cuts, dt)
    fn = getattr(L_.lib(), f"ss_similarity_tanimoto_profile_{_suffix(dt)}")
    dev = _is_torch(Fa)
    keep = []
    pa, na, nw = _fingerprints(Fa, dev, keep)
    pb, nb, nwb = _fingerprints(Fb, dev, keep)
    if Fb is None:
        nb, nwb = na, nw
    if nwb != nw:
        raise ValueError("Fa and Fb have different fingerprint widths")
    out = _profile_call(fn, (pa, na, pb, nb, nw), na, nb, c, weighted, dev, Fa.device if dev else None, Fb is None)
    del keep
    return out


def _feature_profile(name, Fa, Fb, mid, cuts, weighted, dtype):
    """ss_similarity_<name>_profile_*: `mid` are the arguments between d and the cuts."""
    dt = _feature_dtype(dtype)
    c = _profile_cuts(cuts, dt)
    dev = _is_torch(Fa)
    keep = []
    pa, na, d, lda = _features(Fa, dt, dev, keep)
    pb, nb, db, ldb = _features(Fb, dt, dev, keep)
    if Fb is None:
        nb, db, ldb = na, d, lda
    if db != d:
        raise ValueError("Fa and Fb have different numbers of features")
    fn = getattr(L_.lib(), f"ss_similarity_{name}_profile_{_suffix(dt)}")
    out = _profile_call(fn, (pa, na, lda, pb, nb, ldb, d) + tuple(mid), na, nb, c, weighted, dev,
                        Fa.device if dev else None, Fb is None)
    del keep
    return out


def jaccard_profile(Fa, Fb=None, cuts=None, weighted: bool = True, dtype=np.float32):
    """The cutoff profile of ``jaccard_csr`` (weighted Jaccard of real-valued rows), as ``tanimoto_profile``.  A NaN
    feature raises SimSpreadError, as in the producer."""
    return _feature_profile("jaccard", Fa, Fb, (), cuts, weighted, dtype)


def dot_profile(Fa, Fb=None, metric="cosine", cuts=None, weighted: bool = True, dtype=np.float32, storage=None):
    """The cutoff profile of ``dot_csr`` (cosine / Tanimoto / Dice of real-valued rows on the matrix cores), as
    ``tanimoto_profile``: inputs, metric, ``storage`` and the choice of the 16-bit route exactly as ``dot_csr`` with
    ``min_neighbours=0`` (16-bit CUDA tensors and storage "bf16" / "f16" take it; dtype must then be float32).  In
    symmetric mode the diagonal counts with s = 1 exactly, and the degrees are those of the bitwise symmetric matrix."""
    m = _sim_metric(metric)
    code = _h16_storage(storage, (Fa, Fb), dtype)
    if code is None:
        return _feature_profile("dot", Fa, Fb, (m,), cuts, weighted, dtype)
    c = _profile_cuts(cuts, np.float32)
    dev = _is_torch(Fa)
    keep = []
    pa, na, d, lda = _features_h16(Fa, code, dev, keep)
    pb, nb, db, ldb = _features_h16(Fb, code, dev, keep)
    if Fb is None:
        nb, db, ldb = na, d, lda
    if db != d:
        raise ValueError("Fa and Fb have different numbers of features")
    out = _profile_call(L_.lib().ss_similarity_dot_profile_h16, (pa, na, lda, pb, nb, ldb, d, code, m), na, nb, c,
                        weighted, dev, Fa.device if dev else None, Fb is None)
    del keep
    return out


def cutoff_csr(X, alpha: float, weighted: bool = False, dtype=np.float32, shape=None):
    """``featurize(X, alpha, weighted)`` on a sparse matrix, on the device: entry (i, j) with stored value v stays iff
    v >= alpha, as v when weighted and 1 otherwise (alpha > 0: the non-zeros of ``cutoff`` on the densified matrix).
    X: a scipy.sparse matrix (returns a scipy.sparse.csr_matrix), or device CSR parts (ptr int64, idx int32, val or
    None) of torch CUDA tensors with ``shape=(rows, cols)`` (returns (ptr, idx, val) tensors, 0-based)."""
    dt = _feature_dtype(dtype)
    fn = getattr(L_.lib(), f"ss_cutoff_csr_{_suffix(dt)}")
    ctype = C.c_float if dt == np.float32 else C.c_double
    nnz = C.c_int64(0)
    w = 1 if weighted else 0
    if isinstance(X, (tuple, list)) and _is_torch(X[0]):
        import torch
        if shape is None:
            raise TypeError("device CSR parts need shape=(rows, cols)")
        rows, cols = int(shape[0]), int(shape[1])
        want = torch.float32 if dt == np.float32 else torch.float64
        ip, ii, iv = X[0].to(torch.int64).contiguous(), X[1].to(torch.int32).contiguous(), X[2]
        iv = None if iv is None else iv.to(want).contiguous()
        if ip.numel() != rows + 1:
            raise ValueError("ptr must have rows + 1 entries")
        pv = None if iv is None else iv.data_ptr()
        ptr = torch.empty(rows + 1, dtype=torch.int64, device=ip.device)
        L_.check(fn(rows, cols, ip.data_ptr(), ii.data_ptr(), pv, 0, ctype(alpha), w, ptr.data_ptr(), None, None, 0,
                    C.byref(nnz), L_.SS_MEM_DEVICE))
        idx = torch.empty(max(nnz.value, 1), dtype=torch.int32, device=ip.device)
        val = torch.empty(max(nnz.value, 1), dtype=want, device=ip.device)
        L_.check(fn(rows, cols, ip.data_ptr(), ii.data_ptr(), pv, 0, ctype(alpha), w, ptr.data_ptr(), idx.data_ptr(),
                    val.data_ptr(), nnz.value, C.byref(nnz), L_.SS_MEM_DEVICE))
        return ptr, idx[:nnz.value], val[:nnz.value]
    import scipy.sparse as sp
    X = sp.csr_matrix(X)
    rows, cols = X.shape
    ip, ii, iv = _csr_parts(X, dt)
    ptr = np.zeros(rows + 1, np.int64)
    L_.check(fn(rows, cols, _ptr(ip), _ptr(ii), _ptr(iv), 0, ctype(alpha), w, ptr.ctypes.data, None, None, 0,
                C.byref(nnz), L_.SS_MEM_HOST))
    idx = np.empty(max(nnz.value, 1), np.int32)
    val = np.empty(max(nnz.value, 1), dt)
    L_.check(fn(rows, cols, _ptr(ip), _ptr(ii), _ptr(iv), 0, ctype(alpha), w, ptr.ctypes.data, idx.ctypes.data,
                val.ctypes.data, nnz.value, C.byref(nnz), L_.SS_MEM_HOST))
    return sp.csr_matrix((val[:nnz.value], idx[:nnz.value], ptr), shape=(rows, cols))


# ------------------------------------------------------------------ Butina clusters, cluster folds, cross-fold edges
class ButinaClusters:
    """Result of ``butina_clusters``: ``centre[i]`` the index of source i's centre (``centre[c] == c`` for a centre),
    ``label[i]`` its cluster, clusters numbered 0..nclusters-1 in priority order of their centres, ``size[l]`` the number
    of sources with label l, and ``rounds`` the number of rounds the device loop took.  Arrays are numpy for host input
    and CUDA tensors for device input, always 0-based."""

    __slots__ = ("centre", "label", "size", "rounds")

    def __init__(self, centre, label, size, rounds):
        self.centre, self.label, self.size, self.rounds = centre, label, size, int(rounds)

    @property
    def nclusters(self) -> int:
        return int(self.size.shape[0])

    def __repr__(self):
        return f"ButinaClusters(n={int(self.label.shape[0])}, nclusters={self.nclusters}, rounds={self.rounds})"


def _pattern(X, index_base=0):
    """(dev, n, ptr pointer, idx pointer, index_base, keep) of an n x n neighbour pattern: a scipy.sparse matrix (or
    anything csr_matrix accepts), or CSR parts (ptr int64, idx int32[, val]) as numpy arrays or torch CUDA tensors, read
    with ``index_base`` and as they are -- unsorted rows, duplicates and diagonal entries included."""
    if index_base not in (0, 1):
        raise ValueError("index_base must be 0 or 1")
    if isinstance(X, (tuple, list)):
        if len(X) not in (2, 3):
            raise TypeError("CSR parts are (ptr, idx) or (ptr, idx, val)")
        if _is_torch(X[0]):
            import torch
            ptr, idx = X[0].to(torch.int64).contiguous(), X[1].to(torch.int32).contiguous()
            if not (ptr.is_cuda and idx.is_cuda):
                raise TypeError("CSR parts must all live on the host (numpy) or all on the device (CUDA tensors)")
            if ptr.numel() < 1:
                raise ValueError("ptr must have n + 1 entries")
            return True, ptr.numel() - 1, ptr.data_ptr(), idx.data_ptr(), index_base, [ptr, idx]
        ptr = np.ascontiguousarray(X[0], dtype=np.int64)
        idx = np.ascontiguousarray(X[1], dtype=np.int32)
        if ptr.ndim != 1 or ptr.size < 1:
            raise ValueError("ptr must have n + 1 entries")
        if idx.size < ptr[-1] - index_base:
            raise ValueError("idx is shorter than the row pointers say")
        return False, ptr.size - 1, ptr.ctypes.data, idx.ctypes.data, index_base, [ptr, idx]
    import scipy.sparse as sp
    if index_base != 0:
        raise ValueError("a scipy.sparse matrix is 0-based: index_base applies to CSR parts only")
    m = sp.csr_matrix(X)
    if m.shape[0] != m.shape[1]:
        raise ValueError(f"a neighbour pattern is square, got {m.shape}")
    ptr = np.ascontiguousarray(m.indptr, dtype=np.int64)
    idx = np.ascontiguousarray(m.indices, dtype=np.int32)
    return False, m.shape[0], ptr.ctypes.data, idx.ctypes.data, 0, [ptr, idx]


def butina_clusters(X=None, *, fingerprints=None, features=None, vectors=None, metric="cosine", cutoff=None,
                    dtype=np.float32, index_base=0) -> ButinaClusters:
    """Taylor-Butina clusters (without re-counting) of the sources, on the device.  Exactly one input:

    - ``X``: an n x n neighbour pattern (values are not read) -- scipy.sparse, or CSR parts ``(ptr, idx[, val])`` as
      numpy arrays or torch CUDA tensors with ``index_base`` 0 or 1; it is symmetrised by union, diagonal and duplicate
      entries are ignored;
    - ``fingerprints`` (packed, see ``pack_fingerprints``), ``features`` ((n, d) rows, weighted Jaccard) or ``vectors``
      ((n, d) rows, ``metric`` "cosine", "tanimoto" or "dice") with ``cutoff``: the pattern ``s >= cutoff`` of
      ``tanimoto_csr`` / ``jaccard_csr`` / ``dot_csr`` on the rows themselves, made and consumed on the device.

    The rule: neighbours N(i) = {j != i : (i,j) or (j,i) stored}, degree d_i = |N(i)|; i precedes j iff d_i > d_j, or
    d_i == d_j and i < j; in that order every still-unassigned source becomes a centre and takes its still-unassigned
    neighbours.  Ties between equal degrees go to the lower index, which is not RDKit's tie order.  The result is
    unique and bitwise repeatable."""
    given = [a is not None for a in (X, fingerprints, features, vectors)]
    if sum(given) != 1:
        raise TypeError("butina_clusters needs exactly one of X, fingerprints=, features=, vectors=")
    if vectors is not None and _module_is_torch(vectors) and str(vectors.dtype) in ("torch.bfloat16", "torch.float16"):
        raise NotImplementedError("butina_clusters has no 16-bit route (its selection would have to run the 16-bit Gram "
                                  "tile): cluster the pattern of dot_csr(vectors, weighted=False) or widen the vectors")
    lib = L_.lib()
    keep = []
    if X is not None:
        if cutoff is not None:
            raise TypeError("cutoff applies to fingerprints=, features= and vectors=; cut a pattern with cutoff_csr")
        dev, n, pp, pi, base, keep = _pattern(X, index_base)
        fn, head = lib.ss_cluster_butina_csr, (n, pp, pi, base)
    else:
        if cutoff is None:
            raise TypeError("butina_clusters needs cutoff")
        dt = _feature_dtype(dtype)
        ctype = C.c_float if dt == np.float32 else C.c_double
        if fingerprints is not None:
            dev = _is_torch(fingerprints)
            pf, n, nw = _fingerprints(fingerprints, dev, keep)
            fn, head = getattr(lib, f"ss_cluster_butina_fingerprint_{_suffix(dt)}"), (pf, n, nw, ctype(cutoff))
        elif features is not None:
            dev = _is_torch(features)
            pf, n, d, ld = _features(features, dt, dev, keep)
            fn, head = getattr(lib, f"ss_cluster_butina_features_{_suffix(dt)}"), (pf, n, d, ld, ctype(cutoff))
        else:
            dev = _is_torch(vectors)
            pf, n, d, ld = _features(vectors, dt, dev, keep)
            fn = getattr(lib, f"ss_cluster_butina_vectors_{_suffix(dt)}")
            head = (_sim_metric(metric), pf, n, d, ld, ctype(cutoff))
    nc, rounds = C.c_int64(0), C.c_int64(0)
    if dev:
        import torch
        centre, label, size = (torch.empty(max(n, 1), dtype=torch.int32, device="cuda") for _ in range(3))
        L_.check(fn(*head, centre.data_ptr(), label.data_ptr(), size.data_ptr(), C.byref(nc), C.byref(rounds),
                    L_.SS_MEM_DEVICE))
    else:
        centre, label, size = (np.empty(max(n, 1), np.int32) for _ in range(3))
        L_.check(fn(*head, centre.ctypes.data, label.ctypes.data, size.ctypes.data, C.byref(nc), C.byref(rounds),
                    L_.SS_MEM_HOST))
    del keep
    return ButinaClusters(centre[:n], label[:n], size[:nc.value], rounds.value)


def cluster_folds(label, nfolds: int):
    """``fold_of_source`` (int32, ids in [0, nfolds)) that keeps every cluster of ``label`` (``butina_clusters(...).label``)
    in one fold: clusters by size descending (ties: label ascending), each to the fold with the fewest sources so far
    (ties: the lowest fold id).  Deterministic; the folds differ in size by at most the largest cluster.  The vector goes
    straight into ``predict_kfold`` / ``evaluate_kfold``.  numpy in, numpy out; CUDA tensor in, CUDA tensor out."""
    lib = L_.lib()
    if _is_torch(label):
        import torch
        lab = label.to(torch.int32).contiguous()
        n = lab.numel()
        nc = int(lab.max().item()) + 1 if n else 0
        fold = torch.empty(max(n, 1), dtype=torch.int32, device=lab.device)
        L_.check(lib.ss_cluster_folds(lab.data_ptr(), n, nc, int(nfolds), fold.data_ptr(), L_.SS_MEM_DEVICE))
        return fold[:n]
    lab = np.ascontiguousarray(label, dtype=np.int32)
    if lab.ndim != 1:
        raise ValueError("label must be a vector")
    n = lab.size
    nc = int(lab.max()) + 1 if n else 0
    fold = np.empty(max(n, 1), np.int32)
    L_.check(lib.ss_cluster_folds(lab.ctypes.data, n, nc, int(nfolds), fold.ctypes.data, L_.SS_MEM_HOST))
    return fold[:n]


def cross_fold_edges(X, fold_of_source, nfolds: int, index_base=0):
    """How much a split leaks: ``count[f]`` (int64) = the number of stored off-diagonal entries (i, j) of the neighbour
    pattern ``X`` (as for ``butina_clusters``; read as given, not symmetrised) with ``fold_of_source[i] == f !=
    fold_of_source[j]``.  Host input returns numpy, device input (CSR parts and folds as CUDA tensors) a CUDA tensor."""
    lib = L_.lib()
    dev, n, pp, pi, base, keep = _pattern(X, index_base)
    nfolds = int(nfolds)
    if dev:
        import torch
        fold = torch.as_tensor(fold_of_source, device="cuda").to(torch.int32).contiguous()
        if fold.numel() != n:
            raise ValueError("fold_of_source needs one entry per source")
        count = torch.zeros(max(nfolds, 1), dtype=torch.int64, device="cuda")
        L_.check(lib.ss_cluster_cross_edges(n, pp, pi, base, fold.data_ptr(), nfolds, count.data_ptr(),
                                            L_.SS_MEM_DEVICE))
        return count[:max(nfolds, 0)]
    fold = np.ascontiguousarray(fold_of_source, dtype=np.int32)
    if fold.shape != (n,):
        raise ValueError("fold_of_source needs one entry per source")
    count = np.zeros(max(nfolds, 1), np.int64)
    L_.check(lib.ss_cluster_cross_edges(n, pp, pi, base, fold.ctypes.data, nfolds, count.ctypes.data, L_.SS_MEM_HOST))
    del keep
    return count[:max(nfolds, 0)]
