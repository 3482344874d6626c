"""Per-row binary prediction metrics on the device (ss_binary_metrics_rows_*) and the leave-one-out sweep judged by them
in place (ss_evaluate_loo_binary_*), against the host reference of tests/binary_ref.py and the host mirror
(ss.maxperformance / ss.meanstdperformance)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import scipy.sparse as sp

import simspread_jl_amd as ss
from binary_ref import assert_binary_close, ref_rows
from simspread_jl_amd import _lib

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _check(got, Y, S, what):
    want, scale = ref_rows(Y, S, with_scale=True)
    assert_binary_close(got, want, scale, what)


def _cases(ncols, rng, dtype):
    """A batch of rows of one width covering the edge cases; returns dense labels and scores (in dtype)."""
    rows_y, rows_s = [], []

    def add(y, s):
        rows_y.append(np.asarray(y, np.uint8))
        rows_s.append(np.asarray(s, np.float64))

    cont = rng.random(ncols)
    few = rng.choice(np.array([0.0, 0.25, 0.5, 1.0]), ncols)
    y = (rng.random(ncols) < 0.3).astype(np.uint8); y[0] = 1
    add(np.zeros(ncols), cont)                                   # P = 0
    add(np.ones(ncols), cont)                                    # N = 0
    add(np.ones(ncols), few)                                     # N = 0, ties
    add(y, np.full(ncols, 0.5))                                  # one distinct score
    add(y, np.zeros(ncols))                                      # all zeros
    add(y, np.full(ncols, -99.0))                                # all -99 (clean!)
    add(y, few)                                                  # heavy ties
    add(y, rng.integers(0, 5, ncols).astype(np.float64))         # integer-valued scores
    m = few.copy(); m[rng.random(ncols) < 0.3] = -99.0
    add(y, m)                                                    # ties and -99
    z = np.where(rng.random(ncols) < 0.5, 0.0, cont); z[rng.random(ncols) < 0.2] = -0.0
    add(y, z)                                                    # zeros of both signs
    y1 = np.zeros(ncols); y1[rng.integers(ncols)] = 1
    add(y1, cont)                                                # P = 1
    for _ in range(3):
        add((rng.random(ncols) < rng.random()).astype(np.uint8), np.where(rng.random(ncols) < 0.5, 0.0, cont))
    return np.stack(rows_y), np.stack(rows_s).astype(dtype)


def _raw(dtype, ptr, idx, base, S, ld, out, mem, nrows, ncols):
    fn = getattr(_lib.lib(), "ss_binary_metrics_rows_" + ("f32" if dtype == np.float32 else "f64"))
    return fn(ptr, idx, base, S, nrows, ncols, ld, out, mem)


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("ncols, pad", [(1, 0), (2, 3), (37, 0), (300, 7)])
def test_case_matrix_host_device_torch(dtype, ncols, pad):
    import torch
    ss.init(0)
    rng = np.random.default_rng(2000 + ncols)
    Y, S = _cases(ncols, rng, dtype)
    nrows = S.shape[0]
    got = ss.binary_metrics_rows(Y, S)
    assert got.shape == (nrows, 18) and got.dtype == np.float64
    _check(got, Y, S, f"{np.dtype(dtype).name} ncols={ncols}")
    assert "binary_rows_lds" in ss.path_last()
    np.testing.assert_array_equal(ss.binary_metrics_rows(sp.csr_matrix(Y), S), got)   # repeatable, scipy labels
    tS = torch.from_numpy(S).cuda()
    g1 = ss.binary_metrics_rows(Y, tS)
    assert g1.is_cuda and g1.dtype == torch.float64
    np.testing.assert_array_equal(g1.cpu().numpy(), got)
    m = sp.csr_matrix(Y)
    dptr = torch.from_numpy(m.indptr.astype(np.int64)).cuda()
    didx = torch.from_numpy(m.indices.astype(np.int32) if m.nnz else np.zeros(1, np.int32)).cuda()
    np.testing.assert_array_equal(ss.binary_metrics_rows((dptr, didx), tS).cpu().numpy(), got)
    # one row given 1-D
    np.testing.assert_array_equal(ss.binary_metrics_rows(Y[6], S[6]), got[6])
    # raw ABI: ld > ncols, a label slice of a larger CSR (yptr[0] != base), index_base 0 and 1; host and device memory
    ld = ncols + pad
    Sp = np.zeros((nrows, ld), dtype); Sp[:, :ncols] = S
    lead = np.ones((3, ncols), np.uint8)                                       # 3 rows in front of the slice
    big = sp.csr_matrix(np.vstack([lead, Y]))
    for base in (0, 1):
        ptr = (big.indptr.astype(np.int64) + base)[3:]
        idx = big.indices.astype(np.int32) + base
        assert ptr[0] != base
        out = np.full((nrows, 18), -7.0)
        assert _raw(dtype, ptr.ctypes.data, idx.ctypes.data, base, Sp.ctypes.data, ld, out.ctypes.data,
                    _lib.SS_MEM_HOST, nrows, ncols) == 0
        np.testing.assert_array_equal(out, got)
        tp, ti, tsp = (torch.from_numpy(a).cuda() for a in (ptr, idx, Sp))
        tout = torch.full((nrows, 18), -7.0, dtype=torch.float64, device="cuda")
        ss.use_torch_stream()
        assert _raw(dtype, tp.data_ptr(), ti.data_ptr(), base, tsp.data_ptr(), ld, tout.data_ptr(),
                    _lib.SS_MEM_DEVICE, nrows, ncols) == 0
        np.testing.assert_array_equal(tout.cpu().numpy(), got)
    assert _raw(dtype, ptr.ctypes.data, idx.ctypes.data, 0, Sp.ctypes.data, ld, None, _lib.SS_MEM_HOST, 0, ncols) == 0


def test_against_the_host_mirror():
    """Small rows straight against ss.maxperformance / ss.meanstdperformance (max bitwise)."""
    ss.init(0)
    rng = np.random.default_rng(8)
    for dtype in (np.float32, np.float64):
        S = rng.choice(np.array([0.0, 0.1, 0.3, 0.7, -99.0]), (12, 25)).astype(dtype)
        S[6:] = rng.random((6, 25))
        Y = (rng.random((12, 25)) < 0.4).astype(np.uint8)
        Y[:, 0] = 1; Y[:, 1] = 0
        got = ss.binary_metrics_rows(Y, S).reshape(-1, 6, 3)
        fns = [ss.f1score, ss.mcc, ss.accuracy, ss.balancedaccuracy, ss.recall, ss.precision]
        for r in range(12):
            for k, f in enumerate(fns):
                mean, std = ss.meanstdperformance(Y[r], S[r], f)
                assert got[r, k, 0] == ss.maxperformance(Y[r], S[r], f), (r, k)
                assert abs(got[r, k, 1] - mean) <= 1e-12 and abs(got[r, k, 2] - std) <= 1e-10, (r, k)


def test_fp64_scores_below_fp32_resolution_are_not_ties():
    ss.init(0)
    n = 64
    rng = np.random.default_rng(5)
    s64 = (1.0 + rng.permutation(n) * 1e-12)[None]              # distinct in fp64, one value in fp32
    y = (rng.random((1, n)) < 0.3).astype(np.uint8)
    got64 = ss.binary_metrics_rows(y, s64)
    _check(got64, y, s64, "fp64")
    assert not np.isnan(got64[0, 2])                             # U = 64: f1 has a std
    got32 = ss.binary_metrics_rows(y, s64.astype(np.float32))
    _check(got32, y, s64.astype(np.float32), "fp32 rounded")
    assert np.isnan(got32[0, 2])                                 # U = 1


def _path_rows(ncols, dtype, seed):
    rng = np.random.default_rng(seed)
    S = np.empty((5, ncols))
    S[0] = rng.random(ncols)
    S[1] = rng.choice(np.array([0.0, 0.5, 1.0, -99.0]), ncols)
    S[2] = np.round(rng.random(ncols), 3)
    S[3] = np.where(rng.random(ncols) < 0.6, 0.0, rng.random(ncols))
    S[4] = rng.integers(0, 50, ncols)
    Y = (rng.random((5, ncols)) < np.array([[0.3], [0.5], [0.01], [0.9], [0.2]])).astype(np.uint8)
    return Y, S.astype(dtype)


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("ncols, path", [(7, "lds"), (4000, "lds"), (16384, "lds"), (60000, "large"),
                                         (100000, "large")])
def test_both_paths_against_the_reference(dtype, ncols, path):
    ss.init(0)
    Y, S = _path_rows(ncols, dtype, ncols)
    got = ss.binary_metrics_rows(Y, S)
    assert ss.path_last() == ["binary_rows_" + path], ss.path_last()
    _check(got, Y, S, f"{np.dtype(dtype).name} ncols={ncols}")
    for i in range(2):  # a row alone: the same bits
        np.testing.assert_array_equal(ss.binary_metrics_rows(Y[i:i + 1], S[i:i + 1]), got[i:i + 1])


_CHILD = r"""
import json, sys
import numpy as np
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[1] + "/tests")
import simspread_jl_amd as ss
from test_gpu_binary_rows import _path_rows
ss.init(0)
res = {}
for ncols in (7, 4000, 16384):
    for dt in ("float32", "float64"):
        Y, S = _path_rows(ncols, np.dtype(dt).type, ncols)
        got = ss.binary_metrics_rows(Y, S)
        res[f"{ncols}_{dt}"] = [ss.path_last(), got.view(np.int64).tolist()]
with open(sys.argv[2], "w") as f:
    json.dump(res, f)
"""


def test_the_two_paths_agree_bit_for_bit(tmp_path):
    """The same rows through the LDS path (here) and the long path (a fresh process with SS_BINARY_LDS_COLS=0, read
    once at ss_init)."""
    ss.init(0)
    out = tmp_path / "large.json"
    env = dict(os.environ, SS_BINARY_LDS_COLS="0")
    r = subprocess.run([sys.executable, "-c", _CHILD, ROOT, str(out)], env=env, timeout=600, capture_output=True,
                       text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    child = json.loads(out.read_text())
    for ncols in (7, 4000, 16384):
        for dt in (np.float32, np.float64):
            Y, S = _path_rows(ncols, dt, ncols)
            got = ss.binary_metrics_rows(Y, S)
            assert ss.path_last() == ["binary_rows_lds"]
            path, bits = child[f"{ncols}_{np.dtype(dt).name}"]
            assert path == ["binary_rows_large"], path
            np.testing.assert_array_equal(np.array(bits, np.int64).view(np.float64).reshape(got.shape).view(np.int64),
                                          got.view(np.int64), err_msg=f"ncols={ncols} {np.dtype(dt).name}")


@pytest.mark.parametrize("mem", ["host", "device"])
@pytest.mark.parametrize("bad", ["range", "unsorted", "duplicate", "negative"])
def test_bad_labels_are_refused_and_nothing_is_written(mem, bad):
    import torch
    ss.init(0)
    rng = np.random.default_rng(3)
    S = rng.random((3, 10)).astype(np.float32)
    idx = {"range": [1, 3, 10, 2, 5], "unsorted": [1, 3, 2, 0, 5], "duplicate": [1, 3, 3, 2, 5],
           "negative": [1, 3, 4, -1, 5]}[bad]
    ptr = np.array([0, 3, 3, 5], np.int64)
    idx = np.array(idx, np.int32)
    if mem == "host":
        out = np.full((3, 18), -7.0)
        rc = _raw(np.float32, ptr.ctypes.data, idx.ctypes.data, 0, S.ctypes.data, 10, out.ctypes.data,
                  _lib.SS_MEM_HOST, 3, 10)
        assert (out == -7.0).all()
    else:
        tp, ti, ts = (torch.from_numpy(a).cuda() for a in (ptr, idx, S))
        tout = torch.full((3, 18), -7.0, dtype=torch.float64, device="cuda")
        ss.use_torch_stream()
        rc = _raw(np.float32, tp.data_ptr(), ti.data_ptr(), 0, ts.data_ptr(), 10, tout.data_ptr(),
                  _lib.SS_MEM_DEVICE, 3, 10)
        assert (tout.cpu().numpy() == -7.0).all()
    assert rc == -1, rc


def test_bad_shapes_are_refused():
    ss.init(0)
    S = np.zeros((1, 4), np.float32)
    ptr, idx = np.array([0, 1], np.int64), np.array([2], np.int32)
    out = np.zeros((1, 18))
    for ncols, ld in ((0, 4), (1 << 31, 1 << 31), (4, 3)):
        assert _raw(np.float32, ptr.ctypes.data, idx.ctypes.data, 0, S.ctypes.data, ld, out.ctypes.data,
                    _lib.SS_MEM_HOST, 1, ncols) == -1, ncols
    assert (out == 0).all()


# ------------------------------------------------------------------ evaluate_loo_binary
def _square_graph(rng, n, nt):
    Xs = sp.random(n, n, density=0.08, random_state=rng, format="csr")
    Xs = Xs + Xs.T + sp.identity(n)
    Xs.data[:] = rng.uniform(0.5, 1.0, Xs.nnz)
    Ys = sp.random(n, nt, density=0.15, random_state=rng, format="csr")
    Ys.data[:] = 1.0
    Ys.sort_indices()
    return sp.csr_matrix(Xs), sp.csr_matrix(Ys)


def _evaluate_and_compare(g, Ylab, clean, divisor):
    """evaluate_loo_binary == predict_loo into a device buffer + binary_metrics_rows, bit for bit, for several
    block_rows; the two-call route against the host reference."""
    import torch
    n = g.ns
    dt = torch.float32 if g.dtype == np.float32 else torch.float64
    scores = torch.empty((n, g.nt), dtype=dt, device="cuda")
    g.predict_loo(0, n, clean=clean, out=scores)
    m = sp.csr_matrix(Ylab)
    m.eliminate_zeros()
    dptr = torch.from_numpy(m.indptr.astype(np.int64)).cuda()
    didx = torch.from_numpy(m.indices.astype(np.int32) if m.nnz else np.zeros(1, np.int32)).cuda()
    ref = ss.binary_metrics_rows((dptr, didx), scores).cpu().numpy()
    assert n % divisor == 0
    for br in (1, 3, divisor, 0):
        got = g.evaluate_loo_binary(0, n, clean=clean, block_rows=br)
        np.testing.assert_array_equal(got, ref, err_msg=f"block_rows={br}")
    assert "binary_rows_lds" in ss.path_last(), ss.path_last()
    np.testing.assert_array_equal(g.evaluate_loo_binary(3, n - 2, clean=clean, block_rows=5), ref[3:n - 2])
    _check(ref, m.toarray() != 0, scores.cpu().numpy(), "two-call route")
    return ref, scores.cpu().numpy()


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("clean", [False, True])
def test_evaluate_loo_binary_csr_graph(dtype, clean):
    ss.init(0)
    rng = np.random.default_rng(31)
    Xs, Ys = _square_graph(rng, 60, 40)
    g = ss.DeviceGraph.from_sparse(None, Xs, Ys, dtype=dtype)
    _evaluate_and_compare(g, Ys, clean, 12)
    g.evaluate_loo_binary(0, 12, clean=clean)
    assert "transfer_loo" in ss.path_last() and "binary_rows_lds" in ss.path_last(), ss.path_last()
    g.close()


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("clean", [False, True])
def test_evaluate_loo_binary_dense_similarity_graph(dtype, clean):
    ss.init(0)
    rng = np.random.default_rng(32)
    n, nt = 80, 30
    F = rng.random((n, 12))
    S = (np.minimum(F[:, None], F[None]).sum(-1) / np.maximum(F[:, None], F[None]).sum(-1)).astype(dtype)
    Y = sp.random(n, nt, density=0.2, random_state=rng, format="csr"); Y.data[:] = 1.0
    g = ss.DeviceGraph.from_similarity(None, S, Y, alpha=0.6, weighted=True, dtype=dtype)
    _evaluate_and_compare(g, Y, clean, 16)
    g.close()


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("clean", [False, True])
def test_evaluate_loo_binary_fingerprint_graph(dtype, clean):
    ss.init(0)
    rng = np.random.default_rng(33)
    n, nt = 90, 25
    B = rng.random((n, 128)) < 0.3
    Y = sp.random(n, nt, density=0.2, random_state=rng, format="csr"); Y.data[:] = 1.0
    g = ss.DeviceGraph.from_fingerprints(None, ss.pack_fingerprints(B), Y, alpha=0.2, weighted=True, dtype=dtype)
    _evaluate_and_compare(g, Y, clean, 9)
    g.close()


def _iris():
    here = os.path.join(os.path.dirname(__file__), "golden", "iris")

    def read(p):
        with open(os.path.join(here, p)) as f:
            lines = f.read().splitlines()
        return np.array([[float(v) for v in l.split()[1:]] for l in lines[1:]])
    F, Cm = read("iris.features"), read("iris.classes")
    S = np.minimum(F[:, None, :], F[None, :, :]).sum(-1) / np.maximum(F[:, None, :], F[None, :, :]).sum(-1)
    return S, Cm


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_evaluate_loo_binary_iris_against_the_mirror(dtype):
    ss.init(0)
    S, Cm = _iris()
    g = ss.DeviceGraph.from_dense(None, S.astype(dtype), Cm.astype(dtype), alpha=dtype(0.9), weighted=True,
                                  dtype=dtype)
    fns = [ss.f1score, ss.mcc, ss.accuracy, ss.balancedaccuracy, ss.recall, ss.precision]
    for clean in (True, False):
        ref, scores = _evaluate_and_compare(g, sp.csr_matrix(Cm), clean, 50)
        got = ref.reshape(-1, 6, 3)
        for i in range(0, 150, 7):
            for k, f in enumerate(fns):
                assert got[i, k, 0] == ss.maxperformance(Cm[i], scores[i], f), (clean, i, k)
                mean, std = ss.meanstdperformance(Cm[i], scores[i], f)
                assert abs(got[i, k, 1] - mean) <= 1e-12 and abs(got[i, k, 2] - std) <= 1e-10, (clean, i, k)
        assert np.nanmean(got[:, 0, 0]) > 0.9                     # iris is easy: best F1 near 1
    g.close()


# ------------------------------------------------------------------ at size
def test_c3_block_every_row_against_the_reference():
    """C3: 100k x 100k at 1 %, one 2048-fold block on the long path; every row against the host reference and
    evaluate_loo_binary bitwise against the two-call route."""
    import torch
    from tools.c3_loo import rand_csr, rand_sym_csr
    ss.init(0)
    ss.use_torch_stream()
    n, folds, lo = 100_000, 2048, 40_000
    gen = torch.Generator(device="cuda"); gen.manual_seed(20250222 + 3)
    xp, xi = rand_sym_csr(n, 0.01, gen)
    yp, yi = rand_csr(n, n, 0.01, gen)
    xv = (0.5 + 0.5 * torch.rand(xi.numel(), device="cuda", generator=gen)).float()
    g = ss.DeviceGraph.from_device_csr(0, n, n, n, None, (xp, xi, xv), (yp, yi, None), dtype=np.float32)
    out = torch.empty((folds, n), dtype=torch.float32, device="cuda")
    g.predict_loo(lo, lo + folds, clean=True, out=out)
    ptr = yp[lo:lo + folds + 1].contiguous()
    ref = ss.binary_metrics_rows((ptr, yi), out).cpu().numpy()
    assert ss.path_last() == ["binary_rows_large"], ss.path_last()
    got = g.evaluate_loo_binary(lo, lo + folds, clean=True, block_rows=0)
    assert "binary_rows_large" in ss.path_last() and "transfer_loo" in ss.path_last(), ss.path_last()
    np.testing.assert_array_equal(got, ref)
    S = out.cpu().numpy()
    pos, idx_h = ptr.cpu().numpy(), yi.cpu().numpy()
    for r0 in range(0, folds, 256):
        Y = np.zeros((256, n), np.uint8)
        for i in range(256):
            Y[i, idx_h[pos[r0 + i]:pos[r0 + i + 1]]] = 1
        _check(got[r0:r0 + 256], Y, S[r0:r0 + 256], f"C3 folds {lo + r0}..")
    g.close()
