"""Per-target ranking metrics of whole sweeps on the device (ss_target_rank_*): against the definition (rank_ref.ref_row
of every column), the literal oracle, the numpy restatement of the two-pass algorithm (exports compared entry by entry)
and the per-row device metrics on the transposed matrix; one table and one set of bits for every block split, block
order, memory space, leading dimension, search route, merge and export -> import; failed calls leave the handle as it
was."""
import os
import socket
import subprocess
import sys

import numpy as np
import pytest
import scipy.sparse as sp

import simspread_jl_amd as ss
import target_rank_ref as R
from oracle import simspread_oracle as O
from rank_ref import assert_rows_close
from simspread_jl_amd import _lib

pytestmark = pytest.mark.gpu

ALPHA, NT = 20.0, 40
RTOL, ATOL = 1e-9, 1e-12          # the band of the per-row metrics against the literal oracle
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _tables_equal(a, b):
    for x, y in zip(a.export_positives(), b.export_positives()):
        np.testing.assert_array_equal(np.asarray(x), np.asarray(y))
    for x, y in zip(a.export_counts(), b.export_counts()):
        np.testing.assert_array_equal(np.asarray(x), np.asarray(y))


def _state(h):
    i = h.info()
    return (i, h.export_positives(), h.export_counts() if i["phase"] == "count" else None)


def _same_state(a, b):
    assert a[0] == b[0]
    for x, y in zip(a[1], b[1]):
        np.testing.assert_array_equal(np.asarray(x), np.asarray(y))
    if a[2] is not None:
        for x, y in zip(a[2], b[2]):
            np.testing.assert_array_equal(np.asarray(x), np.asarray(y))


def _cuts(n, k):
    if k == 1 or n < 4:
        return [0, n]
    if k == 3:
        return sorted({0, n // 3, (2 * n) // 3 + 1, n})
    return sorted({0, n} | {min(n, c) for c in (1, 3, n // 4 + 2, n // 2, n // 2 + 1, n - 2)})


def _raw_add(h, Y, S, row_begin, ld, mem):
    """add_rows through the ABI: padded leading dimension, a label slice of a larger CSR, index_base 1."""
    import torch
    n, nt = S.shape
    Sp = np.zeros((n, ld), S.dtype)
    Sp[:, :nt] = S
    big = sp.csr_matrix(np.vstack([np.ones((2, nt), np.uint8), Y]))
    ptr = (big.indptr.astype(np.int64) + 1)[2:]
    idx = big.indices.astype(np.int32) + 1
    fn = getattr(_lib.lib(), "ss_target_rank_add_rows_" + h._suf)
    if mem == _lib.SS_MEM_HOST:
        _lib.check(fn(h._h, ptr.ctypes.data, idx.ctypes.data, 1, Sp.ctypes.data, n, nt, ld, row_begin, mem))
    else:
        _lib.use_torch_stream()
        tp, ti, ts = torch.from_numpy(ptr).cuda(), torch.from_numpy(idx).cuda(), torch.from_numpy(Sp).cuda()
        _lib.check(fn(h._h, tp.data_ptr(), ti.data_ptr(), 1, ts.data_ptr(), n, nt, ld, row_begin, mem))
        torch.cuda.synchronize()
    return h


def _run(Y, S, dtype, nblocks=1, reverse=False, raw=None):
    h = ss.TargetRank(Y.shape[1], dtype)
    cuts = _cuts(S.shape[0], nblocks)
    blocks = list(zip(cuts[:-1], cuts[1:]))
    add = (lambda a, b: h.add_rows(Y[a:b], S[a:b], row_begin=a)) if raw is None else \
          (lambda a, b: _raw_add(h, Y[a:b], S[a:b], a, S.shape[1] + raw[0], raw[1]))
    for a, b in blocks:
        add(a, b)
    h.seal()
    for a, b in (blocks[::-1] if reverse else blocks):
        add(a, b)
    return h


def _oracle(Y, S, L):
    out = []
    for t in range(S.shape[1]):
        with np.errstate(invalid="ignore", divide="ignore"):
            out.append([O.auroc(Y[:, t], S[:, t]), O.auprc(Y[:, t], S[:, t]), O.bedroc(Y[:, t], S[:, t], alpha=ALPHA)])
    return np.array(out)


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("n, Ls", [(2, (1,)), (37, (1, 5, 20)), (129, (5, 64)), (300, (20, 64))])
def test_case_matrix_every_split_order_memory_and_ld(dtype, n, Ls):
    import torch
    ss.init(0)
    Y, S = R.case_matrix(n, NT, Ls[-1], dtype)
    h = _run(Y, S, dtype)
    assert h.info() == dict(nt=NT, phase="count", rows=n, npos=int(Y.sum()), rows_counted=n)
    # the numpy restatement of the algorithm: the same sealed positives and the same counts, entry by entry
    ref = R.RefTargetRank(NT, dtype).add_rows(Y, S).seal().add_rows(Y, S)
    got_pos, ref_pos = h.export_positives(), ref.export_positives()
    assert got_pos[3] == ref_pos[3] == n
    for x, y in zip(got_pos[:3], ref_pos[:3]):                               # bit for bit (signed zeros included)
        assert x.dtype == y.dtype
        np.testing.assert_array_equal(x.view(np.uint8), np.ascontiguousarray(y).view(np.uint8))
    for x, y in zip(h.export_counts(), ref.export_counts()):
        np.testing.assert_array_equal(np.asarray(x), np.asarray(y))
    first = {}
    for L in Ls:
        got = h.metrics(ALPHA, L)
        want = R.ref_targets(Y, S.astype(np.float64), ALPHA, L)
        assert_rows_close(got, want, RTOL, ATOL, f"n={n} L={L} vs ref_row")
        np.testing.assert_array_equal(got[:, 4:], want[:, 4:])               # recall@L, precision@L: exact
        assert_rows_close(got[:, :3], _oracle(Y, S.astype(np.float64), L), RTOL, ATOL, f"n={n} L={L} vs oracle")
        np.testing.assert_array_equal(h.metrics(ALPHA, L), got)              # repeatable
        first[L] = got
    assert "target_rank_metrics" in ss.path_last()
    variants = [_run(Y, S, dtype, 3, reverse=True), _run(Y, S, dtype, 7, reverse=True),
                _run(Y, S, dtype, 3, raw=(5, _lib.SS_MEM_HOST)), _run(Y, S, dtype, 7, True, raw=(3, _lib.SS_MEM_DEVICE))]
    tS = torch.from_numpy(S).cuda()
    ht = ss.TargetRank(NT, dtype).add_rows(Y, tS).seal().add_rows(sp.csr_matrix(Y), tS)
    for v in variants + [ht]:
        _tables_equal(v, h)
        for L in Ls:
            np.testing.assert_array_equal(v.metrics(ALPHA, L), first[L])
        v.close()
    h.close()


def test_a_cut_inside_a_tie_group_and_signed_zeros():
    ss.init(0)
    n = 37
    Y, S = R.case_matrix(n, NT, 5, np.float64)
    cuts = _cuts(n, 7)
    col = S[:, 7]                                                            # heavy ties: 4 distinct scores
    assert any(col[c - 1] == col[c] or (col[:c] == col[c]).any() for c in cuts[1:-1])
    assert np.signbit(S[:, NT - 1]).any() and (S[:, NT - 1] == 0).sum() > 2
    got = _run(Y, S, np.float64, 7, reverse=True).metrics(ALPHA, 5)
    assert_rows_close(got, R.ref_targets(Y, S, ALPHA, 5), RTOL, ATOL, "tie cut")


_CHILD = """
import sys, numpy as np
sys.path.insert(0, {tests!r})
import simspread_jl_amd as ss, target_rank_ref as R
ss.init(0)
out = {}
for name, dtype in (("f32", np.float32), ("f64", np.float64)):
    for n, L in ((2, 1), (37, 20), (129, 64), (300, 64)):
        Y, S = R.case_matrix(n, 40, L, dtype)
        c = n // 2
        h = ss.TargetRank(40, dtype).add_rows(Y, S).seal().add_rows(Y[:c], S[:c], 0)
        tags = ss.path_last()
        h.add_rows(Y[c:], S[c:], c)
        out[f"{name}_{n}_counts"] = h.export_counts()[0]
        out[f"{name}_{n}_metrics"] = h.metrics(20.0, 1)
        out[f"{name}_{n}_tags"] = np.array(",".join(tags))
np.savez(sys.argv[1], **out)
"""


def test_both_search_routes_give_the_same_counts(tmp_path):
    """The switch is read at ss_init, so the capped run is a fresh process: with SS_TARGET_RANK_LDS=4 every tile holding
    a target of more than four positives searches in global memory; by default the small sizes of the case matrix
    take the LDS route."""
    ss.init(0)
    env = dict(os.environ, SS_TARGET_RANK_LDS="4")
    path = str(tmp_path / "capped.npz")
    subprocess.run([sys.executable, "-c", _CHILD.replace("{tests!r}", repr(os.path.join(ROOT, "tests"))), path], check=True, env=env,
                   cwd=ROOT, timeout=120)
    z = np.load(path)
    for name, dtype in (("f32", np.float32), ("f64", np.float64)):
        for n, L in ((2, 1), (37, 20), (129, 64), (300, 64)):
            Y, S = R.case_matrix(n, NT, L, dtype)
            h = ss.TargetRank(NT, dtype).add_rows(Y, S).seal().add_rows(Y, S)
            if n <= 37:                                      # far under 2048 positives in the tile
                assert ss.path_last() == ["target_rank_count_lds"], (n, ss.path_last())
            np.testing.assert_array_equal(h.export_counts()[0], z[f"{name}_{n}_counts"])
            np.testing.assert_array_equal(h.metrics(ALPHA, 1), z[f"{name}_{n}_metrics"])
            if n > 2:                                        # some target of the tile holds more than four positives
                assert str(z[f"{name}_{n}_tags"]).split(",") == ["target_rank_count_large"]
            h.close()


def test_fp64_scores_below_fp32_resolution_are_not_ties():
    ss.init(0)
    n = 50
    rng = np.random.default_rng(5)
    S = 0.5 + np.arange(n, dtype=np.float64)[:, None] * 1e-12 * np.ones((1, 3))
    Y = (rng.random((n, 3)) < 0.4).astype(np.uint8)
    assert np.unique(S[:, 0].astype(np.float32)).size == 1
    h = _run(Y, S, np.float64, 3, reverse=True)
    assert_rows_close(h.metrics(ALPHA, 5), R.ref_targets(Y, S, ALPHA, 5), RTOL, ATOL, "fp64")
    ref = R.RefTargetRank(3, np.float64).add_rows(Y, S).seal().add_rows(Y, S)
    np.testing.assert_array_equal(h.export_counts()[0], ref.export_counts()[0])
    assert sum(int(ref._views(t)[3].sum()) for t in range(3)) == 0


# ------------------------------------------------------------------------------------------ sweeps
def _labels(rng, n, nt, dens=0.15):
    Y = sp.random(n, nt, density=dens, random_state=rng, format="csr")
    Y.data[:] = 1.0
    Y.sort_indices()
    return sp.csr_matrix(Y)


def _graph(kind, dtype, rng, n=211, nt=97):
    Y = _labels(rng, n, nt)
    if kind == "csr":
        X = sp.random(n, n, density=0.08, random_state=rng, format="csr")
        X = X + X.T + sp.identity(n)
        X.data[:] = rng.uniform(0.5, 1.0, X.nnz)
        return ss.DeviceGraph.from_sparse(None, sp.csr_matrix(X), Y, dtype=dtype), Y
    if kind == "dense":
        F = rng.random((n, 12))
        S = (np.minimum(F[:, None], F[None]).sum(-1) / np.maximum(F[:, None], F[None]).sum(-1)).astype(dtype)
        return ss.DeviceGraph.from_similarity(None, S, Y, alpha=0.6, weighted=True, dtype=dtype), Y
    B = rng.random((n, 128)) < 0.3
    return ss.DeviceGraph.from_fingerprints(None, ss.pack_fingerprints(B), Y, alpha=0.2, weighted=True, dtype=dtype), Y


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("kind", ["csr", "dense", "fingerprint"])
def test_sweeps_equal_the_per_row_metrics_of_the_transposed_matrix(dtype, kind):
    import torch
    ss.init(0)
    rng = np.random.default_rng(3)
    g, Y = _graph(kind, dtype, rng)
    n, nt, L = g.ns, g.nt, 20
    fold = rng.integers(0, 5, n).astype(np.int32)
    tdt = torch.float32 if dtype == np.float32 else torch.float64
    YT = sp.csr_matrix(Y.T)
    for clean in (False, True):
        for sweep in ("loo", "kfold"):
            out = torch.empty((n, nt), dtype=tdt, device="cuda")
            if sweep == "loo":
                g.predict_loo(0, n, clean=clean, out=out)
                run = lambda br: g.evaluate_loo_targets(0, n, clean=clean, alpha=ALPHA, L=L, block_rows=br)
            else:
                g.predict_kfold_rows(fold, 5, 0, n, clean=clean, out=out)
                run = lambda br: g.evaluate_kfold_targets(fold, 5, 0, n, clean=clean, alpha=ALPHA, L=L, block_rows=br)
            S = out.cpu().numpy()
            got = run(50)
            want = ss.rank_metrics_rows(YT, np.ascontiguousarray(S.T), alpha=ALPHA, L=L)
            assert_rows_close(got, want, RTOL, ATOL, f"{kind} {sweep} clean={clean} vs rank_metrics_rows")
            assert_rows_close(got, R.ref_targets(Y.toarray(), S.astype(np.float64), ALPHA, L), RTOL, ATOL,
                              f"{kind} {sweep} clean={clean} vs ref_row")
            h = ss.TargetRank(nt, dtype).add_rows(Y, out).seal().add_rows(Y, out)
            np.testing.assert_array_equal(got, h.metrics(ALPHA, L))          # the explicit add_rows path, bitwise
            h.close()
            for br in (0, 64):
                np.testing.assert_array_equal(run(br), got)
    g.close()


def test_iris_per_class_table():
    """The tutorial's sweep (alpha 0.9, weighted) judged per class, in fp32 so that ss.rank_metrics, which takes float32
    scores, sees exactly the scores of the sweep."""
    ss.init(0)
    d = os.path.join(ROOT, "tests", "golden", "iris")

    def read(p):
        with open(os.path.join(d, p)) as f:
            lines = f.read().splitlines()
        return lines[0].split(), np.array([[float(v) for v in l.split()[1:]] for l in lines[1:]])
    _, F = read("iris.features")
    names, Y = read("iris.classes")
    assert F.shape[0] == 150 and Y.shape == (150, 3)
    S = ss.jaccard_similarity(F).astype(np.float32)
    g = ss.DeviceGraph.from_dense(None, S, Y.astype(np.float32), alpha=np.float32(0.9), weighted=True, dtype=np.float32)
    got = g.evaluate_loo_targets(clean=True, alpha=ALPHA, L=20)
    yhat = g.predict_loo(clean=True)
    assert yhat.dtype == np.float32 and got.shape == (3, 6)
    for t in range(3):
        m = ss.rank_metrics(Y[:, t], yhat[:, t], ALPHA)
        want = np.array([[m[k] for k in ("AuROC", "AuPRC", "BEDROC", "validity_ratio")]])
        assert_rows_close(got[t:t + 1, :4], want, RTOL, ATOL, f"iris class {names[t]} vs ss.rank_metrics")
    assert_rows_close(got, R.ref_targets(Y, yhat.astype(np.float64), ALPHA, 20), RTOL, ATOL, "iris vs ref_row")
    g.close()


# ------------------------------------------------------------------------------------------ merge, import, errors
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_merge_and_import_equal_one_handle(dtype):
    ss.init(0)
    n, cut = 129, 47
    Y, S = R.case_matrix(n, NT, 20, dtype)
    one = _run(Y, S, dtype)
    want = one.metrics(ALPHA, 20)
    parts = lambda: (ss.TargetRank(NT, dtype).add_rows(Y[:cut], S[:cut], 0),
                     ss.TargetRank(NT, dtype).add_rows(Y[cut:], S[cut:], cut))
    # merge: collect phase, then count phase
    a, b = parts()
    a2, b2 = parts()
    a.merge(b)
    b2.merge(a2)
    a.seal(), b2.seal()
    a.add_rows(Y[:cut], S[:cut], 0)
    b2.add_rows(Y[cut:], S[cut:], cut)
    with pytest.raises(ss.SimSpreadError, match="counted"):
        a.metrics(ALPHA, 20)
    a.merge(b2)
    _tables_equal(a, one)
    np.testing.assert_array_equal(a.metrics(ALPHA, 20), want)
    # the same through export and import
    c, d = parts()
    c.import_positives(*d.export_positives())
    d.import_positives(*parts()[0].export_positives())
    c.seal(), d.seal()
    c.add_rows(Y[:cut], S[:cut], 0)
    d.add_rows(Y[cut:], S[cut:], cut)
    c.import_counts(*d.export_counts())
    _tables_equal(c, one)
    np.testing.assert_array_equal(c.metrics(ALPHA, 20), want)


def _refused(h, call, match):
    before = _state(h)
    with pytest.raises(ss.SimSpreadError, match=match or None) as e:
        call()
    assert e.value.code == -1
    _same_state(_state(h), before)


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_errors_leave_the_handle_as_it_was(dtype):
    ss.init(0)
    n = 37
    other = np.float64 if dtype == np.float32 else np.float32
    Y, S = R.case_matrix(n, NT, 5, dtype)
    bad = S.copy()
    bad[n - 1, NT - 2] = np.nan
    fn = getattr(_lib.lib(), "ss_target_rank_add_rows_" + ("f32" if dtype == np.float32 else "f64"))
    ptr = np.array([0, 2] + [2] * (n - 1), np.int64)
    unsorted = np.array([5, 3], np.int32)

    def raw(h, idx=unsorted, ncols=NT):
        _lib.check(fn(h._h, ptr.ctypes.data, idx.ctypes.data, 0, S.ctypes.data, n, ncols, NT, 0, _lib.SS_MEM_HOST))

    for phase in ("collect", "count"):
        h = ss.TargetRank(NT, dtype).add_rows(Y[:20], S[:20], 0)
        if phase == "count":
            h.add_rows(Y[20:], S[20:], 20).seal().add_rows(Y[:20], S[:20], 0)
        _refused(h, lambda: h.add_rows(Y[20:], bad[20:], 20), "NaN")
        _refused(h, lambda: raw(h), "")
        _refused(h, lambda: raw(h, ncols=NT - 1), "ncols")
        _refused(h, lambda: h.merge(h), "itself")
        with pytest.raises(TypeError):
            h.add_rows(Y, S.astype(other))
        if phase == "collect":
            _refused(h, lambda: h.export_counts(), "not sealed")
            _refused(h, lambda: h.import_counts(np.zeros(3, np.int64), 0), "not sealed")
            _refused(h, lambda: h.metrics(ALPHA, 5), "not sealed")
            sealed = ss.TargetRank(NT, dtype).add_rows(Y, S).seal()
            _refused(h, lambda: h.merge(sealed), "collects")
            _refused(sealed, lambda: sealed.merge(h), "collects")
        else:
            _refused(h, lambda: h.seal(), "sealed already")
            _refused(h, lambda: h.import_positives(*ss.TargetRank(NT, dtype).add_rows(Y, S).export_positives()), "sealed")
            _refused(h, lambda: h.metrics(ALPHA, 5), "counted")
            r, t = np.argwhere(Y[20:])[2]
            S2 = S[20:].copy()
            S2[r, t] = np.nextafter(S2[r, t], dtype(200.0))
            _refused(h, lambda: h.add_rows(Y[20:], S2, 20), f"row {20 + r}, target {t}")
            Y2 = Y[20:].copy()
            r0, t0 = np.argwhere(Y2 == 0)[0]
            Y2[r0, t0] = 1                                                    # a positive that was never collected
            _refused(h, lambda: h.add_rows(Y2, S[20:], 20), "row")
            # other sealed positives: no merge
            o = ss.TargetRank(NT, dtype).add_rows(Y, np.ascontiguousarray(S[::-1])).seal()
            _refused(h, lambda: h.merge(o), "same sealed")
            c, _ = h.export_counts()
            c[0] = -1
            _refused(h, lambda: h.import_counts(c, 0), "negative")
            _refused(h, lambda: h.import_counts(c[:-1], 0), "counts")
            h.add_rows(Y[20:], S[20:], 20)
            _refused(h, lambda: h.metrics(ALPHA, n), "length")
            _refused(h, lambda: h.metrics(ALPHA, 0), "L > 0")
            assert_rows_close(h.metrics(ALPHA, 5), R.ref_targets(Y, S.astype(np.float64), ALPHA, 5), RTOL, ATOL, "after")
    with pytest.raises(ss.SimSpreadError):
        ss.TargetRank(NT, dtype).import_positives(np.array([NT], np.int32), np.array([0], np.int64),
                                                  np.array([0.5], dtype), 1)
    with pytest.raises(ss.SimSpreadError, match="NaN"):
        ss.TargetRank(NT, dtype).import_positives(np.array([0], np.int32), np.array([0], np.int64),
                                                  np.array([np.nan], dtype), 1)


def test_more_than_one_row_group_and_tile(tmp_path):
    """1100 rows (three row groups of a count workgroup) by 150 targets (three tiles, the last one partial), fp32:
    sparse labels, mostly-zero scores -- the regime of the sweeps -- against the numpy algorithm's counts."""
    ss.init(0)
    rng = np.random.default_rng(11)
    n, nt = 1100, 150
    Y = (rng.random((n, nt)) < 0.01).astype(np.uint8)
    S = np.where(rng.random((n, nt)) < 0.9, 0.0, np.round(rng.random((n, nt)) * 16) / 16).astype(np.float32)
    h = ss.TargetRank(nt, np.float32).add_rows(Y, S).seal().add_rows(Y[600:], S[600:], 600).add_rows(Y[:600], S[:600], 0)
    ref = R.RefTargetRank(nt, np.float32).add_rows(Y, S).seal().add_rows(Y, S)
    np.testing.assert_array_equal(h.export_counts()[0], ref.export_counts()[0])
    assert_rows_close(h.metrics(ALPHA, 20), R.ref_targets(Y, S.astype(np.float64), ALPHA, 20), RTOL, ATOL, "big")


# ------------------------------------------------------------------------------------------ two ranks
def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _rank_worker(rank, world, port, tmp):
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import torch.distributed as dist
    import simspread_jl_amd as ss_
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    ss_.init(0)
    g, _ = _graph("csr", np.float32, np.random.default_rng(8))
    lo, hi = ss_.shard_range(g.ns, rank, world)
    h = ss_.TargetRank(g.nt, np.float32).add_loo(g, lo, hi, clean=True, block_rows=50)
    ss_.target_rank_positives(h)
    assert h.info()["rows"] == g.ns and h.info()["phase"] == "collect"
    h.seal().add_loo(g, lo, hi, clean=True, block_rows=50)
    out = ss_.target_rank(h, root=0)
    assert (out is None) == (rank != 0)
    if rank == 0:
        t, r, v, n = out.export_positives()
        c, nc = out.export_counts()
        np.savez(os.path.join(tmp, "rank.npz"), t=t, r=r, v=v, n=n, c=c, nc=nc, m=out.metrics(ALPHA, 20))
    dist.barrier()
    dist.destroy_process_group()


def test_two_ranks_meet_in_dist_target_rank(tmp_path):
    import torch.multiprocessing as mp
    mp.spawn(_rank_worker, args=(2, _free_port(), str(tmp_path)), nprocs=2, join=True)
    ss.init(0)
    g, _ = _graph("csr", np.float32, np.random.default_rng(8))
    one = ss.TargetRank(g.nt, np.float32).add_loo(g, clean=True).seal().add_loo(g, clean=True)
    got = np.load(tmp_path / "rank.npz")
    t, r, v, n = one.export_positives()
    c, nc = one.export_counts()
    np.testing.assert_array_equal(got["t"], t)
    np.testing.assert_array_equal(got["r"], r)
    np.testing.assert_array_equal(got["v"].view(np.uint32), v.view(np.uint32))
    np.testing.assert_array_equal(got["c"], c)
    assert int(got["n"]) == n == int(got["nc"]) == nc == g.ns
    np.testing.assert_array_equal(got["m"], one.metrics(ALPHA, 20))          # bitwise the single-process table
    g.close()


# ------------------------------------------------------------------------------------------ at size
def test_c3_block_of_2048_folds_per_target():
    """One 2048-fold block of the C3 shape (100k targets, 1 % density): tiles over and under the LDS budget, four row
    groups per tile, two million positives.  The reference on the device is, per target, a stable descending sort of
    the 2048 scores; from it come the sealed positives, every count of the export and an exact AuROC numerator."""
    import torch
    sys.path.insert(0, ROOT)
    from tools.c3_loo import rand_csr, rand_sym_csr
    ss.init(0)
    ss.use_torch_stream()
    n, folds = 100_000, 2048
    gen = torch.Generator(device="cuda")
    gen.manual_seed(20250222 + 3)
    xp, xi = rand_sym_csr(n, 0.01, gen)
    yp, yi = rand_csr(n, n, 0.01, gen)
    xv = (0.5 + 0.5 * torch.rand(xi.numel(), device="cuda", generator=gen)).float()
    g = ss.DeviceGraph.from_device_csr(0, n, n, n, None, (xp, xi, xv), (yp, yi, None), dtype=np.float32)
    h = ss.TargetRank(n, np.float32).add_loo(g, 0, folds, clean=True).seal().add_loo(g, 0, folds, clean=True)
    tags = ss.path_last()
    assert "target_rank_count_lds" in tags, tags
    out = torch.empty((folds, n), dtype=torch.float32, device="cuda")
    g.predict_loo(0, folds, clean=True, out=out)
    # labels of the block, dense on the device
    ptr = yp[:folds + 1].to(torch.int64)
    nlab = int(ptr[-1])
    rows_of = torch.repeat_interleave(torch.arange(folds, device="cuda"), ptr[1:] - ptr[:-1])
    Yd = torch.zeros((folds, n), dtype=torch.bool, device="cuda")
    Yd[rows_of, yi[:nlab].to(torch.int64)] = True
    # per target a stable descending sort by value (-0.0 ties with +0.0; ties keep ascending rows)
    vals, order = torch.sort(out, dim=0, descending=True, stable=True)
    ys = torch.gather(Yd, 0, order)
    del Yd
    P = ys.sum(0)                                                             # (n,)
    off = torch.cumsum(P, 0) - P
    # the sealed positives: gather of the scores at the labels, bit for bit
    tt, ii = ys.t().nonzero(as_tuple=True)                                    # target-major, sorted order within
    want_rows = order.t()[tt, ii]
    want_vals = vals.t()[tt, ii]
    st, sr, sv, nrows = h.export_positives()
    assert nrows == folds and st.size == nlab == int(P.sum())
    np.testing.assert_array_equal(st, tt.to(torch.int32).cpu().numpy())
    np.testing.assert_array_equal(sr, want_rows.cpu().numpy())
    np.testing.assert_array_equal(sv.view(np.uint32), want_vals.cpu().numpy().view(np.uint32))
    torch.testing.assert_close(want_vals, out[want_rows, tt], rtol=0, atol=0)
    # tie groups along the sorted columns
    pos = torch.arange(folds, device="cuda", dtype=torch.int32)[:, None]
    new = torch.ones((folds, n), dtype=torch.bool, device="cuda")
    new[1:] = vals[1:] != vals[:-1]
    start = torch.cummax(torch.where(new, pos, torch.zeros_like(pos)), 0).values.to(torch.int64)
    last = torch.ones((folds, n), dtype=torch.bool, device="cuda")
    last[:-1] = new[1:]
    end = torch.flip(torch.cummin(torch.flip(torch.where(last, pos, torch.full_like(pos, folds)), [0]), 0).values,
                     [0]).to(torch.int64)
    cpos = torch.cumsum(ys.to(torch.int32), 0)
    cexcl = cpos - ys.to(torch.int32)                                         # positives before each position
    j = torch.gather(cexcl, 0, start)                                         # positives scoring strictly higher
    grp = torch.gather(cpos, 0, end) - j                                      # positives of the tie group
    neg, tied = ~ys, grp > 0
    base = (3 * (off + torch.arange(n, device="cuda")))[None, :].expand(folds, n)
    P1 = (P + 1)[None, :].expand(folds, n)
    nhist = 3 * (nlab + n)
    hist = torch.zeros(nhist, dtype=torch.int64, device="cuda")
    one = torch.ones(1, dtype=torch.int64, device="cuda")
    m = neg & ~tied
    hist.index_add_(0, (base + j)[m], one.expand(int(m.sum())))                        # gap
    m = neg & tied
    hist.index_add_(0, (base + P1 + j)[m], one.expand(int(m.sum())))                   # tieG
    hist.index_add_(0, (base + 2 * P1 + cexcl)[m], one.expand(int(m.sum())))           # tieK
    counts, counted = h.export_counts()
    assert counted == folds and counts.size == 3 * nlab + 6 * n
    np.testing.assert_array_equal(counts[:nhist], hist.cpu().numpy())
    np.testing.assert_array_equal(counts[nhist:nhist + n], (out != 0).sum(0).cpu().numpy())
    bits = torch.where(out == 0, torch.zeros_like(out), out).view(torch.int32)
    key = torch.where(bits < 0, ~bits, bits | torch.tensor(-2 ** 31, dtype=torch.int32, device="cuda")).to(torch.int64)
    key = key & 0xFFFFFFFF
    kmin, kmax = key.min(0).values, key.max(0).values
    np.testing.assert_array_equal(counts[nhist + n:nhist + 2 * n], kmin.cpu().numpy())
    np.testing.assert_array_equal(counts[nhist + 2 * n:], kmax.cpu().numpy())
    # AuROC: pairs won (a tie counts half) without the top group's, the trapezoid having no (0,0) point
    num2 = torch.where(neg, 2 * j.to(torch.int64) + grp.to(torch.int64), torch.zeros((), dtype=torch.int64, device="cuda")).sum(0)
    top = start == 0
    num2 = num2 - (top & neg).sum(0) * (top & ys).sum(0)
    Pd = P.to(torch.float64)
    Nd = folds - Pd
    want = num2.to(torch.float64) / (2.0 * Pd * Nd)
    missing = (P == 0) | (P == folds)
    want = torch.where(missing, torch.where(kmin != kmax, torch.full_like(want, float("nan")), torch.zeros_like(want)),
                       want).cpu().numpy()
    got = h.metrics(ALPHA, 20)
    assert_rows_close(got[:, :1], want[:, None], RTOL, ATOL, "C3 AuROC")
    np.testing.assert_array_equal(got[:, 3], counts[nhist:nhist + n] / folds)
    g.close()
