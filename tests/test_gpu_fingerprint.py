"""The fingerprint route on the device: packed binary fingerprints -> thresholded Tanimoto CSR -> graph.

Every CSR is checked bitwise against a host reference kept in this file (popcounts of the packed words, the division in
the graph precision, the cutoff of featurize) and against the dense route it replaces (ss_similarity_jaccard_* on the
unpacked 0/1 rows followed by the cutoff), graphs built from fingerprints against graphs built from the reference CSR,
and one 100k x 2048-bit set at production size."""
import ctypes as C

import numpy as np
import pytest
import scipy.sparse as sp

import simspread_jl_amd as ss
from simspread_jl_amd import _lib

pytestmark = pytest.mark.gpu

ALPHAS = (0.0, 0.3, 0.7, 1.0)


# ----------------------------------------------------------------------------------------------- host reference
def ref_counts(Fa, Fb):
    """c = popcount(a & b) for every pair, pa, pb = popcounts of the rows (exact integers)."""
    pa = np.bitwise_count(Fa).sum(axis=1, dtype=np.int64)
    pb = np.bitwise_count(Fb).sum(axis=1, dtype=np.int64)
    c = np.empty((Fa.shape[0], Fb.shape[0]), np.int64)
    step = max(1, (1 << 24) // max(1, Fb.shape[0] * Fa.shape[1]))
    for r in range(0, Fa.shape[0], step):
        c[r:r + step] = np.bitwise_count(Fa[r:r + step, None, :] & Fb[None, :, :]).sum(axis=2, dtype=np.int64)
    return c, pa, pb


def ref_similarity(c, pa, pb, dt):
    u = pa[:, None] + pb[None, :] - c
    with np.errstate(divide="ignore", invalid="ignore"):
        s = c.astype(dt) / u.astype(dt)          # one correctly rounded division in the graph precision
    return np.where(u == 0, dt(1), s).astype(dt)


def ref_cut(s, alpha, weighted, dt):
    """featurize's cutoff as the dense assembly applies it: keep s >= alpha with a non-zero stored value."""
    v = s if weighted else np.ones_like(s)
    keep = (s >= dt(alpha)) & (v != 0)
    return sp.csr_matrix((v[keep], np.nonzero(keep)[1].astype(np.int32),
                          np.concatenate([[0], np.cumsum(keep.sum(axis=1))]).astype(np.int64)), shape=s.shape)


def fingerprints(n, d, seed, zero_rows=()):
    """Bits drawn around a few prototypes (so that every alpha keeps some pairs and drops others), duplicates and
    all-zero rows included."""
    rng = np.random.default_rng(seed)
    k = max(1, n // 16)
    proto = rng.random((k, d)) < rng.uniform(0.05, 0.5, (k, 1))
    member = rng.integers(0, k, n)
    flip = rng.random((n, d)) < rng.uniform(0.0, 0.3, (n, 1))
    bits = proto[member] ^ flip
    if n > 3:
        bits[n // 2] = bits[n // 3]            # an exact duplicate: similarity 1
    for z in zero_rows:
        if z < n:
            bits[z] = False
    return ss.pack_fingerprints(bits), bits


def assert_csr_equal(got, want):
    got, want = sp.csr_matrix(got), sp.csr_matrix(want)
    assert got.shape == want.shape
    assert np.array_equal(got.indptr, want.indptr)
    assert np.array_equal(got.indices, want.indices)
    assert got.data.dtype == want.data.dtype
    assert np.array_equal(got.data.view(np.uint8), want.data.view(np.uint8))   # bitwise


# ----------------------------------------------------------------------------------------------- 1. the case matrix
# (n, d): n in {1, 63, 64, 65, 1000, 4097}, nwords in {1, 3, 32, 64}, d = 150 and 70 not multiples of 64
CASES = [(1, 64), (63, 150), (64, 2048), (65, 4096), (1000, 150), (4097, 2048), (300, 70)]


@pytest.mark.parametrize("n,d", CASES)
def test_tanimoto_csr_matches_the_host_reference_and_the_dense_route(n, d):
    import torch
    ss.init(0)
    F, bits = fingerprints(n, d, seed=n * 7 + d, zero_rows=(0, n - 1, 5))
    nb = max(1, n // 2 + 3)
    G, gbits = fingerprints(nb, d, seed=n + d + 1, zero_rows=(1,))
    c_sym, pa, _ = ref_counts(F, F)
    c_x, _, pg = ref_counts(F, G)
    for dt in (np.float32, np.float64):
        s_sym = ref_similarity(c_sym, pa, pa, dt)
        s_x = ref_similarity(c_x, pa, pg, dt)
        # the dense route: jaccard on the unpacked 0/1 rows, computed by the existing device kernel
        S_dense = ss.jaccard_similarity(bits.astype(dt), dtype=dt)
        assert np.array_equal(S_dense.view(np.uint8), s_sym.view(np.uint8)), "dense jaccard differs from Tanimoto"
        for weighted in (True, False):
            for alpha in ALPHAS:
                want = ref_cut(s_sym, alpha, weighted, dt)
                got = ss.tanimoto_csr(F, alpha=alpha, weighted=weighted, dtype=dt)
                assert_csr_equal(got, want)
                assert_csr_equal(got, ref_cut(S_dense, alpha, weighted, dt))
                assert ss.path_last() == ["tanimoto_csr_sym"]
                got_x = ss.tanimoto_csr(F, G, alpha=alpha, weighted=weighted, dtype=dt)
                assert_csr_equal(got_x, ref_cut(s_x, alpha, weighted, dt))
                assert ss.path_last() == ["tanimoto_csr_cross"]
        # device input gives the same arrays
        Ft = torch.from_numpy(F.view(np.int64)).cuda()
        Gt = torch.from_numpy(G.view(np.int64)).cuda()
        p, i, v = ss.tanimoto_csr(Ft, Gt, alpha=0.3, weighted=True, dtype=dt)
        want = ref_cut(s_x, 0.3, True, dt)
        assert_csr_equal(sp.csr_matrix((v.cpu().numpy(), i.cpu().numpy(), p.cpu().numpy()), shape=want.shape), want)


def test_edge_cases_of_the_rule():
    ss.init(0)
    bits = np.zeros((4, 100), bool)
    bits[2, :10] = True
    bits[3, 50:] = True                         # rows 2 and 3 share nothing: s = 0
    F = ss.pack_fingerprints(bits)
    for dt in (np.float32, np.float64):
        # alpha <= 0 unweighted keeps every pair
        A = ss.tanimoto_csr(F, alpha=0.0, weighted=False, dtype=dt).toarray()
        assert (A == 1).all()
        A = ss.tanimoto_csr(F, alpha=-1.0, weighted=False, dtype=dt).toarray()
        assert (A == 1).all()
        # alpha <= 0 weighted drops s = 0 (a stored zero is no edge)
        W = ss.tanimoto_csr(F, alpha=0.0, weighted=True, dtype=dt)
        Wd = W.toarray()
        assert W.nnz == 6 and (W.data != 0).all()
        assert Wd[0, 1] == 1 and Wd[1, 0] == 1 and Wd[0, 0] == 1          # zero with zero: 1
        assert Wd[0, 2] == 0 and Wd[2, 0] == 0 and Wd[1, 3] == 0          # zero with non-zero: 0
        assert Wd[2, 3] == 0 and Wd[2, 2] == 1 and Wd[3, 3] == 1


# ----------------------------------------------------------------------------------------------- 2. the size protocol
def test_size_protocol_capacity_and_memory_kinds():
    import torch
    lib = ss.init(0)
    F, _ = fingerprints(700, 300, seed=3, zero_rows=(2,))
    nw = F.shape[1]
    fn = lib.ss_similarity_tanimoto_csr_f32
    ptr = np.zeros(701, np.int64)
    nnz = C.c_int64(-1)
    assert fn(F.ctypes.data, 700, None, 700, nw, C.c_float(0.3), 1, ptr.ctypes.data, None, None, 0, C.byref(nnz), 0) == 0
    want = ss.tanimoto_csr(F, alpha=0.3)
    assert nnz.value == want.nnz > 0 and np.array_equal(ptr, want.indptr)
    # capacity too small: SS_EINVAL, nnz still reported, nothing written
    idx = np.full(nnz.value, -5, np.int32)
    val = np.full(nnz.value, -5, np.float32)
    nnz2 = C.c_int64(-1)
    rc = fn(F.ctypes.data, 700, None, 700, nw, C.c_float(0.3), 1, ptr.ctypes.data, idx.ctypes.data, val.ctypes.data,
            nnz.value - 1, C.byref(nnz2), 0)
    assert rc == -1 and nnz2.value == nnz.value
    assert (idx == -5).all()
    # exact capacity
    rc = fn(F.ctypes.data, 700, None, 700, nw, C.c_float(0.3), 1, ptr.ctypes.data, idx.ctypes.data, val.ctypes.data,
            nnz.value, C.byref(nnz2), 0)
    assert rc == 0
    assert_csr_equal(sp.csr_matrix((val, idx, ptr), shape=(700, 700)), want)
    # device memory: the same CSR, and run to run bitwise repeatable
    Ft = torch.from_numpy(F.view(np.int64)).cuda()
    for _ in range(2):
        p, i, v = ss.tanimoto_csr(Ft, alpha=0.3)
        assert np.array_equal(p.cpu().numpy(), ptr)
        assert np.array_equal(i.cpu().numpy(), idx)
        assert np.array_equal(v.cpu().numpy().view(np.uint32), val.view(np.uint32))
    # argument checks return codes, they do not abort
    assert fn(F.ctypes.data, 700, None, 700, 0, C.c_float(0.3), 1, ptr.ctypes.data, None, None, 0, C.byref(nnz2), 0) == -1
    assert fn(None, 700, None, 700, nw, C.c_float(0.3), 1, ptr.ctypes.data, None, None, 0, C.byref(nnz2), 0) == -1
    assert fn(F.ctypes.data, 700, None, 700, nw, C.c_float(0.3), 1, None, None, None, 0, C.byref(nnz2), 0) == -1
    assert fn(F.ctypes.data, 1 << 31, None, 700, nw, C.c_float(0.3), 1, ptr.ctypes.data, None, None, 0,
              C.byref(nnz2), 0) == -5


def test_nnz_of_2_to_the_31_is_refused_on_the_host():
    import torch
    lib = ss.init(0)
    n = 50_000
    Ft = torch.randint(0, 1 << 62, (n, 1), dtype=torch.int64, device="cuda")
    ptr = torch.zeros(n + 1, dtype=torch.int64, device="cuda")
    nnz = C.c_int64(-1)
    rc = lib.ss_similarity_tanimoto_csr_f32(Ft.data_ptr(), n, None, n, 1, C.c_float(0.0), 0, ptr.data_ptr(), None,
                                            None, 0, C.byref(nnz), 1)
    assert rc == -5, rc
    assert nnz.value == n * n
    assert "2^31" in lib.ss_last_error().decode()
    with pytest.raises(ss.SimSpreadError) as e:
        ss.tanimoto_csr(Ft, alpha=0.0, weighted=False)
    assert e.value.code == -5
    # the graph route refuses the same block
    Y = (torch.zeros(n + 1, dtype=torch.int64, device="cuda"), torch.zeros(0, dtype=torch.int32, device="cuda"), None, 4)
    with pytest.raises(ss.SimSpreadError) as e:
        ss.DeviceGraph.from_fingerprints(None, Ft, Y, alpha=0.0, weighted=False)
    assert e.value.code == -5


# ----------------------------------------------------------------------------------------------- 3. graphs
def _labels(ns, nt, seed):
    rng = np.random.default_rng(seed)
    Y = sp.random(ns, nt, density=4.0 / nt, random_state=rng, format="csr")
    Y.data[:] = 1.0
    return Y


@pytest.mark.parametrize("dt,tol", [(np.float32, 1e-5), (np.float64, 1e-12)])
@pytest.mark.parametrize("weighted", [True, False])
def test_graph_from_fingerprints_equals_the_graph_from_the_reference_csr(dt, tol, weighted):
    from oracle import simspread_oracle as O
    ss.init(0)
    ns, nq, nt, d, alpha = 3000, 500, 300, 1024, 0.35
    Fs, _ = fingerprints(ns, d, seed=11, zero_rows=(4, 17))
    Fq, _ = fingerprints(nq, d, seed=12, zero_rows=(0,))
    c, ps, _ = ref_counts(Fs, Fs)
    Xs = ref_cut(ref_similarity(c, ps, ps, dt), alpha, weighted, dt)
    c, pq, _ = ref_counts(Fq, Fs)
    Xq = ref_cut(ref_similarity(c, pq, ps, dt), alpha, weighted, dt)
    Y = _labels(ns, nt, 13)

    g = ss.DeviceGraph.from_fingerprints(Fq, Fs, Y, alpha=alpha, weighted=weighted, dtype=dt)
    assert ss.path_last() == ["tanimoto_csr_sym", "tanimoto_csr_cross"]
    assert (g.nq, g.ns, g.nf, g.nt, g.nnz_xq, g.nnz_xs) == (nq, ns, ns, nt, Xq.nnz, Xs.nnz)
    r = ss.DeviceGraph.from_sparse(Xq, Xs, Y, dtype=dt)
    for rows in ("query", "source"):
        got, want = g.predict(rows), r.predict(rows)
        assert np.array_equal(got.view(np.uint8), want.view(np.uint8)), rows
        ref = O.predict_factored(Xq.astype(np.float64), Xs.astype(np.float64), Y, rows)
        assert np.abs(got - ref).max() <= tol * np.abs(ref).max(), rows

    g3 = ss.DeviceGraph.from_fingerprints(None, Fs, Y, alpha=alpha, weighted=weighted, dtype=dt)
    assert ss.path_last() == ["tanimoto_csr_sym"]
    r3 = ss.DeviceGraph.from_sparse(None, Xs, Y, dtype=dt)
    got, want = g3.predict_loo(clean=True), r3.predict_loo(clean=True)
    assert np.array_equal(got.view(np.uint8), want.view(np.uint8))
    qs = [0, 4, 17, ns // 2, ns - 1]
    ref = O.predict_loo_factored(Xs, Y, clean_flag=True, queries=qs)
    assert np.abs(got[qs] - ref).max() <= tol * np.abs(ref).max()
    fold = np.random.default_rng(5).integers(0, 7, ns).astype(np.int32)
    got, want = g3.predict_kfold(fold, 7, clean=True), r3.predict_kfold(fold, 7, clean=True)
    assert np.array_equal(got.view(np.uint8), want.view(np.uint8))


# ----------------------------------------------------------------------------------------------- 4. at size
def clustered_fingerprints(n, d, clusters, seed, density=0.1, flip=0.015):
    """Cluster prototypes with per-bit flips: members of one cluster are ~0.7 similar, of different clusters ~0.05, so
    alpha = 0.5 keeps (almost exactly) the pairs inside a cluster -- sum of squared cluster sizes, ~1 % of n^2."""
    rng = np.random.default_rng(seed)
    proto = rng.random((clusters, d)) < density
    member = rng.integers(0, clusters, n)
    F = np.empty((n, d // 64), np.uint64)
    for r in range(0, n, 8192):
        m = member[r:r + 8192]
        bits = proto[m] ^ (rng.random((len(m), d), dtype=np.float32) < flip)
        F[r:r + 8192] = ss.pack_fingerprints(bits)
    return F, member


def test_100k_2048_bit_clustered_set():
    import torch
    from oracle import simspread_oracle as O
    ss.init(0)
    n, d, alpha = 100_000, 2048, 0.5
    F, member = clustered_fingerprints(n, d, clusters=100, seed=2026)
    Ft = torch.from_numpy(F.view(np.int64)).cuda()
    p, i, v = ss.tanimoto_csr(Ft, alpha=alpha, weighted=True, dtype=np.float32)
    torch.cuda.synchronize()
    sizes = np.bincount(member)
    implied = int((sizes.astype(np.int64) ** 2).sum())
    nnz = int(i.numel())
    assert 0.99 * implied <= nnz <= 1.01 * implied, (nnz, implied)
    A = sp.csr_matrix((v.cpu().numpy(), i.cpu().numpy(), p.cpu().numpy()), shape=(n, n))
    del p, i, v
    # symmetric, bitwise
    At = A.T.tocsr()
    At.sort_indices()
    assert np.array_equal(A.indptr, At.indptr) and np.array_equal(A.indices, At.indices)
    assert np.array_equal(A.data.view(np.uint32), At.data.view(np.uint32))
    del At
    # every non-empty row holds its diagonal (s(i, i) = 1)
    nonempty = np.diff(A.indptr) > 0
    assert nonempty.all()
    assert (A.diagonal() == 1).all()
    # 256 rows exactly against the host reference: the ends and both sides of tile boundaries
    rng = np.random.default_rng(9)
    rows = {0, n - 1, 127, 128, 255, 256, 99_967, 99_968, 50_047, 50_048}
    rows |= set(rng.integers(0, n, 256 - len(rows)).tolist())
    rows = np.array(sorted(rows))[:256]
    c, pr, pall = ref_counts(F[rows], F)
    want = ref_cut(ref_similarity(c, pr, pall, np.float32), alpha, True, np.float32)
    assert_csr_equal(A[rows], want)
    # the graph at size: a 2048-fold leave-one-out block, 8 folds against the factored oracle
    Y = _labels(n, 2000, 21)
    g = ss.DeviceGraph.from_fingerprints(None, Ft, (torch.from_numpy(Y.indptr.astype(np.int64)).cuda(),
                                                    torch.from_numpy(Y.indices.astype(np.int32)).cuda(), None, 2000),
                                         alpha=alpha, weighted=True, dtype=np.float32)
    assert g.nnz_xs == nnz
    out = g.predict_loo(0, 2048, clean=True)
    assert np.isfinite(out).all()
    qs = [0, 1, 127, 128, 1000, 1500, 2046, 2047]
    ref = O.predict_loo_factored(A, Y, clean_flag=True, queries=qs)
    assert np.abs(out[qs] - ref).max() <= 1e-5 * np.abs(ref).max()
