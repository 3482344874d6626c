"""Host reference of the neighbour floor (include/simspread_hip_neighbours.h): the rule, nothing else.

    c = popcount(a & b), u = popcount(a) + popcount(b) - c, s(i,j) = u == 0 ? 1 : T(c) / T(u)
    P_i   = multiset { s(i,j) : s(i,j) > 0 }
    tau_i = the k-th largest element of P_i (multiplicity counted) when |P_i| >= k, else +0
    v     = weighted ? s : 1
    entry (i,j) is kept iff v != 0 and (s >= alpha or (s > 0 and s >= tau_i))

Similarities come from exact integer counts and one correctly rounded division in the graph precision, so every result
of the device is compared bitwise."""
import numpy as np
import scipy.sparse as sp


def ref_counts(Fa, Fb):
    """c = popcount(a & b) for every pair, pa, pb = popcounts of the rows (exact integers)."""
    pa = np.bitwise_count(Fa).sum(axis=1, dtype=np.int64)
    pb = np.bitwise_count(Fb).sum(axis=1, dtype=np.int64)
    c = np.empty((Fa.shape[0], Fb.shape[0]), np.int64)
    step = max(1, (1 << 24) // max(1, Fb.shape[0] * Fa.shape[1]))
    for r in range(0, Fa.shape[0], step):
        c[r:r + step] = np.bitwise_count(Fa[r:r + step, None, :] & Fb[None, :, :]).sum(axis=2, dtype=np.int64)
    return c, pa, pb


def ref_similarity(Fa, Fb, dt):
    """The dense similarity of packed fingerprints Fa against Fb (None: Fa) in precision dt."""
    dt = np.dtype(dt).type
    c, pa, pb = ref_counts(Fa, Fa if Fb is None else Fb)
    u = pa[:, None] + pb[None, :] - c
    with np.errstate(divide="ignore", invalid="ignore"):
        s = c.astype(dt) / u.astype(dt)          # one correctly rounded division in the graph precision
    return np.where(u == 0, dt(1), s).astype(dt)


def ref_kth(s, k):
    """tau[i]: the k-th largest positive entry of row i of the dense similarity s, +0 when there are fewer than k."""
    assert k >= 1
    tau = np.zeros(s.shape[0], s.dtype)
    for i in range(s.shape[0]):
        p = np.sort(s[i][s[i] > 0])[::-1]
        if len(p) >= k:
            tau[i] = p[k - 1]
    return tau


def _csr(v, keep):
    return sp.csr_matrix((v[keep], np.nonzero(keep)[1].astype(np.int32),
                          np.concatenate([[0], np.cumsum(keep.sum(axis=1))]).astype(np.int64)), shape=keep.shape)


def ref_cut(s, alpha, weighted):
    """The plain producer: keep s >= alpha with a non-zero stored value."""
    v = s if weighted else np.ones_like(s)
    return _csr(v, (s >= s.dtype.type(alpha)) & (v != 0))


def ref_floor(s, alpha, k, weighted):
    """The rule above on a dense similarity; k == 0: the plain cut."""
    if k == 0:
        return ref_cut(s, alpha, weighted)
    tau = ref_kth(s, k)
    v = s if weighted else np.ones_like(s)
    keep = (v != 0) & ((s >= s.dtype.type(alpha)) | ((s > 0) & (s >= tau[:, None])))
    return _csr(v, keep)


def positives(s):
    """|P_i| of every row."""
    return (s > 0).sum(axis=1)


def base_bits(n, d, seed):
    """Bits drawn around a few prototypes, so that every alpha keeps some pairs and drops others."""
    rng = np.random.default_rng(seed)
    kp = max(1, n // 16)
    proto = rng.random((kp, d)) < rng.uniform(0.05, 0.5, (kp, 1))
    member = rng.integers(0, kp, n)
    flip = rng.random((n, d)) < rng.uniform(0.0, 0.3, (n, 1))
    return proto[member] ^ flip


def case_bits(n=300, d=167, seed=41):
    """The source set of the case matrix: zero rows {0, 5, n-1}, rows 10..49 exact copies of row 7, rows 60..79 with two
    set bits each."""
    rng = np.random.default_rng(seed + 1)
    bits = base_bits(n, d, seed)
    bits[[0, 5, n - 1]] = False
    bits[10:50] = bits[7]
    for r in range(60, 80):
        bits[r] = False
        bits[r, rng.choice(d, 2, replace=False)] = True
    return bits


def assert_csr_equal(got, want):
    got, want = sp.csr_matrix(got), sp.csr_matrix(want)
    assert got.shape == want.shape
    assert np.array_equal(got.indptr, want.indptr)
    assert np.array_equal(got.indices, want.indices)
    assert got.data.dtype == want.data.dtype
    assert np.array_equal(got.data.view(np.uint8), want.data.view(np.uint8))   # bitwise
