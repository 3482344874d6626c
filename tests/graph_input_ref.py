"""Inputs, restated rules and raw callers for the tests of the graph-input layer (tests/test_graph_inputs_cpu.py,
tests/test_gpu_graph_inputs.py): everything that turns a caller's matrices into a handle -- csr_from_user, csr_from_dense,
csr_transpose, graph_finalize*, the ss_graph_create_* entry points -- and the element-wise set-up kernels.

Nothing reads a handle's CSR back, so a handle is judged by ss_graph_info, ss_graph_degrees and the bits of the scores it
serves.  The inputs are the exactly summable graphs of tests/sparse_ref.py (plus two of extreme shape built here): on
them float32(oracle) is the only correct answer, so one dropped, doubled, shifted or misplaced entry changes the bits, a
count or a degree (test_graph_inputs_cpu.py shows it for every defect listed in DEFECTS).

The first half needs numpy / scipy only; the raw callers at the end load the library when they are called.
"""
import ctypes as C

import numpy as np
import scipy.sparse as sp

from oracle import simspread_oracle as O

import sparse_ref as S

SS_EINVAL = -1
HOST, DEVICE = 0, 1
LD_PAD = 5


# ----------------------------------------------------------------------------- restated rules
def dense_split(rows, cols):
    """(number of column splits, columns per split, columns of the last split) of csr_from_dense (assemble.hip) for a
    rows x cols block: about 65536 (row, split) threads, at most one split per column and at most 1024 splits; the
    count is then what the rounded-up width leaves."""
    nsplit = max(-(-65536 // int(rows)), 1)
    nsplit = min(nsplit, int(cols), 1024)
    cps = -(-int(cols) // nsplit)
    nsplit = -(-int(cols) // cps)
    return nsplit, cps, int(cols) - (nsplit - 1) * cps


def julia_csr(M, dtype, pattern=False):
    """The triple julia/SimSpreadHIP.jl hands over for a block M (`_csr`: sparse(M')): the CSC of the transpose, colptr
    and rowval 1-based, int64 / int32, nzval of the graph type (None: pattern only, the ABI's "all ones")."""
    t = sp.csc_matrix(sp.csr_matrix(M).T)
    t.sort_indices()
    return ((t.indptr.astype(np.int64) + 1), (t.indices.astype(np.int32) + np.int32(1)),
            None if pattern else t.data.astype(dtype))


def csr_triple(M, dtype, base=0, pattern=False):
    """(ptr int64, idx int32, val) of M with the index base asked for: base 1 is the Julia form, base 0 scipy's CSR
    (stored zeros are kept as they are in both)."""
    if base == 1:
        return julia_csr(M, dtype, pattern)
    m = sp.csr_matrix(M)
    if not m.has_sorted_indices:
        m = m.sorted_indices()
    return m.indptr.astype(np.int64), m.indices.astype(np.int32), None if pattern else m.data.astype(dtype)


def from_triple(ptr, idx, val, shape, base):
    """The matrix a (ptr, idx, val) triple of the given base describes."""
    val = np.ones(len(idx)) if val is None else np.asarray(val, dtype=np.float64)
    return sp.csr_matrix((val, np.asarray(idx, dtype=np.int64) - base, np.asarray(ptr) - base), shape=shape)


# ----------------------------------------------------------------------------- stored zeros
def with_stored_zeros(M, seed, long_rows=12):
    """M with explicitly stored zeros at positions M does not use: per row about half as many as the row has entries
    (every third stored value is then a zero), a few of them -0.0; the first `long_rows` rows whose entries leave the
    first and the last column free get 90 more, those two columns among them, so that they store more than 64 values
    with zeros first, last and in between and csr_compact_kernel's ballot compaction crosses a 64-entry step.  Returns
    CSR with the zeros stored (sorted indices)."""
    rng = np.random.default_rng(seed)
    M = sp.csr_matrix(M)
    rows, cols = M.shape
    r_out, c_out, v_out = [M.tocoo().row], [M.tocoo().col], [M.tocoo().data]
    n_long = 0
    for r in range(rows):
        own = M.indices[M.indptr[r]:M.indptr[r + 1]]
        n = len(own) // 2 + (len(own) % 2)
        long = len(own) > 0 and own.min() > 0 and own.max() < cols - 1 and n_long < long_rows
        if long:
            n += 90
            n_long += 1
        n = min(n, cols - len(own))
        if n <= 0:
            continue
        free = np.setdiff1d(rng.choice(cols, size=min(cols, 2 * n + 2 * len(own)), replace=False), own)[:n]
        if long:                                          # a zero before the first and after the last kept entry
            free = np.union1d(free, [0, cols - 1])
        r_out.append(np.full(len(free), r))
        c_out.append(free)
        v_out.append(np.where(rng.random(len(free)) < 0.1, -0.0, 0.0))
    r_out, c_out, v_out = np.concatenate(r_out), np.concatenate(c_out), np.concatenate(v_out)
    order = np.lexsort((c_out, r_out))
    ptr = np.concatenate(([0], np.cumsum(np.bincount(r_out, minlength=rows))))
    Z = sp.csr_matrix((v_out[order], c_out[order], ptr), shape=M.shape)
    assert Z.nnz == len(v_out) and Z.has_sorted_indices
    return Z


def zero_positions(Z):
    """Of the rows of Z that store more than 64 values: the stored positions (within the row) that hold a zero."""
    out = {}
    for r in np.flatnonzero(np.diff(Z.indptr) > 64):
        v = Z.data[Z.indptr[r]:Z.indptr[r + 1]]
        out[int(r)] = (np.flatnonzero(v == 0), len(v))
    return out


# ----------------------------------------------------------------------------- exactly summable graphs of extreme shape
def _pow2_labels(rng, rx, allowed, ntargets):
    """Labels per source so that rx + labels is a power of two (or zero): allowed[rx] lists the label counts to draw
    from; the labels are distinct targets among the first `ntargets`."""
    nl = np.array([rng.choice(allowed[int(r)]) for r in rx])
    rr = np.repeat(np.arange(len(rx)), nl)
    if not nl.sum():
        return rr, np.zeros(0, int)
    cc = np.concatenate([rng.choice(ntargets, size=int(n), replace=False) for n in nl if n])
    return rr, cc


def tall_graph(weighted=True, seed=11):
    """70 000 sources x 4 features x 3 targets, 5 queries: every block with sources for rows has more than 65536 rows, so
    csr_from_dense cuts it into one split.  kf = 4096, 8192, 4096, 1024; a source has 0..3 features and so many labels
    that ks is 0, 1, 2 or 4 (0: an isolated source); the last target is empty.  Weights k/4 (k = 2..4) or ones:
    quantum 2^-e with e = 4 + 13 + 2, scores at most 4."""
    rng = np.random.default_rng(seed)
    ns, nf, nt, nq = 70000, 4, 3, 5
    src = [np.arange(0, 4096), np.arange(2048, 2048 + 8192), np.sort(rng.choice(ns - 2000, 4096, replace=False)),
           np.arange(ns - 1024, ns)]
    rows = np.concatenate(src)
    cols = np.concatenate([np.full(len(s), a) for a, s in enumerate(src)])
    w = (lambda n: rng.integers(2, 5, size=n) / 4.0) if weighted else (lambda n: np.ones(n))
    Xs = sp.csr_matrix((w(len(rows)), (rows, cols)), shape=(ns, nf))
    Xs.sort_indices()
    rx = np.diff(Xs.indptr)
    rr, cc = _pow2_labels(rng, rx, {0: [0, 1, 2], 1: [0, 1], 2: [0, 2], 3: [1]}, nt - 1)
    Ys = sp.csr_matrix((np.ones(len(rr)), (rr, cc)), shape=(ns, nt))
    Ys.sort_indices()
    q = np.array([[1, 0, 0, 1], [0, 1, 1, 0], [1, 1, 1, 1], [0, 0, 0, 0], [0, 0, 1, 0]], dtype=np.float64)
    Xq = sp.csr_matrix(q * (rng.integers(2, 5, size=q.shape) / 4.0 if weighted else 1.0))
    Xq.sort_indices()
    return dict(Xq=Xq, Xs=Xs, Ys=Ys, e=(4 if weighted else 0) + 13 + 2, weighted=weighted)


def wide_graph(weighted=True, seed=12):
    """One query x 70 001 features, 8 sources, 5 targets: csr_from_dense cuts the feature blocks into 1015 splits of 69
    columns (the cap of 1024 splits) with a last split of 35.  1024 features belong to all eight sources, 2 x 256 to
    four, 4 x 512 to two and 2304 - nl_s to source s alone (nl_s = 1..4 labels), so every ks is 4096 and every kf is 0, 1,
    2, 4 or 8; more than two thirds of the features are empty; the first and the last column are not.  The query names
    about 3000 features.  Quantum 2^-e with e = 8 + 3 + 12."""
    rng = np.random.default_rng(seed)
    ns, nf, nt = 8, 70001, 5
    perm = rng.permutation(nf)
    for want, pos in ((0, 0), (nf - 1, 1)):
        at = int(np.flatnonzero(perm == want)[0])
        perm[[pos, at]] = perm[[at, pos]]
    nl = np.arange(ns) % 4 + 1
    rows, cols, o = [], [], 0

    def give(sources, n):
        nonlocal o
        c = perm[o:o + n]
        o += n
        rows.append(np.repeat(sources, n))
        cols.append(np.tile(c, len(sources)))

    give(np.arange(8), 1024)
    for quad in (np.arange(0, 4), np.arange(4, 8)):
        give(quad, 256)
    for p in range(4):
        give(np.array([2 * p, 2 * p + 1]), 512)
    for s in range(ns):
        give(np.array([s]), 2304 - int(nl[s]))
    rows, cols = np.concatenate(rows), np.concatenate(cols)
    w = (lambda n: rng.integers(8, 17, size=n) / 16.0) if weighted else (lambda n: np.ones(n))
    Xs = sp.csr_matrix((w(len(rows)), (rows, cols)), shape=(ns, nf))
    Xs.sort_indices()
    yr = np.repeat(np.arange(ns), nl)
    yc = np.concatenate([rng.choice(nt - 1, size=int(n), replace=False) for n in nl])
    Ys = sp.csr_matrix((np.ones(len(yr)), (yr, yc)), shape=(ns, nt))
    Ys.sort_indices()
    qc = np.union1d(rng.choice(nf, size=3000, replace=False), [0, nf - 1])
    Xq = sp.csr_matrix((w(len(qc)), (np.zeros(len(qc), int), qc)), shape=(1, nf))
    Xq.sort_indices()
    return dict(Xq=Xq, Xs=Xs, Ys=Ys, e=(8 if weighted else 0) + 3 + 12, weighted=weighted)


def small_query(nq, weighted=True, seed=21):
    """sparse_ref.exact_query at 300 sources and 100 targets with nq queries (63, 64, 65: the 64-thread row block of the
    dense kernels)."""
    return S.exact_query(ns=300, nt=100, nq=nq, SC=300, weighted=weighted, seed=seed)


# ----------------------------------------------------------------------------- raw similarities whose cut is a given graph
def raw_similarities(M, alpha, weighted, dtype, seed):
    """A dense matrix of raw similarities (fp64 values that `dtype` represents exactly) whose featurize cutoff at alpha
    is M: weighted, the kept entries carry M's values (all >= alpha; those equal to alpha stay in); unweighted, they are
    drawn from [alpha, 1], a tenth exactly alpha.  Every other entry is drawn below alpha, a tenth of them exactly
    nextafter(alpha, 0) in `dtype`, a few zero."""
    rng = np.random.default_rng(seed)
    dt = np.dtype(dtype).type
    D = sp.csr_matrix(M).toarray()
    kept = D != 0
    below = (rng.random(D.shape) * alpha * 0.999).astype(dt).astype(np.float64)
    u = rng.random(D.shape)
    below[u < 0.1] = float(np.nextafter(dt(alpha), dt(0)))
    below[u > 0.97] = 0.0
    assert (below < alpha).all()
    if weighted:
        assert (D[kept] >= alpha).all() and (D[kept] == alpha).any()
        return np.where(kept, D, below)
    above = (alpha + rng.random(D.shape) * (1.0 - alpha)).astype(dt).astype(np.float64)
    above[rng.random(D.shape) < 0.1] = alpha
    assert (above >= alpha).all()
    return np.where(kept, above, below)


def domain_blocks(nq=37, ns=150, nt=31, seed=31):
    """Raw dense blocks over the whole input domain of featurize: values in (-1, 1), a fifth exact zeros of either sign,
    a twentieth NaN (Sq and Ss only); Y is 0 / 1 with some -0.0."""
    rng = np.random.default_rng(seed)

    def block(r, c):
        a = (rng.random((r, c)) * 2 - 1).astype(np.float32).astype(np.float64)
        u = rng.random((r, c))
        a[u < 0.1] = 0.0
        a[(u >= 0.1) & (u < 0.2)] = -0.0
        a[u > 0.95] = np.nan
        return a

    Y = (rng.random((ns, nt)) < 0.1).astype(np.float64)
    Y[rng.random((ns, nt)) < 0.05] *= -1.0            # -0.0 where there is no label, -1 labels elsewhere: both non-zero rules
    Y[:, -1] = 0.0
    return block(nq, ns), block(ns, ns), Y


def canonical_cut(D, alpha, weighted):
    """The canonical CSR of featurize(D, alpha, weighted): an entry is an edge iff x >= alpha (NaN is not) and its
    value, x or 1, is non-zero.  alpha None: the non-zeros as they are."""
    D = np.asarray(D, dtype=np.float64)
    if alpha is None:
        edge, v = D != 0, D
    else:
        with np.errstate(invalid="ignore"):
            keep = D >= alpha
        v = np.where(keep, D if weighted else 1.0, 0.0)
        edge = keep & (v != 0)
    out = sp.csr_matrix(np.where(edge, v, 0.0))
    out.sort_indices()
    assert out.nnz == int(edge.sum())
    return out


# ----------------------------------------------------------------------------- the general graph
def general_blocks(Xq, Xs, Ys):
    """(L, B, Wt, degrees) of the tri-partite graph as one adjacency matrix, node order queries, sources, features,
    targets (construct, src/core.jl:165-187), never densified: B is A without the query edges, L = A[queries, :],
    Wt = B[:, targets]'.  degrees: the row counts of B."""
    Xq, Xs, Ys = sp.csr_matrix(Xq), sp.csr_matrix(Xs), sp.csr_matrix(Ys)
    nq, nf = Xq.shape
    ns, nt = Ys.shape
    A = sp.bmat([[None, None, Xq, None], [None, None, Xs, Ys], [Xq.T, Xs.T, None, None],
                 [sp.csr_matrix((nt, nq)), Ys.T, None, sp.csr_matrix((nt, nt))]], format="csr")
    B = sp.bmat([[sp.csr_matrix((nq, nq)), None, None, None], [None, None, Xs, Ys],
                 [sp.csr_matrix((nf, nq)), Xs.T, None, None], [None, Ys.T, None, sp.csr_matrix((nt, nt))]], format="csr")
    n = nq + ns + nf + nt
    assert A.shape == B.shape == (n, n)
    L = sp.csr_matrix(A[:nq])
    Wt = sp.csr_matrix(B[:, n - nt:].T)
    for m in (L, B, Wt):
        m.sort_indices()
    return L, B, Wt, np.diff(B.indptr)


def directed_graph(n=600, nr=31, nc=37, seed=41):
    """A directed B (n x n, six entries per row, positive 24-bit weights, B != B', row 7 and column 11 empty), rows L of
    an unrelated A (nr x n, 1..12 entries each, some on rows of B that are empty) and nc columns of B that are no
    block of the node order."""
    rng = np.random.default_rng(seed)
    rr = np.repeat(np.arange(n), 6)
    cc = np.concatenate([rng.choice(n, 6, replace=False) for _ in range(n)])
    keep = (rr != 7) & (cc != 11)
    val = (1.0 - 0.5 * rng.random(int(keep.sum()))).astype(np.float32).astype(np.float64)
    B = sp.csr_matrix((val, (rr[keep], cc[keep])), shape=(n, n))
    B.sort_indices()
    lr = np.concatenate([np.full(1 + r % 12, r) for r in range(nr)])
    lc = np.concatenate([np.sort(rng.choice(n, 1 + r % 12, replace=False)) for r in range(nr)])
    lc[0] = 7                                            # a row of A that names only the node without out-edges
    lv = (1.0 - 0.5 * rng.random(len(lr))).astype(np.float32).astype(np.float64)
    L = sp.csr_matrix((lv, (lr, lc)), shape=(nr, n))
    L.sort_indices()
    cols = np.sort(rng.choice(n, nc, replace=False))
    cols[0] = 11 if 11 not in cols else cols[0]
    cols = np.unique(cols)
    return dict(L=L, B=B, cols=cols, Wt=sp.csr_matrix(B[:, cols].T))


def spread_sparse(B):
    B = sp.csr_matrix(B, dtype=np.float64)
    k = np.diff(B.indptr).astype(np.float64)
    return sp.diags(np.where(k > 0, 1.0 / np.maximum(k, 1), 0.0)) @ B


def general_reference(L, B, cols):
    """The literal L * spread(B) * spread(B)[:, cols] in fp64."""
    W = sp.csr_matrix(spread_sparse(B))
    return np.asarray(((sp.csr_matrix(L) @ W) @ W[:, cols]).todense())


def general_band(L, B, cols, want, dtype):
    """Per-score band of the general graph: the same two kernels as query rows run, so k is counted as
    sparse_ref.band_graph_scores counts it -- fl(1/k) and the coefficient product, one per fma of the longest stage-1
    chain, fl(1/k) and its product, one per non-structural stage-2 addend, one for the single SELL chunk.  fp32:
    gamma(k) * want at u = 2^-24; fp64: gamma(k) * want at u = 2^-53 plus the same again for the reference's own
    roundings.  Structural zeros have band 0."""
    Ln, Bn = S._nz(L), S._nz(B)
    k = np.diff(Bn.indptr)
    live = (k > 0).astype(np.float64)
    N = (Ln @ sp.diags(live) @ Bn).toarray() * live[None, :]
    chain, addends = S._score_counts(N, Bn[:, cols])
    kk = 2 + chain + 2 + addends + 1
    g = S.gamma(kk, S.U32) if np.dtype(dtype) == np.float32 else 2.0 * S.gamma(kk, S.U64)
    return np.where(want > 0, g * want, 0.0)


def emulate_general(L, B, cols, dtype=np.float32, transposed=()):
    """The literal formula one operation at a time in `dtype`, every product and sum rounded.  transposed: the stages
    (1, 2) that read B' where they should read B (with the degrees of what they read)."""
    dt = np.dtype(dtype).type
    L = sp.csr_matrix(L)
    B1 = sp.csr_matrix(B.T if 1 in transposed else B)
    B2 = sp.csr_matrix(B.T if 2 in transposed else B)
    B1.sort_indices()
    W2 = sp.csr_matrix(B2[:, cols])
    W2.sort_indices()
    inv1, inv2 = S._inv(np.diff(B1.indptr), dt), S._inv(np.diff(B2.indptr), dt)
    out = np.zeros((L.shape[0], len(cols)), dtype=dt)
    for r in range(L.shape[0]):
        acc = np.zeros(B.shape[0], dtype=dt)
        for p in range(L.indptr[r], L.indptr[r + 1]):
            a = L.indices[p]
            cf = dt(L.data[p]) * inv1[a]
            idx = B1.indices[B1.indptr[a]:B1.indptr[a + 1]]
            acc[idx] = acc[idx] + cf * B1.data[B1.indptr[a]:B1.indptr[a + 1]].astype(dt)
        z = acc * inv2
        for s in np.flatnonzero(z):
            c = W2.indices[W2.indptr[s]:W2.indptr[s + 1]]
            out[r, c] = out[r, c] + z[s] * W2.data[W2.indptr[s]:W2.indptr[s + 1]].astype(dt)
    return out


# ----------------------------------------------------------------------------- what a handle shows, and single defects
DEFECTS = ("dropped entry", "entry moved one column", "entry assigned to the next row")
BLOCK_DEFECTS = ("indices left 1-based", "split written at the next split's offset")


def sample_entries(M, n, seed):
    """Positions (into M.data) of n stored entries of M, the first and the last of its longest row among them."""
    M = sp.csr_matrix(M)
    rng = np.random.default_rng(seed)
    r = int(np.argmax(np.diff(M.indptr)))
    pick = rng.choice(M.nnz, size=min(n, M.nnz), replace=False)
    return np.unique(np.concatenate((pick, [M.indptr[r], M.indptr[r + 1] - 1])))


def apply_defect(M, defect, p):
    """M (canonical CSR) with one defect at stored position p; None when the defect does not apply there (the place the
    entry would move to is taken or outside the matrix)."""
    M = sp.csr_matrix(M)
    ptr, idx, val = M.indptr.copy(), M.indices.copy(), M.data.copy()
    r = int(np.searchsorted(ptr, p, side="right")) - 1
    c = int(idx[p])
    if defect == "dropped entry":
        idx, val = np.delete(idx, p), np.delete(val, p)
        ptr[r + 1:] -= 1
    elif defect == "entry moved one column":
        if c + 1 >= M.shape[1] or (p + 1 < ptr[r + 1] and idx[p + 1] == c + 1):
            return None
        idx[p] = c + 1
    elif defect == "entry assigned to the next row":
        if r + 1 >= M.shape[0]:
            return None
        nxt = idx[ptr[r + 1]:ptr[r + 2]]
        if c in nxt:
            return None
        at = int(ptr[r + 1] + np.searchsorted(nxt, c)) - 1          # its place once position p is gone
        idx, val = np.insert(np.delete(idx, p), at, c), np.insert(np.delete(val, p), at, val[p])
        ptr[r + 1] -= 1
    else:
        raise ValueError(defect)
    out = sp.csr_matrix((val, idx, ptr), shape=M.shape)
    assert out.has_sorted_indices
    return out


def one_based_read_as_zero_based(M):
    """The block a reader gets that takes 1-based column indices for 0-based ones: every entry one column to the right;
    None when an index leaves the matrix (the check kernel then refuses the block: detected)."""
    M = sp.csr_matrix(M)
    if M.nnz and M.indices.max() + 1 >= M.shape[1]:
        return None
    return sp.csr_matrix((M.data, M.indices + 1, M.indptr), shape=M.shape)


def split_written_late(M, r, s):
    """The block dense_fill_kernel would leave if row r's split s started at the offset of split s + 1: its n entries
    land n places later, on top of what follows (the next row's entries past the end of the row), and the n places they
    should have filled keep an unwritten (column 0, value 0).  Stored zeros stay stored: counts do not move."""
    M = sp.csr_matrix(M)
    nsplit, cps, _ = dense_split(*M.shape)
    idx, val = M.indices.copy(), M.data.copy()
    b, e = M.indptr[r], M.indptr[r + 1]
    mine = np.flatnonzero(M.indices[b:e] // cps == s) + b
    n = len(mine)
    if n == 0 or mine[-1] + n >= M.nnz:
        return None
    src_i, src_v = idx[mine].copy(), val[mine].copy()
    idx[mine], val[mine] = 0, 0.0
    idx[mine + n], val[mine + n] = src_i, src_v
    return (val, idx, M.indptr.copy())


def shown(Xq, Xs, Ys):
    """What ss_graph_info and ss_graph_degrees show of a graph: (nnz of the three blocks after dropping zeros, kf, ks,
    kt)."""
    nz = lambda m: int(np.count_nonzero(sp.csr_matrix(m).data))
    kf, ks, kt = O.degrees(Xs, Ys)
    return (nz(Xq), nz(Xs), nz(Ys)), kf, ks, kt


def same_shown(a, b):
    return a[0] == b[0] and all(np.array_equal(x, y) for x, y in zip(a[1:], b[1:]))


# ----------------------------------------------------------------------------- raw callers (need the library; GPU tests)
class Buffers:
    """Caller buffers in host or device memory: call it with a numpy array (or None) for the pointer the ABI takes; the
    arrays and tensors stay alive as long as the object."""

    def __init__(self, mem):
        self.mem, self.keep = mem, []

    def __call__(self, a):
        if a is None:
            return None
        a = np.ascontiguousarray(a)
        if self.mem == HOST:
            self.keep.append(a)
            return a.ctypes.data
        import torch
        t = torch.from_numpy(a).cuda()
        self.keep.append(t)
        return t.data_ptr() or None

    def ready(self):
        if self.mem == DEVICE:
            import torch
            torch.cuda.synchronize()

    def back(self, i):
        """Buffer number i as a numpy array (after the library's stream has drained)."""
        import simspread_jl_amd as ss
        ss._lib.check(ss._lib.lib().ss_synchronize())
        t = self.keep[i]
        return t if self.mem == HOST else t.cpu().numpy()


def _suf(dtype):
    return "f32" if np.dtype(dtype) == np.float32 else "f64"


def last_error():
    import simspread_jl_amd as ss
    return ss._lib.lib().ss_last_error().decode("utf-8", "replace")


def create_csr(dims, q, s, y, dtype, base, mem):
    """ss_graph_create_csr_* on three (ptr, idx, val) triples (q may be None: NULL pointers) -> (rc, handle)."""
    import simspread_jl_amd as ss
    buf = Buffers(mem)
    args = []
    for t in (q if q is not None else (None, None, None), s, y):
        args += [buf(t[0]), buf(t[1]), buf(t[2])]
    buf.ready()
    h = C.c_void_p(0xdead)               # must come back NULL on a refusal
    rc = getattr(ss._lib.lib(), f"ss_graph_create_csr_{_suf(dtype)}")(*dims, *args, base, mem, C.byref(h))
    return rc, h


def graph_csr(Xq, Xs, Ys, dtype, base=0, mem=HOST, pattern=(False, False, False), xq="null"):
    """A fresh handle through ss_graph_create_csr_* from matrices (stored zeros are handed over as they are).  Xq None
    is the 3-layer graph: xq = "null" passes NULL pointers, "one" a valid one-element pointer array."""
    import simspread_jl_amd as ss
    ns, nf = Xs.shape
    nt = Ys.shape[1]
    if Xq is None:
        nq = 0
        q = None if xq == "null" else (np.array([base], np.int64), np.zeros(1, np.int32), np.zeros(1, dtype))
    else:
        nq = Xq.shape[0]
        q = csr_triple(Xq, dtype, base, pattern[0])
    rc, h = create_csr((nq, ns, nf, nt), q, csr_triple(Xs, dtype, base, pattern[1]), csr_triple(Ys, dtype, base, pattern[2]),
                       dtype, base, mem)
    assert rc == 0, last_error()
    return ss.DeviceGraph(h, dtype)


def create_general(n, L, B, Wt, dtype, base, mem):
    import simspread_jl_amd as ss
    buf = Buffers(mem)
    args = []
    for m in (L, B, Wt):
        t = csr_triple(m, dtype, base)
        args += [buf(t[0]), buf(t[1]), buf(t[2])]
    buf.ready()
    h = C.c_void_p(0xdead)
    rc = getattr(ss._lib.lib(), f"ss_graph_create_general_{_suf(dtype)}")(n, L.shape[0], Wt.shape[0], *args, base, mem,
                                                                         C.byref(h))
    assert rc == 0, last_error()
    return ss.DeviceGraph(h, dtype, general=True)


def create_spmat(shape, triple, dtype, base, mem):
    """ss_spmat_create_csr_* -> (rc, handle)."""
    import simspread_jl_amd as ss
    buf = Buffers(mem)
    args = [buf(t) for t in triple]
    buf.ready()
    h = C.c_void_p(0xdead)
    rc = getattr(ss._lib.lib(), f"ss_spmat_create_csr_{_suf(dtype)}")(shape[0], shape[1], *args, base, mem, C.byref(h))
    return rc, h


def spmat(W, dtype, base, mem, pattern=False):
    import simspread_jl_amd as ss
    rc, h = create_spmat(W.shape, csr_triple(W, dtype, base, pattern), dtype, base, mem)
    assert rc == 0, last_error()
    w = ss.DeviceSpMat.__new__(ss.DeviceSpMat)
    w.shape, w.dtype, w._suf, w.nnz, w._h = W.shape, np.dtype(dtype), _suf(dtype), int(W.nnz), h
    return w


def dense_blocks(blocks, dtype, mem):
    """The blocks as from_dense takes them: numpy arrays, or CUDA tensors."""
    if mem == HOST:
        return [None if b is None else np.asarray(b, dtype=dtype) for b in blocks]
    import torch
    return [None if b is None else torch.from_numpy(np.ascontiguousarray(b, dtype=dtype)).cuda() for b in blocks]


def elementwise(name, X, dtype, mem, ld_pad=3, **kw):
    """ss_cutoff_* / ss_row_degree_* / ss_spread_* on X (rows x cols) handed over column-major with ld = rows + ld_pad
    and NaN in the padding; outputs likewise, pre-filled with a sentinel.  Returns (result, output buffer with its
    padding) -- for row_degree (int64 degrees, None)."""
    import simspread_jl_amd as ss
    lib = ss._lib.lib()
    dt = np.dtype(dtype).type
    rows, cols = X.shape
    ld = rows + ld_pad
    src = np.full((cols, ld), np.nan, dtype=dt)          # C-order (cols, ld) == column-major ld x cols
    src[:, :rows] = np.asarray(X, dtype=dt).T
    buf = Buffers(mem)
    ps = buf(src)
    ft = C.c_float if dt == np.float32 else C.c_double
    if name == "row_degree":
        deg = np.full(rows, -7, np.int64)
        pd = buf(deg)
        buf.ready()
        ss._lib.check(getattr(lib, f"ss_row_degree_{_suf(dt)}")(ps, rows, cols, ld, pd, mem))
        return buf.back(1), None
    out = np.full((cols, ld), -7.0, dtype=dt)
    po = buf(out)
    buf.ready()
    if name == "cutoff":
        rc = getattr(lib, f"ss_cutoff_{_suf(dt)}")(ps, rows, cols, ld, ft(kw["alpha"]), 1 if kw["weighted"] else 0, po,
                                                   ld, mem)
    else:
        rc = getattr(lib, f"ss_spread_{_suf(dt)}")(ps, rows, cols, ld, po, ld, mem)
    ss._lib.check(rc)
    full = buf.back(1)
    return np.ascontiguousarray(full[:, :rows].T), full
