"""Inputs, references, term counts and rounding bands for the tests of the sparse regime (numpy / scipy, no device):
stage 1 (transfer_kernel and its variants), stage 2 (spmm_sell_kernel) and the raw W*R routes.

Two families of inputs.

Exactly summable: every degree a kernel divides by is a power of two, every weight is k/16 with k = 8..16 (or 1), Ys is
0/1.  Every term of a score, x_qa * (1/kf_a) * x_sa * (1/ks_s) * y_st, is then a non-negative multiple of a quantum
q = 2^-e, and so is every partial sum in any order; while the largest sum stays below 2^24 quanta all of them are
representable in fp32, so any kernel, chunking or summation order must return float32(oracle) bit for bit (and the fp64
kernels the fp64 oracle).  The builders also plant the structural edges of the kernels (sub-row lengths around one and
two waves, neighbour counts around the metadata group of 64 and the batches of U, empty features, sources and targets).

Ordinary inputs with per-score rounding bands: arbitrary degrees, 24-bit random weights, low fill.  Every score is held
to gamma(k) * score with k the worst-case number of roundings a term of that score passes through (band_graph).

References are oracle/simspread_oracle.py in fp64.  `emulate` is a sequential model of the two stages with one rounding
per operation in a chosen precision; its `defect` parameter holds every defect the tests must be able to see.
"""
import math

import numpy as np
import scipy.sparse as sp

from oracle import simspread_oracle as O

import dense_ref as D

U32 = 2.0 ** -24          # unit roundoff of fp32
U64 = 2.0 ** -53
SUBROW_EDGES = (1, 63, 64, 65, 127, 128, 129)        # and one of at least 193 entries
NEIGHBOUR_EDGES = (0, 1, 7, 8, 9, 16, 17, 63, 64, 65, 128, 129)
DEFECTS = ("dropped entry", "doubled entry")
DEFECTS_LOO = DEFECTS + ("ks instead of ks - 1", "kept dropped feature")


def _ceil_div(a, b):
    return -(-int(a) // int(b))


def _pow2_at_least(n):
    return 1 << max(int(n) - 1, 0).bit_length()


def is_pow2(a):
    a = np.asarray(a, dtype=np.int64)
    return (a > 0) & ((a & (a - 1)) == 0)


# ----------------------------------------------------------------------------- the sizing rules of the host layer
def chunk_width(ns, nf, nnz, elem=4, env_chunk=None):
    """(SC, number of chunks) of the stage-1 operand X' (nf rows, ns columns, nnz entries) as graph_chunked in
    simspread.jl_amd/csrc/api.hip sizes it: SC ~ 64 * ns / (mean row length of X'), at most 20 KiB of accumulators less
    one wave, at least 256; SS_TRANSFER_CHUNK (16..8192) replaces that; the chunk count is rounded up to a multiple of 8
    (unless it is 1), then SC = 4 * ceil(ceil(ns / nch) / 4).  The count returned is what chunked_build (assemble.hip) then
    cuts, ceil(ns / SC), which the rounding of SC can leave one short of the multiple of 8 (the launch order by groups
    of 8 chunks needs the multiple: CHUNK_ENV picks values that keep it)."""
    ns1 = max(int(ns), 1)
    mean_len = nnz / nf if nf > 0 else 0.0
    sc = int(64.0 * ns1 / mean_len) if mean_len > 1.0 else ns1
    sc = max(min(sc, (20 * 1024) // elem - 64), 256)
    if env_chunk is not None and 16 <= env_chunk <= 8192:
        sc = int(env_chunk)
    nch = _ceil_div(ns1, sc)
    if nch > 1:
        nch = _ceil_div(nch, 8) * 8
    sc = _ceil_div(_ceil_div(ns1, nch), 4) * 4
    return sc, _ceil_div(ns1, sc)


# SS_TRANSFER_CHUNK that cuts each family of inputs into exactly 8 and exactly 16 chunks (test_sparse_inputs_cpu.py)
CHUNK_ENV = {"query": {8: 376, 16: 190}, "loo": {8: 64, 16: 32}, "kfold": {8: 32, 16: 16}, "band": {8: 76, 16: 38}}


def transfer_batch_rows(nrows, ns, elem, cap_bytes):
    """Rows of T held at once (transfer_batch_rows in api.hip) under SS_TRANSFER_BYTES = cap_bytes (>= 2^20)."""
    rb = max((cap_bytes // (max(ns, 1) * elem)) & ~7, 8)
    return min(rb, nrows)


def subrow_lengths(Xs, SC):
    """Multiset (sorted array) of the sub-row lengths of X' cut into chunks of SC columns: for every feature and chunk
    the number of the feature's sources inside the chunk (zeros left out)."""
    X = sp.csc_matrix(Xs)
    X.sort_indices()
    nch = max(_ceil_div(X.shape[0], SC), 1)
    feat = np.repeat(np.arange(X.shape[1]), np.diff(X.indptr))
    cnt = np.bincount(feat * nch + X.indices // SC, minlength=X.shape[1] * nch)
    return np.sort(cnt[cnt > 0])


def promised_subrow_lengths(ns, SC):
    """The lengths of SUBROW_EDGES (and 256 for "at least 193") that exact_query plants for this SC.  A feature's degree
    is a power of two, so a length that is none comes from a feature cut by a chunk boundary (65 | 63, 129 | 127,
    1 | 127): with a single chunk only 1, 64, 128, 256 exist, and no sub-row is longer than SC (with more than 8 chunks
    and ns <= 3000, SC <= 188: nothing beyond two waves)."""
    multi = _ceil_div(ns, SC) > 1
    out = {1, 64}
    if SC >= 128:
        out.add(128)
    if SC >= 256:
        out.add(256)
    if multi and SC >= 65:
        out |= {65, 63}
    if multi and SC >= 129:
        out |= {129, 127}
    if multi and SC >= 127:
        out |= {1, 127}
    return out


# ----------------------------------------------------------------------------- exactly summable inputs
def _weights(rng, n, weighted):
    return rng.integers(8, 17, size=n) / 16.0 if weighted else np.ones(n)


def _forced_features(ns, SC):
    """(first source, degree) of the features with contiguous sources that give the promised sub-row lengths."""
    out = [(0, 64)]
    if SC >= 128:
        out.append((0, 128))
    if SC >= 256:
        out.append((0, 256))
    if _ceil_div(ns, SC) > 1:
        B = SC      # the first chunk boundary
        if SC >= 65:
            out.append((B - 65, 128))
        if SC >= 129:
            out.append((B - 129, 256))
        if SC >= 127:
            out.append((B - 1, 128))
    return out


def exact_query(ns=3000, nt=300, nq=70, SC=None, weighted=True, labels="random", seed=0):
    """Exactly summable query-row inputs (nf = ns).  Feature a has kf = 2^j sources, j = 0..7 at random, plus the
    contiguous features of _forced_features (kf = 64, 128, 256, inside a chunk and across the first chunk boundary);
    one feature has no source and is named by queries; source ns - 1 is isolated (no feature, no label).  Source s with
    rx features gets 2^ceil(log2(rx + 1)) - rx labels, so ks is a power of two; the last target stays empty.  The first
    queries have NEIGHBOUR_EDGES features, the long ones among them name every forced feature and the empty one.
    labels: "random"; "hub": target 0 is the first label of all but a few sources (a long row of Ys' for the
    length-sorted stage-2 operand); "private": target s belongs to source s alone and the padding labels sit in columns
    ns.., so that score column s is the transfer element T[q][s] (stage 1 in isolation; nt is then ns + padding).
    Returns Xq, Xs, Ys (scipy CSR, fp64), SC, e (the quantum of scores, T and sums is 2^-e), the feature ids
    forced / empty, isolated."""
    rng = np.random.default_rng(seed)
    SC = _ceil_div(ns, 4) * 4 if SC is None else int(SC)
    nf = ns
    forced = _forced_features(ns, SC)
    cols, srcs = [], []
    for a in range(nf - 1):                 # feature nf - 1 stays without sources
        if a < len(forced):
            s = np.arange(forced[a][0], forced[a][0] + forced[a][1])
        else:
            s = rng.choice(ns - 1, size=1 << int(rng.integers(0, 8)), replace=False)       # never the isolated source
        cols.append(np.full(len(s), a))
        srcs.append(s)
    cols, srcs = np.concatenate(cols), np.concatenate(srcs)
    Xs = sp.csr_matrix((_weights(rng, len(cols), weighted), (srcs, cols)), shape=(ns, nf))
    Xs.sort_indices()
    rx = np.diff(Xs.indptr)
    nlab = np.array([_pow2_at_least(r + 1) - r for r in rx])
    nlab[ns - 1] = 0
    pad = int(nlab.max())
    if labels == "private":
        nt = ns + pad
    assert pad < nt - 1, "a source needs more labels than there are targets"
    yr, yc = [], []
    for s in range(ns):
        n = int(nlab[s])
        if n == 0:
            continue
        if labels == "private":
            c = np.concatenate(([s], ns + rng.choice(pad, size=n - 1, replace=False)))
        elif labels == "hub" and s % 97 != 5:
            c = np.concatenate(([0], 1 + rng.choice(nt - 2, size=n - 1, replace=False)))
        else:
            c = (1 if labels == "hub" else 0) + rng.choice(nt - 1 - (labels == "hub"), size=n, replace=False)
        yr.append(np.full(n, s))
        yc.append(c)
    Ys = sp.csr_matrix((np.ones(int(nlab.sum())), (np.concatenate(yr), np.concatenate(yc))), shape=(ns, nt))
    Ys.sort_indices()
    qr, qc = [], []
    special = np.concatenate((np.arange(len(forced)), [nf - 1]))
    for q in range(nq):
        n = NEIGHBOUR_EDGES[q] if q < len(NEIGHBOUR_EDGES) else int(rng.integers(1, 41))
        c = rng.choice(nf - 1 - len(forced), size=n, replace=False) + len(forced)
        if n >= len(special) * 2 and (q < len(NEIGHBOUR_EDGES) or q % 5 == 0):
            c[rng.choice(n, size=len(special), replace=False)] = special
        qr.append(np.full(n, q))
        qc.append(c)
    qr, qc = np.concatenate(qr), np.concatenate(qc)
    Xq = sp.csr_matrix((_weights(rng, len(qr), weighted), (qr, qc)), shape=(nq, nf))
    Xq.sort_indices()
    kf, ks, _ = O.degrees(Xs, Ys)
    e = (8 if weighted else 0) + int(math.log2(kf.max())) + int(math.log2(ks.max()))
    return dict(Xq=Xq, Xs=Xs, Ys=Ys, SC=SC, e=e, forced=np.arange(len(forced)), empty_feature=nf - 1, isolated=ns - 1,
                weighted=weighted)


QUERY_NS = 3000
# SS_TRANSFER_CHUNK of the tests at QUERY_NS: None: graph_chunked's own choice (one chunk in fp32, where up to 5056
# sums fit; eight chunks of 376 in fp64, where 2496 do), 376: 8 chunks of 376, 190: 16 chunks of 188
QUERY_CHUNKS = (None, 376, 190)


def exact_query_for(elem, env_chunk=None, ns=QUERY_NS, **kw):
    """exact_query whose planted edges sit where graph_chunked will cut for this precision and SS_TRANSFER_CHUNK: the
    cut depends (without the switch) on the mean degree, which depends on the planted features; two rounds settle it."""
    SC = chunk_width(ns, ns, 32 * ns, elem, env_chunk)[0]        # (mean degree about 32: right unless the cap decides)
    for _ in range(4):
        inp = exact_query(ns=ns, SC=SC, **kw)
        SC, nch = chunk_width(ns, inp["Xs"].shape[1], inp["Xs"].nnz, elem, env_chunk)
        if SC == inp["SC"]:
            return dict(inp, nchunks=nch)
    raise AssertionError("the chunk width did not settle")


LOO_BLOCKS = (3, 5, 9, 17, 33, 65, 129, 65, 33, 129)      # n = 488


def _block_square(rng, sizes, weighted, labels_of_size, nt):
    """Block-diagonal X with full blocks and 0/1 labels, labels_of_size(size) per source among the first nt - 1 targets."""
    n = int(sum(sizes))
    r, c = [], []
    o = 0
    for size in sizes:
        i = np.arange(o, o + size)
        r.append(np.repeat(i, size))
        c.append(np.tile(i, size))
        o += size
    r, c = np.concatenate(r), np.concatenate(c)
    X = sp.csr_matrix((_weights(rng, len(r), weighted), (r, c)), shape=(n, n))
    X.sort_indices()
    yr, yc = [], []
    o = 0
    for size in sizes:
        for s in range(o, o + size):
            yr.append(np.full(labels_of_size(size), s))
            yc.append(rng.choice(nt - 1, size=labels_of_size(size), replace=False))
        o += size
    yr, yc = np.concatenate(yr), np.concatenate(yc)
    Y = sp.csr_matrix((np.ones(len(yr)), (yr, yc)), shape=(n, nt))
    Y.sort_indices()
    return X, Y


def exact_loo(weighted=True, nt=200, seed=1):
    """Exactly summable leave-one-out inputs: X block-diagonal with full blocks of 2^j + 1 sources (kf - 1 = 2^j, and
    every source of a block owns the dropped feature), 2^j labels per source (ks - 1 = 2^(j+1)); the last target is
    empty.  Quantum 2^-e with e = 8 + 7 + 8."""
    rng = np.random.default_rng(seed)
    X, Y = _block_square(rng, LOO_BLOCKS, weighted, lambda size: size - 1, nt)
    j = int(math.log2(max(LOO_BLOCKS) - 1))
    return dict(X=X, Y=Y, e=(8 if weighted else 0) + j + j + 1, weighted=weighted)


KFOLD_BLOCKS = (36,) * 7                                 # ns = 252, 9 folds x 4 members per block


def exact_kfold(weighted=True, nt=100, seed=2):
    """Exactly summable k-fold inputs, as the dense suite builds them: full blocks of 36 = 9 folds x 4 members, so that
    without a fold kf = 32, and with 32 labels per source ks = 64.  Quantum 2^-e with e = 8 + 5 + 6."""
    rng = np.random.default_rng(seed)
    X, Y = _block_square(rng, KFOLD_BLOCKS, weighted, lambda size: 32, nt)
    fold = (np.arange(X.shape[0]) % 36 % 9).astype(np.int32)
    return dict(X=X, Y=Y, fold=fold, nfolds=9, e=(8 if weighted else 0) + 5 + 6, weighted=weighted)


SPMM_RMAX = 8            # R holds i / 16 with |i| <= SPMM_RMAX


def spmm_operands(M=301, K=1300, weighted=True, exact=True, seed=3, widest=65):
    """W (M x K; M no multiple of 64): every seventh row empty, row 11 full, the others 1..40 entries, the last row one
    entry in the last column; weights k/16 (k = 8..16) or all ones.  R (K x widest): exact, i/16 with integers
    |i| <= SPMM_RMAX; else standard normal.  Exact operands: a term is a multiple of 2^-8 (2^-4
    pattern-only) and at most 16 * SPMM_RMAX quanta, so every partial sum of a row, in any order and with any sign
    pattern, stays below spmm_quanta_bound(W) quanta; below 2^24 it is exact in fp32."""
    rng = np.random.default_rng(seed)
    rows = []
    for m in range(M):
        n = 0 if m % 7 == 0 else (K if m == 11 else int(rng.integers(1, 41)))
        rows.append(np.sort(rng.choice(K, n, replace=False)))
    rows[M - 1] = np.array([K - 1])
    indptr = np.cumsum([0] + [len(r) for r in rows])
    W = sp.csr_matrix((_weights(rng, int(indptr[-1]), weighted), np.concatenate(rows), indptr), shape=(M, K))
    if exact:
        R = rng.integers(-SPMM_RMAX, SPMM_RMAX + 1, size=(K, widest)) / 16.0
    else:
        R = rng.standard_normal((K, widest))       # (an fp32 test rounds it to fp32 before it takes the reference)
    return W, R


def spmm_quanta_bound(W):
    """Largest |partial sum| of W @ R on exact operands, in quanta of 2^-8: longest row x 16 x SPMM_RMAX."""
    return int(np.diff(sp.csr_matrix(W).indptr).max()) * 16 * SPMM_RMAX


# ----------------------------------------------------------------------------- ordinary inputs for the bands
def band_graph(weighted=True, ns=608, nt=130, nq=67, seed=5):
    """Low-fill inputs with arbitrary degrees: X (ns x ns, about six entries per row, non-zero diagonal, not symmetric),
    Xq (nq x ns, 0..12 features per row), Ys (0..5 labels per source, target 0 on six sources of seven -- a row of Ys'
    that the length-sorted stage-2 operand splits at SS_SELL_LMAX = 256 --, the last target empty).  Weights are fp32 numbers in (0.5, 1] or all ones.  Most scores have fewer than ten terms.  The same
    X serves query rows, source rows, leave-one-out (most sources that share a feature with the held-out one do not own
    its feature: their bit of the kernel's bitmap is 0) and k-fold (fold = index % 5)."""
    rng = np.random.default_rng(seed)

    def values(n):
        return (1.0 - 0.5 * rng.random(n)).astype(np.float32).astype(np.float64) if weighted else np.ones(n)

    X = sp.random(ns, ns, density=5.0 / ns, format="lil", random_state=rng)
    X.setdiag(1.0)
    X = sp.csr_matrix(X)
    X.sort_indices()
    X.data = values(X.nnz)
    Xq = sp.random(nq, ns, density=6.0 / ns, format="csr", random_state=rng)
    Xq.sort_indices()
    Xq.data = values(Xq.nnz)
    Y = sp.random(ns, nt - 1, density=2.0 / nt, format="lil", random_state=rng)
    Y[np.flatnonzero(np.arange(ns) % 7 != 0), 0] = 1.0
    Y = sp.csr_matrix(sp.hstack([sp.csr_matrix(Y), sp.csr_matrix((ns, 1))]))
    Y.data[:] = 1.0
    Y.sort_indices()
    fold = (np.arange(ns) % 5).astype(np.int32)
    return dict(Xq=Xq, X=X, Y=Y, fold=fold, nfolds=5, weighted=weighted)


# ----------------------------------------------------------------------------- fp64 references (the oracle)
def oracle_query(Xq, Xs, Ys):
    return O.predict_factored(Xq, Xs, Ys, "query")


def oracle_source(Xs, Ys):
    return O.predict_factored(None, Xs, Ys, "source")


def oracle_transfer(Xq, Xs, Ys):
    return O.transfer_factored(Xq, Xs, Ys, "query")


def oracle_loo(X, Y, rows=None, clean=False):
    return O.predict_loo_factored(X, Y, clean_flag=clean, queries=rows)


def oracle_kfold(X, Y, fold):
    return D.oracle_folds(sp.csr_matrix(X).toarray(), sp.csr_matrix(Y).toarray(), fold)


def clean_mask(Ys, loo_rows=None):
    """Positions that clean! sets to -99: targets without a source; leave-one-out: also the targets whose only source is
    the held-out one."""
    Ys = sp.csr_matrix(Ys)
    kt = np.asarray((Ys != 0).sum(axis=0)).ravel()
    if loo_rows is None:
        return kt == 0
    return (kt[None, :] - (Ys[np.asarray(loo_rows)] != 0).toarray()) == 0


# ----------------------------------------------------------------------------- term counts
def _nz(M):
    M = sp.csr_matrix(M)
    M.eliminate_zeros()
    return sp.csr_matrix((np.ones(M.nnz), M.indices, M.indptr), shape=M.shape)


def _score_counts(N, Y):
    """From N[r][s] (fma steps of stage 1 behind T[r][s]; 0 where T[r][s] is a structural zero) and the labels: per
    score the longest stage-1 chain among its addends and the number of non-zero addends."""
    Yc = sp.csc_matrix(_nz(Y))
    chain = np.zeros((N.shape[0], Y.shape[1]))
    for t in range(Y.shape[1]):
        s = Yc.indices[Yc.indptr[t]:Yc.indptr[t + 1]]
        if len(s):
            chain[:, t] = N[:, s].max(axis=1)
    return chain, (N > 0).astype(np.float64) @ Yc.toarray()


def counts_query(Xq, Xs, Ys, source_rows=False):
    """(chain, addends) per score of query rows (or of all source rows: Xq is Xs and the target path Ys (1/kt) Ys' is
    folded into the same accumulator)."""
    Xs, Ys = _nz(Xs), _nz(Ys)
    kf, ks, _ = O.degrees(Xs, Ys)
    L = _nz(Xs if source_rows else Xq)
    N = (L @ sp.diags((kf > 0).astype(np.float64)) @ Xs.T).toarray()
    if source_rows:
        N = N + (Ys @ Ys.T).toarray()
    return _score_counts(N * (ks > 0)[None, :], Ys)


def counts_loo(X, Y, rows=None):
    X, Y = _nz(X), _nz(Y)
    n = X.shape[0]
    rows = np.arange(n) if rows is None else np.asarray(rows)
    kf, ks, _ = O.degrees(X, Y)
    Xd = X.toarray()
    L = Xd[rows] * (kf - 1 > 0)[None, :]
    L[np.arange(len(rows)), rows] = 0.0                 # the dropped feature
    N = L @ Xd.T
    N *= (ks[None, :] - Xd[:, rows].T) > 0
    N[np.arange(len(rows)), rows] = 0.0                 # the held-out source
    return _score_counts(N, Y)


def counts_kfold(X, Y, fold):
    return D._fold_apply(lambda a, b, y: counts_query(a, b, y), sp.csr_matrix(X).toarray(), sp.csr_matrix(Y).toarray(),
                         fold, None)


# ----------------------------------------------------------------------------- bands
def gamma(k, u):
    k = np.asarray(k, dtype=np.float64)
    return k * u / (1.0 - k * u)


def band_graph_scores(want, chain, addends, dtype, sell_chunks=1, parts=0, dual=False):
    """|got - oracle| <= band for every score of a graph prediction with non-negative inputs: band = gamma(k) * score,
    k the largest number of roundings any term x_qa (1/kf_a) x_sa (1/ks_s) y_st of the score passes through, counted in
    simspread.jl_amd/csrc/transfer.hip (stage 1) and kernels.hip (stage 2):
      1  fl(1/kf): degree_kernel (assemble.hip), fold_inverse for k-fold; leave-one-out: T(1) / T(kf - 1) in
         transfer_kernel; the target path of source rows: fl(1/kt)
      1  the coefficient cf = L[r,a] * inv1[a] (transfer_kernel, transfer_coef_kernel)
      chain  one per fma of subrows_fold, acc[j] = fma(cf, v, acc[j]): T[r][s] is a chain of one fma per feature that r
         and s share, and for source rows per target they share (second term, same accumulator); the longest chain
         among the sources that feed the score
      1  SS_TRANSFER_DUAL=1 only (`dual`): the two accumulator copies are added when T is written
      1  fl(1/ks) (degree_kernel, fold_inverse; leave-one-out: T(1) / T(ks - bit))
      1  z = sum * inv2[s], the element of T
      addends  stage 2, spmm_sell_kernel: acc = fma(w, t, acc) (pattern-only: pairwise adds of four), one rounding per
         add at most, over the sources of the target whose T[r][s] is not a structural zero (adding an exact zero does
         not round)
      sell_chunks  one per chunk of the SELL operand: r = mine + fprev
      parts  length-sorted operand: unpermute_kernel adds the part sums of a split row (v += src[inv[x]])
    with u = 2^-24 or 2^-53.  The reference is itself an fp64 computation of the same operations, at most k roundings
    per term: gamma(k) at 2^-53 is added (for fp32 that is 2^-29 of the band).  A structural zero has band 0."""
    want = np.asarray(want, dtype=np.float64)
    k = 2 + chain + (1 if dual else 0) + 2 + addends + sell_chunks + parts
    u = U32 if np.dtype(dtype) == np.float32 else U64
    return np.where(want > 0, (gamma(k, u) + gamma(k, U64)) * want, 0.0)


def band_spmm(W, R, dtype, nchunks):
    """Raw W @ R with signed R: |got - want| <= gamma(n_row + nchunks + 1) * (|W| |R|)_ij, n_row the entries of row i:
    one rounding per fma of the row (n_row), one per partial sum of a column chunk that is added (nchunks), one for a
    final combination of workgroup partials; plus the fp64 reference's own n_row roundings.  (The length-sorted SELL
    operand splits a row of more than lmax >= 256 entries into parts that unpermute_kernel adds: fma chains of at most
    lmax steps and at most n_row / lmax + 1 further adds, fewer than the n_row counted here.)"""
    W = sp.csr_matrix(W)
    n = np.diff(W.indptr).astype(np.float64)[:, None]
    mag = np.asarray(abs(W) @ np.abs(R))
    u = U32 if np.dtype(dtype) == np.float32 else U64
    return (gamma(n + nchunks + 1, u) + gamma(n, U64)) * mag


def parts_of_targets(Ys, lmax):
    """Virtual rows per target of the length-sorted stage-2 operand (vrow_parts in assemble.hip): ceil(len / lmax),
    counted only where a row is split."""
    kt = np.asarray((sp.csr_matrix(Ys) != 0).sum(axis=0)).ravel()
    p = -(-kt // lmax)
    return np.where(p > 1, p, 0).astype(np.float64)[None, :]


# ----------------------------------------------------------------------------- the assertions
def assert_bitwise(got, want64, dtype, label=""):
    """got equals the oracle rounded to dtype, bit for bit (fp64: the oracle itself)."""
    got = np.ascontiguousarray(got)
    want = np.ascontiguousarray(np.asarray(want64, dtype=np.float64).astype(dtype))
    assert got.dtype == np.dtype(dtype) and got.shape == want.shape, (got.dtype, got.shape, want.shape)
    bits = np.uint32 if np.dtype(dtype) == np.float32 else np.uint64
    bad = got.view(bits) != want.view(bits)
    if bad.any():
        idx = np.argwhere(bad)
        d = np.abs(got.astype(np.float64)[bad] - np.asarray(want64)[bad])
        raise AssertionError(f"{label}: {int(bad.sum())} of {bad.size} scores differ from the oracle's bits; first at "
                             f"{idx[:8].tolist()}, largest |diff| {d.max():.3e}")


def assert_band(got, want64, band, label=""):
    """Every score within its band (band 0: an exact zero); returns the largest error / band."""
    got = np.asarray(got, dtype=np.float64)
    assert got.shape == want64.shape == band.shape, (got.shape, want64.shape, band.shape)
    err = np.abs(got - want64)
    bad = ~(err <= band)
    nz = band > 0
    ratio = float((err[nz] / band[nz]).max()) if nz.any() else 0.0
    print(f"[sparse] {label}: largest error / band = {ratio:.3f} over {int(nz.sum())} non-zero scores")
    if bad.any():
        idx = np.argwhere(bad)
        raise AssertionError(f"{label}: {int(bad.sum())} of {bad.size} scores outside their band, largest error / band "
                             f"{ratio:.3f}; first at {idx[:8].tolist()}")
    return ratio


# ----------------------------------------------------------------------------- sequential model of the two stages
def _inv(d, dt):
    d = np.asarray(d)
    out = np.zeros(d.shape, dtype=dt)
    out[d > 0] = dt(1) / d[d > 0].astype(dt)
    return out


def used_entry(L, Xs, Ys, long_row=False):
    """(source, feature) of an entry of Xs that a score depends on: the feature is named by a row of L, has a source
    with a label; long_row: the entry sits in the feature with the most sources."""
    L, Xc, Ys = sp.csr_matrix(L), sp.csc_matrix(Xs), sp.csr_matrix(Ys)
    named = np.unique(L.indices)
    kf = np.diff(Xc.indptr)[named]
    order = named[np.argsort(-kf, kind="stable")] if long_row else named[kf > 0]
    for a in order:
        for s in Xc.indices[Xc.indptr[a]:Xc.indptr[a + 1]][::-1]:
            if Ys.indptr[s + 1] > Ys.indptr[s]:
                return int(s), int(a)
    raise AssertionError("no entry of Xs reaches a score")


def emulate(L, Xs, Ys, dtype=np.float32, loo_rows=None, source_rows=None, defect=None, entry=None):
    """The two stages one operation at a time in `dtype`, every product and every sum rounded (no fma: it rounds at
    least as often as the kernels).  L: the rows (CSR, nr x nf); loo_rows: the source ids of the rows for the
    leave-one-out form, source_rows: for source rows, whose target path is folded into the same sums (L = X[rows] in
    both).  Degrees are counted on the unmodified operands, as graph_degrees does.
    defect: None, or with entry = (source, feature) "dropped entry" / "doubled entry" (the entry of X' is skipped / added
    twice in stage 1), or for leave-one-out "ks instead of ks - 1" (the bitmap is ignored) / "kept dropped feature"."""
    dt = np.dtype(dtype).type
    L, Xs, Ys = sp.csr_matrix(L), sp.csr_matrix(Xs), sp.csr_matrix(Ys)
    ns = Xs.shape[0]
    kf, ks, kt = O.degrees(Xs, Ys)
    XT = sp.csr_matrix(Xs.T)
    XT.sort_indices()
    YT = sp.csr_matrix(Ys.T)
    Xc = sp.csc_matrix(Xs)
    inv_kf, inv_ks, inv_kt = _inv(kf, dt), _inv(ks, dt), _inv(kt, dt)
    out = np.zeros((L.shape[0], Ys.shape[1]), dtype=dt)

    def fold(acc, M, a, cf):
        idx = M.indices[M.indptr[a]:M.indptr[a + 1]]
        val = M.data[M.indptr[a]:M.indptr[a + 1]].astype(dt)
        if entry is not None and M is XT and a == entry[1] and defect in DEFECTS:
            hit = idx == entry[0]
            if defect == "dropped entry":
                idx, val = idx[~hit], val[~hit]
            else:
                acc[idx[hit]] = acc[idx[hit]] + cf * val[hit]
        acc[idx] = acc[idx] + cf * val          # the indices of a sub-row are distinct

    for r in range(L.shape[0]):
        acc = np.zeros(ns, dtype=dt)
        i = None if loo_rows is None else int(loo_rows[r])
        for p in range(L.indptr[r], L.indptr[r + 1]):
            a, lv = int(L.indices[p]), dt(L.data[p])
            if i is None:
                cf = lv * inv_kf[a]
            else:
                d = int(kf[a]) - 1
                cf = lv * (dt(1) / dt(d)) if d > 0 and (a != i or defect == "kept dropped feature") else dt(0)
            if cf != 0:
                fold(acc, XT, a, cf)
        if source_rows is not None:
            sr = int(source_rows[r])
            for p in range(Ys.indptr[sr], Ys.indptr[sr + 1]):
                t = int(Ys.indices[p])
                cf = dt(Ys.data[p]) * inv_kt[t]
                if cf != 0:
                    fold(acc, YT, t, cf)
        if i is None:
            z = acc * inv_ks
        else:
            d = ks.copy()
            if defect != "ks instead of ks - 1":
                d[Xc.indices[Xc.indptr[i]:Xc.indptr[i + 1]]] -= 1
            z = acc * _inv(d, dt)
            z[i] = 0
        row = out[r]
        for s in np.flatnonzero(z):
            c = Ys.indices[Ys.indptr[s]:Ys.indptr[s + 1]]
            row[c] = row[c] + z[s] * Ys.data[Ys.indptr[s]:Ys.indptr[s + 1]].astype(dt)
    return out


def emulate_kfold(X, Y, fold, dtype=np.float32, defect=None, entry=None):
    """k-fold through emulate on the graph without each fold's members.  entry = (source, feature) in the numbering of
    the whole graph; it takes effect in the folds that hold neither."""
    Xd, Yd, fold = sp.csr_matrix(X).toarray(), sp.csr_matrix(Y).toarray(), np.asarray(fold)
    out = np.zeros(Yd.shape, dtype=dtype)
    for phi in np.unique(fold):
        mem, keep = np.flatnonzero(fold == phi), np.flatnonzero(fold != phi)
        ent = None
        if entry is not None and entry[0] in keep and entry[1] in keep:
            ent = (int(np.searchsorted(keep, entry[0])), int(np.searchsorted(keep, entry[1])))
        out[mem] = emulate(Xd[np.ix_(mem, keep)], Xd[np.ix_(keep, keep)], Yd[keep], dtype,
                           defect=defect if ent else None, entry=ent)
    return out
