"""Host model, references, bands and input builders for the tests of the dense-similarity regime (numpy, no device).

The model restates what dense_bf16.hip's header comment promises, not its code: an fp32 operand is the sum of three bf16
numbers (hi = bf16(x), mid = bf16(x - hi), lo = bf16(x - hi - mid), round to nearest even), the query side is
cut(S) * fl32(1/kf) rounded once to fp32 and then split, the source side is cut(S) split, and the transfer element is the
sum of the kept plane products (all three query planes against the single 0/1 source plane when unweighted, the six
products hi*hi, hi*mid, mid*hi, mid*mid, hi*lo, lo*hi when weighted) times fl32(1/ks).  Sums are taken in fp64, so the
model is the kernel with ideal accumulation.  Every defect the tests must be able to see is a parameter of the model.

References are oracle/simspread_oracle.py in fp64.  The fold modes (leave-one-out, k-fold) go through
O.predict_factored on the graph without the fold's members, which is what construct(y, X, queries) builds
(src/core.jl:148-201): the members' rows leave the sources and the features named after them leave the columns.
"""
import numpy as np
import scipy.sparse as sp

from oracle import simspread_oracle as O

EPS = 2.0 ** -24          # unit roundoff of fp32
PAIRS_W = ((0, 0), (0, 1), (1, 0), (1, 1), (0, 2), (2, 0))   # (query plane, source plane), 0 = hi, 1 = mid, 2 = lo
PAIRS_U = ((0, 0), (1, 0), (2, 0))


# ----------------------------------------------------------------------------- bf16 planes
def bf16_rne(x):
    """fp32 -> nearest bf16 (ties to even), returned as fp32.  Finite inputs."""
    u = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32).astype(np.uint64)
    u = (u + 0x7FFF + ((u >> 16) & 1)) & 0xFFFF0000
    return u.astype(np.uint32).view(np.float32)


def planes(x):
    """[hi, mid, lo] with hi + mid + lo == x exactly (each an fp32 array holding bf16 values)."""
    x = np.ascontiguousarray(x, dtype=np.float32)
    hi = bf16_rne(x)
    r1 = x - hi            # exact: at most 16 significant bits remain
    mid = bf16_rne(r1)
    lo = bf16_rne(r1 - mid)
    return [hi, mid, lo]


def _inv(d):
    d = np.asarray(d, dtype=np.float64)
    out = np.zeros_like(d)
    out[d > 0] = 1.0 / d[d > 0]
    return out


def _inv32(d):
    d = np.asarray(d)
    out = np.zeros(d.shape, dtype=np.float32)
    out[d > 0] = np.float32(1.0) / d[d > 0].astype(np.float32)
    return out


def _degrees(Xs, Y):
    kf = np.count_nonzero(Xs, axis=0)
    ks = np.count_nonzero(Xs, axis=1) + np.count_nonzero(Y, axis=1)
    return kf, ks


# ----------------------------------------------------------------------------- the plane model and its defects
def mutants(weighted):
    """name -> keyword arguments of plane_scores for every single defect the tests must see."""
    pairs = PAIRS_W if weighted else PAIRS_U
    out = {}
    for i, p in enumerate(pairs):
        out[f"drop q{p[0]}*s{p[1]}"] = dict(pairs=pairs[:i] + pairs[i + 1:])
    for i in range(3):
        out[f"zero query plane {i}"] = dict(zero=("q", i))
    for i in range(3 if weighted else 1):
        out[f"zero source plane {i}"] = dict(zero=("s", i))
    if weighted:  # the two lo pairs read the other one's source plane (a ring-slot mix-up)
        out["lo pairs swap source planes"] = dict(pairs=PAIRS_W[:4] + ((0, 0), (2, 2)))
    return out


def plane_scores(Xq, Xs, Y, weighted, pairs=None, zero=None):
    """Scores of the rows Xq (M x K thresholded query-side values) against sources Xs (N x K) with labels Y (N x nt,
    dense) by the plane algorithm: fp32 operands, bf16 planes, the kept products, fp64 sums."""
    Xq, Xs, Y = (np.asarray(a, dtype=np.float32) for a in (Xq, Xs, Y))
    if pairs is None:
        pairs = PAIRS_W if weighted else PAIRS_U
    kf, ks = _degrees(Xs, Y)
    Ap = planes(Xq * _inv32(kf)[None, :])          # one fp32 rounding, then an exact split
    Bp = planes(Xs)                                # unweighted: 0/1, mid = lo = 0
    if zero is not None:
        (Ap if zero[0] == "q" else Bp)[zero[1]][...] = 0
    T = np.zeros((Xq.shape[0], Xs.shape[0]))
    for i, j in pairs:
        T += Ap[i].astype(np.float64) @ Bp[j].astype(np.float64).T
    T *= _inv32(ks).astype(np.float64)[None, :]
    return T @ Y.astype(np.float64)


def _fold_apply(fn, X, Y, fold, rows):
    """fn(Xq, Xs, Ys) on the graph without each fold's members, rows of `rows` only (construct(y, X, members))."""
    X, Y, fold = np.asarray(X), np.asarray(Y), np.asarray(fold)
    rows = np.arange(X.shape[0]) if rows is None else np.asarray(rows)
    out = None
    for phi in np.unique(fold[rows]):
        mem = np.flatnonzero(fold == phi)
        keep = np.flatnonzero(fold != phi)
        sel = np.isin(rows, mem)
        res = fn(X[np.ix_(rows[sel], keep)], X[np.ix_(keep, keep)], Y[keep])
        res = res if isinstance(res, tuple) else (res,)
        if out is None:
            out = tuple(np.zeros((len(rows), Y.shape[1])) for _ in res)
        for o, r in zip(out, res):
            o[sel] = r
    return out if len(out) > 1 else out[0]


def plane_scores_folds(X, Y, fold, weighted, rows=None, **defect):
    """k-fold by the plane model (leave-one-out: fold = arange(n))."""
    return _fold_apply(lambda a, b, y: plane_scores(a, b, y, weighted, **defect), X, Y, fold, rows)


def plane_scores_source(X, Y, weighted, rows, **defect):
    """Source rows: feature path by the plane model, target path (sparse fp32 kernel, not under test here) in fp64."""
    X, Y = np.asarray(X), np.asarray(Y, dtype=np.float64)
    return plane_scores(X[rows], X, Y, weighted, **defect) + _target_scores(X, Y, rows)[0]


# ----------------------------------------------------------------------------- the orientation of Ss and its defects
# Element (s, f) of the thresholded source similarity X is source s (row) against feature f (column).  Every place of
# the regime that indexes it is a parameter of transposed_scores: name -> the modes whose device path goes through it
# (k-fold recounts its degrees per fold and never reads the graph's kf / ks).
TRANSPOSE_DEFECTS = {
    "has_transposed": ("loo",),                                    # the LOO divisor ks - has reads X[q, s], not X[s, q]
    "degrees_swapped": ("query", "source", "loo"),                 # kf from row counts, ks from column counts
    "fold_recount_transposed": ("kfold",),                         # per-fold kf / ks counted over X[f, m] / X[f, s]
    "source_operand_transposed": ("query", "source", "loo", "kfold"),   # the product reads X[f, s]
    "input_transposed": ("query", "source", "loo", "kfold"),       # the whole Ss handed over transposed
}


def transposed_scores(mode, X, Y, Xq=None, fold=None, rows=None, defect=None):
    """What the device computes in `mode` ("query", "source", "loo", "kfold"), in fp64 and in the device's own form
    (degrees counted once, leave-one-out by the rank-1 corrections of the degrees, k-fold by a recount per fold), with
    one index pair of X swapped by `defect` (a key of TRANSPOSE_DEFECTS; None: the correct device).  On a symmetric X
    every defect performs the very same operations on the very same numbers as the correct form, bit for bit."""
    assert defect is None or mode in TRANSPOSE_DEFECTS[defect], (mode, defect)
    X, Y = np.asarray(X, dtype=np.float64), np.asarray(Y, dtype=np.float64)
    if defect == "input_transposed":
        X = np.ascontiguousarray(X.T)
    n = X.shape[0]
    nz = X != 0
    ny = np.count_nonzero(Y, axis=1)
    col, row = nz.sum(axis=0), nz.sum(axis=1)
    kf, ks = (row, col + ny) if defect == "degrees_swapped" else (col, row + ny)
    # B[f, s], the source side of the product: X[s, f] (a copy, so that both orientations multiply from the same layout)
    B = np.ascontiguousarray(X if defect == "source_operand_transposed" else X.T)
    if mode in ("query", "source"):
        A = np.asarray(Xq, dtype=np.float64) if mode == "query" else X[rows]
        out = ((A * _inv(kf)[None, :]) @ B * _inv(ks)[None, :]) @ Y
        if mode == "source":
            kt = np.count_nonzero(Y, axis=0)
            out = out + ((Y[rows] * _inv(kt)[None, :]) @ Y.T * _inv(ks)[None, :]) @ Y
        return out
    q = np.arange(n) if rows is None else np.asarray(rows)
    r = np.arange(len(q))
    if mode == "loo":
        U = X[q] * _inv(kf[None, :] - nz[q])
        U[r, q] = 0.0
        has = nz[q] if defect == "has_transposed" else nz[:, q].T
        V = U @ B * _inv(ks[None, :] - has)
        V[r, q] = 0.0
        return V @ Y
    assert mode == "kfold"
    fold = np.asarray(fold)
    out = np.zeros((len(q), Y.shape[1]))
    for phi in np.unique(fold[q]):
        keep = np.flatnonzero(fold != phi)
        sel = fold[q] == phi
        nzk = nz[np.ix_(keep, keep)]
        if defect == "fold_recount_transposed":
            fkf, fks = nzk.sum(axis=1), nzk.sum(axis=0) + ny[keep]
        else:
            fkf, fks = nzk.sum(axis=0), nzk.sum(axis=1) + ny[keep]
        A = X[np.ix_(q[sel], keep)]
        out[sel] = ((A * _inv(fkf)[None, :]) @ B[np.ix_(keep, keep)] * _inv(fks)[None, :]) @ Y[keep]
    return out


# ----------------------------------------------------------------------------- fp64 references (the oracle)
def _target_scores(X, Y, rows):
    """Target path of the source rows, (Ys D_t^-1) Ys' (D_s^-1 Ys), and its count of non-zero terms per score."""
    Y = np.asarray(Y, dtype=np.float64)
    _, ks = _degrees(np.asarray(X), Y)
    kt = np.count_nonzero(Y, axis=0)
    nzY = (Y != 0).astype(np.float64)
    val = ((Y[rows] * _inv(kt)[None, :]) @ Y.T * _inv(ks)[None, :]) @ Y
    cnt = (nzY[rows] @ nzY.T) @ nzY
    return val, cnt


def oracle_query(Xq, Xs, Y):
    return O.predict_factored(Xq, Xs, sp.csr_matrix(np.asarray(Y, dtype=np.float64)), "query")


def oracle_source(X, Y, rows, Xcsr=None):
    """Rows of predict_factored(rows="source") without forming all ns x ns transfer rows: the feature path of row s is
    the query form with Xq = Xs[s]; the target path is added in fp64.  test_dense_inputs_cpu.py pins it against the
    oracle's own source form.  Xcsr: X as scipy CSR, to convert a large block once."""
    X = np.asarray(X, dtype=np.float64)
    return oracle_query(X[rows], X if Xcsr is None else Xcsr, Y) + _target_scores(X, Y, rows)[0]


def oracle_folds(X, Y, fold, rows=None):
    """Row i = predict(construct(y, X, members of i's fold), y[[i], :]) through O.predict_factored."""
    return _fold_apply(oracle_query, np.asarray(X, dtype=np.float64), np.asarray(Y, dtype=np.float64), fold, rows)


# ----------------------------------------------------------------------------- bands
def terms(Xq, Xs, Y):
    """(sum of |terms|, number of non-zero terms) of every score, in fp64: |Xq|/kf @ |Xs|' / ks @ |Y|."""
    Xq, Xs, Y = (np.asarray(a, dtype=np.float64) for a in (Xq, Xs, Y))
    kf, ks = _degrees(Xs, Y)
    mag = ((np.abs(Xq) * _inv(kf)[None, :]) @ np.abs(Xs).T * _inv(ks)[None, :]) @ np.abs(Y)
    cnt = ((((Xq != 0) & (kf > 0)[None, :]).astype(np.float64) @ (Xs != 0).T.astype(np.float64)) * (ks > 0)[None, :]) @ (Y != 0)
    return mag, cnt


def terms_folds(X, Y, fold, rows=None):
    return _fold_apply(terms, np.asarray(X, dtype=np.float64), np.asarray(Y, dtype=np.float64), fold, rows)


def terms_loo(X, Y, rows):
    """terms() of the leave-one-out rows `rows` as matrix products over the whole block (the identity of
    O.predict_loo_dense_blocked with magnitudes and counts; test_dense_inputs_cpu.py pins it against terms_folds)."""
    X, Y = np.asarray(X, dtype=np.float64), np.asarray(Y, dtype=np.float64)
    q = np.asarray(rows)
    r = np.arange(len(q))
    nz = X != 0
    kf, ks = _degrees(X, Y)
    dk = kf[None, :] - nz[q]
    U = np.abs(X[q]) * _inv(dk)
    Uc = (nz[q] & (dk > 0)).astype(np.float64)
    U[r, q] = 0.0
    Uc[r, q] = 0.0
    dn = ks[None, :] - nz[:, q].T
    V = U @ np.abs(X).T * _inv(dn)
    Vc = Uc @ nz.T.astype(np.float64) * (dn > 0)
    V[r, q] = 0.0
    Vc[r, q] = 0.0
    return V @ np.abs(Y), Vc @ (Y != 0)


def terms_source(X, Y, rows):
    mag, cnt = terms(np.asarray(X)[rows], X, Y)
    tv, tc = _target_scores(X, Y, rows)
    return mag + tv, cnt + tc


def band_general(mag, cnt, dropped_products=False):
    """(n + 2) * 2^-24 * sum|terms| per score, n the number of non-zero terms.  For the fp32-input engine (an fma chain
    with one rounding per step) this is the worst case on the inputs of random_inputs: n roundings for the terms,
    fl(1/ks) and the final product.  The weighted plane engines drop three of nine plane products, together below
    2^-24 of the term: one more unit.  For the plane engines the band is not a worst case: the bf16 matrix instruction
    adds in fixed point with one guard bit, up to one ulp per accumulation instead of half;
    what they reach is printed by the GPU tests and recorded in DESIGN.md section 5."""
    return (cnt + 2 + (1 if dropped_products else 0)) * EPS * mag


def band_single_term(want):
    """Unweighted, one feature per query row, one source per target: the score is fl(fl(1/kf) * fl(1/ks)), three
    roundings, (1 + 2^-24)^3 - 1 < 4 * 2^-24."""
    return 4 * EPS * np.abs(want)


# ----------------------------------------------------------------------------- the assertions (shared by CPU and GPU tests)
def bitwise_violations(got, want64):
    """Elements of the fp32 result that are not float32(oracle), bit for bit (-0 and +0 are told apart)."""
    got = np.ascontiguousarray(got, dtype=np.float32)
    want = np.ascontiguousarray(np.asarray(want64, dtype=np.float64).astype(np.float32))
    assert got.shape == want.shape
    return got.view(np.uint32) != want.view(np.uint32)


def assert_bitwise(got, want64, label=""):
    bad = bitwise_violations(got, want64)
    if bad.any():
        idx = np.argwhere(bad)
        g = np.asarray(got, dtype=np.float64)[bad]
        w = np.asarray(want64)[bad]
        raise AssertionError(f"{label}: {int(bad.sum())} of {bad.size} scores differ from float32(oracle); first at "
                             f"{idx[:8].tolist()}, largest |diff| {np.abs(g - w).max():.3e}")


def band_violations(got, want64, band):
    got = np.asarray(got, dtype=np.float64)
    assert got.shape == want64.shape == band.shape
    return ~(np.abs(got - want64) <= band)      # a NaN violates; band 0 demands an exact zero


def assert_band(got, want64, band, label=""):
    """Element-wise |got - oracle| <= band; returns the largest error / band (over the scores with a non-zero band)."""
    bad = band_violations(got, want64, band)
    err = np.abs(np.asarray(got, dtype=np.float64) - want64)
    nz = band > 0
    ratio = float((err[nz] / band[nz]).max()) if nz.any() else 0.0
    print(f"[dense] {label}: largest error / band = {ratio:.3f} over {int(nz.sum())} non-zero scores")
    if bad.any():
        idx = np.argwhere(bad)
        raise AssertionError(f"{label}: {int(bad.sum())} of {bad.size} scores outside their band, largest error / band "
                             f"{ratio:.3f}; first at {idx[:8].tolist()}")
    return ratio


# ----------------------------------------------------------------------------- input builders
ALPHA = float(np.float32(0.4))
FAMILY_LOW = float(np.float32(0.5 + 2.0 ** -10 - 2.0 ** -19))
BLOCKS_QUERY = (32,) * 3 + (16,) * 4 + (8,) * 5 + (4,) * 6 + (2,) * 8 + (1,) * 15        # ns = 255
BLOCKS_LOO = (33,) * 2 + (17,) * 2 + (9,) * 3 + (5,) * 3 + (3,) * 4 + (2,) * 5           # ns = 164
BLOCKS_KFOLD = (36,) * 4                                                                 # ns = 144, 9 folds x 4 members
# asymmetric values: no leave-one-out block of two (its one product reads only the diagonal of the source operand)
BLOCKS_LOO_ASYM = (33,) * 2 + (17,) * 2 + (9,) * 3 + (5,) * 5 + (3,) * 4                 # ns = 164


def _family(rng, shape):
    """0.5 + 2^-10 + l * 2^-19, l in {-1, 0, 1}: hi = 0.5, mid = 2^-10, lo = l * 2^-19, stable planes, every kept
    plane product a multiple of 2^-20."""
    return (0.5 + 2.0 ** -10 + rng.integers(-1, 2, size=shape) * 2.0 ** -19).astype(np.float32)


def _filler(rng, shape, alpha):
    """Values below alpha: one ulp below, a little below, far below, zero."""
    a = np.float32(alpha)
    pool = np.array([np.nextafter(a, np.float32(0)), a * np.float32(0.97), 0.25, 0.01, 0.0], dtype=np.float32)
    return pool[rng.integers(0, len(pool), size=shape)]


def _sym(a):
    return np.triu(a) + np.triu(a, 1).T


def _family_asym(rng, n):
    """_family values on an n x n matrix with element (i, j) != element (j, i) for every i != j (the lo plane of the
    lower triangle is one of the two other values of its mirror)."""
    up = rng.integers(-1, 2, size=(n, n))
    low = (up.T + 1 + rng.integers(1, 3, size=(n, n))) % 3 - 1
    return (0.5 + 2.0 ** -10 + (np.triu(up) + np.tril(low, -1)) * 2.0 ** -19).astype(np.float32)


def exact_inputs(mode, seed=0, nq=130, alpha_edge=False, symmetric=True):
    """Exactly summable weighted inputs (tier 1).  mode "query": blocks of 2^j sources with 2^j targets each (kf = 2^j,
    ks = 2^(j+1)); "loo": blocks of 2^j + 1 with 2^j targets (kf - 1 = 2^j, ks - has = 2^(j+1)); "kfold": blocks of 36 =
    9 folds x 4 members with 32 targets per source (per-fold kf = 32, ks = 64).  All pairs inside a block are kept and
    nothing else, members are scattered by a random permutation, every target has exactly one source.  alpha is 0.4,
    or with alpha_edge the lowest value of the family, so that a third of the kept entries sit exactly at alpha (a kept
    entry of value float32(0.4) cannot belong to an exactly summable family: its planes are not stable).
    symmetric=False: the same block pattern (the exactness argument needs it) with Ss[i, j] != Ss[j, i] for every pair
    inside a block and an independent filler on either side of the diagonal; leave-one-out blocks have three or more
    members.  The values stay exactly summable.
    Returns a dict: Sq, Ss (fp32), Y (dense fp32), alpha, fold (kfold) and the block id of every source."""
    rng = np.random.default_rng(seed)
    sizes = {"query": BLOCKS_QUERY, "loo": BLOCKS_LOO if symmetric else BLOCKS_LOO_ASYM, "kfold": BLOCKS_KFOLD}[mode]
    alpha = FAMILY_LOW if alpha_edge else ALPHA
    ns = int(sum(sizes))
    perm = rng.permutation(ns)
    block = np.empty(ns, dtype=np.int64)
    fold = np.zeros(ns, dtype=np.int32)
    if symmetric:
        Ss = _sym(_filler(rng, (ns, ns), alpha))
        fam = _sym(_family(rng, (ns, ns)))
    else:
        Ss = _filler(rng, (ns, ns), alpha)
        fam = _family_asym(rng, ns)
    tcount = np.zeros(ns, dtype=np.int64)
    o = 0
    for b, size in enumerate(sizes):
        mem = perm[o:o + size]
        o += size
        block[mem] = b
        Ss[np.ix_(mem, mem)] = fam[np.ix_(mem, mem)]
        tcount[mem] = {"query": size, "loo": size - 1, "kfold": 32}[mode]
        if mode == "kfold":
            fold[mem] = np.arange(size) % 9
    nt = int(tcount.sum())
    Y = np.zeros((ns, nt), dtype=np.float32)
    Y[np.repeat(np.arange(ns), tcount), rng.permutation(nt)] = 1.0     # every target column: exactly one source
    keep = rng.random((nq, ns)) < 0.5
    Sq = np.where(keep, _family(rng, (nq, ns)), _filler(rng, (nq, ns), alpha)).astype(np.float32)
    return dict(Sq=Sq, Ss=Ss, Y=Y, alpha=alpha, fold=fold, block=block, mode=mode)


def single_feature_inputs(seed=1, nq=129, ns=260, alpha=0.85, symmetric=True):
    """Unweighted, one feature per query row, one source per target (tier 2): the score is the single term
    fl(1/kf) * fl(1/ks).  Degrees are whatever the random symmetric pattern gives (15 % of the pairs kept: around
    40, odd and even, hardly a power of two).  symmetric=False: an iid pattern, kf a column count and ks a row count
    that differ."""
    rng = np.random.default_rng(seed)
    Ss = rng.random((ns, ns)).astype(np.float32)
    if symmetric:
        Ss = _sym(Ss)
    np.fill_diagonal(Ss, 1.0)
    Sq = (rng.random((nq, ns)) * np.float32(alpha) * 0.99).astype(np.float32)      # all below alpha ...
    Sq[np.arange(nq), rng.integers(0, ns, nq)] = np.float32(alpha) + rng.random(nq).astype(np.float32) * 0.2  # ... but one
    tcount = rng.integers(0, 3, ns)
    nt = int(tcount.sum())
    Y = np.zeros((ns, nt), dtype=np.float32)
    Y[np.repeat(np.arange(ns), tcount), rng.permutation(nt)] = 1.0
    return dict(Sq=Sq, Ss=Ss, Y=Y, alpha=float(np.float32(alpha)))


WEIGHTED_BLOCKS = {"query": (1, 2, 4, 8), "loo": (2, 3, 5, 9), "kfold": (3, 6, 12)}


def _column_pattern(rng, m, per_class, nclass):
    """m x m boolean pattern, position p in class p % nclass: every column keeps `per_class` positions of each class,
    its own diagonal among them, the others drawn at random.  Column degrees are per_class * nclass, row degrees are
    whatever the draw gives, and a kept pair's mirror is kept only by chance."""
    pat = np.zeros((m, m), dtype=bool)
    for j in range(m):
        pat[j, j] = True
        for c in range(nclass):
            cand = np.arange(c, m, nclass)
            own = c == j % nclass
            pat[rng.choice(cand[cand != j], per_class - own, replace=False), j] = True
    return pat


def random_inputs(nq, ns, weighted, mode="query", seed=None, symmetric=True):
    """General inputs (tiers 2 and 3) with 24-bit random values, one entry exactly at alpha on either side, one source
    per target and 0..2 targets per source, so that a score is one transfer element.

    A band of (n + 2) * 2^-24 * sum|terms| resolves a missing lo product (2^-18 of one term, random sign) only while n
    is small (test_dense_inputs_cpu.py: with 20 terms a missing hi*lo product shows on 1 % of the scores, with 3 on
    70 %), so both kinds keep a score at a handful of terms.

    Unweighted (the same graph serves every mode): iid U(0,1), Ss symmetric with unit diagonal, sqrt(3 / ns) of the
    pairs kept: about three terms per score, arbitrary degrees.  The band is then the worst case of an fp32 sum: one
    rounding for fl(1/kf) (the products with 1.0 are exact), n - 1 additions, fl(1/ks) and the final product.

    Weighted: U(alpha, 1] values on a block pattern (all pairs of a block kept, nothing else, members scattered by a
    permutation, a few sources left without any edge) whose block sizes make the feature scaling of `mode` exact:
    powers of two for "query" (also predict("source")), 2^j + 1 for "loo" (1/(kf - 1)), 3 * 2^j over three folds for
    "kfold" (per-fold kf = 2^(j+1)).  A weighted term otherwise carries two more roundings, fl(1/kf) and fl(x * fl(1/kf)),
    which the band does not count: with them the fp32-input engine, an exact fma chain, left the band by up to 1.26 on
    iid inputs.  With exact scaling the band is the worst case of that engine: n roundings of the fma chain, fl(1/ks)
    and the final product.  ks stays arbitrary (block size + 0..2 targets).

    symmetric=False.  Unweighted: the iid matrix as drawn, the entry exactly at alpha on one side only; pattern, kf
    (column counts) and ks (row counts) are all asymmetric.  Weighted: a block of 2 w members for a column degree w
    from the list above; every column keeps w of the block's rows (its diagonal and a random choice; for "kfold" w / 3
    of each fold, fold = position % 3), so kf, kf - 1 and the per-fold kf are the same powers of two and the scaling
    stays exact, while the row degrees, ks and the leave-one-out divisor ks - has vary with the pair."""
    rng = np.random.default_rng((1000 * ns + nq if seed is None else seed) + {"query": 0, "loo": 1, "kfold": 2}[mode] * weighted)
    tcount = rng.integers(0, 3, ns)
    nt = int(tcount.sum())
    Y = np.zeros((ns, nt), dtype=np.float32)
    Y[np.repeat(np.arange(ns), tcount), rng.permutation(nt)] = 1.0
    if not weighted:
        alpha = np.float32(1.0 - np.sqrt(3.0 / ns))
        Ss = rng.random((ns, ns)).astype(np.float32)
        if symmetric:
            Ss = _sym(Ss)
        np.fill_diagonal(Ss, 1.0)
        Ss[3, 7] = Ss[7, 3] = alpha        # exactly alpha: kept
        if not symmetric:
            Ss[7, 3] = alpha * np.float32(0.5)     # ... on one side only
        Sq = rng.random((nq, ns)).astype(np.float32)
        Sq[0, 1] = alpha
        return dict(Sq=Sq, Ss=Ss, Y=Y, alpha=float(alpha), fold=(np.arange(ns) * 7 % 4).astype(np.int32), nfolds=4)
    alpha = np.float32(0.5)
    value = lambda shape: (alpha + np.float32(0.5) * (1.0 - rng.random(shape))).astype(np.float32)     # (alpha, 1]
    below = lambda shape: (rng.random(shape) * 0.495).astype(np.float32)
    sizes = WEIGHTED_BLOCKS[mode]
    perm = rng.permutation(ns)
    Ss, vals = below((ns, ns)), value((ns, ns))
    if symmetric:
        Ss, vals = _sym(Ss), _sym(vals)
    fold = rng.integers(0, 3, ns).astype(np.int32)
    o, first = 0, None
    while ns - o >= (1 if symmetric else 2) * sizes[-1] + 3:    # the last three or more sources stay without any edge (kf = 0)
        size = int(rng.choice(sizes))
        if not symmetric:
            # `size` is the column degree w, the block has 2 w members and every column keeps a set of its own
            pat = _column_pattern(rng, 2 * size, size // 3 if mode == "kfold" else size, 3 if mode == "kfold" else 1)
            size *= 2
        mem = perm[o:o + size]
        o += size
        if symmetric:
            Ss[np.ix_(mem, mem)] = vals[np.ix_(mem, mem)]
        else:
            Ss[np.ix_(mem, mem)] = np.where(pat, vals[np.ix_(mem, mem)], Ss[np.ix_(mem, mem)])
        fold[mem] = np.arange(size) % 3
        if symmetric and size > 1 and first is None:
            first = mem
        if not symmetric and first is None and (pat & ~pat.T).any():      # a kept pair whose mirror is cut
            first = mem[np.argwhere(pat & ~pat.T)[0]]
    Ss[first[0], first[1]] = alpha         # exactly alpha: kept
    if symmetric:
        Ss[first[1], first[0]] = alpha
    Sq = np.where(rng.random((nq, ns)) < 0.5, value((nq, ns)), below((nq, ns))).astype(np.float32)
    Sq[0, 1] = alpha
    return dict(Sq=Sq, Ss=Ss, Y=Y, alpha=float(alpha), fold=fold, nfolds=3)


def cut(S, alpha, weighted):
    """featurize's cutoff of fp32 similarities at the fp32 alpha, in fp64 (O.cutoff)."""
    return O.cutoff(np.asarray(S, dtype=np.float32).astype(np.float64), float(np.float32(alpha)), weighted)


def row_ranges(ns):
    """Row ranges for predict("source") / predict_loo: begin % 4 in {0, 1, 2, 3}, lengths 128, 129, below 4, and one
    that ends with the last row."""
    last = max(3, ((ns - 128) // 4) * 4 - 1)
    b = 5 if ns >= 134 else 1
    return [(0, min(128, ns)), (b, b + 129), (6, 9), (last, ns)]
