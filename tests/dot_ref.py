"""Host reference of the inner-product similarity producer (ss_similarity_dot_csr_*, csrc/dot_csr.hip), no GPU.

The rule: g = sum a_k b_k, A = sum a_k^2, B = sum b_k^2 in the graph precision dt (any order), then, fixed and in dt,
    cosine    den = sqrt(A) * sqrt(B)   s = clamp(g / den, -1, 1)
    tanimoto  den = (A + B) - g         s = g / den
    dice      den = A + B               s = (g + g) / den
    den == 0: s = 1 when A == 0 and B == 0, else 0;   symmetric mode: the diagonal is exactly 1.

ref_s64 evaluates the rule in fp64 on the inputs rounded to dt: what the device result is compared against inside a
band.  ref_exact evaluates it in dt with the three sums taken as exact integers: on integer-valued inputs the sums are
exact in any order, so the device result must equal it bit for bit.

band(dt, d) = 4 (d + 4) eps is derived, not measured: any-order summation of d products has error <= gamma_d *
sum|a_k b_k| <= gamma_d * sqrt(A B) with gamma_d ~ d eps / 2; through the three formulas that is at most 2 gamma_d
(cosine, Dice) and 6 gamma_d (Tanimoto, with den >= (A + B) / 2), and a few roundings of the epilogue come on top:
8 (d + 4) eps / 2 covers all three."""
import numpy as np

from test_gpu_jaccard_csr import (assert_csr_equal, clustered_features, features, ref_cut,  # noqa: F401  (re-exported)
                                  sample_rows, to_csr)

METRICS = ("cosine", "tanimoto", "dice")
ALPHAS = (0.3, 0.5, 0.7, 0.9)
# the case matrix of the GPU test: tile edges, BK edges, 33 tiles for the triangle enumeration, a long k loop
CASES = [(1, 1), (63, 4), (127, 15), (128, 16), (129, 17), (129, 1), (1000, 64), (300, 300), (4097, 16), (257, 1024)]
EXTRA_ALPHA_CASE = (4097, 16)      # alpha = 0.0 and -0.5 run on this case only
EXTRA_ALPHAS = (0.0, -0.5)


def band(dt, d):
    return 4.0 * (d + 4) * float(np.finfo(dt).eps)


def vectors(n, d, seed, signed, zero_rows=()):
    """The Jaccard test's features(); signed: 0.4 subtracted from half the entries.  Zero rows and the duplicated row
    are put back afterwards."""
    X = features(n, d, seed)
    if signed:
        X = X - 0.4 * (np.random.default_rng(seed + 1000).random(X.shape) < 0.5)
    if n > 3:
        X[n // 2] = X[n // 3]
    for z in zero_rows:
        if z < n:
            X[z] = 0
    return X


def case_inputs(n, d, signed):
    """(F, G) of one case of the matrix: the symmetric block is F x F, the cross block F x G with nb = n // 2 + 3."""
    F = vectors(n, d, seed=n * 7 + d, signed=signed, zero_rows=(0, n - 1, 5))
    G = vectors(max(1, n // 2 + 3), d, seed=n + d + 1, signed=signed, zero_rows=(1,))
    return F, G


def rule(g, a, b, metric, dt, sym=False):
    """Everything after the three sums, in dt.  g: (na, nb), a: (na,), b: (nb,)."""
    g, a, b = np.asarray(g, dt), np.asarray(a, dt)[:, None], np.asarray(b, dt)[None, :]
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        if metric == "cosine":
            den, num = np.sqrt(a) * np.sqrt(b), g
        elif metric == "tanimoto":
            den, num = (a + b) - g, g
        elif metric == "dice":
            den, num = a + b, g + g
        else:
            raise ValueError(metric)
        s = num / np.where(den == 0, dt(1), den)
        if metric == "cosine":
            s = np.where(s < dt(-1), dt(-1), np.where(s > dt(1), dt(1), s))      # a NaN stays a NaN
        s = np.where(den == 0, np.where((a == 0) & (b == 0), dt(1), dt(0)), s).astype(dt)
    if sym:
        np.fill_diagonal(s, dt(1))
    return s


def sums64(A, B, dt):
    A, B = np.asarray(A, dt).astype(np.float64), np.asarray(B, dt).astype(np.float64)
    return A @ B.T, (A * A).sum(axis=1), (B * B).sum(axis=1)


def ref_s64(A, B, metric, dt=np.float64, sym=False):
    """The rule in fp64 from the inputs rounded to dt."""
    return rule(*sums64(A, B, dt), metric, np.float64, sym)


def ref_exact(A, B, metric, dt, sym=False):
    """The rule in dt with g, A, B the exact integer sums (integer-valued inputs only)."""
    A, B = np.asarray(A), np.asarray(B)
    Ai, Bi = A.astype(np.int64), B.astype(np.int64)
    assert np.array_equal(Ai, A) and np.array_equal(Bi, B), "ref_exact needs integer-valued inputs"
    g, a, b = Ai @ Bi.T, (Ai * Ai).sum(axis=1), (Bi * Bi).sum(axis=1)
    lim = 2 ** (np.finfo(dt).nmant + 1)
    assert max(np.abs(g).max(initial=0), a.max(initial=0), b.max(initial=0)) * 2 <= lim, "sums not exact in dt"
    return rule(g, a, b, metric, dt, sym)


def in_band_share(s64, alpha, dt, d):
    with np.errstate(invalid="ignore"):
        return float((np.abs(s64 - float(dt(alpha))) <= band(dt, d)).mean())


def integer_rows(n, d, seed):
    """Integer features in -3 .. 3 with exact duplicates, a zero row and rows whose similarity is exactly 0.5:
    cosine (2,0,0,0,..) x (1,1,1,1,0,..), Tanimoto (1,1,0,..) x (1,0,..), Dice (1,1,0,..) x (1,0,1,0,..)."""
    rng = np.random.default_rng(seed)
    X = rng.integers(-3, 4, (n, d)).astype(np.float64)
    X[7] = 0
    for i, head in enumerate([(2, 0, 0, 0), (1, 1, 1, 1), (1, 1, 0, 0), (1, 0, 0, 0), (1, 0, 1, 0)]):
        X[10 + i] = 0
        X[10 + i, :4] = head
    X[n // 2] = X[n // 3]
    X[n - 1] = X[3]
    X[n - 2] = X[3]
    return X
