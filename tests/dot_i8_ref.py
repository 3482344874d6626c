"""Host reference and inputs of the int8 route of the inner-product producer (include/simspread_hip_int8.h), no GPU.

The rule: g, A, B are exact integers (computed here in fp64 matrix products, exact below 2^53, and held as int64); each is
converted to float32 once, round to nearest even (numpy's int64 -> float32 conversion), and dot_ref.rule does the rest in
float32.  Every comparison against the device is bitwise.  Keep rule and floor: neighbour_ref (ref_cut, ref_floor,
ref_kth), as restated by real_floor_ref."""
import functools

import numpy as np

import dot_ref as R

F32 = np.float32


def sums(A, B):
    """(g, a, b) as exact int64 arrays."""
    A, B = np.asarray(A), np.asarray(B)
    assert A.dtype == np.int8 and B.dtype == np.int8
    Af, Bf = A.astype(np.float64), B.astype(np.float64)
    g = (Af @ Bf.T).astype(np.int64)                      # |g| <= d 2^14 < 2^53: exact
    return g, (Af * Af).sum(axis=1).astype(np.int64), (Bf * Bf).sum(axis=1).astype(np.int64)


def ref_s(A, B, metric, sm=None):
    """Dense float32 similarity of the int8 rows of A against those of B (None: A against itself, diagonal exactly 1)."""
    g, a, b = sm if sm is not None else sums(A, A if B is None else B)
    return np.ascontiguousarray(R.rule(g, a, b, metric, F32, sym=B is None), dtype=F32)


def rows(n, d, seed, big=False):
    """Full-range int8 rows (-128 .. 127, both ends present) drawn around prototypes with row-dependent noise, so that
    every alpha keeps some pairs and drops others at any d; a zero row (7), exact duplicates, and, from d = 4 on, the
    rows of dot_ref.integer_rows whose similarity is exactly 0.5.  big: four rows of large magnitude, whose sums pass
    2^24 from d = 1025 on, so that the integer-to-float conversion rounds."""
    rng = np.random.default_rng(seed)
    kp = max(1, n // 16)
    proto = rng.integers(-128, 128, (kp, d))
    noise = rng.integers(-128, 128, (n, d)) * rng.uniform(0.0, 0.9, (n, 1))
    X = np.clip(np.rint(proto[rng.integers(0, kp, n)] * rng.uniform(0.3, 1.0, (n, 1)) + noise), -128, 127)
    X = X.astype(np.int8)
    X[0, 0], X[1, 0] = -128, 127
    if n > 20:
        X[7] = 0
        if d >= 4:
            for i, head in enumerate([(2, 0, 0, 0), (1, 1, 1, 1), (1, 1, 0, 0), (1, 0, 0, 0), (1, 0, 1, 0)]):
                X[10 + i] = 0
                X[10 + i, :4] = head
        if big:
            X[20:24] = rng.choice(np.array([-128, -127, 127, 125]), (4, d), p=[0.1, 0.1, 0.4, 0.4])
        X[n // 2] = X[n // 3]
        X[n - 1] = X[3]
        X[n - 2] = X[3]
    return X


@functools.lru_cache(maxsize=4)
def case_inputs(n, d):
    """(F, G) of one case: the symmetric block is F x F, the cross block F x G with nb = n // 2 + 3."""
    F = rows(n, d, seed=n * 7 + d, big=d > 1024)
    G = rows(n // 2 + 3, d, seed=n + d + 1, big=d > 1024)
    rng = np.random.default_rng(n + 3 * d)
    m = G.shape[0] // 2                                     # half of G: noisy copies of rows of F, so that the cross
    src = F[rng.integers(0, n, m)].astype(np.float64)       # block has pairs on both sides of every alpha
    G[30:30 + m] = np.clip(np.rint(src + rng.integers(-128, 128, (m, d)) * rng.uniform(0.0, 0.8, (m, 1))), -128, 127)
    if d > 1024:                                            # Gram values past 2^24 off the diagonal, both blocks
        for j in range(4):                                  # near copies: sums of either parity past 2^24, where
            F[24 + j] = F[20]                               # float32 holds even integers only
            F[24 + j, :5 + j] = 1
        G[24:32] = F[20:28]
    F.setflags(write=False)
    G.setflags(write=False)
    return F, G


@functools.lru_cache(maxsize=4)
def floor_inputs(n, d):
    """(F, G, Q) of the floor cases: F the symmetric set, Q x G the cross block (G: n // 2 + 3 rows).  F and G start
    with two blocks of c identical rows each, u and a noisy copy w of u (c = 33 below 100 rows, else 40): a row that is
    close to u has c columns tied at its ranks 1 .. c and c more at c + 1 .. 2 c, so that k = 1, 5, 33 and 64 all fall on
    a tie.  F ends with a zero row (its only positive is the diagonal); Q holds noisy copies of u and w, rows of its own
    and a zero row, which has no positive against G (G has no zero row)."""
    rng = np.random.default_rng(n * 31 + d)

    def noisy(v, amp, m):
        return np.clip(v[None, :] + np.rint(rng.integers(-128, 128, (m, d)) * amp), -128, 127).astype(np.int8)
    u = rng.integers(-100, 101, d).astype(np.int8)
    w = noisy(u, 0.5, 1)[0]

    def side(m, zero):
        c = 33 if m < 100 else 40
        X = rows(m, d, seed=int(rng.integers(1 << 30)))
        X[:c] = u
        X[c:2 * c] = w
        X[2 * c:2 * c + 20] = noisy(u, 0.3, 20)[:max(0, min(20, m - 2 * c))]
        near = (X[2 * c:].astype(np.int64) != 0).any(axis=1)
        X[2 * c:][~near] = 1                                # no zero row but the one asked for
        if zero:
            X[m - 1] = 0
        return X
    F, G = side(n, True), side(n // 2 + 3, False)
    Q = rows(n, d, seed=int(rng.integers(1 << 30)))
    Q[(Q.astype(np.int64) != 0).sum(axis=1) == 0] = 1
    Q[:40] = noisy(u, 0.3, 40)
    Q[40:60] = noisy(w, 0.3, 20)
    Q[3] = 0
    for X in (F, G, Q):
        X.setflags(write=False)
    return F, G, Q
