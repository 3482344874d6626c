"""Host reference for the per-target ranking metrics (ss_target_rank_*).

ref_targets: the definition -- rank_ref.ref_row of every column of the whole matrix, rows in row-id order.

RefTargetRank: the counts-based two-pass algorithm of include/simspread_hip_target_rank.h in numpy, with the header's
export layout (sealed positives; hist | nz | kmin | kmax), so that a device handle's exports can be compared entry by
entry, and with the metrics written from the issue's formulas (per distinct positive score: counts of positives and
negatives above and at it), not from the device's integer form."""
import numpy as np

from rank_ref import ref_row


def ref_targets(Y, S, alpha=20.0, L=20):
    """Y: dense 0/1 (n, nt), S: scores (n, nt), rows in row-id order -> (nt, 6)."""
    Y, S = np.asarray(Y), np.asarray(S)
    return np.stack([ref_row(Y[:, t], S[:, t], alpha, L) for t in range(S.shape[1])])


def score_keys(v):
    """Order-preserving uint64 keys of fp32 / fp64 scores compared by value (-0.0 as +0.0), as the device builds them."""
    v = np.ascontiguousarray(v)
    v = np.where(v == 0, np.zeros((), v.dtype), v)
    if v.dtype == np.float32:
        u = v.view(np.uint32)
        k = np.where(u >> np.uint32(31), ~u, u | np.uint32(1 << 31))
    else:
        u = v.view(np.uint64)
        k = np.where(u >> np.uint64(63), ~u, u | np.uint64(1 << 63))
    return k.astype(np.uint64)


class RefTargetRank:
    def __init__(self, nt, dtype=np.float64):
        self.nt, self.dtype = int(nt), np.dtype(dtype)
        self.phase = 0
        self.rows = self.rows_counted = 0
        self.t, self.r, self.v = [], [], []

    # ---- collect
    def add_rows(self, Y, S, row_begin=0):
        Y = np.asarray(Y) != 0
        S = np.asarray(S, self.dtype)
        assert not np.isnan(S).any()
        ids = row_begin + np.arange(S.shape[0], dtype=np.int64)
        return self._count(Y, S, ids) if self.phase else self._collect(Y, S, ids)

    def _collect(self, Y, S, ids):
        rr, tt = np.nonzero(Y)                      # row-major: the block's label order
        self.t.append(tt.astype(np.int32))
        self.r.append(ids[rr])
        self.v.append(S[rr, tt])
        self.rows += S.shape[0]
        return self

    def seal(self):
        assert self.phase == 0
        t = np.concatenate(self.t) if self.t else np.zeros(0, np.int32)
        r = np.concatenate(self.r) if self.r else np.zeros(0, np.int64)
        v = np.concatenate(self.v) if self.v else np.zeros(0, self.dtype)
        k = score_keys(v)
        order = np.lexsort((r, ~k, t))              # target, score descending, row ascending
        self.st, self.sr, self.sv, self.sk = t[order], r[order], v[order], k[order]
        self.off = np.searchsorted(self.st, np.arange(self.nt + 1)).astype(np.int64)
        P = self.st.size
        self.hist = np.zeros(3 * (P + self.nt), np.int64)
        self.nz = np.zeros(self.nt, np.int64)
        self.kmin = np.full(self.nt, np.iinfo(np.uint64).max, np.uint64)
        self.kmax = np.zeros(self.nt, np.uint64)
        self.phase = 1
        return self

    def _views(self, t):
        o, P = int(self.off[t]), int(self.off[t + 1] - self.off[t])
        b = 3 * (o + t)
        return o, P, self.hist[b:b + P + 1], self.hist[b + P + 1:b + 2 * (P + 1)], self.hist[b + 2 * (P + 1):b + 3 * (P + 1)]

    # ---- count
    def _count(self, Y, S, ids):
        K = score_keys(S)
        for t in range(self.nt):
            o, P, gap, tieG, tieK = self._views(t)
            col = K[:, t]
            if col.size:
                self.nz[t] += int(np.count_nonzero(S[:, t]))
                self.kmin[t] = min(self.kmin[t], col.min())
                self.kmax[t] = max(self.kmax[t], col.max())
            pk, pr = self.sk[o:o + P], self.sr[o:o + P]
            pos = Y[:, t]
            for i in np.flatnonzero(pos):           # the second pass must be the first
                hit = np.flatnonzero((pr == ids[i]) & (self.sv[o:o + P].view(f"u{self.dtype.itemsize}")
                                                       == S[i:i + 1, t].view(f"u{self.dtype.itemsize}")))
                assert hit.size == 1, f"row {ids[i]}, target {t}: not the collected positive"
            asc = pk[::-1]
            for i in np.flatnonzero(~pos):
                k = col[i]
                j = P - int(np.searchsorted(asc, k, side="right"))       # positives scoring higher
                e = P - int(np.searchsorted(asc, k, side="left"))        # ... or equal
                if e > j:
                    tieG[j] += 1
                    tieK[j + int(np.searchsorted(pr[j:e], ids[i], side="left"))] += 1
                else:
                    gap[j] += 1
        self.rows_counted += S.shape[0]
        return self

    # ---- exports, in the device's format
    def export_positives(self):
        return self.st, self.sr, self.sv, self.rows

    def export_counts(self):
        return np.concatenate([self.hist, self.nz, self.kmin.view(np.int64), self.kmax.view(np.int64)]), self.rows_counted

    # ---- metrics
    def metrics(self, alpha=20.0, L=20):
        assert self.phase == 1 and self.rows_counted == self.rows and 1 <= L < self.rows
        return np.stack([self._target(t, alpha, L) for t in range(self.nt)])

    def _target(self, t, alpha, L):
        n = self.rows
        o, P, gap, tieG, tieK = self._views(t)
        N = n - P
        distinct = self.kmin[t] != self.kmax[t]
        pk = self.sk[o:o + P]
        starts = np.flatnonzero(np.r_[True, pk[1:] != pk[:-1]]) if P else np.zeros(0, np.int64)   # first of every group
        ends = np.r_[starts[1:], P] if P else starts
        cgap, ctie = np.cumsum(gap), np.cumsum(tieG)
        with np.errstate(invalid="ignore", divide="ignore"):
            auroc = auprc = 0.0
            prev_Nge = prev_Pge = 0
            for g, (a, e) in enumerate(zip(starts, ends)):
                Pgt, Pge = int(a), int(e)
                Ngt = int(cgap[a]) + (int(ctie[a - 1]) if a else 0)
                Nge = Ngt + int(tieG[a])
                if g > 0:
                    auroc += np.float64(Ngt - prev_Nge) / N * (np.float64(prev_Pge) / P)
                if Pgt + Ngt > 0:
                    auroc += np.float64(Nge - Ngt) / N * (np.float64(Pge + Pgt) / (2.0 * P))
                    auprc += (np.float64(Pge - Pgt) / P) * (np.float64(Pge) / (Pge + Nge)
                                                          + np.float64(Pgt) / (Pgt + Ngt)) / 2.0
                prev_Nge, prev_Pge = Nge, Pge
            auroc = abs(auroc + np.float64(N - prev_Nge) / N)
            auprc = abs(auprc)
            if P == 0 or N == 0:                     # a class is missing
                auroc = np.nan if distinct else 0.0
            if P == 0:
                auprc = np.nan if distinct else 0.0
            rank = np.cumsum(gap[:P] + tieK[:P] + 1).astype(np.float64)   # 1-based sortperm ranks of the positives
            Ra = P / n
            rand_sum = Ra * (1 - np.exp(-alpha)) / (np.exp(alpha / n) - 1)
            fac = Ra * np.sinh(alpha / 2) / (np.cosh(alpha / 2) - np.cosh(alpha / 2 - alpha * Ra))
            cte = 1 / (1 - np.exp(alpha * (1 - Ra)))
            bedroc = float(np.sum(np.exp(-alpha * rank / n)) * fac / rand_sum + cte)
        hits = int(np.count_nonzero(rank <= L))
        return np.array([auroc, auprc, bedroc, self.nz[t] / n, hits / P if P else np.nan, hits / L])


def _cases(n, L, rng):
    """The edge-case vectors of the per-row tests (tests/test_gpu_rank_rows.py:_cases), n entries each."""
    ys, ss = [], []

    def add(y, s):
        ys.append(np.asarray(y, np.uint8))
        ss.append(np.asarray(s, np.float64))

    cont = rng.random(n)
    few = rng.choice(np.array([0.0, 0.25, 0.5, 1.0]), n)
    add(np.zeros(n), cont)                                       # P = 0, many scores
    add(np.zeros(n), np.full(n, 0.5))                            # P = 0, one score
    y1 = np.zeros(n); y1[rng.integers(n)] = 1
    add(y1, cont)                                                # P = 1
    add(np.ones(n), cont)                                        # P = n
    add(np.ones(n), few)                                         # P = n, ties
    y = (rng.random(n) < 0.3).astype(np.uint8); y[0] = 1
    add(y, np.zeros(n))                                          # all zero
    add(y, np.full(n, -99.0))                                    # all -99 (clean!)
    add(y, few)                                                  # heavy ties
    m = few.copy(); m[rng.random(n) < 0.3] = -99.0
    add(y, m)                                                    # ties and -99
    # a tie group straddling rank L: L - 1 top scores, then a group of 3 holding positives and negatives
    s = np.full(n, 0.1); s[:max(L - 1, 0)] = 2.0 + np.arange(max(L - 1, 0))
    grp = np.arange(max(L - 1, 0), min(L + 2, n)); s[grp] = 1.0
    yt = np.zeros(n); yt[grp[-1]] = 1; yt[-1] = 1
    add(yt, s)
    yf = np.zeros(n); yf[0] = 1; yf[-1] = 1
    add(yf, cont)                                                # positives in the first and the last row
    add(yf, few)
    for _ in range(4):                                           # random densities, half the scores zero
        yr = (rng.random(n) < rng.random()).astype(np.uint8)
        add(yr, np.where(rng.random(n) < 0.5, 0.0, rng.random(n)))
    return ys, ss


def case_matrix(n, nt=40, L=5, dtype=np.float64, seed=0):
    """(Y, S): n rows and nt target columns, every column one of the vectors of _cases (drawn anew for every batch of 16
    columns); the last column holds signed zeros, which tie."""
    rng = np.random.default_rng(1000 + n + 7919 * seed)
    ys, ss = [], []
    while len(ys) < nt:
        y, s = _cases(n, L, rng)
        ys += y
        ss += s
    Y, S = np.stack(ys[:nt], axis=1), np.stack(ss[:nt], axis=1)
    S[:, nt - 1] = np.where(rng.random(n) < 0.5, -0.0, 0.0)
    S[rng.integers(n), nt - 1] = 0.5
    Y[:, nt - 1] = rng.random(n) < 0.4
    return np.ascontiguousarray(Y), np.ascontiguousarray(S.astype(dtype))
