"""Host reference of the Butina clustering (include/simspread_hip_clusters.h): the sequential rule, nothing else.

    N(i)     = { j != i : (i,j) in P or (j,i) in P }, d_i = |N(i)|
    priority   i precedes j iff d_i > d_j, or d_i == d_j and i < j
    visit the sources in priority order; an unassigned source becomes a centre and takes its still-unassigned neighbours

on a dense boolean matrix, plus the largest-first fold rule and the cross-fold edge count, and the graphs the CPU and GPU
tests share.  Everything is integers, so every comparison with the device is exact."""
import functools

import numpy as np
import scipy.sparse as sp


def neighbours(P):
    """The symmetric, diagonal-free boolean neighbour matrix of a pattern (dense bool or scipy.sparse)."""
    A = (P.toarray() if sp.issparse(P) else np.asarray(P)) != 0
    A = A | A.T
    np.fill_diagonal(A, False)
    return A


def order(A):
    """The sources in priority order: degree descending, index ascending."""
    deg = A.sum(axis=1)
    return np.lexsort((np.arange(len(deg)), -deg))


def ref_butina(P):
    """(centre, label, size) of the sequential rule."""
    A = neighbours(P)
    n = A.shape[0]
    centre = np.full(n, -1, np.int32)
    label = np.full(n, -1, np.int32)
    size = []
    for i in order(A):
        if centre[i] >= 0:
            continue
        take = A[i] & (centre < 0)
        take[i] = True
        centre[take] = i
        label[take] = len(size)
        size.append(int(take.sum()))
    return centre, label, np.array(size, np.int32)


def ref_folds(label, nfolds):
    """Clusters by size descending (ties: label ascending), each to the fold with the fewest sources so far (ties: the
    lowest fold id)."""
    label = np.asarray(label)
    size = np.bincount(label) if label.size else np.zeros(0, np.int64)
    load = np.zeros(nfolds, np.int64)
    fold_of_cluster = np.zeros(len(size), np.int32)
    for c in np.lexsort((np.arange(len(size)), -size)):
        f = int(np.argmin(load))                     # the first minimum: the lowest fold id
        fold_of_cluster[c] = f
        load[f] += size[c]
    return fold_of_cluster[label].astype(np.int32)


def ref_cross_edges(ptr, idx, fold, nfolds, index_base=0):
    """count[f] = stored off-diagonal entries (i, j) with fold[i] == f != fold[j]; the pattern as given."""
    ptr, idx, fold = np.asarray(ptr, np.int64) - index_base, np.asarray(idx, np.int64) - index_base, np.asarray(fold)
    rows = np.repeat(np.arange(len(ptr) - 1), np.diff(ptr))
    cols = idx[:ptr[-1]]
    leak = (rows != cols) & (fold[rows] != fold[cols])
    return np.bincount(fold[rows][leak], minlength=nfolds).astype(np.int64)


# ------------------------------------------------------------------------------------------------ the graphs
def random_symmetric(n, p, seed):
    rng = np.random.default_rng(seed)
    A = np.triu(rng.random((n, n)) < p, 1)
    return A | A.T


def hub(n=600, p=0.004, seed=5):
    """Sparse random rows plus row 17 adjacent to all: one row far above a wave's width next to short ones."""
    A = random_symmetric(n, p, seed)
    A[17, :] = A[:, 17] = True
    A[17, 17] = False
    return A


def directed_knn(n=257, k=5, seed=9):
    """(i, j) stored for the k nearest j of i among random points: not symmetric."""
    rng = np.random.default_rng(seed)
    X = rng.random((n, 3))
    d = ((X[:, None, :] - X[None, :, :]) ** 2).sum(axis=2)
    np.fill_diagonal(d, np.inf)
    A = np.zeros((n, n), bool)
    A[np.arange(n)[:, None], np.argsort(d, axis=1)[:, :k]] = True
    return A


def path(n=300):
    A = np.zeros((n, n), bool)
    i = np.arange(n - 1)
    A[i, i + 1] = A[i + 1, i] = True
    return A


def ring_lattice(n=300, k=2):
    A = np.zeros((n, n), bool)
    i = np.arange(n)
    for s in range(1, k + 1):
        A[i, (i + s) % n] = A[(i + s) % n, i] = True
    return A


def complete(n=70):
    return ~np.eye(n, dtype=bool)


def empty(n=65):
    return np.zeros((n, n), bool)


@functools.lru_cache(maxsize=None)
def graphs():
    """name -> dense boolean pattern (read-only), the cases of the issue's table."""
    g = {f"random_p{p}": random_symmetric(257, p, seed=int(p * 1000)) for p in (0.01, 0.05, 0.3)}
    g.update(hub=hub(), directed_knn=directed_knn(), path=path(), ring_lattice=ring_lattice(), k70=complete(),
             empty65=empty(), one=np.zeros((1, 1), bool))
    for a in g.values():
        a.setflags(write=False)
    return g


@functools.lru_cache(maxsize=None)
def reference(name):
    """ref_butina of graphs()[name], computed once; read-only."""
    out = ref_butina(graphs()[name])
    for a in out:
        a.setflags(write=False)
    return out


def csr_parts(A, index_base=0, noise_seed=None):
    """(ptr int64, idx int32) of a dense boolean pattern.  noise_seed: every row also gets its diagonal entry and a
    duplicate of each of its first two entries, and the row is shuffled (unsorted, duplicates, diagonal)."""
    n = A.shape[0]
    rng = None if noise_seed is None else np.random.default_rng(noise_seed)
    rows = []
    for i in range(n):
        r = np.nonzero(A[i])[0]
        if rng is not None:
            r = np.concatenate([r, [i], r[:2]])
            rng.shuffle(r)
        rows.append(r)
    ptr = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int64) + index_base
    idx = (np.concatenate(rows) if rows else np.zeros(0)).astype(np.int32) + index_base
    return ptr, idx


def check_properties(A, centre, label, size):
    """What the rule promises, on the symmetric neighbour matrix A."""
    n = A.shape[0]
    deg = A.sum(axis=1)
    key = (deg.astype(np.int64) << 32) | (0xFFFFFFFF - np.arange(n, dtype=np.int64))
    centres = np.nonzero(centre == np.arange(n))[0]
    assert not A[np.ix_(centres, centres)].any()                          # centres are pairwise non-adjacent
    assert np.isin(centre, centres).all()
    members = np.nonzero(centre != np.arange(n))[0]
    assert A[members, centre[members]].all()                              # every member is adjacent to its centre
    is_centre = np.zeros(n, bool)
    is_centre[centres] = True
    for i in members:                                                     # and to no earlier-priority centre
        nb = np.nonzero(A[i] & is_centre)[0]
        assert key[centre[i]] == key[nb].max()
    # labels number the clusters in priority order of their centres
    assert np.array_equal(label[centres[np.argsort(-key[centres])]], np.arange(len(centres)))
    assert np.array_equal(label, label[centre])
    assert np.array_equal(size, np.bincount(label, minlength=len(centres))) and size.sum() == n
