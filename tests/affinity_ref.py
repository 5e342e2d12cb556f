"""NumPy restatement in fp64 of sklearn.cluster.AffinityPropagation(damping, max_iter, convergence_iter, preference).fit(X) as
scikit-learn 1.7.2 executes it (sklearn/cluster/_affinity_propagation.py), on an input of fp64: what hsefr_affinity_fit and
hsefr_affinity_fit_dense (include/hsefr_affinity.h) answer.

The statements of the loop are scikit-learn's own, with its temporaries; what differs is the noise -- none, or the header's counter hash
in place of the unseeded generator -- and the history of the exemplar decisions, kept as the last ``convergence_iter`` columns.

Besides the result the restatement reports the margins by which a test proves that a case is decidable in another arithmetic:
    diag     the least |A_kk + R_kk| over all iterations and points (the exemplar decisions and with them n_iter)
    assign   the least gap between a non-exemplar's best and second-best exemplar similarity, in both assignments (inf with one exemplar)
    refine   per cluster, the gap between the best and the second-best member sum of the refinement (inf for a cluster of one)"""
from collections import namedtuple

import numpy as np

Result = namedtuple("Result", "exemplars labels n_iter converged equal preference diag margins member_sums first_labels")
Margins = namedtuple("Margins", "diag assign refine")

MASK = (1 << 64) - 1
SEED_MUL, GAMMA, MUL1, MUL2 = 0xD1342543DE82EF95, 0x9E3779B97F4A7C15, 0xBF58476D1CE4E5B9, 0x94D049BB133111EB
SQRT3 = 1.7320508075688772


def noise_factor(seed, n):
    """the header's g(seed, i, j) for the whole matrix: [n, n] float64, uniform on (-sqrt 3, sqrt 3)"""
    with np.errstate(over="ignore"):
        z = np.arange(n * n, dtype=np.uint64) + np.uint64((seed * SEED_MUL + GAMMA) & MASK)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(MUL1)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(MUL2)
        z = z ^ (z >> np.uint64(31))
    u = ((z >> np.uint64(12)).astype(np.float64) + 0.5) * 2.0 ** -52
    return ((u * 2.0 - 1.0) * SQRT3).reshape(n, n)


def similarities(X):
    """-|x_i - x_j|^2 of the fp32 rows widened to fp64, from the differences themselves (no cancellation), zeros on the diagonal"""
    X32 = np.asarray(X)
    assert X32.dtype == np.float32 and X32.ndim == 2
    X = X32.astype(np.float64)
    S = np.empty((len(X), len(X)))
    for i in range(len(X)):
        diff = X - X[i]
        S[i] = -np.einsum("ij,ij->i", diff, diff)
    S = np.minimum(S, S.T)                                            # (equal already: the same differences with the other sign)
    np.fill_diagonal(S, 0.0)
    return S + 0.0


def first_occurrence(labels):
    """labels renumbered in order of first occurrence: equal for equal partitions"""
    labels = np.asarray(labels)
    _, first, inverse = np.unique(labels, return_index=True, return_inverse=True)
    rank = np.empty(len(first), np.int64)
    rank[np.argsort(first)] = np.arange(len(first))
    return rank[inverse]


def _assign(S, I):
    sub = S[:, I]
    c = np.argmax(sub, axis=1)
    gap = np.inf
    if len(I) > 1:
        two = np.sort(sub, axis=1)[:, -2:]
        rest = np.ones(len(S), bool)
        rest[I] = False
        if rest.any():
            gap = float((two[rest, 1] - two[rest, 0]).min())
    c[I] = np.arange(len(I))
    return c, gap


def affinity_propagation(S, damping=0.5, max_iter=200, convergence_iter=15, preference=None, seed=None, perturb=None):
    """``S`` [n, n] float64 similarities (not written).  ``seed``: None for no noise, else the header's hash noise with that seed.
    ``perturb``: a relative perturbation of every entry (S * (1 + perturb * N(0, 1)), symmetric, generator 12345): the decidability probe."""
    S = np.array(S, dtype=np.float64)
    n = S.shape[0]
    assert S.shape == (n, n) and n >= 1
    if perturb:
        P = np.random.RandomState(12345).standard_normal((n, n))
        S = S * (1.0 + perturb * np.triu(P, 1) + perturb * np.triu(P, 1).T)
    pref = float(np.median(S)) if preference is None else float(preference)
    off = S[~np.eye(n, dtype=bool)]
    if n == 1 or off.min() == off.max():                              # _equal_similarities_and_preferences
        if pref > S.flat[n - 1]:
            ex, lab = np.arange(n), np.arange(n)
        else:
            ex, lab = np.array([0]), np.zeros(n, np.int64)
        return Result(ex.astype(np.int64), lab.astype(np.int64), 0, True, True, pref, np.zeros(n), Margins(np.inf, np.inf, np.zeros(0)), [], lab)
    S.flat[::n + 1] = pref
    if seed is not None:
        S += (np.finfo(np.float64).eps * S + np.finfo(np.float64).tiny * 100) * noise_factor(seed, n)
    A = np.zeros((n, n))
    R = np.zeros((n, n))
    tmp = np.zeros((n, n))
    e = np.zeros((n, convergence_iter))
    ind = np.arange(n)
    m_diag = np.inf
    converged = False
    it = -1
    E = np.zeros(n, bool)
    diag = np.zeros(n)
    for it in range(max_iter):
        np.add(A, S, tmp)
        I = np.argmax(tmp, axis=1)
        Y = tmp[ind, I]
        tmp[ind, I] = -np.inf
        Y2 = np.max(tmp, axis=1)
        np.subtract(S, Y[:, None], tmp)
        tmp[ind, I] = S[ind, I] - Y2
        tmp *= 1 - damping
        R *= damping
        R += tmp
        np.maximum(R, 0, tmp)
        tmp.flat[::n + 1] = R.flat[::n + 1]
        tmp -= np.sum(tmp, axis=0)
        dA = np.diag(tmp).copy()
        tmp.clip(0, np.inf, tmp)
        tmp.flat[::n + 1] = dA
        tmp *= 1 - damping
        A *= damping
        A -= tmp
        diag = np.diag(A) + np.diag(R)
        m_diag = min(m_diag, float(np.abs(diag).min()))
        E = diag > 0
        e[:, it % convergence_iter] = E
        K = np.sum(E, axis=0)
        if it >= convergence_iter:
            se = np.sum(e, axis=1)
            unconverged = np.sum((se == convergence_iter) + (se == 0)) != n
            if not unconverged and K > 0:
                converged = True
                break
    I = np.flatnonzero(E)
    K = I.size
    if K == 0:
        return Result(np.zeros(0, np.int64), np.full(n, -1, np.int64), it + 1, converged, False, pref, diag.copy(),
                      Margins(m_diag, np.inf, np.zeros(0)), [], np.full(n, -1, np.int64))
    c, gap1 = _assign(S, I)
    first_labels = c.copy()
    refine = np.full(K, np.inf)
    sums = []
    for k in range(K):
        ii = np.flatnonzero(c == k)
        s = np.sum(S[ii[:, np.newaxis], ii], axis=0)
        sums.append((ii, s))
        if len(ii) > 1:
            top = np.sort(s)[-2:]
            refine[k] = top[1] - top[0]
        I[k] = ii[np.argmax(s)]
    c, gap2 = _assign(S, I)
    labels = I[c]
    exemplars = np.unique(labels)
    labels = np.searchsorted(exemplars, labels)
    return Result(exemplars.astype(np.int64), labels.astype(np.int64), it + 1, converged, False, pref, diag.copy(),
                  Margins(m_diag, min(gap1, gap2), refine), sums, first_labels)


def fit_features(X, **kw):
    return affinity_propagation(similarities(X), **kw)


def nearest_center(Q, C):
    """the nearest row of C for every row of Q in fp64, the lowest index on an exact tie"""
    Q = np.asarray(Q, np.float32).astype(np.float64)
    C = np.asarray(C, np.float64)
    D = np.empty((len(Q), len(C)))
    for i in range(len(Q)):
        diff = C - Q[i]
        D[i] = np.einsum("ij,ij->i", diff, diff)
    return D.argmin(axis=1).astype(np.int64), D


def cluster_lists(labels):
    """the reference's result form: the members of every label >= 0, the largest cluster first (stable)"""
    labels = np.asarray(labels)
    groups = [np.flatnonzero(labels == c) for c in range(int(labels.max()) + 1 if len(labels) else 0)]
    groups = [g for g in groups if len(g)]
    groups.sort(key=len, reverse=True)
    return [[int(i) for i in g] for g in groups]
