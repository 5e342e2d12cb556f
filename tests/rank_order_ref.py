"""The rank-order clustering rule of csrc/rank_order.hip (the reference's find_clusters, facial_clustering_test.py:23-239, behind
get_facial_clusters' rank-order branch) restated on matrices in NumPy, vectorised so that it runs at a few thousand faces.

No Python objects: clusters are kept in the order of their smallest face, C is the cluster distance matrix (minimum over face pairs),
every cluster lists its first NB clusters by (C, order), and an iteration joins a with each listed b whose normalised distance and
symmetric rank order are under the thresholds; the new clusters are the connected components."""
import numpy as np
from scipy.sparse import coo_matrix
from scipy.sparse.csgraph import connected_components

NB, KN = 20, 12


def symmetrised(D):
    """What the device reads: the upper triangle on both sides and a zero diagonal."""
    U = np.triu(np.asarray(D, dtype=np.float64), 1)
    return U + U.T


def first_by_value_then_index(C, k):
    """Per row the first k columns by (C[row, col], col) -> (indices [m, k], values [m, k])."""
    m = C.shape[1]
    if k >= m:
        idx = np.argsort(C, axis=1, kind="stable")
        return idx, np.take_along_axis(C, idx, 1)
    kth = np.partition(C, k - 1, axis=1)[:, k - 1]
    r, c = np.nonzero(C <= kth[:, None])                       # every row keeps at least k columns
    v = C[r, c]
    order = np.lexsort((c, v, r))
    r, c = r[order], c[order]
    start = np.searchsorted(r, np.arange(C.shape[0]))
    take = (start[:, None] + np.arange(k)[None, :]).reshape(-1)
    idx = c[take].reshape(C.shape[0], k)
    return idx, np.take_along_axis(C, idx, 1)


def _asym(pos):
    """pos [.., L]: the position of each entry of one list in the other (-1: absent) -> (penalty, entries walked)."""
    L = pos.shape[-1]
    zero = pos == 0
    stop = np.where(zero.any(-1), zero.argmax(-1), L)
    before = np.arange(L) < stop[..., None]
    pen = np.where(before & (pos > 0), pos, 0).sum(-1)
    return pen, np.where(zero.any(-1), stop + 1, L)


def rank_order(D, norm_threshold=0.9, rank_threshold=14, chunk=512):
    """-> (clusters, iterations, margin): the clusters of at least two faces as sorted lists, longest first and equal lengths by
    smallest face; the iterations run; the smallest |nd - norm_threshold| / norm_threshold over every pair tested (inf if none)."""
    D = symmetrised(D)
    n = D.shape[0]
    _, fdist = first_by_value_then_index(D, min(NB, n))
    k = min(KN, fdist.shape[1])
    S = np.zeros(n)
    for j in range(k):                                         # added in list order
        S = S + fdist[:, j]
    lab = np.arange(n)
    C = D
    margin = np.inf
    iters = 0
    while True:
        iters += 1
        m = C.shape[0]
        L = min(NB, m)
        cidx, cval = first_by_value_then_index(C, L)
        T = np.bincount(lab, weights=S, minlength=m)
        cnt = np.bincount(lab, minlength=m)
        a_of = np.repeat(np.arange(m), L).reshape(m, L)
        other = cidx != a_of
        with np.errstate(divide="ignore", invalid="ignore"):
            mean = (T[a_of] + T[cidx]) / k / (cnt[a_of] + cnt[cidx])
            nd = np.where(mean != 0, (1 / mean) * cval, 0.0)
        if other.any():
            margin = min(margin, float((np.abs(nd[other] - norm_threshold) / norm_threshold).min()))
        ok = other & ~(nd >= norm_threshold)
        ro = np.zeros((m, L))
        for a0 in range(0, m, chunk):
            la = cidx[a0:a0 + chunk]                            # [c, L]    a's list
            lb = cidx[la]                                       # [c, L, L] the list of each listed b
            eq = lb[:, :, None, :] == la[:, None, :, None]      # [c, e, i, j]: a's entry i is b's entry j
            pos_ab = np.where(eq.any(3), eq.argmax(3), -1)
            pos_ba = np.where(eq.any(2), eq.argmax(2), -1)
            pab, nab = _asym(pos_ab)
            pba, nba = _asym(pos_ba)
            ro[a0:a0 + chunk] = (pab + pba) / np.minimum(nab, nba)
        ok &= ~(ro >= rank_threshold)
        ea, eb = a_of[ok], cidx[ok]
        _, comp = connected_components(coo_matrix((np.ones(len(ea)), (ea, eb)), shape=(m, m)), directed=False)
        _, first = np.unique(comp, return_index=True)
        new = np.argsort(np.argsort(first))[comp]               # components numbered by their smallest cluster
        m2 = int(new.max()) + 1
        if m2 == m:
            break
        lab = new[lab]
        order = np.argsort(new, kind="stable")
        starts = np.searchsorted(new[order], np.arange(m2))
        R = np.minimum.reduceat(C[order], starts, axis=0)
        C = np.minimum.reduceat(R[:, order], starts, axis=1)
        np.fill_diagonal(C, 0.0)
    return clusters_of(lab), iters, margin


def clusters_of(lab):
    """Face labels -> clusters of at least two faces, longest first, equal lengths by smallest face."""
    lab = np.asarray(lab)
    order = np.argsort(lab, kind="stable")
    groups = np.split(order, np.flatnonzero(np.diff(lab[order])) + 1)
    out = [g.tolist() for g in groups if len(g) > 1]
    out.sort(key=lambda c: (-len(c), c[0]))
    return out


def integer_case(n, classes, seed, dim=32, noise=2, duplicates=3):
    """The fixture's faces: integer class centres in [-6, 6]^dim plus uniform integer noise in [-noise, noise], a few rows duplicated ->
    (X float64 [n, dim] of integers, D = sqrt of the exact integer squared distances)."""
    rs = np.random.RandomState(seed)
    centres = rs.randint(-6, 7, (classes, dim))
    X = centres[rs.randint(0, classes, n)] + rs.randint(-noise, noise + 1, (n, dim))
    for _ in range(min(duplicates, n // 4)):
        X[rs.randint(0, n)] = X[rs.randint(0, n)]
    X = X.astype(np.float64)
    return X, integer_distances(X)


def integer_distances(X):
    sq = (X * X).sum(1)
    K = sq[:, None] + sq[None, :] - 2 * X @ X.T                 # exact: small integers
    np.fill_diagonal(K, 0)
    return np.sqrt(K)


def coincident_case(n, seed, blocks=(15, 13)):
    """integer_case with two blocks of coincident faces (rows 0..14 and 15..27): the faces whose first KN neighbours sit at distance 0,
    where the study's zero guard decides."""
    X, _ = integer_case(n, 6, seed)
    at = 0
    for b in blocks:
        X[at:at + b] = X[at]
        at += b
    return X, integer_distances(X)
