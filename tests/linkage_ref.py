"""fp64 restatement of single linkage for the clustering tests: Prim's minimum spanning tree on a dense matrix's upper triangle
(what squareform(D, checks=False) reads) and the flat cut of a tree at a threshold.  NumPy only."""
import numpy as np


def upper_symmetric(D):
    D = np.asarray(D, dtype=np.float64)
    U = np.triu(D, 1)
    return U + U.T


def prim_mst(D):
    """-> (a, b, h): the n - 1 edges of a minimum spanning tree of the complete graph weighted by D's upper triangle."""
    W = upper_symmetric(D)
    n = W.shape[0]
    in_tree = np.zeros(n, dtype=bool)
    in_tree[0] = True
    best = W[0].copy()
    src = np.zeros(n, dtype=np.int64)
    a, b, h = [], [], []
    for _ in range(n - 1):
        cand = np.where(in_tree, np.inf, best)
        v = int(np.argmin(cand))
        a.append(int(src[v]))
        b.append(v)
        h.append(float(best[v]))
        in_tree[v] = True
        closer = W[v] < best
        best = np.where(closer, W[v], best)
        src = np.where(closer, v, src)
    return np.array(a, dtype=np.int64), np.array(b, dtype=np.int64), np.array(h, dtype=np.float64)


def canonical(labels):
    """Labels renumbered 0.. by first occurrence: equal partitions give equal arrays."""
    labels = np.asarray(labels).reshape(-1)
    _, first, inv = np.unique(labels, return_index=True, return_inverse=True)
    rank = np.empty(len(first), dtype=np.int64)
    rank[np.argsort(first)] = np.arange(len(first))
    return rank[inv.reshape(-1)]


def flat_cut(n, a, b, h, t):
    """Connected components of the tree edges with height <= t (fcluster(Z, t, 'distance') of single linkage), canonical labels."""
    parent = np.arange(n)

    def find(v):
        while parent[v] != v:
            parent[v] = parent[parent[v]]
            v = parent[v]
        return v
    for x, y, w in zip(a, b, h):
        if w <= t:
            parent[find(int(x))] = find(int(y))
    return canonical([find(v) for v in range(n)])


def cut_thresholds(heights):
    """Every distinct height and every midpoint between neighbours, plus one below and one above them all."""
    hs = np.unique(np.asarray(heights, dtype=np.float64))
    if len(hs) == 0:
        return np.array([0.0])
    mids = (hs[:-1] + hs[1:]) / 2
    return np.concatenate([[hs[0] - 1.0], hs, mids, [hs[-1] + 1.0]])


def gap_thresholds(heights, want, min_gap):
    """For each wanted threshold: itself if no height lies within min_gap / 2 of it, else the midpoint of the nearest gap between
    consecutive sorted heights that is wider than min_gap."""
    hs = np.sort(np.asarray(heights, dtype=np.float64))
    out = []
    for t in want:
        if len(hs) == 0 or np.min(np.abs(hs - t)) > min_gap / 2:
            out.append(float(t))
            continue
        lo, hi = hs[:-1], hs[1:]
        ok = np.flatnonzero(hi - lo > min_gap)
        mids = (lo[ok] + hi[ok]) / 2
        out.append(float(mids[np.argmin(np.abs(mids - t))]))
    return out
