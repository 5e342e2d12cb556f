"""NumPy/scipy restatement of DBSCAN's labels for the clustering tests (the rule of csrc/dbscan.hip, with no traversal order in it):
core points have at least min_samples points within eps, themselves included; core clusters are the connected components of the
core-core edges within eps, numbered by their smallest core index; a non-core point joins the cluster of the smallest seed among its
core neighbours, else it is noise (-1).  A dense matrix is read as its upper triangle."""
import numpy as np
from scipy.sparse import coo_matrix
from scipy.sparse.csgraph import connected_components


def dbscan_from_adjacency(n, rows, cols, min_samples):
    """(core_sample_indices, labels) int64 from the pairs i != j with w(i, j) <= eps, each listed in both directions."""
    rows = np.asarray(rows, dtype=np.int64)
    cols = np.asarray(cols, dtype=np.int64)
    core = np.bincount(rows, minlength=n) + 1 >= min_samples
    cc = core[rows] & core[cols]
    A = coo_matrix((np.ones(int(cc.sum()), dtype=np.int8), (rows[cc], cols[cc])), shape=(n, n))
    _, comp = connected_components(A, directed=False)
    idx = np.arange(n)
    seed = np.full(n, n, dtype=np.int64)
    np.minimum.at(seed, comp[core], idx[core])
    cs = np.where(core, seed[comp], n)                   # n: no seed
    border = np.full(n, n, dtype=np.int64)
    np.minimum.at(border, rows, cs[cols])
    s = np.where(core, cs, border)
    rank = np.full(n + 1, -1, dtype=np.int64)
    seeds = np.flatnonzero(core & (cs == idx))
    rank[seeds] = np.arange(len(seeds))
    return np.flatnonzero(core).astype(np.int64), rank[s]


def dbscan_dense(D, eps, min_samples):
    """The rule on D's upper triangle D[min(i,j), max(i,j)] (the diagonal is not read)."""
    D = np.asarray(D, dtype=np.float64)
    n = D.shape[0]
    iu, ju = np.nonzero(np.triu(D <= eps, 1))
    return dbscan_from_adjacency(n, np.concatenate([iu, ju]), np.concatenate([ju, iu]), min_samples)


def clusters_of(labels):
    """Noise dropped, the members of each label ascending, longest first then by smallest member (clustering._finish's order)."""
    labels = np.asarray(labels)
    out = [sorted(np.flatnonzero(labels == v).tolist()) for v in np.unique(labels[labels >= 0])]
    out.sort(key=lambda c: (-len(c), c[0]))
    return out
