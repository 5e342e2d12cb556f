"""Cases and host restatements shared by tests/test_group_split_cpu.py and tests/test_group_split_gpu.py: groups of points with photos,
the penalised matrix P of a group built on the host, and the expected sublabels (clustering.complete_linkage_labels and scipy)."""
import numpy as np

PENALTY, CUT = 100.0, 50.0
WAVE_MAX, LDS_MAX = 32, 128                     # the chain classes' limits (include/hsefr_split.h)
# one below, at and one above each class limit, the smallest groups, and one well inside the global class
SIZES = [1, 2, 3, 31, 32, 33, 64, 65, 127, 128, 129, 300]


def integer_matrix(n, seed, lo=1, hi=5):
    """Symmetric, integer-valued in lo .. hi (many ties), zero diagonal."""
    rs = np.random.RandomState(seed)
    D = np.triu(rs.randint(lo, hi + 1, (n, n)).astype(np.float64), 1)
    return D + D.T


def grouping(sizes, seed, n=None, shuffled=False):
    """-> (members int32, offsets int64, n): the groups of ``sizes`` over n points (default: all of them, in natural order).  With a
    larger n the members are a non-contiguous subset; ``shuffled``: every group's members in a random, non-ascending order."""
    rs = np.random.RandomState(seed)
    total = int(np.sum(sizes))
    n = total if n is None else n
    pool = np.sort(rs.choice(n, total, replace=False)) if n > total else np.arange(total)
    if shuffled:
        pool = rs.permutation(pool)
    offsets = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    return pool.astype(np.int32), offsets, n


def photos_with_shared(members, offsets, n, seed, share=1 / 3):
    """A photo per point, its own, except that about ``share`` of every group's faces are in one photo of the group."""
    rs = np.random.RandomState(seed)
    photo = np.arange(n, dtype=np.int32) + 1000
    for g in range(len(offsets) - 1):
        m = members[offsets[g]:offsets[g + 1]]
        together = m[rs.rand(len(m)) < share]
        photo[together] = g
    return photo


def host_P(D, m, photo, penalty=PENALTY):
    """The matrix the split of the members m works on, from the upper triangle of D (what the device reads)."""
    m = np.asarray(m, dtype=np.int64)
    lo, hi = np.minimum(m[:, None], m[None, :]), np.maximum(m[:, None], m[None, :])
    P = np.asarray(D, dtype=np.float64)[lo, hi].copy()
    same = photo[m][:, None] == photo[m][None, :]
    P = P + penalty * same
    np.fill_diagonal(P, 0.0)
    return P


def expected_sublabels(P_of_group, offsets, cut=CUT):
    """complete_linkage_labels of every group's P, concatenated; and whether each group needs a chain (more than one member and an
    entry above the cut)."""
    from hse_facerec_tf_amd import clustering
    out, chained = [], []
    for g in range(len(offsets) - 1):
        P = P_of_group(g)
        out.append(clustering.complete_linkage_labels(P, cut))
        k = P.shape[0]
        chained.append(bool(k > 1 and (P[~np.eye(k, dtype=bool)] > cut).any()))
    return np.concatenate(out).astype(np.int32), np.array(chained)


def scipy_partition(P, cut=CUT):
    """fcluster(linkage(squareform(P), 'complete'), cut, 'distance') with the labels renumbered by first occurrence."""
    from scipy.cluster import hierarchy as hac
    from scipy.spatial.distance import squareform
    if P.shape[0] == 1:
        return np.zeros(1, dtype=np.int32)
    lab = hac.fcluster(hac.linkage(squareform(P, checks=False), "complete"), cut, "distance")
    _, first, inverse = np.unique(lab, return_index=True, return_inverse=True)
    rank = np.empty(len(first), dtype=np.int32)
    rank[np.argsort(first)] = np.arange(len(first))
    return rank[inverse.reshape(-1)]


def expected_stats(offsets, chained, bad=0):
    """hsefr_split_groups' five counts for groups of which ``chained`` run a chain"""
    k = np.diff(offsets)
    lds = int(np.sum(chained & (k <= LDS_MAX)))
    glob = int(np.sum(chained & (k > LDS_MAX)))
    return [int(len(k) - lds - glob), lds, glob, int(np.sum(k[chained] - 1)), bad]
