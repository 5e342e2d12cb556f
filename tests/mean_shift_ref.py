"""NumPy restatement in fp64 of sklearn.cluster.MeanShift(bandwidth=h, seeds=None, bin_seeding=False, max_iter=m) as scikit-learn 1.7.2
executes it (sklearn/cluster/_mean_shift.py), with all seeds advanced together: what hsefr_shift_fit (include/hsefr_shift.h) answers.

Every row of X is a seed whose mean starts at the row.  An active seed's members are the rows with |x - mean| <= h; the new mean is their
average and ``count`` their number; the seed stops when |new - old| <= 1e-3 h or its completed iterations equal max_iter, else
completed += 1.  Means equal as tuples of doubles collapse (scikit-learn's dict keyed by the mean; the last seed's count stays), the
survivors are ordered by (count, mean tuple) descending, a centre not yet suppressed suppresses every later one within h, and a point's
label is its nearest surviving centre, the lowest index on an exact tie.

Besides the result the restatement reports four margins, by which a test proves that a case is decidable in another arithmetic:
    member   the least | |x - mean| - h |  over all member tests of all iterations
    shift    the least | |new - old| - 1e-3 h |
    centre   the least | |c - c'| - h |  over the pairs of distinct means
    label    the least gap between a point's two nearest centres (inf with one centre)"""
from collections import namedtuple

import numpy as np

Result = namedtuple("Result", "centers labels label_dist n_iter intensity completed distinct stopped_by_max_iter margins")
Margins = namedtuple("Margins", "member shift centre label")


def _dist(A, B):
    """|a - b| for every row pair, from the differences themselves (no cancellation): [len(A), len(B)] float64"""
    out = np.empty((len(A), len(B)))
    for i in range(len(A)):
        diff = B - A[i]
        out[i] = np.sqrt(np.einsum("ij,ij->i", diff, diff))
    return out


def mean_shift(X, bandwidth, max_iter=300, cluster_all=True):
    X32 = np.asarray(X)
    assert X32.dtype == np.float32 and X32.ndim == 2
    X = X32.astype(np.float64)                                        # exact
    n = len(X)
    h = float(bandwidth)
    stop = 1e-3 * h
    means = X.copy()
    count = np.zeros(n, np.int64)
    completed = np.zeros(n, np.int64)
    active = np.arange(n)
    m_member = m_shift = np.inf
    by_max_iter = 0
    while len(active):                                                # at most max_iter + 1 passes
        D = _dist(means[active], X)
        m_member = min(m_member, float(np.abs(D - h).min()))
        inside = D <= h
        keep = []
        for r, s in enumerate(active):
            members = X[inside[r]]
            count[s] = len(members)
            new = members.mean(axis=0)
            shift = float(np.linalg.norm(new - means[s]))
            means[s] = new
            m_shift = min(m_shift, abs(shift - stop))
            if shift <= stop or completed[s] == max_iter:
                by_max_iter += int(shift > stop)
                continue
            completed[s] += 1
            keep.append(s)
        active = np.array(keep, np.int64)
    table = {}
    for s in range(n):
        table[tuple(means[s])] = int(count[s])
    ordered = sorted(table.items(), key=lambda kv: (kv[1], kv[0]), reverse=True)
    C = np.array([kv[0] for kv in ordered]).reshape(len(ordered), X.shape[1])
    weight = np.array([kv[1] for kv in ordered], np.int64)
    DC = _dist(C, C)
    off = DC[~np.eye(len(C), dtype=bool)]
    m_centre = float(np.abs(off - h).min()) if len(off) else np.inf
    unique = np.ones(len(C), bool)
    for i in range(len(C)):
        if unique[i]:
            unique[i + 1:] &= ~(DC[i, i + 1:] <= h)
    centers, intensity = C[unique], weight[unique]
    DL = _dist(X, centers)
    labels = DL.argmin(axis=1).astype(np.int64)                       # the first of equal minima
    label_dist = DL[np.arange(n), labels]
    m_label = float(np.diff(np.sort(DL, axis=1)[:, :2], axis=1).min()) if len(centers) > 1 else np.inf
    if not cluster_all:
        labels = np.where(label_dist <= h, labels, -1)
    return Result(centers, labels, label_dist, int(completed.max()), intensity, completed, len(C), by_max_iter,
                  Margins(m_member, m_shift, m_centre, m_label))


def nearest_center(Q, centers):
    """MeanShift.predict in fp64: (index of the nearest centre, the lowest on a tie; its distance)"""
    D = _dist(np.asarray(Q, np.float32).astype(np.float64), np.asarray(centers, np.float64))
    idx = D.argmin(axis=1)
    return idx.astype(np.int64), D[np.arange(len(D)), idx]


def cluster_lists(labels):
    """The reference's result form of its scikit-learn branch (facial_clustering_test.py:265-266, 285): the members of every label >= 0,
    the largest cluster first (stable)."""
    labels = np.asarray(labels)
    groups = [np.flatnonzero(labels == c) for c in range(int(labels.max()) + 1 if len(labels) else 0)]
    groups = [g for g in groups if len(g)]
    groups.sort(key=len, reverse=True)
    return [[int(i) for i in g] for g in groups]
