"""hsefr_knn's contract restated in NumPy: squared distances in float64, the k nearest gallery rows of every probe in ascending order of
(dist2, gallery index) -- exact ties to the lowest index at every position, the k-th / (k+1)-th boundary included -- and the uniform
vote: the label with the most occurrences among the k, equal counts to the smallest label value (scikit-learn's predict: the mode over
sorted classes_, first maximum)."""
import numpy as np


def dist2(q, g):
    """|q|^2 + |g|^2 - 2 q.g in float64, clipped at 0 (exact for small-integer features)."""
    q = np.asarray(q, dtype=np.float64)
    g = np.asarray(g, dtype=np.float64)
    return np.maximum((q ** 2).sum(1)[:, None] + (g ** 2).sum(1)[None, :] - 2.0 * q @ g.T, 0.0)


def knn_from_dist2(d2, k, labels=None):
    """(index [nq,k], dist2 [nq,k], pred [nq] or None) of a distance matrix [nq,ng]."""
    d2 = np.asarray(d2)
    nq, ng = d2.shape
    assert 1 <= k <= ng
    cols = np.broadcast_to(np.arange(ng), d2.shape)
    order = np.lexsort((cols, d2), axis=1)[:, :k]             # last key first: by dist2, then by index
    near = np.take_along_axis(d2, order, axis=1)
    if labels is None:
        return order, near, None
    labels = np.asarray(labels)
    pred = np.empty(nq, dtype=labels.dtype)
    for i in range(nq):
        values, counts = np.unique(labels[order[i]], return_counts=True)      # sorted values: argmax takes the first maximum
        pred[i] = values[np.argmax(counts)]
    return order, near, pred


def knn(q, g, k, labels=None):
    return knn_from_dist2(dist2(q, g), k, labels)
