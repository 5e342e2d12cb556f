"""hsefr_metric_dist's and hsefr_knn_metric's contract restated in float64 on the float32 inputs: the study's chi2dist and KL_dist
(facerec_test.py:157-164) between probe rows x and gallery rows y, and the error bound the header gives for each, u = 2^-24:

    chi2  D = sum_c (x - y)^2 / (x + y) over the columns with x + y > 0                  |error| <= (d + 6) u D
    kl    D = sum_c t_c, t_c = a (log a - log b), a = fl32(x + 0.001f), b = fl32(y + 0.001f)
                                                          |error| <= u [(d + 2) sum |t_c| + 4 sum a_c (|log a_c| + |log b_c|)]

A NaN distance (a kl entry <= -0.001) is +inf, as the library returns it.  The order and the vote are knn_ref.knn_from_dist2's.  The
[n, m, d] terms are walked in blocks of probe rows (torch on the CPU in float64: NumPy's single thread takes ten times as long at the
sizes of the GPU suite)."""
import numpy as np
import torch

import knn_ref

U = 2.0 ** -24
METRICS = ("chi2", "kl")


def _row_blocks(n, m, d, elems=1 << 24):
    step = max(1, elems // max(1, m * d))
    return [(a, min(a + step, n)) for a in range(0, n, step)]


def dist_and_bound(x, y, metric):
    """(D [n,m], bound [n,m]) in float64 for float32 x [n,d], y [m,d]."""
    assert metric in METRICS
    x = np.ascontiguousarray(x, dtype=np.float32)
    y = np.ascontiguousarray(y, dtype=np.float32)
    n, d = x.shape
    m = y.shape[0]
    D = np.empty((n, m), np.float64)
    B = np.empty((n, m), np.float64)
    if metric == "chi2":
        xt, yt = torch.from_numpy(x).double(), torch.from_numpy(y).double()
    else:
        xt = torch.from_numpy(x + np.float32(0.001)).double()         # a and b are float32 sums
        yt = torch.from_numpy(y + np.float32(0.001)).double()
        with np.errstate(all="ignore"):
            lx, ly = torch.log(xt), torch.log(yt)
    for a, b in _row_blocks(n, m, d):
        if metric == "chi2":
            s = xt[a:b, None, :] + yt[None, :, :]
            t = torch.where(s > 0, (xt[a:b, None, :] - yt[None, :, :]) ** 2 / s, torch.zeros((), dtype=torch.float64))
            dist = t.sum(-1)
            bound = (d + 6) * U * dist
        else:
            t = xt[a:b, None, :] * (lx[a:b, None, :] - ly[None, :, :])
            dist = t.sum(-1)
            logs = (xt[a:b].abs() * lx[a:b].abs()).sum(-1)[:, None] + xt[a:b].abs() @ ly.abs().T
            bound = U * ((d + 2) * t.abs().sum(-1) + 4 * logs)
        D[a:b], B[a:b] = dist.numpy(), bound.numpy()
    nan = np.isnan(D)
    D[nan] = np.inf
    B[nan | np.isnan(B)] = 0.0
    return D, B


def dist(x, y, metric):
    return dist_and_bound(x, y, metric)[0]


def knn(q, g, k, metric, labels=None):
    """(index [nq,k], dist [nq,k], pred [nq] or None): ascending (distance, gallery index), the uniform vote."""
    return knn_ref.knn_from_dist2(dist(q, g, metric), k, labels)


def clear_rows(D, B, k):
    """Rows whose first k + 1 sorted distances are pairwise further apart than the sum of their two bounds: the float32 search has
    no choice there."""
    order = np.argsort(D, axis=1, kind="stable")[:, :k + 1]
    d = np.take_along_axis(D, order, axis=1)
    b = np.take_along_axis(B, order, axis=1)
    return np.all(np.diff(d, axis=1) > b[:, 1:] + b[:, :-1], axis=1)


# the reference's two distances as Python callables of two rows, the form scikit-learn's metric= takes (facerec_test.py:157-164)
def chi2dist(x, y):
    total = x + y
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(total > 0, (x - y) ** 2 / total, 0).sum()


def KL_dist(x, y):
    return ((x + 0.001) * np.log((x + 0.001) / (y + 0.001))).sum()


CALLABLES = {"chi2": chi2dist, "kl": KL_dist}
