"""hsefr_pca_fit / hsefr_pca_transform's contract restated in NumPy: the column means and the covariance (X - mean)^T (X - mean) / (n - 1)
in float64, numpy.linalg.eigh, the k largest eigenvalues in descending order with their unit eigenvectors, each signed so that its entry
of largest magnitude is positive (the first one on ties: scikit-learn 1.7's svd_flip(u_based_decision=False)), and the projection
accumulated in float64 and cast once to float32."""
import numpy as np


def fit(x, k):
    """(mean [d], components [k,d], explained_variance [k]) in float64, of x [n,d]."""
    x = np.asarray(x, dtype=np.float64)
    n, d = x.shape
    assert 1 <= k <= min(n - 1, d)
    mean = x.mean(axis=0)
    xc = x - mean
    w, v = np.linalg.eigh(xc.T @ xc / (n - 1))
    order = np.argsort(-w, kind="stable")
    components = v[:, order[:k]].T.copy()
    lead = np.argmax(np.abs(components), axis=1)                 # the first maximum
    components *= np.where(components[np.arange(k), lead] < 0, -1.0, 1.0)[:, None]
    return mean, components, w[order[:k]]


def eigenvalues(x):
    """Every eigenvalue of the covariance, descending (the gaps of a fixture)."""
    x = np.asarray(x, dtype=np.float64)
    xc = x - x.mean(axis=0)
    return np.sort(np.linalg.eigvalsh(xc.T @ xc / (len(x) - 1)))[::-1]


def transform64(x, mean, components):
    return (np.asarray(x, dtype=np.float64) - mean) @ np.asarray(components).T


def transform(x, mean, components):
    """float32 [n,k]: one rounding of the float64 projection."""
    return transform64(x, mean, components).astype(np.float32)


def neighbour_margin(z_probe, z_gallery, first=5):
    """The smallest gap between consecutive squared distances among each probe's ``first`` nearest gallery rows, relative to the last of
    them, minimised over the probes."""
    q = np.asarray(z_probe, dtype=np.float64)
    g = np.asarray(z_gallery, dtype=np.float64)
    d2 = ((q[:, None, :] - g[None, :, :]) ** 2).sum(-1)
    near = np.sort(d2, axis=1)[:, :first]
    return float((np.diff(near, axis=1).min(axis=1) / near[:, -1]).min())
