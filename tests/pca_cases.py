"""Inputs shared by the PCA suites (tests/test_pca_cpu.py, tests/test_pca_gpu.py): the exact Hadamard case, matrices with a designed
spectrum, and the gallery / probe fixture of tests/golden/protocols.npz."""
import os

import numpy as np

from oracle import identification as oid

from conftest import GOLDEN

# (n, d, k): one partial tile; several row tiles with d and b off the 32 / 64 tile edges; n over 1024 with an odd d / 8; n - 1 < d
DESIGNED_SHAPES = [(5, 8, 3), (300, 72, 40), (1030, 136, 17), (170, 256, 16)]


def hadamard_case():
    """X = H[:, :32] * (32, 31, ..., 1) with H the 64 x 64 Hadamard matrix: column 0 is constant, every other column has mean zero and
    the columns are orthogonal, so the covariance is diag(0, 31^2, ..., 1) * 64 / 63 exactly and every value is exact in float32."""
    from scipy.linalg import hadamard
    s = np.arange(32, 0, -1).astype(np.float64)
    return (hadamard(64)[:, :32] * s).astype(np.float32), s


def designed_spectrum(n, d, k):
    """U diag(0.95^i) W^T with orthonormal U [n,r], W [d,r], r = min(n, d), from a seeded RandomState, cast to float32."""
    rs = np.random.RandomState(1000 * n + 10 * d + k)
    r = min(n, d)
    u, _ = np.linalg.qr(rs.randn(n, r))
    w, _ = np.linalg.qr(rs.randn(d, r))
    return ((u * 0.95 ** np.arange(r)) @ w.T).astype(np.float32)


def relative_gap(x, k):
    """min over i < k of (lambda_i - lambda_{i+1}) / lambda_1."""
    import pca_ref
    lam = pca_ref.eigenvalues(x)
    return float(np.min(lam[:k] - lam[1:k + 1]) / lam[0])


def protocol_fixture():
    """(npz, raw features, L2-normalised features) of the filtered protocols.npz samples."""
    z = np.load(os.path.join(GOLDEN, "protocols.npz"))
    X, y = oid.synthetic_gallery(int(z["n_classes"]), int(z["dim"]), int(z["seed"]), float(z["noise"]))
    Xn, y2, kept = oid.filter_and_encode(X, y)
    assert np.array_equal(y2, z["y"])
    return z, X[kept], Xn


def golden_split():
    """(X, y, normalised filtered features, encoded labels, train, test) of tests/golden/nn1.npz's stratified half split."""
    z = np.load(os.path.join(GOLDEN, "nn1.npz"))
    X, y = oid.synthetic_gallery(int(z["n_classes"]), int(z["dim"]), int(z["seed"]), float(z["noise"]))
    Xn, y2, kept = oid.filter_and_encode(X, y)
    assert np.array_equal(kept, z["kept"]) and np.array_equal(y2, z["y"])
    return X, y, Xn, y2, z["train"], z["test"]
