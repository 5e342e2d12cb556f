"""Inputs shared by the PCA suites (tests/test_pca_cpu.py, tests/test_pca_gpu.py): the exact Hadamard case, matrices with a designed
spectrum (a geometric one for small blocks, a stepped one for the protocol's block sizes), and the gallery / probe fixture of tests/golden/protocols.npz."""
import os

import numpy as np

from oracle import identification as oid

from conftest import GOLDEN

# (n, d, k): one partial tile; several row tiles with d and b off the 32 / 64 tile edges; n over 1024 with an odd d / 8; n - 1 < d
DESIGNED_SHAPES = [(5, 8, 3), (300, 72, 40), (1030, 136, 17), (170, 256, 16)]


def hadamard_case(order=64, cols=32):
    """X = H[:, :cols] * (cols, cols - 1, ..., 1) with H the order x order Hadamard matrix: column 0 is constant, every other column has
    mean zero and the columns are orthogonal, so the covariance is diag(0, (cols - 1)^2, ..., 1) * order / (order - 1) exactly and every
    value is exact in float32.  The default is 64 x 32; 512 x 256 with k = 255 makes the block the whole space at b = d = 256."""
    from scipy.linalg import hadamard
    s = np.arange(cols, 0, -1).astype(np.float64)
    return (hadamard(order)[:, :cols] * s).astype(np.float32), s


def designed_spectrum(n, d, k):
    """U diag(0.95^i) W^T with orthonormal U [n,r], W [d,r], r = min(n, d), from a seeded RandomState, cast to float32."""
    rs = np.random.RandomState(1000 * n + 10 * d + k)
    r = min(n, d)
    u, _ = np.linalg.qr(rs.randn(n, r))
    w, _ = np.linalg.qr(rs.randn(d, r))
    return ((u * 0.95 ** np.arange(r)) @ w.T).astype(np.float32)


# (n, d, k) at the block sizes of the protocol's own k (b = k + max(16, k / 2) in sixteens, at most min(n - 1, d)): b = 11 capped and
# odd; b = 112 off the 64 edge; b = 96 = d, the whole space; b = 192, the protocol's k = 128; b = 384, the largest; b = 192 at d = 1024
BLOCK_SHAPES = [(12, 16, 9), (200, 120, 70), (300, 96, 80), (300, 200, 128), (420, 392, 256), (300, 1024, 128)]
# (n, d, k, offset, scale): every entry positive, their mean about 700 times the centred spread, as raw post-ReLU6 embeddings are
OFFSET_CASE = (300, 200, 128, 3.0, 0.1)


def block_size(n, d, k):
    """hsefr_pca_fit's iterated block."""
    return min((k + max(16, k // 2) + 15) // 16 * 16, n - 1, d)


def stepped_spectrum(n, d, k, offset=0.0, scale=1.0):
    """offset + scale U diag(sqrt lam) W^T cast to float32, with U [n,r] orthonormal with columns of mean zero, W [d,r] orthonormal,
    r = min(n - 1, d), and lam_i = 1 - i / 2k up to i = k, then 0.5 * 0.97^(i - k): the covariance's eigenvalues are lam / (n - 1), so the
    smallest gap among the first k is 1 / 2k of lambda_1 at any k, and the tail falls fast enough for a few convergence checks."""
    rs = np.random.RandomState(1000 * n + 10 * d + k)
    r = min(n - 1, d)
    a = rs.randn(n, r)
    u, _ = np.linalg.qr(a - a.mean(axis=0))
    w, _ = np.linalg.qr(rs.randn(d, r))
    i = np.arange(r)
    lam = np.where(i <= k, 1.0 - 0.5 * i / k, 0.5 * 0.97 ** (i - float(k)))
    return (offset + scale * (u * np.sqrt(lam)) @ w.T).astype(np.float32)


def block_cases():
    """(name, x, k) of BLOCK_SHAPES and OFFSET_CASE."""
    cases = [("stepped %d x %d" % (n, d), stepped_spectrum(n, d, k), k) for n, d, k in BLOCK_SHAPES]
    n, d, k, offset, scale = OFFSET_CASE
    return cases + [("stepped %d x %d + %g" % (n, d, offset), stepped_spectrum(n, d, k, offset, scale), k)]


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
