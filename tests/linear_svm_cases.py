"""Inputs shared by the linear SVM suites (tests/test_linear_svm_cpu.py, tests/test_linear_svm_gpu.py): the known answer, designed cases
at shapes off every tile edge, and the gallery / probe fixture of tests/golden/protocols.npz with its recorded scikit-learn answers
(tests/golden/linear_svm.npz, written by tools/record_linear_svm_golden.py)."""
import functools
import os

import numpy as np

import linear_svm_ref
import pca_cases

from conftest import GOLDEN

GOLDEN_FILE = os.path.join(GOLDEN, "linear_svm.npz")
HELD_OUT = 96          # rows of a designed case that the fit does not see

# (n, d, K): binary with one partial tile; three classes off every edge; several row tiles with d and K off the 64 / 32 tile edges;
# more than 1024 rows.  The fixture gallery (170, 256, 66) is the fifth case.
DESIGNED_SHAPES = [(5, 8, 2), (37, 19, 3), (300, 72, 40), (1030, 136, 17)]
# the sixth case: more classes than the 512 the library solves at once -- two class blocks, 301 and 300 rows, so the second block's
# workspace reset, its row and class offsets, its shorter length and the merge of the blocks' info are all exercised
MANY_CLASSES_SHAPE = (700, 16, 601)
N_CASES = len(DESIGNED_SHAPES) + 2


def known_answer():
    """X = [[1], [-1]], labels [1, 0], C = 1/4: by symmetry b = 0, and w minimises w^2 / 2 + 2 C (1 - w)^2, w = 4C / (1 + 4C) = 1/2.
    Every value on the way is exact in binary floating point.  Returns (X, labels, C, coef, intercept, decisions of X)."""
    X = np.array([[1.0], [-1.0]], dtype=np.float32)
    return X, np.array([1, 0], dtype=np.int32), 0.25, np.array([[0.5]]), np.array([0.0]), np.array([[0.5], [-0.5]])


def designed_case(n, d, K):
    """Gaussian class centres of standard deviation 0.3 per coordinate under noise of 1.5 from a seeded RandomState, float32: where n > d some
    classes cannot be separated from the rest and many training rows stay inside the margin.  Every class has a row (labels are a
    permutation of i mod K).  Returns (X [n,d], labels [n] int32, held-out rows [HELD_OUT,d])."""
    rs = np.random.RandomState(7000 + 100 * n + 10 * d + K)
    centres = 0.3 * rs.randn(K, d)
    labels = rs.permutation(np.arange(n) % K).astype(np.int32)
    X = (centres[labels] + 1.5 * rs.randn(n, d)).astype(np.float32)
    held = (centres[rs.randint(0, K, HELD_OUT)] + 1.5 * rs.randn(HELD_OUT, d)).astype(np.float32)
    return X, labels, held


def fixture_case():
    """The raw gallery of protocols.npz with np.unique label codes, and its probes as the held-out rows."""
    z, Xraw, _ = pca_cases.protocol_fixture()
    g, p = z["gallery"], z["probe"]
    classes, codes = np.unique(z["y"][g], return_inverse=True)
    return Xraw[g], codes.astype(np.int32), Xraw[p], len(classes)


@functools.lru_cache(maxsize=None)
def case(index):
    """(name, X, labels, n_classes, held-out rows) of designed case ``index`` in 0..5."""
    if index == len(DESIGNED_SHAPES) + 1:
        n, d, K = MANY_CLASSES_SHAPE
        X, labels, held = designed_case(n, d, K)
        return "designed %d x %d, %d classes (two class blocks)" % (n, d, K), X, labels, K, held
    if index < len(DESIGNED_SHAPES):
        n, d, K = DESIGNED_SHAPES[index]
        X, labels, held = designed_case(n, d, K)
        return "designed %d x %d, %d classes" % (n, d, K), X, labels, K, held
    X, labels, held, K = fixture_case()
    return "protocols.npz gallery %d x %d, %d classes" % (X.shape[0], X.shape[1], K), X, labels, K, held


@functools.lru_cache(maxsize=None)
def reference(index):
    """linear_svm_ref.fit of case ``index``, computed once per process and shared: (coef, intercept, info)."""
    _, X, labels, K, _ = case(index)
    return linear_svm_ref.fit(X, labels, K)


def protocol_variant(normalize, pca_components=None, moved=False):
    """(gallery rows, gallery label codes, probe rows, classes) of the fixture as gallery_probe_identification sees them: raw or
    L2-normalised features, after pca_ref's float32 projection fitted on the gallery when ``pca_components`` is set.
    ``moved``: the same rows moved by as much as the device's own float32 steps may differ from the host's (input_rounding_shift)."""
    import pca_ref
    z, Xraw, Xn = pca_cases.protocol_fixture()
    A = Xn if normalize else Xraw
    g, p = z["gallery"], z["probe"]
    classes, codes = np.unique(z["y"][g], return_inverse=True)
    gal, prb = A[g].astype(np.float32), A[p].astype(np.float32)
    rs = np.random.RandomState(16 * (pca_components or 0) + int(normalize))
    if moved and normalize:
        gal = (gal * (1.0 + rs.choice([-1.0, 1.0], (len(gal), 1)) * 2.0 ** -21)).astype(np.float32)
        prb = (prb * (1.0 + rs.choice([-1.0, 1.0], (len(prb), 1)) * 2.0 ** -21)).astype(np.float32)
    if pca_components:
        mean, comp, _ = pca_ref.fit(gal, pca_components)
        gal, prb = pca_ref.transform(gal, mean, comp), pca_ref.transform(prb, mean, comp)
        if moved:
            gal = (gal + np.spacing(np.abs(gal)) * rs.choice([-1.0, 1.0], gal.shape).astype(np.float32)).astype(np.float32)
            prb = (prb + np.spacing(np.abs(prb)) * rs.choice([-1.0, 1.0], prb.shape).astype(np.float32)).astype(np.float32)
    return gal, codes.astype(np.int32), prb, classes


@functools.lru_cache(maxsize=None)
def protocol_reference(normalize, pca_components=None):
    """linear_svm_ref's probe decisions and predicted labels of a protocol variant, computed once: (decision, y_pred, info)."""
    gal, codes, prb, classes = protocol_variant(normalize, pca_components)
    coef, intercept, info = linear_svm_ref.fit(gal, codes, len(classes))
    dec = linear_svm_ref.decision(prb, coef, intercept)
    return dec, classes[linear_svm_ref.predict(dec)], info



def decision_bound(gal, codes, n_classes, prb, tol, C=1.0):
    """An upper bound on |decision - decision at the optimum| over the probes ``prb`` for a fit that ends with |grad f_k| <= 2 tol
    |grad f_k(0)| (what the GPU suite asserts of the device): f_k is 1-strongly convex, so |w~ - w~*| <= |grad f_k(w~)|, and a
    decision value moves by at most that times |x~|."""
    zero = np.zeros((1 if n_classes == 2 else n_classes, gal.shape[1] + 1))
    g0 = np.sqrt((linear_svm_ref.gradient(zero, gal, codes, n_classes, C) ** 2).sum(1))
    xq = float(np.sqrt((np.asarray(prb, dtype=np.float64) ** 2).sum(1) + 1.0).max())
    return float((2.0 * tol * g0).max()) * xq


@functools.lru_cache(maxsize=None)
def input_rounding_shift(normalize, pca_components=None):
    """How far the reference's probe decisions move when the classifier's input rows move by as much as the device's float32 steps in
    front of the fit may differ from the host's.  This is a MEASURED SAMPLE of the reference's sensitivity, not an upper bound: one
    seeded draw of signs, every row and entry moved by the largest amount the step allows (a rigorous bound through
    |w~*' - w~*| <= |grad f'(w~*)| sums |x~_i| |w~| over all rows and comes out near 1, useless next to gaps of 1e-3):
      - L2 normalisation: either side divides a row by a float32 norm, the square root of a float32 sum of 256 squares in its own
        order; each sum is within a few units of 2^-24 of the exact one, so the two rows differ by a common factor within 1 +- 2^-21
        (eight units) before one rounding per entry.  Every row is scaled by 1 + 2^-21 or 1 - 2^-21.
      - PCA: the device's projection and pca_ref's are the float32 roundings of float64 values that agree to about 1e-9
        (tests/test_pca_gpu.py), so they differ by one unit in the last place in the few entries on a rounding boundary and
        nowhere else.  EVERY projected entry is moved by one unit, up or down.
    Raw features without PCA reach the device bit for bit: no shift."""
    if not normalize and not pca_components:
        return 0.0
    gal, codes, prb, classes = protocol_variant(normalize, pca_components, moved=True)
    coef, intercept, _ = linear_svm_ref.fit(gal, codes, len(classes))
    return float(np.abs(linear_svm_ref.decision(prb, coef, intercept) - protocol_reference(normalize, pca_components)[0]).max())
