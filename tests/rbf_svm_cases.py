"""Inputs shared by the RBF SVM suites (tests/test_rbf_svm_cpu.py, tests/test_rbf_svm_gpu.py): the known answer, designed cases at the
smallest shapes at which each part of the device code can still go wrong, the gallery / probe fixture of tests/golden/protocols.npz, and
scikit-learn's recorded answers (tests/golden/rbf_svm.npz, written by tools/record_rbf_svm_golden.py)."""
import functools
import os

import numpy as np

import pca_cases
import rbf_svm_ref

from conftest import GOLDEN

GOLDEN_FILE = os.path.join(GOLDEN, "rbf_svm.npz")
HELD_OUT = 96          # rows of a designed case that the fit does not see
DECISION_ROWS = 8      # held-out rows whose pair decisions are recorded
DECISION_PAIRS = 4096  # ... for every pair up to this many, beyond it for every DECISION_STRIDE-th pair (the file stays small)
DECISION_STRIDE = 64

# (name, class sizes, d, seed): K = 2 (one pair, one dual_coef row); a one-row class and every tile edge; pairs of 3, 71, ..., 330 rows --
# past one wave and past one 256-thread workgroup; 300 classes, 44 850 pairs -- more than any grid, all tiny
DESIGNED = [("binary", [2, 3], 8, 1), ("three classes", [1, 12, 24], 19, 2), ("large pairs", [1, 2, 70, 130, 200], 24, 3),
            ("many pairs", [1] * 100 + [2] * 100 + [4] * 100, 16, 5)]
N_CASES = len(DESIGNED) + 2
MANY_PAIRS = 3         # the index of the case whose decisions are recorded for a subset of the pairs


def known_answer(C):
    """Rows [[0], [1]], classes 0 / 1, gamma = ln 2, so k = 1/2 between them.  C = 1: the unconstrained a = 1 / (1 - k) = 2 is cut to
    the bound 1 for both and rho = 0 by the midpoint rule; C = 4: a = 2 is free and rho = 0.  dec(q) = a (2^-q^2 - 2^-(q-1)^2).
    Returns (X, labels, gamma, a, probes, their decisions)."""
    a = min(2.0, C)
    q = np.array([[0.0], [1.0], [0.5], [-1.0], [2.0], [0.25]], dtype=np.float32)
    qq = q[:, 0].astype(np.float64)
    return (np.array([[0.0], [1.0]], dtype=np.float32), np.array([0, 1], dtype=np.int32), float(np.log(2.0)), a, q,
            a * (2.0 ** -(qq * qq) - 2.0 ** -((qq - 1.0) * (qq - 1.0))))


def designed_case(sizes, d, seed):
    """Gaussian class centres of standard deviation 0.3 per coordinate under noise of 1.5, float32, the rows NOT grouped by class.
    Returns (X [n,d], labels [n] int32, held-out rows [HELD_OUT,d])."""
    K = len(sizes)
    rs = np.random.RandomState(seed)
    labels = rs.permutation(np.repeat(np.arange(K), sizes))
    centres = 0.3 * rs.randn(K, d)
    X = (centres[labels] + 1.5 * rs.randn(len(labels), d)).astype(np.float32)
    held = (centres[rs.randint(0, K, HELD_OUT)] + 1.5 * rs.randn(HELD_OUT, d)).astype(np.float32)
    return X, labels.astype(np.int32), held


@functools.lru_cache(maxsize=None)
def case(index):
    """(name, X, labels, n_classes, held-out rows) of case ``index`` in 0..5; the last two are the fixture's gallery with its probes as the
    held-out rows, raw and L2-normalised."""
    if index < len(DESIGNED):
        name, sizes, d, seed = DESIGNED[index]
        X, labels, held = designed_case(sizes, d, seed)
        return name, X, labels, len(sizes), held
    z, Xraw, Xn = pca_cases.protocol_fixture()
    A = Xn if index == len(DESIGNED) + 1 else Xraw
    g, p = z["gallery"], z["probe"]
    classes, codes = np.unique(z["y"][g], return_inverse=True)
    return ("fixture normalised" if A is Xn else "fixture raw"), A[g].astype(np.float32), codes.astype(np.int32), len(classes), \
        A[p].astype(np.float32)


def gamma(index):
    return rbf_svm_ref.gamma_scale(case(index)[1])


@functools.lru_cache(maxsize=None)
def reference(index):
    """rbf_svm_ref.fit of case ``index`` at tol = 1e-12, computed once per process and shared: (dual_coef, rho, pairs, iterations)."""
    _, X, labels, K, _ = case(index)
    return rbf_svm_ref.fit(X, labels, K, gamma(index), tol=1e-12)


@functools.lru_cache(maxsize=None)
def reference_decision(index):
    _, X, labels, K, held = case(index)
    dual_coef, rho, _, _ = reference(index)
    return rbf_svm_ref.decision(held, X, labels, K, gamma(index), dual_coef, rho)


@functools.lru_cache(maxsize=None)
def decision_bound(index, eps):
    """rbf_svm_ref.decision_bound of case ``index``: (decision values, rho alone)."""
    _, X, labels, _, _ = case(index)
    return rbf_svm_ref.decision_bound(X, labels, gamma(index), reference(index)[2], eps)


def recorded_pairs(n_pairs):
    """The pairs whose decisions the golden file holds for the first DECISION_ROWS held-out rows."""
    return np.arange(n_pairs) if n_pairs <= DECISION_PAIRS else np.arange(0, n_pairs, DECISION_STRIDE)


@functools.lru_cache(maxsize=None)
def golden():
    z = np.load(GOLDEN_FILE)
    return {k: z[k] for k in z.files}


def pca_variant(moved=False):
    """(gallery rows, label codes, probe rows, classes) of the raw fixture after pca_ref's float32 projection to 16 components, as
    gallery_probe_identification(pca="device", pca_components=16) sees them; ``moved``: every projected entry one unit in the last
    place up or down, as far as the device's projection may differ (linear_svm_cases.input_rounding_shift)."""
    import linear_svm_cases
    return linear_svm_cases.protocol_variant(False, 16, moved)


@functools.lru_cache(maxsize=None)
def pca_reference(moved=False):
    """rbf_svm_ref on pca_variant: (gamma, decisions of the probes, votes, predicted codes, pairs, bound at eps = 2e-10)."""
    gal, codes, prb, classes = pca_variant(moved)
    K = len(classes)
    g = rbf_svm_ref.gamma_scale(gal)
    dual_coef, rho, pairs, _ = rbf_svm_ref.fit(gal, codes, K, g, tol=1e-12)
    dec = rbf_svm_ref.decision(prb, gal, codes, K, g, dual_coef, rho)
    votes, pred = rbf_svm_ref.votes_of(dec, K)
    return g, dec, votes, pred, pairs, rbf_svm_ref.decision_bound(gal, codes, g, pairs, 2e-10)[0]
