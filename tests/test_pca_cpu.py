"""CPU suite for the device PCA (hsefr_pca_fit / hsefr_pca_transform): tests/pca_ref.py against scikit-learn's exact solver, the entry
points' place in the ABI, their argument checks and those of the Python entry points (all before any device work), and the properties
of the fixtures that the GPU suite relies on -- eigenvalue gaps and neighbour margins."""
import ctypes
import os

import numpy as np
import pytest

import knn_ref
import pca_cases
import pca_ref

from conftest import GOLDEN

PROTOCOL_CASES = [(False, 16), (False, 20), (True, 16), (True, 20)]


@pytest.mark.parametrize("normalised,k", PROTOCOL_CASES)
def test_restatement_equals_sklearn_full_solver(normalised, k):
    """PCA(svd_solver="full") on the float64 copy of the gallery is the exact answer in another formulation (an SVD of the centred rows).
    Measured: 1.6e-13 of max|Z| in the projections, 3e-15 lambda_1 in the eigenvalues."""
    from sklearn.decomposition import PCA
    z, Xraw, Xn = pca_cases.protocol_fixture()
    A = (Xn if normalised else Xraw).astype(np.float64)
    g, p = z["gallery"], z["probe"]
    assert A[g].shape == (170, 256)
    want = PCA(n_components=k, svd_solver="full").fit(A[g])
    mean, comp, var = pca_ref.fit(A[g], k)
    assert np.abs(mean - want.mean_).max() <= 1e-14 * np.abs(want.mean_).max()
    assert np.abs(var - want.explained_variance_).max() <= 1e-12 * var[0]
    assert np.all(np.diff(var) < 0)
    assert np.abs(np.abs(comp) - np.abs(want.components_)).max() <= 1e-9
    assert np.array_equal(np.sign(comp), np.sign(want.components_))
    for rows in (g, p):
        Z, Zw = pca_ref.transform64(A[rows], mean, comp), want.transform(A[rows])
        assert np.abs(Z - Zw).max() <= 1e-12 * np.abs(Zw).max()
        assert np.array_equal(Z.astype(np.float32), Zw.astype(np.float32))
    assert np.array_equal(pca_ref.transform(A[p], mean, comp), pca_ref.transform64(A[p], mean, comp).astype(np.float32))


def test_restatement_sign_rule_takes_the_first_largest_entry():
    x = np.array([[1.0, -1.0], [-1.0, 1.0], [1.0, -1.0], [-1.0, 1.0]])            # the component is +-(1, -1) / sqrt 2: a tie in magnitude
    _, comp, var = pca_ref.fit(x, 1)
    assert comp[0, 0] > 0 and comp[0, 1] < 0 and var[0] == pytest.approx(8.0 / 3.0)


def test_pca_is_declared_exported_and_bound():
    from hse_facerec_tf_amd import _lib
    header = open(os.path.join(os.path.dirname(GOLDEN), os.pardir, "include", "hsefr.h")).read()
    flat = " ".join(header.split())
    assert ("int hsefr_pca_fit(const float* x, int n, int d, int k, int max_iter, double* mean, double* components, "
            "double* explained_variance, int* info /* [2]: iterations, converged */, hsefr_stream_t stream);") in flat
    assert ("int hsefr_pca_transform(const float* x, int n, int d, int k, const double* mean, const double* components, float* z, "
            "int ldz, hsefr_stream_t stream);") in flat
    assert "+PCA" in header[:header.index("#ifndef HSEFR_H")]
    assert len(_lib.SIGNATURES["hsefr_pca_fit"][1]) == 10 and len(_lib.SIGNATURES["hsefr_pca_transform"][1]) == 9
    L = _lib.lib()
    assert hasattr(L, "hsefr_pca_fit") and hasattr(L, "hsefr_pca_transform")
    assert L.hsefr_version() == 141


def test_pca_rejects_bad_arguments_without_a_gpu():
    from hse_facerec_tf_amd import _lib
    L = _lib.lib()
    buf = ctypes.create_string_buffer(256)
    p = ctypes.cast(buf, ctypes.c_void_p).value
    fit_ok = dict(x=p, n=40, d=16, k=5, max_iter=10, mean=p, comp=p, var=p, info=p)
    tr_ok = dict(x=p, n=40, d=16, k=5, mean=p, comp=p, z=p, ldz=8)

    def fit(**kw):
        a = dict(fit_ok, **kw)
        rc = L.hsefr_pca_fit(a["x"], a["n"], a["d"], a["k"], a["max_iter"], a["mean"], a["comp"], a["var"], a["info"], None)
        return rc, _lib.last_error()

    def transform(**kw):
        a = dict(tr_ok, **kw)
        rc = L.hsefr_pca_transform(a["x"], a["n"], a["d"], a["k"], a["mean"], a["comp"], a["z"], a["ldz"], None)
        return rc, _lib.last_error()

    for call, name, kw, code, words in (
            (fit, "hsefr_pca_fit", dict(x=None), _lib.ERR_INVALID, ("null pointer",)),
            (fit, "hsefr_pca_fit", dict(mean=None), _lib.ERR_INVALID, ("null pointer",)),
            (fit, "hsefr_pca_fit", dict(comp=None), _lib.ERR_INVALID, ("null pointer",)),
            (fit, "hsefr_pca_fit", dict(var=None), _lib.ERR_INVALID, ("null pointer",)),
            (fit, "hsefr_pca_fit", dict(info=None), _lib.ERR_INVALID, ("null pointer",)),
            (fit, "hsefr_pca_fit", dict(n=1, k=1), _lib.ERR_INVALID, ("n=1",)),
            (fit, "hsefr_pca_fit", dict(k=0), _lib.ERR_INVALID, ("k=0", "n=40", "d=16")),
            (fit, "hsefr_pca_fit", dict(k=17), _lib.ERR_INVALID, ("k=17", "d=16")),
            (fit, "hsefr_pca_fit", dict(n=6, k=6), _lib.ERR_INVALID, ("k=6", "n=6")),               # k = n: not even n - 1
            (fit, "hsefr_pca_fit", dict(n=1000, d=512, k=257), _lib.ERR_INVALID, ("k=257", "256")),
            (fit, "hsefr_pca_fit", dict(max_iter=0), _lib.ERR_INVALID, ("max_iter=0",)),
            (fit, "hsefr_pca_fit", dict(d=12), _lib.ERR_UNSUPPORTED, ("d=12", "multiple of 8")),
            (transform, "hsefr_pca_transform", dict(x=None), _lib.ERR_INVALID, ("null pointer",)),
            (transform, "hsefr_pca_transform", dict(z=None), _lib.ERR_INVALID, ("null pointer",)),
            (transform, "hsefr_pca_transform", dict(mean=None), _lib.ERR_INVALID, ("null pointer",)),
            (transform, "hsefr_pca_transform", dict(comp=None), _lib.ERR_INVALID, ("null pointer",)),
            (transform, "hsefr_pca_transform", dict(k=0), _lib.ERR_INVALID, ("k=0", "d=16")),
            (transform, "hsefr_pca_transform", dict(k=17, ldz=24), _lib.ERR_INVALID, ("k=17", "d=16")),
            (transform, "hsefr_pca_transform", dict(n=-1), _lib.ERR_INVALID, ("n=-1",)),
            (transform, "hsefr_pca_transform", dict(k=9, ldz=8), _lib.ERR_INVALID, ("ldz=8", "k=9")),
            (transform, "hsefr_pca_transform", dict(ldz=12), _lib.ERR_INVALID, ("ldz=12", "multiple of 8")),
            (transform, "hsefr_pca_transform", dict(d=12), _lib.ERR_UNSUPPORTED, ("d=12", "multiple of 8"))):
        rc, msg = call(**kw)
        assert rc == code, (name, kw, rc, msg)
        assert all(w in msg for w in words), (name, kw, msg)
        with pytest.raises(NotImplementedError if code == _lib.ERR_UNSUPPORTED else ValueError):
            _lib.check(rc, name)
    assert transform(n=0)[0] == 0
    assert transform(n=0, x=None, mean=None, comp=None, z=None)[0] == 0
    assert transform(n=0, ldz=4)[0] == _lib.ERR_INVALID                                # an empty set does not excuse a bad ldz


def test_python_entry_points_reject_bad_pca_arguments_without_a_gpu():
    import torch
    from hse_facerec_tf_amd import identification, ops
    for k in (0, -1, 257, 2.0, True):
        with pytest.raises(ValueError, match="pca_components"):
            ops.check_pca_components(k, 1000, 512)
    with pytest.raises(ValueError, match="exceeds n - 1"):
        ops.check_pca_components(6, 6, 16)
    with pytest.raises(ValueError, match="exceeds the 16 features"):
        ops.check_pca_components(17, 100, 16)
    assert ops.check_pca_components(5, 6, 16) == 5 and ops.check_pca_components(np.int64(16), 100, 16) == 16
    x = torch.zeros((6, 16))
    with pytest.raises(ValueError, match="pca_components"):
        ops.pca_fit(x, 6)
    with pytest.raises(ValueError, match="max_iter"):
        ops.pca_fit(x, 3, max_iter=0)
    X = np.zeros((6, 8), np.float32)
    y = np.array([0, 0, 1, 1, 2, 2])
    for mode in ("nonsense", None, "Device"):
        with pytest.raises(ValueError, match="pca="):
            identification.gallery_probe_identification(X, y, X, y, pca_components=2, pca=mode)
        with pytest.raises(ValueError, match="pca="):
            identification.one_nn_identification(X, y, pca_components=2, pca=mode)
    with pytest.raises(ValueError, match="pca_components"):
        identification.gallery_probe_identification(X, y, X, y, pca_components=6, pca="device")
    with pytest.raises(ValueError, match="pca_components"):
        identification.one_nn_identification(X, y, pca_components=300, pca="device")


@pytest.mark.parametrize("n,d,k", pca_cases.DESIGNED_SHAPES)
def test_designed_spectra_keep_their_gaps(n, d, k):
    """The GPU suite's component bound is 20 * 1e-10 / gap: the gap is a property of the seeded inputs, measured 2e-3 to 1e-1."""
    assert pca_cases.relative_gap(pca_cases.designed_spectrum(n, d, k), k) >= 1e-3


@pytest.mark.parametrize("case", range(len(pca_cases.BLOCK_SHAPES) + 1))
def test_stepped_spectra_keep_their_gaps(case):
    """The same precondition at the block sizes of the protocol's own k, where 0.95^i leaves no gap: by construction 1 / 2k of lambda_1,
    measured 5.56e-2, 7.14e-3, 6.25e-3, 3.91e-3, 1.95e-3, 3.91e-3, and 3.90e-3 for the large-mean case, which has no negative entry."""
    name, x, k = pca_cases.block_cases()[case]
    gap = pca_cases.relative_gap(x, k)
    print("%s k=%d b=%d: gap %.2e" % (name, k, pca_cases.block_size(x.shape[0], x.shape[1], k), gap))
    assert gap >= 1e-3
    if case == len(pca_cases.BLOCK_SHAPES):
        assert x.min() > 0 and x.mean() >= 100 * (x - x.mean(axis=0)).std()


def test_protocol_gallery_keeps_its_gap():
    z, Xraw, _ = pca_cases.protocol_fixture()
    assert pca_cases.relative_gap(Xraw[z["gallery"]], 16) >= 1e-3


@pytest.mark.parametrize("normalised,k", PROTOCOL_CASES)
def test_fixture_neighbour_margins_and_sklearn_pipeline(normalised, k):
    """The precondition of the GPU suite's protocol test: in the pca_ref projections no probe has two of its five nearest gallery rows
    closer together than 4e-5 of the fifth squared distance (measured 1.0e-4, 5.1e-5, 4.9e-5, 6.2e-4), so an error of order 1e-7 moves no
    neighbour -- and scikit-learn's own float32 pipeline, a hundred times less accurate than the device, already finds the same ones."""
    from sklearn.decomposition import PCA
    from sklearn.neighbors import KNeighborsClassifier
    from sklearn.pipeline import Pipeline
    z, Xraw, Xn = pca_cases.protocol_fixture()
    A = Xn if normalised else Xraw
    g, p = z["gallery"], z["probe"]
    yg = z["y"][g]
    mean, comp, _ = pca_ref.fit(A[g], k)
    zg, zp = pca_ref.transform(A[g], mean, comp), pca_ref.transform(A[p], mean, comp)
    margin = pca_ref.neighbour_margin(zp, zg)
    print("normalised=%s k=%d: margin %.2e" % (normalised, k, margin))
    assert margin >= 4e-5
    for nn in (1, 3):
        pipe = Pipeline(steps=[("pca", PCA(n_components=k)), ("classifier", KNeighborsClassifier(n_neighbors=nn, p=2))]).fit(A[g], yg)
        idx, _, pred = knn_ref.knn(zp, zg, nn, yg)
        _, want_idx = pipe.named_steps["classifier"].kneighbors(pipe.named_steps["pca"].transform(A[p]))
        assert np.array_equal(idx, want_idx)
        assert np.array_equal(pred, pipe.predict(A[p]))


def test_golden_split_neighbour_margin():
    """The same precondition for one_nn_identification(pca_components=16) on the stratified half split of tests/golden/nn1.npz: the
    nearest and the second nearest gallery row of every probe (n_neighbors = 1 reads no further) are further apart than 4e-5 of the
    second squared distance."""
    _, _, Xn, _, train, test = pca_cases.golden_split()
    mean, comp, _ = pca_ref.fit(Xn[train], 16)
    margin = pca_ref.neighbour_margin(pca_ref.transform(Xn[test], mean, comp), pca_ref.transform(Xn[train], mean, comp), first=2)
    print("golden split: margin %.2e" % margin)
    assert margin >= 4e-5


def test_raw_gallery_at_the_reference_k():
    """k = 128 (facerec_test.py:417) on the raw gallery, 170 x 256, so the block is capped at b = 169, an odd size: the restatement
    agrees with PCA(svd_solver="full") on the float64 copy (measured 3.2e-15 lambda_1, 7.0e-14, 1.2e-13 max|Z|), the neighbour margin
    is over the 4e-5 floor (measured 6.19e-5) and scikit-learn's pipeline finds the same neighbours.  The normalised gallery is left out:
    its margin at k = 128 is 2.49e-5."""
    from sklearn.decomposition import PCA
    from sklearn.neighbors import KNeighborsClassifier
    from sklearn.pipeline import Pipeline
    k = 128
    z, Xraw, _ = pca_cases.protocol_fixture()
    g, p = z["gallery"], z["probe"]
    yg = z["y"][g]
    assert Xraw[g].shape == (170, 256) and pca_cases.block_size(170, 256, k) == 169
    A = Xraw.astype(np.float64)
    want = PCA(n_components=k, svd_solver="full").fit(A[g])
    mean, comp, var = pca_ref.fit(A[g], k)
    assert np.abs(var - want.explained_variance_).max() <= 1e-12 * var[0]
    assert np.abs(np.abs(comp) - np.abs(want.components_)).max() <= 1e-9
    assert np.array_equal(np.sign(comp), np.sign(want.components_))
    for rows in (g, p):
        Z, Zw = pca_ref.transform64(A[rows], mean, comp), want.transform(A[rows])
        assert np.abs(Z - Zw).max() <= 1e-12 * np.abs(Zw).max()
    zg, zp = pca_ref.transform(Xraw[g], mean, comp), pca_ref.transform(Xraw[p], mean, comp)
    margin = pca_ref.neighbour_margin(zp, zg)
    print("raw gallery k=%d: eigenvalues %.1e lambda_1, components %.1e, margin %.2e"
          % (k, np.abs(var - want.explained_variance_).max() / var[0], np.abs(np.abs(comp) - np.abs(want.components_)).max(), margin))
    assert margin >= 4e-5
    for nn in (1, 3):
        pipe = Pipeline(steps=[("pca", PCA(n_components=k)), ("classifier", KNeighborsClassifier(n_neighbors=nn, p=2))]).fit(Xraw[g], yg)
        idx, _, pred = knn_ref.knn(zp, zg, nn, yg)
        _, want_idx = pipe.named_steps["classifier"].kneighbors(pipe.named_steps["pca"].transform(Xraw[p]))
        assert np.array_equal(idx, want_idx)
        assert np.array_equal(pred, pipe.predict(Xraw[p]))
