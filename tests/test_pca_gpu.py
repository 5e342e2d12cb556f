"""GPU suite for the device PCA (hsefr_pca_fit / hsefr_pca_transform through ops.pca_fit / ops.pca_transform) and the pca="device"
keyword of the identification protocols, against tests/pca_ref.py: a known answer on exact inputs, designed spectra at shapes off every
tile edge, run-to-run determinism, the iteration cap, and the protocols' neighbours."""
import numpy as np
import pytest

import knn_ref
import pca_cases
import pca_ref

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def torch_():
    import torch
    assert torch.cuda.is_available()
    return torch


def device_fit(torch_, x, k, **kw):
    from hse_facerec_tf_amd import ops
    xd = torch_.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).cuda()
    mean, comp, var, info = ops.pca_fit(xd, k, **kw)
    assert mean.dtype == comp.dtype == var.dtype == torch_.float64
    assert tuple(mean.shape) == (x.shape[1],) and tuple(comp.shape) == (k, x.shape[1]) and tuple(var.shape) == (k,)
    return xd, mean, comp, var, info


def test_known_answer_on_exact_input(torch_):
    """The Hadamard case: mean (32, 0, ..., 0) exactly, explained_variance[i] = s[i+1]^2 64 / 63, component i = +e_{i+1}, and the
    projection is the centred column itself.  k = 31 = d - 1 makes the block the whole space (b = d = 32) although the covariance has
    rank 31: the constant column must not break the orthonormalisation."""
    from hse_facerec_tf_amd import ops
    x, s = pca_cases.hadamard_case()
    xd, mean, comp, var, info = device_fit(torch_, x, 31)
    assert info["converged"]
    want_mean = np.zeros(32)
    want_mean[0] = 32.0
    assert np.array_equal(mean.cpu().numpy(), want_mean)
    want_var = s[1:] ** 2 * 64.0 / 63.0
    rel = np.abs(var.cpu().numpy() - want_var) / want_var
    print("iterations %d, eigenvalues: max relative error %.2e" % (info["iterations"], rel.max()))
    assert rel.max() <= 1e-12
    want_comp = np.eye(32)[1:]
    print("components: max error %.2e" % np.abs(comp.cpu().numpy() - want_comp).max())
    assert np.abs(comp.cpu().numpy() - want_comp).max() <= 1e-9
    z = ops.pca_transform(xd, mean, comp).cpu().numpy()
    assert z.shape == (64, 32) and z.dtype == np.float32
    want_z = x[:, 1:].astype(np.float32)                        # the centred columns 1..31 (their mean is zero)
    assert np.all(np.abs(z[:, :31] - want_z) <= np.spacing(np.abs(want_z)))
    assert np.all(z[:, 31] == 0)


def _designed_inputs():
    cases = [("designed %d x %d" % (n, d), pca_cases.designed_spectrum(n, d, k), k) for n, d, k in pca_cases.DESIGNED_SHAPES]
    z, Xraw, _ = pca_cases.protocol_fixture()
    return cases + [("protocols.npz gallery", Xraw[z["gallery"]], 16)]


@pytest.mark.parametrize("case", range(5))
def test_designed_spectra_vs_fp64(torch_, case):
    """Eigenvalues within 1e-9 lambda_1 (ten times the residual bound: an eigenvalue's error is at most its residual), components within
    20 * 1e-10 / gap (an eigenvector's error is at most residual / gap), equal signs, projections within 1e-6 max|Z|, zero padding."""
    from hse_facerec_tf_amd import ops
    name, x, k = _designed_inputs()[case]
    n, d = x.shape
    gap = pca_cases.relative_gap(x, k)
    assert gap >= 1e-3, "the fixture drifted: relative eigenvalue gap %.2e" % gap
    mean_w, comp_w, var_w = pca_ref.fit(x, k)
    xd, mean, comp, var, info = device_fit(torch_, x, k)
    mean, comp, var = mean.cpu().numpy(), comp.cpu().numpy(), var.cpu().numpy()
    z = ops.pca_transform(xd, torch_.from_numpy(mean).cuda(), torch_.from_numpy(comp).cuda()).cpu().numpy()
    z_w = pca_ref.transform(x, mean_w, comp_w)
    ld = (k + 7) // 8 * 8
    print("%s k=%d: gap %.2e, %d iterations, eigenvalues %.2e lambda_1, components %.2e (bound %.2e), Z %.2e max|Z|"
          % (name, k, gap, info["iterations"], np.abs(var - var_w).max() / var_w[0], np.abs(comp - comp_w).max(), 20 * 1e-10 / gap,
             np.abs(z[:, :k] - z_w).max() / np.abs(z_w).max()))
    assert info["converged"] and 1 <= info["iterations"] <= 1000
    assert np.abs(mean - mean_w).max() <= 1e-13 * max(np.abs(mean_w).max(), np.abs(x).max())
    assert np.abs(var - var_w).max() <= 1e-9 * var_w[0]
    assert np.abs(comp - comp_w).max() <= 20 * 1e-10 / gap
    lead = np.argmax(np.abs(comp_w), axis=1)
    assert np.array_equal(np.sign(comp[np.arange(k), lead]), np.sign(comp_w[np.arange(k), lead])) and np.all(comp[np.arange(k), lead] > 0)
    assert np.abs((comp * comp).sum(1) - 1.0).max() <= 1e-12
    assert z.shape == (n, ld) and z.dtype == np.float32
    assert np.abs(z[:, :k] - z_w).max() <= 1e-6 * np.abs(z_w).max()
    assert np.all(z[:, k:] == 0)


def test_two_fits_are_bit_equal(torch_):
    x = pca_cases.designed_spectrum(300, 72, 40)
    a, b = device_fit(torch_, x, 40), device_fit(torch_, x, 40)
    for i in (1, 2, 3):
        assert torch_.equal(a[i], b[i])
    assert a[4] == b[4]


def test_iteration_cap_is_reported_and_raised(torch_, monkeypatch):
    from hse_facerec_tf_amd import identification
    z, Xraw, _ = pca_cases.protocol_fixture()
    g, p = z["gallery"], z["probe"]
    _, _, _, _, info = device_fit(torch_, Xraw[g], 16, max_iter=1)
    assert info == {"iterations": 1, "converged": False}
    monkeypatch.setattr(identification, "PCA_MAX_ITER", 1)
    with pytest.raises(RuntimeError, match="did not converge in 1 iterations"):
        identification.gallery_probe_identification(Xraw[g], z["y"][g], Xraw[p], z["y"][p], pca_components=16, pca="device")


@pytest.mark.parametrize("normalize", [False, True])
@pytest.mark.parametrize("k", [16, 20])
def test_gallery_probe_protocol_with_device_pca(torch_, k, normalize):
    """gallery_probe_identification(pca="device") finds pca_ref + knn_ref's neighbours and predictions exactly, for 1 and 3 neighbours:
    tests/test_pca_cpu.py shows a margin of 4e-5 between any two of a probe's five nearest rows, the device's error is of order 1e-7."""
    from hse_facerec_tf_amd import identification
    z, Xraw, Xn = pca_cases.protocol_fixture()
    A = Xn if normalize else Xraw
    g, p = z["gallery"], z["probe"]
    yg, yp = z["y"][g], z["y"][p]
    mean, comp, _ = pca_ref.fit(A[g], k)
    zg, zp = pca_ref.transform(A[g], mean, comp), pca_ref.transform(A[p], mean, comp)
    for nn in (1, 3):
        want_idx, _, want_pred = knn_ref.knn(zp, zg, nn, yg)
        r = identification.gallery_probe_identification(Xraw[g], yg, Xraw[p], yp, normalize=normalize, pca_components=k, pca="device",
                                                        n_neighbors=nn)
        got_idx = r["nn_index"] if nn > 1 else r["nn_index"][:, None]
        assert np.array_equal(got_idx, want_idx)
        assert np.array_equal(r["y_pred"], want_pred)
        assert r["accuracy"] == float((want_pred == yp).mean())


def test_one_nn_protocol_with_device_pca(torch_):
    from hse_facerec_tf_amd import identification
    X, y, Xn, y2, train, test = pca_cases.golden_split()
    mean, comp, _ = pca_ref.fit(Xn[train], 16)
    want_idx, _, want_pred = knn_ref.knn(pca_ref.transform(Xn[test], mean, comp), pca_ref.transform(Xn[train], mean, comp), 1, y2[train])
    timings = {}
    r = identification.one_nn_identification(X, y, pca_components=16, pca="device", timings=timings)
    assert np.array_equal(r["train"], train) and np.array_equal(r["test"], test)
    assert np.array_equal(r["nn_index"], want_idx[:, 0])
    assert np.array_equal(r["y_pred"], want_pred)
    assert r["accuracy"] == float((want_pred == y2[test]).mean())
    assert timings["pca_s"] > 0 and timings["nn1_shape"] == (len(test), len(train), 16)
    host = {}
    identification.one_nn_identification(X, y, pca_components=16, timings=host)
    assert "pca_s" not in host                                  # the host path's keys stay what they were
