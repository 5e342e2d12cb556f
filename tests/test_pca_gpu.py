"""GPU suite for the device PCA (hsefr_pca_fit / hsefr_pca_transform through ops.pca_fit / ops.pca_transform) and the pca="device"
keyword of the identification protocols, against tests/pca_ref.py: a known answer on exact inputs, designed spectra at shapes off every
tile edge, run-to-run determinism, the iteration cap, and the protocols' neighbours -- and all of these again at the block sizes of the
reference's own pca_components=128 (b = 192) up to the largest block (k = 256, b = 384), where the Gram and Rayleigh-Ritz matrices span
several tiles, the one-workgroup kernels use all their waves, and an exact-integer product pins the fp64 MFMA's operand maps."""
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


def check_against_fp64(torch_, name, x, k):
    """Eigenvalues within 1e-9 lambda_1 (ten times the residual bound: an eigenvalue's error is at most its residual), components within
    20 * 1e-10 / gap (an eigenvector's error is at most residual / gap), equal signs, projections within 1e-6 max|Z|, zero padding.
    Returns (gap, components, explained_variance) of the device."""
    from hse_facerec_tf_amd import ops
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
    return gap, comp, var


@pytest.mark.parametrize("case", range(5))
def test_designed_spectra_vs_fp64(torch_, case):
    check_against_fp64(torch_, *_designed_inputs()[case])


def host_residual(x, comp, var):
    """max over i of |C v_i - var_i v_i|_2 / var_0 with C formed in float64 by NumPy from the same float32 rows: the contract's residual
    (at most 1e-10), judged by another hand; the bound on it is doubled for the host's own rounding in C."""
    xc = x.astype(np.float64)
    xc -= xc.mean(axis=0)
    C = xc.T @ xc / (len(x) - 1)
    return float(np.linalg.norm(comp @ C - var[:, None] * comp, axis=1).max() / var[0])


@pytest.mark.parametrize("case", range(len(pca_cases.BLOCK_SHAPES) + 1))
def test_block_shapes_vs_fp64(torch_, case):
    """The same assertions on stepped spectra at b = 11 (capped, odd), 112, 96 = d, 192 (the reference's k = 128), 384 (the largest) and
    192 at d = 1024, and on rows with a mean far above their spread; then two checks that need no gap: the residual against a host-formed
    covariance, and orthogonality within 2e-10 / gap (two eigenvectors with residual eps are orthogonal to 2 eps over the distance of
    their eigenvalues)."""
    name, x, k = pca_cases.block_cases()[case]
    print("b=%d" % pca_cases.block_size(x.shape[0], x.shape[1], k), end=" ")
    gap, comp, var = check_against_fp64(torch_, name, x, k)
    res = host_residual(x, comp, var)
    dots = np.abs(comp @ comp.T - np.diag((comp * comp).sum(1))).max()
    print("    residual %.2e lambda_1 (bound 2e-10), orthogonality %.2e (bound %.2e)" % (res, dots, 2e-10 / gap))
    assert res <= 2e-10
    assert dots <= 2e-10 / gap


def test_known_answer_at_the_whole_space_of_256(torch_):
    """The Hadamard case at 512 x 256 with k = 255: b is capped to d = 256, so the first Rayleigh-Ritz step is the eigen-decomposition
    of a 256 x 256 matrix whose answer no library eigensolver supplied.  Component i lies within 20 * 1e-10 lambda_1 / gap_i of e_{i+1},
    gap_i the distance from eigenvalue i to its nearer neighbour (the zero eigenvalue of the constant column included)."""
    from hse_facerec_tf_amd import ops
    x, s = pca_cases.hadamard_case(512, 256)
    xd, mean, comp, var, info = device_fit(torch_, x, 255)
    mean, comp, var = mean.cpu().numpy(), comp.cpu().numpy(), var.cpu().numpy()
    want_mean = np.zeros(256)
    want_mean[0] = 256.0
    lam = np.append(s[1:] ** 2 * 512.0 / 511.0, 0.0)
    gaps = np.minimum(np.append(np.inf, lam[:-2] - lam[1:-1]), lam[:-1] - lam[1:])
    err = np.abs(comp - np.eye(256)[1:]).max(axis=1)
    print("b=256, %d iterations, eigenvalues %.2e lambda_1, components: largest error / bound %.2e, largest error %.2e"
          % (info["iterations"], np.abs(var - lam[:-1]).max() / lam[0], (err / (20 * 1e-10 * lam[0] / gaps)).max(), err.max()))
    assert info["converged"]
    assert np.array_equal(mean, want_mean)
    assert np.abs(var - lam[:-1]).max() <= 1e-9 * lam[0]
    assert np.all(err <= 20 * 1e-10 * lam[0] / gaps)
    z = ops.pca_transform(xd, torch_.from_numpy(mean).cuda(), torch_.from_numpy(comp).cuda()).cpu().numpy()
    assert z.shape == (512, 256) and z.dtype == np.float32
    want_z = x[:, 1:]                                           # the centred columns 1..255 (their mean is zero)
    assert np.all(np.abs(z[:, :255] - want_z) <= np.spacing(np.abs(want_z)))
    assert np.all(z[:, 255] == 0)


@pytest.mark.parametrize("n,d,k", [(1, 8, 1), (33, 24, 5), (70, 264, 129), (65, 1024, 256)])
def test_transform_operand_maps_with_exact_integers(torch_, n, d, k):
    """components[j][c] = 131 c + 7 j + 1 (asymmetric), an integer mean, and rows mean + e_(i mod d) + 2 e_((5 i + 3) mod d): every
    product and sum is an integer below 2^24, so any row / column / k-slot mix-up in the f64 MFMA's lane map, at the contraction's tail
    or at a partial row or column tile gives an exactly wrong integer.  One tile; a 24-long contraction and partial row tile; ldz = 136,
    three column tiles with the last partial; the largest k at the real feature width."""
    from hse_facerec_tf_amd import ops
    comp = 131 * np.arange(d)[None, :] + 7 * np.arange(k)[:, None] + 1
    mean = np.arange(d) % 13 - 6
    sel = np.zeros((n, d), np.int64)
    sel[np.arange(n), np.arange(n) % d] += 1
    sel[np.arange(n), (5 * np.arange(n) + 3) % d] += 2
    want = sel @ comp.T
    assert want.max() < 2 ** 24
    x = (sel + mean).astype(np.float32)
    z = ops.pca_transform(torch_.from_numpy(x).cuda(), torch_.from_numpy(mean.astype(np.float64)).cuda(),
                          torch_.from_numpy(comp.astype(np.float64)).cuda()).cpu().numpy()
    assert z.shape == (n, (k + 7) // 8 * 8) and z.dtype == np.float32
    assert np.array_equal(z[:, :k].astype(np.int64), want) and np.array_equal(z[:, :k], np.rint(z[:, :k]))
    assert np.all(z[:, k:] == 0)


def test_two_fits_are_bit_equal(torch_):
    x = pca_cases.designed_spectrum(300, 72, 40)
    a, b = device_fit(torch_, x, 40), device_fit(torch_, x, 40)
    for i in (1, 2, 3):
        assert torch_.equal(a[i], b[i])
    assert a[4] == b[4]


def test_two_fits_are_bit_equal_at_the_protocol_block(torch_):
    """k = 128, b = 192: several Gram tiles, three waves of Cholesky columns, six trips of the Jacobi kernel's waves per step."""
    x = pca_cases.stepped_spectrum(300, 200, 128)
    a, b = device_fit(torch_, x, 128), device_fit(torch_, x, 128)
    for i in (1, 2, 3):
        assert torch_.equal(a[i], b[i])
    assert a[4] == b[4] and a[4]["converged"]


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


def test_gallery_probe_protocol_at_the_reference_k(torch_):
    """The same at the reference's own pca_components=128 (facerec_test.py:417) on the raw gallery, 170 x 256: b is capped at 169, an odd
    size, so the Jacobi schedule has its dummy.  tests/test_pca_cpu.py shows the 4e-5 margin there.  The gallery's own gap is 2e-4, so
    the components are judged by their residual against a host-formed covariance, which needs no gap."""
    from hse_facerec_tf_amd import identification
    k = 128
    z, Xraw, _ = pca_cases.protocol_fixture()
    g, p = z["gallery"], z["probe"]
    yg, yp = z["y"][g], z["y"][p]
    mean, comp, _ = pca_ref.fit(Xraw[g], k)
    zg, zp = pca_ref.transform(Xraw[g], mean, comp), pca_ref.transform(Xraw[p], mean, comp)
    for nn in (1, 3):
        want_idx, _, want_pred = knn_ref.knn(zp, zg, nn, yg)
        r = identification.gallery_probe_identification(Xraw[g], yg, Xraw[p], yp, normalize=False, pca_components=k, pca="device",
                                                        n_neighbors=nn)
        got_idx = r["nn_index"] if nn > 1 else r["nn_index"][:, None]
        assert np.array_equal(got_idx, want_idx)
        assert np.array_equal(r["y_pred"], want_pred)
        assert r["accuracy"] == float((want_pred == yp).mean())
    _, _, dcomp, dvar, info = device_fit(torch_, Xraw[g], k)
    res = host_residual(Xraw[g], dcomp.cpu().numpy(), dvar.cpu().numpy())
    print("b=%d, %d iterations, residual %.2e lambda_1 (bound 2e-10)" % (pca_cases.block_size(170, 256, k), info["iterations"], res))
    assert info["converged"] and res <= 2e-10


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
