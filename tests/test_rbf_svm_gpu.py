"""GPU suite for the RBF SVM (hsefr_rbf_svm_gamma_scale / _fit / _decision / _predict through ops) and the classifier="rbf_svm" keyword of
the identification protocols, against tests/rbf_svm_ref.py and scikit-learn's recorded tests/golden/rbf_svm.npz: a known answer, the KKT
conditions of every pair recomputed from the device's dual_coef, rho and pair decisions within the derived bound of libsvm's, EQUAL votes
and labels (tests/test_rbf_svm_cpu.py shows that every vote is certain), run-to-run determinism, the iteration cap, label errors, and
the protocols."""
import numpy as np
import pytest

import pca_cases
import rbf_svm_cases as cases
import rbf_svm_ref as ref

pytestmark = pytest.mark.gpu

TOL = 1e-10


@pytest.fixture(scope="module")
def torch_():
    import torch
    assert torch.cuda.is_available()
    return torch


def up(torch_, a, dtype=np.float32):
    return torch_.from_numpy(np.ascontiguousarray(a, dtype=dtype)).cuda()


def device_fit(torch_, x, labels, n_classes, gamma, **kw):
    from hse_facerec_tf_amd import ops
    xd, ld = up(torch_, x), up(torch_, labels, np.int32)
    dual_coef, rho, info = ops.rbf_svm_fit(xd, ld, n_classes, gamma, **kw)
    assert dual_coef.dtype == rho.dtype == torch_.float64
    assert tuple(dual_coef.shape) == (n_classes - 1, x.shape[0]) and tuple(rho.shape) == (n_classes * (n_classes - 1) // 2,)
    return xd, ld, dual_coef, rho, info


@pytest.fixture(scope="module")
def fitted(torch_):
    """Every case fitted once on the device at its recorded gamma and shared, unchanged, by the tests below."""
    memo = {}

    def get(index):
        if index not in memo:
            _, X, labels, K, _ = cases.case(index)
            memo[index] = device_fit(torch_, X, labels, K, float(cases.golden()["c%d_gamma" % index]), tol=TOL)
        return memo[index]
    return get


@pytest.mark.parametrize("C", [1.0, 4.0])
def test_known_answer(torch_, C):
    """Rows 0 and 1 at gamma = ln 2: both a at the bound 1 (C = 1, rho = 0 by the midpoint rule) or free at 2 (C = 4), to 1e-15 relative."""
    from hse_facerec_tf_amd import ops
    X, labels, gamma, a, q, dec_w = cases.known_answer(C)
    xd, ld, dual_coef, rho, info = device_fit(torch_, X, labels, 2, gamma, C=C)
    print(dual_coef.cpu().numpy(), rho.cpu().numpy(), info)
    assert info["converged"] and info["pairs_at_max_iter"] == 0 and info["iterations"] >= 1
    assert np.allclose(dual_coef.cpu().numpy(), [[a, -a]], rtol=1e-15, atol=0)
    assert np.abs(rho.cpu().numpy()).max() <= 1e-15
    dec = ops.rbf_svm_decision(up(torch_, q), xd, ld, 2, gamma, dual_coef, rho)
    assert dec.dtype == torch_.float64 and tuple(dec.shape) == (len(q), 1)
    assert np.allclose(dec.cpu().numpy()[:, 0], dec_w, rtol=1e-15, atol=a * 2.0 ** -52)
    pred, votes = ops.rbf_svm_predict(up(torch_, q), xd, ld, 2, gamma, dual_coef, rho)
    sign = np.where(dec.cpu().numpy()[:, 0] > 0, 0, 1)
    assert pred.dtype == votes.dtype == torch_.int32 and np.array_equal(pred.cpu().numpy(), sign)
    assert np.array_equal(pred.cpu().numpy()[[0, 1, 3, 4]], [0, 1, 0, 1])
    assert np.array_equal(votes.cpu().numpy(), np.stack([1 - sign, sign], axis=1))


@pytest.mark.parametrize("index", range(cases.N_CASES))
def test_every_pair_is_at_its_optimum(torch_, fitted, index):
    """From the device's dual_coef alone: m - M <= 2 TOL on a fresh Q a - e (the second TOL covers the drift of the incrementally updated
    gradient, about iterations x 2^-52), 0 <= a <= C exactly, |y^T a| <= 2^-52 C (iterations + n_i + n_j); rho within the derived bound
    of libsvm's."""
    name, X, labels, K, _ = cases.case(index)
    g, c = cases.golden(), "c%d_" % index
    _, _, dual_coef, rho, info = fitted(index)
    gap, balance, inside = ref.kkt_violation(X, labels, dual_coef.cpu().numpy(), float(g[c + "gamma"]), 1.0)
    sizes = np.bincount(labels)
    rows = np.array([sizes[i] + sizes[j] for i, j in ref.pair_list(K)])
    rho_bound = cases.decision_bound(index, 2.0 * TOL)[1]
    d_rho = float(np.abs(rho.cpu().numpy() - g[c + "rho"]).max())
    print("%s: %s, m - M <= %.2e, |y^T a| <= %.2e, |rho - libsvm's| %.2e (bound %.2e)" % (name, info, gap.max(), balance.max(), d_rho, rho_bound))
    assert info["converged"] and info["pairs_at_max_iter"] == 0
    assert gap.max() <= 2.0 * TOL
    assert inside.all()
    assert np.all(balance <= 2.0 ** -52 * (info["iterations"] + rows))
    assert d_rho <= rho_bound


@pytest.mark.parametrize("index", range(cases.N_CASES))
def test_decisions_votes_and_labels_are_libsvms(torch_, fitted, index):
    """The recorded pair decisions of the first 8 held-out rows within decision_bound(2 TOL); votes and labels EQUAL for every held-out
    row, the tied ones included; predict equals the votes taken from decision."""
    from hse_facerec_tf_amd import ops
    name, X, labels, K, held = cases.case(index)
    g, c = cases.golden(), "c%d_" % index
    gamma = float(g[c + "gamma"])
    xd, ld, dual_coef, rho, _ = fitted(index)
    hd = up(torch_, held)
    dec = ops.rbf_svm_decision(hd, xd, ld, K, gamma, dual_coef, rho).cpu().numpy()
    pred, votes = ops.rbf_svm_predict(hd, xd, ld, K, gamma, dual_coef, rho)
    pred, votes = pred.cpu().numpy(), votes.cpu().numpy()
    bound = cases.decision_bound(index, 2.0 * TOL)[0]
    d_dec = float(np.abs(dec[:cases.DECISION_ROWS][:, cases.recorded_pairs(dec.shape[1])] - g[c + "dec"]).max())
    print("%s: |decision - libsvm's| %.2e (bound %.2e), smallest |decision| %.2e" % (name, d_dec, bound, np.abs(dec).min()))
    assert d_dec <= bound
    votes_w, pred_w = ref.votes_of(dec, K)
    assert np.array_equal(votes, votes_w) and np.array_equal(pred, pred_w)            # predict against the votes taken from decision
    assert np.array_equal(votes, g[c + "votes"]) and np.array_equal(pred, g[c + "pred"])
    alone, none = ops.rbf_svm_predict(hd, xd, ld, K, gamma, dual_coef, rho, return_votes=False)
    assert none is None and np.array_equal(alone.cpu().numpy(), pred)


def test_gamma_scale(torch_):
    """Within 1e-14 relative of NumPy's 1 / (d Var), over the first d_used columns too; 1.0 where the variance is 0."""
    from hse_facerec_tf_amd import ops
    for index in range(cases.N_CASES):
        X = cases.case(index)[1]
        got = ops.rbf_svm_gamma(up(torch_, X))
        assert abs(got / cases.gamma(index) - 1.0) <= 1e-14, (index, got)
        assert abs(got / float(cases.golden()["c%d_gamma" % index]) - 1.0) <= 1e-14
    X = cases.case(2)[1]
    padded = np.pad(X[:, :19], ((0, 0), (0, 5)))
    assert abs(ops.rbf_svm_gamma(up(torch_, padded), 19) / ref.gamma_scale(X[:, :19]) - 1.0) <= 1e-14
    assert ops.rbf_svm_gamma(up(torch_, np.full((7, 8), 3.0))) == 1.0


@pytest.mark.parametrize("index", [2, 3])
def test_two_fits_are_bit_equal(torch_, fitted, index):
    _, X, labels, K, _ = cases.case(index)
    _, _, dual_coef, rho, info = fitted(index)
    _, _, again, rho2, info2 = device_fit(torch_, X, labels, K, float(cases.golden()["c%d_gamma" % index]), tol=TOL)
    assert torch_.equal(dual_coef, again) and torch_.equal(rho, rho2) and info == info2


def test_iteration_cap_is_reported_and_raised(torch_, monkeypatch):
    from hse_facerec_tf_amd import identification
    _, X, labels, K, _ = cases.case(1)
    _, _, _, _, info = device_fit(torch_, X, labels, K, cases.gamma(1), max_iter=1)
    assert info == {"iterations": 1, "converged": False, "pairs_at_max_iter": 3}
    z, Xraw, _ = pca_cases.protocol_fixture()
    g, p = z["gallery"], z["probe"]
    monkeypatch.setattr(identification, "RBF_SVM_MAX_ITER", 1)
    with pytest.raises(RuntimeError, match="short of the optimum after 1 iterations"):
        identification.gallery_probe_identification(Xraw[g], z["y"][g], Xraw[p], z["y"][p], classifier="rbf_svm")


def test_label_errors_are_errors(torch_):
    """A code out of range and a class without a row end the call as ValueError before the solver starts -- in fit, decision and predict."""
    from hse_facerec_tf_amd import ops
    _, X, labels, K, held = cases.case(1)
    xd, hd = up(torch_, X), up(torch_, held)
    dual_coef = torch_.zeros((K - 1, len(labels)), dtype=torch_.float64).cuda()
    rho = torch_.zeros((K * (K - 1) // 2,), dtype=torch_.float64).cuda()
    for bad, word in ((np.where(np.arange(len(labels)) == 5, K, labels), "outside 0..2"), (np.where(np.arange(len(labels)) == 5, -1, labels), "outside"),
                      (np.where(labels == 0, 1, labels), "has no row")):
        ld = up(torch_, bad, np.int32)
        with pytest.raises(ValueError, match=word):
            ops.rbf_svm_fit(xd, ld, K, 0.02)
        with pytest.raises(ValueError, match=word):
            ops.rbf_svm_decision(hd, xd, ld, K, 0.02, dual_coef, rho)
        with pytest.raises(ValueError, match=word):
            ops.rbf_svm_predict(hd, xd, ld, K, 0.02, dual_coef, rho)


@pytest.mark.parametrize("normalize", [False, True])
def test_gallery_probe_protocol(torch_, normalize):
    """gallery_probe_identification(classifier="rbf_svm") reproduces scikit-learn's recorded labels -- and its votes: on the raw features
    the rows reach the device bit for bit; the device's own float32 normalisation moves no vote
    (tests/test_rbf_svm_cpu.py::test_normalised_votes_survive_the_device_normalisation)."""
    from hse_facerec_tf_amd import identification
    z, Xraw, _ = pca_cases.protocol_fixture()
    gi, pi = z["gallery"], z["probe"]
    yg, yp = z["y"][gi], z["y"][pi]
    g, c = cases.golden(), "c%d_" % (5 if normalize else 4)
    classes = np.unique(yg)
    r = identification.gallery_probe_identification(Xraw[gi], yg, Xraw[pi], yp, normalize=normalize, classifier="rbf_svm")
    assert sorted(r) == ["accuracy", "svm_iterations", "votes", "y_pred"]
    print("normalize=%s: %d iterations, accuracy %.4f, votes that differ %d" % (normalize, r["svm_iterations"], r["accuracy"],
                                                                             int((r["votes"] != g[c + "votes"]).sum())))
    assert np.array_equal(r["y_pred"], classes[g[c + "pred"]])
    assert r["votes"].shape == (len(pi), 66) and np.array_equal(r["votes"], g[c + "votes"])
    assert r["accuracy"] == float((classes[g[c + "pred"]] == yp).mean())
    # a number for svm_gamma, and another C
    fixed = identification.gallery_probe_identification(Xraw[gi], yg, Xraw[pi], yp, normalize=normalize, classifier="rbf_svm",
                                                        svm_gamma=float(g[c + "gamma"]))
    assert np.array_equal(fixed["votes"], r["votes"])


def test_gallery_probe_protocol_with_device_pca(torch_):
    """pca="device", pca_components=16 + classifier="rbf_svm" gives pca_ref + rbf_svm_ref's votes and labels, gamma from the 16 projected
    columns (tests/test_rbf_svm_cpu.py::test_pca_variant_votes_are_certain)."""
    from hse_facerec_tf_amd import identification
    z, Xraw, _ = pca_cases.protocol_fixture()
    gi, pi = z["gallery"], z["probe"]
    yg, yp = z["y"][gi], z["y"][pi]
    _, _, votes_w, pred_w, _, _ = cases.pca_reference()
    classes = np.unique(yg)
    r = identification.gallery_probe_identification(Xraw[gi], yg, Xraw[pi], yp, pca_components=16, pca="device", classifier="rbf_svm")
    print("pca 16: %d iterations, votes that differ %d" % (r["svm_iterations"], int((r["votes"] != votes_w).sum())))
    assert np.array_equal(r["y_pred"], classes[pred_w]) and np.array_equal(r["votes"], votes_w)
    assert r["accuracy"] == float((classes[pred_w] == yp).mean())


def test_one_nn_protocol_with_the_rbf_svm(torch_):
    from hse_facerec_tf_amd import identification
    X, y, Xn, y2, train, test = pca_cases.golden_split()
    classes, codes = np.unique(y2[train], return_inverse=True)
    K = len(classes)
    gal, prb = Xn[train].astype(np.float32), Xn[test].astype(np.float32)
    gamma = ref.gamma_scale(gal)
    dual_coef, rho, pairs, _ = ref.fit(gal, codes, K, gamma, tol=1e-12)
    dec_w = ref.decision(prb, gal, codes, K, gamma, dual_coef, rho)
    votes_w, pred_w = ref.votes_of(dec_w, K)
    bound = ref.decision_bound(gal, codes, gamma, pairs, 2.0 * TOL)[0]
    print("smallest |decision| %.2e, bound %.2e" % (np.abs(dec_w).min(), bound))
    assert bound < np.abs(dec_w).min() / 4.0
    timings = {}
    r = identification.one_nn_identification(X, y, classifier="rbf_svm", timings=timings)
    assert sorted(r) == ["accuracy", "indices", "num_classes", "svm_iterations", "test", "train", "votes", "y", "y_pred"]
    assert np.array_equal(r["train"], train) and np.array_equal(r["test"], test)
    assert r["votes"].shape == votes_w.shape and int(r["votes"].sum()) == len(test) * K * (K - 1) // 2
    assert np.array_equal(r["y_pred"], classes[pred_w])
    assert r["accuracy"] == float((classes[pred_w] == y2[test]).mean())
    assert timings["svm_fit_s"] > 0 and timings["svm_predict_s"] > 0 and "nn1_s" not in timings


def test_default_calls_return_the_keys_they_returned_before(torch_):
    from hse_facerec_tf_amd import identification
    z, Xraw, _ = pca_cases.protocol_fixture()
    g, p = z["gallery"], z["probe"]
    r = identification.gallery_probe_identification(Xraw[g], z["y"][g], Xraw[p], z["y"][p])
    assert sorted(r) == ["accuracy", "nn_dist", "nn_index", "y_pred"]
    r = identification.gallery_probe_identification(Xraw[g], z["y"][g], Xraw[p], z["y"][p], classifier="linear_svm")
    assert sorted(r) == ["accuracy", "decision", "svm_iterations", "y_pred"]
    X, y, _, _, _, _ = pca_cases.golden_split()
    timings = {}
    r = identification.one_nn_identification(X, y, timings=timings)
    assert sorted(r) == ["accuracy", "indices", "nn_dist", "nn_index", "num_classes", "test", "train", "y", "y_pred"]
    assert sorted(timings) == ["host_split_s", "nn1_s", "nn1_shape", "normalize_s", "readback_s", "select_s"]


def test_gallery_probe_protocol_without_a_probe(torch_):
    """An empty probe set is fitted on and labels nothing: accuracy nan, as on the other paths."""
    from hse_facerec_tf_amd import identification
    z, Xraw, _ = pca_cases.protocol_fixture()
    g = z["gallery"]
    r = identification.gallery_probe_identification(Xraw[g], z["y"][g], Xraw[:0], z["y"][:0], classifier="rbf_svm")
    assert r["votes"].shape == (0, 66) and len(r["y_pred"]) == 0 and np.isnan(r["accuracy"]) and r["svm_iterations"] >= 1
