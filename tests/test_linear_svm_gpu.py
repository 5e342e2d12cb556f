"""GPU suite for the linear SVM (hsefr_linear_svm_fit / _decision / _predict through ops) and the classifier="linear_svm" keyword of the
identification protocols, against tests/linear_svm_ref.py and the recorded tests/golden/linear_svm.npz: a known answer on exact inputs,
designed cases at shapes off every tile edge, run-to-run determinism, the iteration cap, the tie rules of predict, and the protocols.
Every tolerance follows from |w~ - w~*| <= |grad f_k(w~)| (the objective is 1-strongly convex); tests/test_linear_svm_cpu.py shows that
the fixtures' margins carry the exact comparisons of predictions."""
import numpy as np
import pytest

import linear_svm_cases as cases
import linear_svm_ref as ref
import pca_cases

pytestmark = pytest.mark.gpu

TOL = 1e-10


@pytest.fixture(scope="module")
def torch_():
    import torch
    assert torch.cuda.is_available()
    return torch


def device_fit(torch_, x, labels, n_classes, **kw):
    from hse_facerec_tf_amd import ops
    xd = torch_.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).cuda()
    ld = torch_.from_numpy(np.ascontiguousarray(labels, dtype=np.int32)).cuda()
    coef, intercept, info = ops.linear_svm_fit(xd, ld, n_classes, **kw)
    rows = 1 if n_classes == 2 else n_classes
    assert coef.dtype == intercept.dtype == torch_.float64
    assert tuple(coef.shape) == (rows, x.shape[1]) and tuple(intercept.shape) == (rows,)
    return xd, coef, intercept, info


def test_known_answer_on_exact_input(torch_):
    from hse_facerec_tf_amd import ops
    X, labels, C, coef_w, intercept_w, dec_w = cases.known_answer()
    xd, coef, intercept, info = device_fit(torch_, X, labels, 2, C=C)
    print(coef.cpu().numpy(), intercept.cpu().numpy(), info)
    assert info["converged"] and info["iterations"] >= 1 and info["hessian_products"] >= 1
    assert np.abs(coef.cpu().numpy() - coef_w).max() <= 1e-15
    assert np.abs(intercept.cpu().numpy() - intercept_w).max() <= 1e-15
    dec = ops.linear_svm_decision(xd, coef, intercept)
    assert dec.dtype == torch_.float64 and tuple(dec.shape) == (2, 1)
    assert np.abs(dec.cpu().numpy() - dec_w).max() <= 1e-15
    pred = ops.linear_svm_predict(dec)
    assert pred.dtype == torch_.int32 and pred.cpu().tolist() == [1, 0]


@pytest.mark.parametrize("index", range(cases.N_CASES))
def test_designed_cases_vs_fp64(torch_, index):
    """The returned (coef, intercept) has |grad f_k| <= 2 TOL |grad f_k(0)| for every class (evaluated by linear_svm_ref.gradient; the
    factor 2 covers the other summation order), lies within |grad f_k(device)| + |grad f_k(reference)| of the reference's row, gives
    held-out decisions within that times |x~|, and the same predictions wherever the reference's top-two gap exceeds twice that --
    which leaves out at most 1 % of the rows (none, by the reference alone: tests/test_linear_svm_cpu.py).  The last case has 601
    classes: two of the library's class blocks, the second one shorter."""
    from hse_facerec_tf_amd import ops
    name, X, labels, K, held = cases.case(index)
    coef_w, intercept_w, _ = cases.reference(index)
    W_w = ref.pack(coef_w, intercept_w)
    xd, coef, intercept, info = device_fit(torch_, X, labels, K)
    W = ref.pack(coef.cpu().numpy(), intercept.cpu().numpy())
    g0 = np.sqrt((ref.gradient(np.zeros_like(W), X, labels, K) ** 2).sum(1))
    g_dev = np.sqrt((ref.gradient(W, X, labels, K) ** 2).sum(1))
    g_ref = np.sqrt((ref.gradient(W_w, X, labels, K) ** 2).sum(1))
    bound = g_dev + g_ref                                        # per class, on |w~ - w~ref|
    dist = np.sqrt(((W - W_w) ** 2).sum(1))
    hd = torch_.from_numpy(held).cuda()
    dec = ops.linear_svm_decision(hd, coef, intercept)
    pred = ops.linear_svm_predict(dec).cpu().numpy()
    dec = dec.cpu().numpy()
    dec_w = ref.decision(held, coef_w, intercept_w)
    xnorm = np.sqrt((held.astype(np.float64) ** 2).sum(1) + 1.0)
    print("%s: %d iterations, %d Hessian products, max |grad| / |grad(0)| %.2e, max |w - wref| %.2e (bound %.2e), decisions %.2e (bound %.2e)"
          % (name, info["iterations"], info["hessian_products"], (g_dev / g0).max(), dist.max(), bound.max(), np.abs(dec - dec_w).max(),
             (bound[None, :] * xnorm[:, None]).max()))
    assert info["converged"] and 1 <= info["iterations"] <= 1000
    assert np.all(g_dev <= 2.0 * TOL * g0)
    assert np.all(dist <= bound)
    assert np.all(np.abs(dec - dec_w) <= bound[None, :] * xnorm[:, None])
    sure = ref.top_two_gap(dec_w) > 2.0 * bound.max() * xnorm
    assert (~sure).mean() <= 0.01
    assert np.array_equal(pred[sure], ref.predict(dec_w)[sure])
    assert np.array_equal(pred, ref.predict(dec))               # the device's arg-max of its own decisions


def test_two_fits_are_bit_equal(torch_):
    _, X, labels, K, _ = cases.case(2)
    a, b = device_fit(torch_, X, labels, K), device_fit(torch_, X, labels, K)
    assert torch_.equal(a[1], b[1]) and torch_.equal(a[2], b[2])
    assert a[3] == b[3]


def test_iteration_cap_is_reported_and_raised(torch_, monkeypatch):
    from hse_facerec_tf_amd import identification
    _, X, labels, K, _ = cases.case(4)
    _, _, _, info = device_fit(torch_, X, labels, K, max_iter=1)
    assert info["iterations"] == 1 and info["converged"] is False and info["hessian_products"] >= 1
    assert sorted(info) == ["converged", "hessian_products", "iterations"]
    z, Xraw, _ = pca_cases.protocol_fixture()
    g, p = z["gallery"], z["probe"]
    monkeypatch.setattr(identification, "LINEAR_SVM_MAX_ITER", 1)
    with pytest.raises(RuntimeError, match=r"n=170 x d=256 gallery \(K=66 classes\) did not converge in 1 iterations"):
        identification.gallery_probe_identification(Xraw[g], z["y"][g], Xraw[p], z["y"][p], classifier="linear_svm")
    X, y, _, _, _, _ = pca_cases.golden_split()
    with pytest.raises(RuntimeError, match="did not converge in 1 iterations"):
        identification.one_nn_identification(X, y, classifier="linear_svm")


def test_label_code_out_of_range_is_an_error_not_a_fault(torch_):
    _, X, labels, K, _ = cases.case(1)
    bad = labels.copy()
    bad[5] = K
    with pytest.raises(ValueError, match="label code"):
        device_fit(torch_, X, bad, K)
    bad[5] = -1
    with pytest.raises(ValueError, match="label code"):
        device_fit(torch_, X, bad, K)


def test_predict_ties_and_the_binary_threshold(torch_):
    from hse_facerec_tf_amd import ops
    dec = np.array([[1.0, 1.0, 0.5], [0.0, 2.0, 2.0], [-1.0, -1.0, -1.0], [0.25, 0.5, 0.75], [3.0, -3.0, 3.0], [-0.0, 0.0, -0.0]])
    wide = np.full((3, 200), -1.0)                              # more columns than a wave: ties across lanes and across rounds
    wide[0, [70, 6, 134]] = 4.0
    wide[1, [199, 64]] = 4.0
    wide[2, 199] = 4.0
    for m in (dec, wide):
        got = ops.linear_svm_predict(torch_.from_numpy(m).cuda()).cpu().numpy()
        assert got.dtype == np.int32 and np.array_equal(got, np.argmax(m, axis=1)), (got, np.argmax(m, axis=1))
    one = np.array([[0.5], [0.0], [-0.0], [-2.0], [1e-300]])
    assert ops.linear_svm_predict(torch_.from_numpy(one).cuda()).cpu().tolist() == [1, 0, 0, 0, 1]


@pytest.mark.parametrize("normalize", [False, True])
def test_gallery_probe_protocol_reproduces_the_golden_file(torch_, normalize):
    """gallery_probe_identification(classifier="linear_svm") against LinearSVC(tol=1e-10)'s recorded probe decisions: equal predictions
    (the top-two gap is at least 100 times the bound: tests/test_linear_svm_cpu.py) and decision values within the derived bound:
    linear_svm_cases.decision_bound (the solver's) + linear_svm_cases.input_rounding_shift (the device normalises the rows itself, in
    float32 and in its own order; zero for the raw features) + 1e-8, the distance the CPU suite allows between the golden file and the
    optimum."""
    from hse_facerec_tf_amd import identification
    z, Xraw, _ = pca_cases.protocol_fixture()
    gold = np.load(cases.GOLDEN_FILE)
    name = "norm" if normalize else "raw"
    g, p = z["gallery"], z["probe"]
    yg, yp = z["y"][g], z["y"][p]
    gal, codes, prb, classes = cases.protocol_variant(normalize)
    bound = cases.decision_bound(gal, codes, len(classes), prb, TOL) + cases.input_rounding_shift(normalize) + 1e-8
    r = identification.gallery_probe_identification(Xraw[g], yg, Xraw[p], yp, normalize=normalize, classifier="linear_svm")
    assert sorted(r) == ["accuracy", "decision", "svm_iterations", "y_pred"]
    diff = float(np.abs(r["decision"] - gold["decision_" + name]).max())
    print("normalize=%s: %d iterations, max |decision - golden| %.2e (bound %.2e)" % (normalize, r["svm_iterations"], diff, bound))
    assert r["decision"].shape == (len(p), len(classes)) and r["decision"].dtype == np.float64
    assert diff <= bound
    assert np.array_equal(r["y_pred"], gold["y_pred_" + name])
    assert r["accuracy"] == float((gold["y_pred_" + name] == yp).mean())
    assert 1 <= r["svm_iterations"] <= 1000


@pytest.mark.parametrize("normalize", [False, True])
@pytest.mark.parametrize("k", [16, 20])
def test_gallery_probe_protocol_with_device_pca(torch_, k, normalize):
    """pca="device" + classifier="linear_svm" gives pca_ref + linear_svm_ref's predictions: all four variants keep a top-two gap of at
    least 100 times their bound (tests/test_linear_svm_cpu.py::test_fixture_margins_carry_the_gpu_protocol_tests), none is dropped."""
    from hse_facerec_tf_amd import identification
    z, Xraw, _ = pca_cases.protocol_fixture()
    g, p = z["gallery"], z["probe"]
    yg, yp = z["y"][g], z["y"][p]
    dec_w, pred_w, _ = cases.protocol_reference(normalize, k)
    r = identification.gallery_probe_identification(Xraw[g], yg, Xraw[p], yp, normalize=normalize, pca_components=k, pca="device",
                                                    classifier="linear_svm")
    print("normalize=%s k=%d: %d iterations, max |decision - reference| %.2e" % (normalize, k, r["svm_iterations"],
                                                                               np.abs(r["decision"] - dec_w).max()))
    assert np.array_equal(r["y_pred"], pred_w)
    assert r["accuracy"] == float((pred_w == yp).mean())


def test_one_nn_protocol_with_the_linear_svm(torch_):
    from hse_facerec_tf_amd import identification
    X, y, Xn, y2, train, test = pca_cases.golden_split()
    classes, codes = np.unique(y2[train], return_inverse=True)
    coef, intercept, info = ref.fit(Xn[train], codes, len(classes))
    assert info["gradient_ratio"] <= 1e-12
    dec_w = ref.decision(Xn[test], coef, intercept)
    pred_w = classes[ref.predict(dec_w)]
    # the rows are normalised on the device: the same float32 steps as the normalised fixture's, whose measured shift is taken here
    bound = cases.decision_bound(Xn[train], codes, len(classes), Xn[test], TOL) + cases.input_rounding_shift(True)
    print("top-two gap %.2e, bound %.2e" % (ref.top_two_gap(dec_w).min(), bound))
    assert ref.top_two_gap(dec_w).min() >= 100.0 * bound
    timings = {}
    r = identification.one_nn_identification(X, y, classifier="linear_svm", timings=timings)
    assert sorted(r) == ["accuracy", "decision", "indices", "num_classes", "svm_iterations", "test", "train", "y", "y_pred"]
    assert np.array_equal(r["train"], train) and np.array_equal(r["test"], test)
    assert r["decision"].shape == dec_w.shape
    assert np.array_equal(r["y_pred"], pred_w)
    assert r["accuracy"] == float((pred_w == y2[test]).mean())
    assert timings["svm_fit_s"] > 0 and timings["svm_predict_s"] > 0 and "nn1_s" not in timings


def test_default_calls_return_the_keys_they_returned_before(torch_):
    from hse_facerec_tf_amd import identification
    z, Xraw, _ = pca_cases.protocol_fixture()
    g, p = z["gallery"], z["probe"]
    r = identification.gallery_probe_identification(Xraw[g], z["y"][g], Xraw[p], z["y"][p])
    assert sorted(r) == ["accuracy", "nn_dist", "nn_index", "y_pred"]
    X, y, _, _, _, _ = pca_cases.golden_split()
    timings = {}
    r = identification.one_nn_identification(X, y, timings=timings)
    assert sorted(r) == ["accuracy", "indices", "nn_dist", "nn_index", "num_classes", "test", "train", "y", "y_pred"]
    assert sorted(timings) == ["host_split_s", "nn1_s", "nn1_shape", "normalize_s", "readback_s", "select_s"]


def test_gallery_probe_protocol_without_a_probe(torch_):
    """An empty probe set is fitted on and labels nothing: accuracy nan, as on the k-NN path."""
    from hse_facerec_tf_amd import identification
    z, Xraw, _ = pca_cases.protocol_fixture()
    g = z["gallery"]
    r = identification.gallery_probe_identification(Xraw[g], z["y"][g], Xraw[:0], z["y"][:0], classifier="linear_svm")
    assert r["decision"].shape == (0, 66) and len(r["y_pred"]) == 0 and np.isnan(r["accuracy"]) and r["svm_iterations"] >= 1
