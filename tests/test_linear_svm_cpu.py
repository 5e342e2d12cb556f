"""CPU suite for the linear SVM: the NumPy reference (tests/linear_svm_ref.py) against scikit-learn at a tight tolerance, the recorded
golden file, every argument check of ops / identification / the three C entry points without a GPU, and the margins of the fixture
that tests/test_linear_svm_gpu.py relies on."""
import ctypes

import numpy as np
import pytest

import linear_svm_cases as cases
import linear_svm_ref as ref

TOL = 1e-10            # the device's default tolerance: |grad f_k| <= TOL |grad f_k(0)|


def test_known_answer_of_the_reference():
    X, labels, C, coef_w, intercept_w, dec_w = cases.known_answer()
    coef, intercept, info = ref.fit(X, labels, 2, C=C)
    assert np.array_equal(coef, coef_w) and np.array_equal(intercept, intercept_w) and info["iterations"] == 1
    assert np.array_equal(ref.decision(X, coef, intercept), dec_w)
    assert np.array_equal(ref.predict(dec_w), labels)
    assert np.array_equal(ref.objective(ref.pack(coef, intercept), X, labels, 2, C), [0.25])      # 1/8 + 1/4 * 2 * 1/4
    assert np.array_equal(ref.gradient(ref.pack(coef, intercept), X, labels, 2, C), [[0.0, 0.0]])


@pytest.mark.parametrize("normalize", [False, True])
def test_reference_equals_scikit_learn_at_a_tight_tolerance(normalize):
    """linear_svm_ref.fit against LinearSVC(tol=1e-10, max_iter=10**6) on the fixture gallery: the probes' decision values agree to 1e-8.
    Measured: 3.9e-11 on the raw features, 2.2e-11 on the L2-normalised ones (scikit-learn 1.7.2), with the reference's own gradient at
    6e-17 |grad f(0)|."""
    from sklearn.svm import LinearSVC
    gal, codes, prb, classes = cases.protocol_variant(normalize)
    dec, y_pred, info = cases.protocol_reference(normalize)
    assert info["gradient_ratio"] <= 1e-12
    clf = LinearSVC(tol=1e-10, max_iter=10 ** 6, random_state=0).fit(gal, codes)
    diff = float(np.abs(clf.decision_function(prb) - dec).max())
    print("normalize=%s: max |decision difference| %.2e" % (normalize, diff))
    assert diff <= 1e-8
    assert np.array_equal(classes[clf.predict(prb)], y_pred)


def test_golden_file_is_what_the_recorder_writes():
    import importlib.util
    import os
    from conftest import ROOT
    spec = importlib.util.spec_from_file_location("record_linear_svm_golden", os.path.join(ROOT, "tools", "record_linear_svm_golden.py"))
    rec = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(rec)
    again, z = rec.record(), np.load(cases.GOLDEN_FILE)
    assert sorted(z.files) == sorted(again) == ["decision_norm", "decision_raw", "y_pred_norm", "y_pred_raw"]
    for name in ("raw", "norm"):
        assert z["decision_" + name].shape == (146, 66) and z["decision_" + name].dtype == np.float64
        assert np.abs(z["decision_" + name] - again["decision_" + name]).max() <= 1e-9
        assert np.array_equal(z["y_pred_" + name], again["y_pred_" + name])
        dec, y_pred, _ = cases.protocol_reference(name == "norm")
        assert np.abs(z["decision_" + name] - dec).max() <= 1e-8 and np.array_equal(z["y_pred_" + name], y_pred)


@pytest.mark.parametrize("index", range(cases.N_CASES))
def test_designed_cases_exclude_no_row_and_exercise_the_margin(index):
    """The GPU suite compares predictions where the reference's top-two gap exceeds twice its bound and allows 1 % of the held-out rows to
    fall out: with the reference's own gradients in place of the device's NO row falls out, so the allowance is the device's alone.  And
    the cases are what they claim: every class present, rows inside the margin at the optimum, converged to float64's floor."""
    name, X, labels, K, held = cases.case(index)
    coef, intercept, info = cases.reference(index)
    assert info["gradient_ratio"] <= 1e-12, name
    assert sorted(set(labels.tolist())) == list(range(K))
    W = ref.pack(coef, intercept)
    slack = 1.0 - ref.signs(labels, K) * (W @ ref.augmented(X).T)
    inside = float((slack > 0).mean())
    gn = np.sqrt((ref.gradient(W, X, labels, K) ** 2).sum(1))
    bound = 2.0 * gn.max() * np.sqrt((held.astype(np.float64) ** 2).sum(1) + 1.0)          # both sides at the reference's gradient
    gap = ref.top_two_gap(ref.decision(held, coef, intercept))
    print("%s: %d iterations, %.0f %% of (row, class) pairs inside the margin, smallest top-two gap %.2e, bound %.2e"
          % (name, info["iterations"], 100 * inside, gap.min(), bound.max()))
    assert inside >= 0.05                                       # 5 % with 601 classes (600 easy negatives per row), 14 % to 80 % otherwise
    assert np.all(gap > 2.0 * bound)
    # the device may end at 2 TOL |grad f_k(0)|: even then fewer than 1 % of the rows could fall out
    g0 = np.sqrt((ref.gradient(np.zeros_like(W), X, labels, K) ** 2).sum(1))
    worst = (2.0 * TOL * g0.max() + gn.max()) * np.sqrt((held.astype(np.float64) ** 2).sum(1) + 1.0)
    assert (gap <= 2.0 * worst).mean() <= 0.01


def test_fixture_margins_carry_the_gpu_protocol_tests():
    """For every variant tests/test_linear_svm_gpu.py runs through gallery_probe_identification, the smallest top-two gap of the optimum's
    probe decisions is at least 100 times the bound used there: linear_svm_cases.decision_bound (the device's gradient bound times
    |x~|) + linear_svm_cases.input_rounding_shift (the float32 steps in front of the fit) + the 1e-8 by which the golden file may miss
    the optimum.  Measured gaps: raw 1.09e-2, normalised 6.0e-3, raw + 16 / 20 components 3.5e-3 / 2.2e-3, normalised + 16 / 20
    components 2.5e-4 / 2.1e-3 -- at least 140 times the bounds printed here: no variant is dropped."""
    for normalize in (False, True):
        for k in (None, 16, 20):
            gal, codes, prb, classes = cases.protocol_variant(normalize, k)
            dec, _, info = cases.protocol_reference(normalize, k)
            assert info["gradient_ratio"] <= 1e-12
            bound = cases.decision_bound(gal, codes, len(classes), prb, TOL) + cases.input_rounding_shift(normalize, k) + 1e-8
            gap = float(ref.top_two_gap(dec).min())
            print("normalize=%s pca_components=%s: gap %.3e, bound %.3e (of which input rounding %.3e)"
                  % (normalize, k, gap, bound, cases.input_rounding_shift(normalize, k)))
            assert gap >= 100.0 * bound, (normalize, k, gap, bound)
            if not k:
                assert gap >= 6e-3


def test_check_linear_svm_args_without_a_gpu():
    from hse_facerec_tf_amd import ops
    ops.check_linear_svm_args(4582, 1024, 1680)                 # the LFW half split is inside the limits
    bad = [dict(n=0), dict(d=0), dict(n_classes=1), dict(max_iter=0), dict(n=1.5), dict(n_classes=True), dict(C=0.0), dict(C=-1.0),
           dict(C=float("inf")), dict(C=float("nan")), dict(C="1"), dict(tol=0.0), dict(tol=float("nan")), dict(tol=None),
           dict(n=(1 << 20) + 1), dict(d=(1 << 14) + 1), dict(n_classes=(1 << 16) + 1), dict(n=1 << 20, d=1 << 14)]
    for kw in bad:
        args = dict(n=10, d=8, n_classes=3, C=1.0, tol=1e-10, max_iter=10)
        args.update(kw)
        with pytest.raises(ValueError):
            ops.check_linear_svm_args(**args)
    with pytest.raises(ValueError, match="n_classes=1 must be at least 2"):
        ops.linear_svm_fit(np.zeros((4, 8), np.float32), np.zeros(4, np.int32), 1)
    with pytest.raises(ValueError, match="x must be"):
        ops.linear_svm_fit(np.zeros(4, np.float32), np.zeros(4, np.int32), 2)


def test_protocol_keywords_without_a_gpu():
    from hse_facerec_tf_amd import identification
    X, y = np.zeros((8, 8), np.float32), np.arange(8) % 2
    for fn in (lambda **kw: identification.gallery_probe_identification(X, y, X, y, **kw),
               lambda **kw: identification.one_nn_identification(X, y, **kw)):
        with pytest.raises(ValueError, match="classifier='svm' must be 'knn'"):
            fn(classifier="svm")
        with pytest.raises(ValueError, match="n_neighbors=3 has no meaning"):
            fn(classifier="linear_svm", n_neighbors=3)
        for C in (0.0, -2.0, float("inf"), float("nan"), "1"):
            with pytest.raises(ValueError, match="C"):
                fn(classifier="linear_svm", svm_C=C)
        with pytest.raises(ValueError, match="pca="):
            fn(classifier="linear_svm", pca="gpu")
    assert identification.LINEAR_SVM_MAX_ITER == 1000 and identification.LINEAR_SVM_TOL == TOL


def test_c_entry_points_refuse_bad_arguments_without_a_gpu():
    """Every HSEFR_ERR_INVALID of hsefr_linear_svm_fit / _decision / _predict comes before any device call."""
    from hse_facerec_tf_amd import _lib
    L = _lib.lib()
    buf = ctypes.create_string_buffer(4096)
    p = ctypes.cast(buf, ctypes.c_void_p)

    def fit(x=p, n=10, d=8, labels=p, n_classes=3, C=1.0, tol=1e-10, max_iter=10, coef=p, intercept=p, info=p):
        return L.hsefr_linear_svm_fit(x, n, d, labels, n_classes, C, tol, max_iter, coef, intercept, info, None)
    for kw, word in ((dict(x=None), "null"), (dict(labels=None), "null"), (dict(coef=None), "null"), (dict(intercept=None), "null"),
                     (dict(info=None), "null"), (dict(n=0), "n=0"), (dict(d=0), "d=0"), (dict(n_classes=1), "n_classes=1"),
                     (dict(C=0.0), "C=0"), (dict(C=-1.0), "C=-1"), (dict(C=float("inf")), "C=inf"), (dict(C=float("nan")), "C="),
                     (dict(tol=0.0), "tol=0"), (dict(tol=float("nan")), "tol="), (dict(max_iter=0), "max_iter=0"),
                     (dict(n=(1 << 20) + 1), "limits"), (dict(d=(1 << 14) + 1), "limits"), (dict(n_classes=(1 << 16) + 1), "limits"),
                     (dict(n=1 << 20, d=1 << 14), "limits")):
        assert fit(**kw) == _lib.ERR_INVALID, kw
        assert "linear_svm_fit" in _lib.last_error() and word in _lib.last_error(), (kw, _lib.last_error())

    def decision(x=p, n=10, d=8, coef=p, intercept=p, k_rows=3, out=p):
        return L.hsefr_linear_svm_decision(x, n, d, coef, intercept, k_rows, out, None)
    for kw, word in ((dict(x=None), "null"), (dict(coef=None), "null"), (dict(intercept=None), "null"), (dict(out=None), "null"),
                     (dict(n=0), "n=0"), (dict(d=0), "d=0"), (dict(k_rows=0), "k_rows=0"), (dict(n=(1 << 20) + 1), "limits"),
                     (dict(d=(1 << 14) + 1), "limits"), (dict(k_rows=(1 << 16) + 1), "limits"), (dict(n=1 << 20, k_rows=1 << 16), "limits")):
        assert decision(**kw) == _lib.ERR_INVALID, kw
        assert "linear_svm_decision" in _lib.last_error() and word in _lib.last_error(), (kw, _lib.last_error())

    def predict(dec=p, n=10, k_rows=3, pred=p):
        return L.hsefr_linear_svm_predict(dec, n, k_rows, pred, None)
    for kw, word in ((dict(dec=None), "null"), (dict(pred=None), "null"), (dict(n=0), "n=0"), (dict(k_rows=0), "k_rows=0"),
                     (dict(n=(1 << 20) + 1), "limits"), (dict(k_rows=(1 << 16) + 1), "limits"), (dict(n=1 << 20, k_rows=1 << 16), "limits")):
        assert predict(**kw) == _lib.ERR_INVALID, kw
        assert "linear_svm_predict" in _lib.last_error() and word in _lib.last_error(), (kw, _lib.last_error())
    with pytest.raises(ValueError):
        _lib.check(predict(n=0), "hsefr_linear_svm_predict")
