"""CPU suite for the RBF SVM: the NumPy reference (tests/rbf_svm_ref.py) against scikit-learn's recorded answers at tol = 1e-12, the
derived decision bound and the three conditions under which tests/test_rbf_svm_gpu.py may demand EQUAL votes, the golden file, and
every argument check of ops / identification / the four C entry points without a GPU."""
import ctypes
import os

import numpy as np
import pytest

import rbf_svm_cases as cases
import rbf_svm_ref as ref

TOL = 1e-10            # identification.RBF_SVM_TOL: a pair is converged at m(a) - M(a) <= TOL


@pytest.mark.parametrize("C", [1.0, 4.0])
def test_known_answer_of_the_reference(C):
    X, labels, gamma, a, q, dec_w = cases.known_answer(C)
    dual_coef, rho, pairs, _ = ref.fit(X, labels, 2, gamma, C=C)
    assert np.allclose(dual_coef, [[a, -a]], rtol=1e-15, atol=0) and np.allclose(rho, [0.0], atol=1e-16)
    assert np.allclose(ref.decision(q, X, labels, 2, gamma, dual_coef, rho), dec_w[:, None], rtol=1e-15, atol=1e-16)
    votes, pred = ref.votes_of(dec_w[:, None], 2)
    assert pred.tolist() == [0, 1, 1, 0, 1, 0]                 # dec(0.5) is exactly 0: the vote goes to j


@pytest.mark.parametrize("index", range(cases.N_CASES))
def test_reference_equals_scikit_learn_at_a_tight_tolerance(index):
    """rbf_svm_ref at tol = 1e-12 against SVC(tol=1e-12)'s recorded rho, pair decisions, votes and labels.  Both stop with a violation
    of at most 1e-12, so they differ by at most twice the derived bound at that eps, plus 1e-12 for the rounding of sums of up to 330
    terms.  Measured: 1.3e-13 ... 4.2e-13 in decision values -- with the kernel matrix rounded to float32 as libsvm holds it (against the
    unrounded matrix scikit-learn's optimum sits 4e-9 ... 5e-8 away, outside the bound)."""
    name, X, labels, K, held = cases.case(index)
    g, c = cases.golden(), "c%d_" % index
    assert abs(cases.gamma(index) / float(g[c + "gamma"]) - 1.0) <= 1e-15
    dual_coef, rho, pairs, iterations = cases.reference(index)
    dec = cases.reference_decision(index)
    bound, rho_bound = cases.decision_bound(index, 1e-12)
    sel = cases.recorded_pairs(dec.shape[1])
    d_dec = float(np.abs(dec[:cases.DECISION_ROWS][:, sel] - g[c + "dec"]).max())
    d_rho = float(np.abs(rho - g[c + "rho"]).max())
    print("%s: %d iterations, |decision difference| %.2e, |rho difference| %.2e, bound(1e-12) %.2e" % (name, iterations, d_dec, d_rho, bound))
    assert d_dec <= 2.0 * bound + 1e-12 and d_rho <= 2.0 * rho_bound + 1e-12
    votes, pred = ref.votes_of(dec, K)
    assert np.array_equal(votes, g[c + "votes"]) and np.array_equal(pred, g[c + "pred"])
    gap, balance, inside = ref.kkt_violation(X, labels, dual_coef, cases.gamma(index), 1.0)
    assert gap.max() <= 2e-12 and balance.max() <= 1e-13 and inside.all()


@pytest.mark.parametrize("index", range(cases.N_CASES))
def test_the_bound_holds_for_scikit_learn_and_makes_every_vote_certain(index):
    """(a) scikit-learn's tol = 1e-10 decisions lie within decision_bound(eps = 1e-10) of its tol = 1e-12 ones; (b) at eps = 2 TOL the bound
    stays below a quarter of the smallest recorded |decision|, so every vote of the device is certain, the tied rows' too; (c) no bounded
    variable of the reference sits within 1e-6 of its KKT threshold, so the bounded set the bound assumes is unambiguous."""
    name = cases.case(index)[0]
    g, c = cases.golden(), "c%d_" % index
    at_1e10, at_2tol = cases.decision_bound(index, 1e-10)[0], cases.decision_bound(index, 2.0 * TOL)[0]
    slack = ref.bounded_slack(cases.reference(index)[2], 1.0)
    print("%s: bound(1e-10) %.2e against scikit-learn's %.2e; bound(2 TOL) %.2e against min |dec| / 4 = %.2e; bounded slack %.2e"
          % (name, at_1e10, float(g[c + "tol_gap"]), at_2tol, float(g[c + "min_abs"]) / 4.0, slack))
    assert float(g[c + "tol_gap"]) <= at_1e10
    assert at_2tol < float(g[c + "min_abs"]) / 4.0
    assert slack >= 1e-6


def test_the_cases_are_what_they_claim():
    sizes = [np.bincount(cases.case(i)[2]).tolist() for i in range(cases.N_CASES)]
    assert sizes[0] == [2, 3] and sizes[1] == [1, 12, 24] and sizes[2] == [1, 2, 70, 130, 200] and sizes[3] == [1] * 100 + [2] * 100 + [4] * 100
    assert cases.case(4)[1].shape == (170, 256) and cases.case(4)[3] == 66 and cases.case(5)[1].shape == (170, 256)
    for i in range(cases.N_CASES):
        labels = cases.case(i)[2]
        assert np.any(np.diff(labels) < 0)                      # the rows are not grouped by class
    g = cases.golden()
    ties = [int((np.sort(g["c%d_votes" % i], 1)[:, -1] == np.sort(g["c%d_votes" % i], 1)[:, -2]).sum()) for i in range(1, cases.N_CASES)]
    assert ties == [0, 0, 11, 0, 1]                             # the first arg-max rule is exercised: 11 of 96 and 1 of 146 rows


def test_pca_variant_votes_are_certain():
    """The certainty condition (b) for the variant that tests/test_rbf_svm_gpu.py runs with pca="device", pca_components=16: the bound
    at eps = 2 TOL stays below a quarter of the smallest |decision| of the probes (1.8e-8 against 1.4e-7 / 4), and no bounded variable
    is within 1e-6 of its threshold.  The device projects the rows itself; its float32 entries may differ from pca_ref's by one unit in
    the last place in the few entries on a rounding boundary.  Moving EVERY entry by one unit, up or down (a measured sample of the
    reference's sensitivity, as linear_svm_cases.input_rounding_shift: decisions move by up to 1.9e-7), changes no vote and no label."""
    gamma, dec, votes, pred, pairs, bound = cases.pca_reference()
    moved = cases.pca_reference(True)
    least = float(np.abs(dec).min())
    print("pca 16: gamma %.6g, bound(2 TOL) %.2e, min |dec| %.2e, bounded slack %.2e; every entry moved by one unit: decisions by %.2e"
          % (gamma, bound, least, ref.bounded_slack(pairs, 1.0), float(np.abs(moved[1] - dec).max())))
    assert bound < least / 4.0
    assert ref.bounded_slack(pairs, 1.0) >= 1e-6
    assert np.array_equal(moved[2], votes) and np.array_equal(moved[3], pred)


def test_normalised_votes_survive_the_device_normalisation():
    """gallery_probe_identification(normalize=True) normalises the rows on the device: its float32 rows differ from the host's by a
    common factor within 1 +- 2^-21 per row (linear_svm_cases.input_rounding_shift).  With EVERY row scaled by 1 + 2^-21 or 1 - 2^-21 (a
    measured sample: decisions move by up to 4.1e-7) the reference's votes and labels are still the recorded ones."""
    import linear_svm_cases
    gal, codes, prb, classes = linear_svm_cases.protocol_variant(True, None, moved=True)
    K, gamma = len(classes), ref.gamma_scale(gal)
    dual_coef, rho, _, _ = ref.fit(gal, codes, K, gamma, tol=1e-12)
    dec = ref.decision(prb, gal, codes, K, gamma, dual_coef, rho)
    votes, pred = ref.votes_of(dec, K)
    print("every row moved: decisions by %.2e" % float(np.abs(dec - cases.reference_decision(5)).max()))
    assert np.array_equal(votes, cases.golden()["c5_votes"]) and np.array_equal(pred, cases.golden()["c5_pred"])


def test_golden_file_is_what_the_recorder_writes():
    import importlib.util
    from conftest import ROOT
    spec = importlib.util.spec_from_file_location("record_rbf_svm_golden", os.path.join(ROOT, "tools", "record_rbf_svm_golden.py"))
    rec = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(rec)
    again, z = rec.record(), cases.golden()
    assert sorted(z) == sorted(again)
    for k in z:
        assert z[k].shape == again[k].shape and z[k].dtype == again[k].dtype, k
        if k.endswith(("votes", "pred")):
            assert np.array_equal(z[k], again[k]), k
        elif k.endswith("tol_gap"):
            assert abs(float(z[k]) - float(again[k])) <= 1e-11, k
        else:
            assert np.abs(z[k] - again[k]).max() <= 1e-12, k
    assert z["c3_dec"].shape == (cases.DECISION_ROWS, 701) and z["c4_dec"].shape == (cases.DECISION_ROWS, 2145)
    largest = max(os.path.getsize(os.path.join(os.path.dirname(cases.GOLDEN_FILE), f)) for f in os.listdir(os.path.dirname(cases.GOLDEN_FILE))
                  if f != os.path.basename(cases.GOLDEN_FILE))
    assert os.path.getsize(cases.GOLDEN_FILE) <= largest


def test_check_rbf_svm_args_without_a_gpu():
    from hse_facerec_tf_amd import ops
    ops.check_rbf_svm_args(4582, 1024, 1680)                    # the LFW half split is inside the limits
    ops.check_rbf_svm_args(4582, 128, 1680, C=2.0, gamma=0.5)
    bad = [dict(n=1), dict(d=0), dict(n_classes=1), dict(max_iter=0), dict(n=1.5), dict(n_classes=True), dict(C=0.0), dict(C=-1.0),
           dict(C=float("inf")), dict(C=float("nan")), dict(C="1"), dict(tol=0.0), dict(tol=float("nan")), dict(tol=None),
           dict(gamma=0.0), dict(gamma=-1.0), dict(gamma=float("inf")), dict(gamma=float("nan")), dict(gamma="auto"), dict(gamma=None),
           dict(gamma=True), dict(n=(1 << 14) + 1), dict(d=(1 << 14) + 1), dict(n=8192, n_classes=(1 << 12) + 1), dict(n=10, n_classes=11)]
    for kw in bad:
        args = dict(n=10, d=8, n_classes=3, C=1.0, gamma="scale", tol=1e-10, max_iter=10)
        args.update(kw)
        with pytest.raises(ValueError):
            ops.check_rbf_svm_args(**args)
    x, labels = np.zeros((4, 8), np.float32), np.zeros(4, np.int32)
    with pytest.raises(ValueError, match="n_classes=1 must be at least 2"):
        ops.rbf_svm_fit(x, labels, 1, 0.5)
    with pytest.raises(ValueError, match="x must be"):
        ops.rbf_svm_fit(np.zeros(4, np.float32), labels, 2, 0.5)
    with pytest.raises(ValueError, match="gamma must be a number here"):
        ops.rbf_svm_fit(x, labels, 2, "scale")
    with pytest.raises(ValueError, match="d_used"):
        ops.rbf_svm_gamma(x, d_used=9)
    with pytest.raises(ValueError, match="over the limit of"):
        ops.rbf_svm_decision(np.zeros((4582, 8), np.float32), np.zeros((4582, 8), np.float32), None, 1680, 0.5, None, None)
    with pytest.raises(ValueError, match="nq=0"):
        ops.rbf_svm_predict(np.zeros((0, 8), np.float32), x, labels, 2, 0.5, None, None)


def test_protocol_keywords_without_a_gpu():
    from hse_facerec_tf_amd import identification
    X, y = np.zeros((8, 8), np.float32), np.arange(8) % 2
    for fn in (lambda **kw: identification.gallery_probe_identification(X, y, X, y, **kw),
               lambda **kw: identification.one_nn_identification(X, y, **kw)):
        for gamma in ("auto", 0.0, -1.0, float("inf"), float("nan"), None, True):
            with pytest.raises(ValueError, match="gamma"):
                fn(classifier="rbf_svm", svm_gamma=gamma)
        with pytest.raises(ValueError, match="n_neighbors=3 has no meaning"):
            fn(classifier="rbf_svm", n_neighbors=3)
        for C in (0.0, -2.0, float("inf"), float("nan"), "1"):
            with pytest.raises(ValueError, match="C"):
                fn(classifier="rbf_svm", svm_C=C)
        with pytest.raises(ValueError, match="pca="):
            fn(classifier="rbf_svm", pca="gpu")
        with pytest.raises(ValueError, match="classifier='rbf' must be 'knn'"):
            fn(classifier="rbf")
    assert identification.RBF_SVM_TOL == TOL and identification.RBF_SVM_MAX_ITER == 100000


def test_c_entry_points_refuse_bad_arguments_without_a_gpu():
    """Every HSEFR_ERR_INVALID of the four hsefr_rbf_svm_* entry points comes before any device call."""
    from hse_facerec_tf_amd import _lib
    L = _lib.lib()
    buf = ctypes.create_string_buffer(4096)
    p = ctypes.cast(buf, ctypes.c_void_p)
    inf, nan = float("inf"), float("nan")

    def gamma_scale(x=p, n=10, d=8, d_used=8, gamma=p):
        return L.hsefr_rbf_svm_gamma_scale(x, n, d, d_used, gamma, None)
    for kw, word in ((dict(x=None), "null"), (dict(gamma=None), "null"), (dict(n=0), "n=0"), (dict(d=0), "d=0"), (dict(d_used=0), "d_used=0"),
                     (dict(d_used=9), "d_used=9"), (dict(n=(1 << 20) + 1), "limits"), (dict(d=(1 << 14) + 1, d_used=1), "limits")):
        assert gamma_scale(**kw) == _lib.ERR_INVALID, kw
        assert "rbf_svm_gamma_scale" in _lib.last_error() and word in _lib.last_error(), (kw, _lib.last_error())

    def fit(x=p, n=10, d=8, labels=p, n_classes=3, gamma=0.5, C=1.0, tol=1e-10, max_iter=10, dual_coef=p, rho=p, info=p):
        return L.hsefr_rbf_svm_fit(x, n, d, labels, n_classes, gamma, C, tol, max_iter, dual_coef, rho, info, None)
    for kw, word in ((dict(x=None), "null"), (dict(labels=None), "null"), (dict(dual_coef=None), "null"), (dict(rho=None), "null"),
                     (dict(info=None), "null"), (dict(n=0), "n=0"), (dict(n=1), "n=1"), (dict(d=0), "d=0"), (dict(n_classes=1), "n_classes=1"),
                     (dict(C=0.0), "C=0"), (dict(C=-1.0), "C=-1"), (dict(C=inf), "C=inf"), (dict(C=nan), "C="),
                     (dict(gamma=0.0), "gamma=0"), (dict(gamma=-1.0), "gamma=-1"), (dict(gamma=inf), "gamma=inf"), (dict(gamma=nan), "gamma="),
                     (dict(tol=0.0), "tol=0"), (dict(tol=inf), "tol=inf"), (dict(tol=nan), "tol="), (dict(max_iter=0), "max_iter=0"),
                     (dict(n=(1 << 14) + 1), "limits"), (dict(d=(1 << 14) + 1), "limits"), (dict(n=8192, n_classes=(1 << 12) + 1), "limits"),
                     (dict(n_classes=11), "limits")):
        assert fit(**kw) == _lib.ERR_INVALID, kw
        assert "rbf_svm_fit" in _lib.last_error() and word in _lib.last_error(), (kw, _lib.last_error())

    def decision(q=p, nq=4, x=p, n=10, d=8, labels=p, n_classes=3, gamma=0.5, dual_coef=p, rho=p, out=p):
        return L.hsefr_rbf_svm_decision(q, nq, x, n, d, labels, n_classes, gamma, dual_coef, rho, out, None)

    def predict(q=p, nq=4, x=p, n=10, d=8, labels=p, n_classes=3, gamma=0.5, dual_coef=p, rho=p, out=p):
        return L.hsefr_rbf_svm_predict(q, nq, x, n, d, labels, n_classes, gamma, dual_coef, rho, out, None, None)
    for fn, who in ((decision, "rbf_svm_decision"), (predict, "rbf_svm_predict")):
        for kw, word in ((dict(q=None), "null"), (dict(x=None), "null"), (dict(labels=None), "null"), (dict(dual_coef=None), "null"),
                         (dict(rho=None), "null"), (dict(out=None), "null"), (dict(nq=0), "nq=0"), (dict(n=0), "n=0"), (dict(d=0), "d=0"),
                         (dict(n_classes=1), "n_classes=1"), (dict(gamma=0.0), "gamma=0"), (dict(gamma=nan), "gamma="), (dict(gamma=inf), "gamma=inf"),
                         (dict(nq=(1 << 20) + 1), "limits"), (dict(n=(1 << 14) + 1), "limits"), (dict(d=(1 << 14) + 1), "limits"),
                         (dict(n=8192, n_classes=(1 << 12) + 1), "limits"), (dict(n_classes=11), "limits")):
            assert fn(**kw) == _lib.ERR_INVALID, (who, kw)
            assert who in _lib.last_error() and word in _lib.last_error(), (who, kw, _lib.last_error())
    # the LFW-sized decision table (4582 probes x 1 410 360 pairs, 51 GB) is refused; its labels are not
    assert decision(nq=4582, n=4582, d=1024, n_classes=1680) == _lib.ERR_INVALID
    assert "over the limit of 134217728 decision values" in _lib.last_error()
    with pytest.raises(ValueError):
        _lib.check(decision(nq=0), "hsefr_rbf_svm_decision")


def test_the_product_library_has_room_and_exports_the_entry_points():
    from hse_facerec_tf_amd import _lib
    L = _lib.lib()
    if hasattr(L, "hsefr_debug_set"):
        pytest.skip("a development build is loaded")
    assert os.path.getsize(_lib.LIB_PATH) < 4_000_000
    for name in ("hsefr_rbf_svm_gamma_scale", "hsefr_rbf_svm_fit", "hsefr_rbf_svm_decision", "hsefr_rbf_svm_predict"):
        assert hasattr(L, name) and name in _lib.SIGNATURES
    assert L.hsefr_version() == 141
