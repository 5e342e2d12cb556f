"""GPU suite for what the identification protocols share: one_nn_identification, gallery_probe_identification(normalize=True) and
cross_validated_1nn are the same computation on the same rows -- the L2 normalisation is per row, and every stage after it (the device
PCA, both SVM fits, the searches' tie rules) is deterministic -- so their results are EQUAL, bit for bit, for every classifier with and
without the device PCA; and each classifier leaves exactly its own keys in ``timings``."""
import numpy as np
import pytest

import pca_cases

pytestmark = pytest.mark.gpu

CLASSIFIERS = [{}, {"n_neighbors": 3}, {"classifier": "linear_svm"}, {"classifier": "rbf_svm"}]
DEVICE_PCA = {"pca_components": 16, "pca": "device"}
EXTRAS = {"knn": ("nn_index", "nn_dist"), "linear_svm": ("decision", "svm_iterations"), "rbf_svm": ("votes", "svm_iterations")}


@pytest.fixture(scope="module")
def split():
    """tests/golden/nn1.npz's stratified half split: (X, y, the filtered rows of X, their encoded labels, train, test)."""
    from hse_facerec_tf_amd import identification
    X, y, _, y_enc, train, test = pca_cases.golden_split()
    kept, again = identification.filter_classes(y)
    assert np.array_equal(again, y_enc)
    return X, y, X[kept], y_enc, train, test


def same_bits(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


@pytest.mark.parametrize("pca", [{}, DEVICE_PCA], ids=["features", "device_pca"])
@pytest.mark.parametrize("kw", CLASSIFIERS, ids=["nn1", "knn3", "linear_svm", "rbf_svm"])
def test_the_two_protocols_agree_bit_for_bit(split, kw, pca):
    from hse_facerec_tf_amd import identification
    X, y, X_f, y_enc, train, test = split
    kw = dict(kw, **pca)
    one = identification.one_nn_identification(X, y, **kw)
    two = identification.gallery_probe_identification(X_f[train], y_enc[train], X_f[test], y_enc[test], normalize=True, **kw)
    assert np.array_equal(one["train"], train) and np.array_equal(one["test"], test) and np.array_equal(one["y"], y_enc)
    assert same_bits(one["y_pred"], two["y_pred"]) and one["accuracy"] == two["accuracy"]
    for key in EXTRAS[kw.get("classifier", "knn")]:
        assert same_bits(one[key], two[key]), key
    assert sorted(set(one) - set(two)) == ["indices", "num_classes", "test", "train", "y"] and not set(two) - set(one)


@pytest.mark.parametrize("k", [1, 3])
def test_cross_validation_agrees_with_the_gallery_probe_protocol(split, k):
    from hse_facerec_tf_amd import identification
    _, _, X_f, y_enc, train, test = split
    cv = identification.cross_validated_1nn(X_f, y_enc, [(train, test)], n_neighbors=k)
    two = identification.gallery_probe_identification(X_f[train], y_enc[train], X_f[test], y_enc[test], normalize=True, n_neighbors=k)
    assert len(cv["y_pred"]) == 1 and same_bits(cv["y_pred"][0], two["y_pred"])
    assert cv["accuracies"].tolist() == [two["accuracy"]] and cv["mean"] == two["accuracy"]


def test_cross_validation_scores_an_empty_fold_as_nan(split):
    """A fold without a probe -- ``[]`` or NumPy's float64 ``array([])``, which single_image_per_class_splits returns when every class
    has one image -- is searched with zero queries and scored nan.  (n_neighbors=1: ops.knn refuses zero queries with labels.)"""
    from hse_facerec_tf_amd import identification
    _, _, X_f, y_enc, train, test = split
    cv = identification.cross_validated_1nn(X_f, y_enc, [(train, []), (train, np.array([])), (train, test)])
    assert [len(p) for p in cv["y_pred"]] == [0, 0, len(test)]
    assert np.isnan(cv["accuracies"][:2]).all() and not np.isnan(cv["accuracies"][2]) and np.isnan(cv["mean"])


PHASES = ["host_split_s", "normalize_s", "pca_s", "readback_s", "select_s"]


@pytest.mark.parametrize("kw, keys", [({}, PHASES + ["nn1_s", "nn1_shape"]), ({"n_neighbors": 3}, PHASES + ["nn1_s", "nn1_shape"]),
                                      ({"classifier": "linear_svm"}, PHASES + ["svm_fit_s", "svm_predict_s"]),
                                      ({"classifier": "rbf_svm"}, PHASES + ["svm_fit_s", "svm_predict_s"])],
                         ids=["nn1", "knn3", "linear_svm", "rbf_svm"])
def test_each_classifier_leaves_its_own_timings_keys(split, kw, keys):
    from hse_facerec_tf_amd import identification
    X, y, _, _, train, test = split
    timings = {}
    identification.one_nn_identification(X, y, timings=timings, **dict(kw, **DEVICE_PCA))
    assert sorted(timings) == sorted(keys)
    assert all(timings[key] > 0 for key in keys if key != "nn1_shape")
    if "nn1_shape" in keys:
        assert timings["nn1_shape"] == (len(test), len(train), 16)


def says(message, fn, *args):
    with pytest.raises(ValueError) as e:
        fn(*args)
    assert str(e.value) == message


def test_float64_tensors_of_another_shape_or_type_are_refused():
    """The shape and the type of the fitted tensors, on CUDA tensors (tests/test_identification_shared_cpu.py reaches only 'no CUDA
    tensor').  A tensor on another device never gets as far as this check: the entry points refuse mixed devices first."""
    import torch
    from hse_facerec_tf_amd import ops
    x, q, labels = torch.zeros((4, 8), device="cuda"), torch.zeros((2, 8), device="cuda"), torch.zeros(4, dtype=torch.int32, device="cuda")

    def f64(*shape, dtype=torch.float64):
        return torch.zeros(shape, dtype=dtype, device="cuda")
    mean = "mean must be a contiguous float64 CUDA tensor of shape (8,)"
    says(mean, ops.pca_transform, x, f64(7), f64(2, 8))
    says(mean, ops.pca_transform, x, f64(8, dtype=torch.float32), f64(2, 8))
    says(mean, ops.pca_transform, x, f64(16)[::2], f64(2, 8))
    says("components must be a contiguous float64 CUDA tensor of shape (2, 8)", ops.pca_transform, x, f64(8), f64(2, 7))
    coef = "coef must be a contiguous float64 CUDA tensor of shape (1, 8) on x's device"
    says(coef, ops.linear_svm_decision, x, f64(1, 7), f64(1))
    says(coef, ops.linear_svm_decision, x, f64(1, 8, dtype=torch.float32), f64(1))
    says("intercept must be a contiguous float64 CUDA tensor of shape (1,) on x's device", ops.linear_svm_decision, x, f64(1, 8), f64(2))
    for fn in (ops.rbf_svm_predict, ops.rbf_svm_decision):
        says("dual_coef must be a contiguous float64 CUDA tensor of shape (2, 4) on x's device", fn, q, x, labels, 3, 0.5, f64(2, 3), f64(3))
        says("rho must be a contiguous float64 CUDA tensor of shape (3,) on x's device", fn, q, x, labels, 3, 0.5, f64(2, 4), f64(2))
        says("rho must be a contiguous float64 CUDA tensor of shape (3,) on x's device",
             fn, q, x, labels, 3, 0.5, f64(2, 4), f64(3, dtype=torch.float32))
    says("labels must be a contiguous int32 tensor of 4 values on the gallery's device", ops.knn, q, x, 3, labels.long())
    says("labels must be a contiguous int32 tensor of 4 values on x's device", ops.linear_svm_fit, x, labels[:3].contiguous(), 2)
