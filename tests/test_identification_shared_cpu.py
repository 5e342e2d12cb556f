"""CPU suite for the argument checks that the identification entry points of ops share, and for the one keyword check of the
protocols: the literal message of every site, one bad value each, through the public callers -- the words are the library's user
interface, and the GPU suites' ``match=`` patterns do not run without a device."""
import numpy as np
import pytest


def says(message, fn, *args, **kw):
    with pytest.raises(ValueError) as e:
        fn(*args, **kw)
    assert str(e.value) == message


def test_integer_arguments():
    from hse_facerec_tf_amd import ops
    says("n_neighbors must be an integer, got 1.5", ops.check_n_neighbors, 1.5)
    says("n_neighbors must be an integer, got True", ops.check_n_neighbors, True)
    says("n_neighbors=0 must be in 1..16", ops.check_n_neighbors, 0)
    says("n_neighbors=17 must be in 1..16", ops.check_n_neighbors, ops.KNN_MAX_K + 1)
    says("n_neighbors=3 exceeds the 2 gallery rows", ops.check_n_neighbors, 3, 2)
    assert ops.check_n_neighbors(np.int64(3), 3) == 3 and type(ops.check_n_neighbors(np.int64(3))) is int
    says("pca_components must be an integer, got '8'", ops.check_pca_components, "8")
    says("pca_components=0 must be in 1..256", ops.check_pca_components, 0)
    says("pca_components=257 must be in 1..256", ops.check_pca_components, ops.PCA_MAX_K + 1)
    says("pca_components=8 exceeds n - 1 for the 8 rows to fit on", ops.check_pca_components, 8, 8)
    says("pca_components=8 exceeds the 4 features", ops.check_pca_components, 8, 16, 4)
    assert ops.check_pca_components(np.int32(8), 9, 8) == 8
    x = np.zeros((8, 8), np.float32)
    says("max_iter must be a positive integer, got 0", ops.pca_fit, x, 2, max_iter=0)
    says("max_iter must be a positive integer, got 2.5", ops.pca_fit, x, 2, max_iter=2.5)
    says("d_used=9 must be an integer in 1..8", ops.rbf_svm_gamma, x, d_used=9)
    says("d_used=0 must be an integer in 1..8", ops.rbf_svm_gamma, x, d_used=0)
    says("d_used=2.0 must be an integer in 1..8", ops.rbf_svm_gamma, x, d_used=2.0)
    says("d_used=True must be an integer in 1..8", ops.rbf_svm_gamma, x, d_used=True)


@pytest.mark.parametrize("name, least_n", [("check_linear_svm_args", 1), ("check_rbf_svm_args", 2)])
def test_integer_arguments_of_the_svm_checkers(name, least_n):
    from hse_facerec_tf_amd import ops
    check = getattr(ops, name)
    says("n=%d must be at least %d" % (least_n - 1, least_n), check, least_n - 1, 8, 2)
    says("n must be an integer, got 10.0", check, 10.0, 8, 2)
    says("d=0 must be at least 1", check, 10, 0, 2)
    says("d must be an integer, got 1.5", check, 10, 1.5, 2)
    says("n_classes=1 must be at least 2", check, 10, 8, 1)
    says("n_classes must be an integer, got True", check, 10, 8, True)
    says("max_iter=0 must be at least 1", check, 10, 8, 2, max_iter=0)
    says("max_iter must be an integer, got None", check, 10, 8, 2, max_iter=None)
    says("n must be an integer, got None", check, None, 0, 1)                       # the arguments in their order


def test_number_arguments():
    from hse_facerec_tf_amd import ops
    lin, rbf = ops.check_linear_svm_args, ops.check_rbf_svm_args
    for check in (lin, rbf):
        says("C must be a number, got '1'", check, 10, 8, 2, C="1")
        says("C must be a number, got True", check, 10, 8, 2, C=True)
        says("C=0.0 must be positive and finite", check, 10, 8, 2, C=0.0)
        says("C=inf must be positive and finite", check, 10, 8, 2, C=float("inf"))
        says("C=nan must be positive and finite", check, 10, 8, 2, C=float("nan"))
        says("tol must be a number, got None", check, 10, 8, 2, tol=None)
    says("tol=0.0 must be positive", lin, 10, 8, 2, tol=0.0)
    says("tol=nan must be positive", lin, 10, 8, 2, tol=float("nan"))
    lin(10, 8, 2, tol=float("inf"))                                                 # the linear SVM's tol need only be positive
    says("tol=0.0 must be positive and finite", rbf, 10, 8, 2, tol=0.0)
    says("tol=inf must be positive and finite", rbf, 10, 8, 2, tol=float("inf"))
    says("tol must be a number, got None", lin, 10, 8, 2, C=-1.0, tol=None)         # LinearSVC's: both types before either range
    says("C=-1.0 must be positive and finite", rbf, 10, 8, 2, C=-1.0, tol=None)     # SVC's: argument by argument
    says("gamma must be a number or 'scale', got None", rbf, 10, 8, 2, gamma=None)
    says("gamma must be a number or 'scale', got 'auto'", rbf, 10, 8, 2, gamma="auto")
    says("gamma=-1.0 must be positive and finite", rbf, 10, 8, 2, gamma=-1.0)
    says("gamma=inf must be positive and finite", rbf, 10, 8, 2, gamma=float("inf"))
    rbf(10, 8, 2, C=2, gamma=np.float32(0.5), tol=1e-3)


@pytest.fixture
def host_torch(monkeypatch):
    """The tensor checks sit behind require_gpu() and the float32-CUDA check of x.  With both stood in for, a host tensor reaches them,
    and nothing runs after them: every call below raises there."""
    import torch
    from hse_facerec_tf_amd import _lib, ops
    monkeypatch.setattr(_lib, "require_gpu", lambda: torch)
    monkeypatch.setattr(ops, "_f32c", lambda t, name: t)
    return torch


def test_label_tensors(host_torch):
    from hse_facerec_tf_amd import ops
    torch = host_torch
    x, q = torch.zeros((4, 8)), torch.zeros((2, 8))
    for bad in (torch.zeros(4, dtype=torch.int64), torch.zeros(5, dtype=torch.int32), torch.zeros((4, 1), dtype=torch.int32),
                torch.zeros(8, dtype=torch.int32)[::2]):
        says("labels must be a contiguous int32 tensor of 4 values on the gallery's device", ops.knn, q, x, 3, bad)
        says("labels must be a contiguous int32 tensor of 4 values on x's device", ops.linear_svm_fit, x, bad, 2)
        says("labels must be a contiguous int32 tensor of 4 values on x's device", ops.rbf_svm_fit, x, bad, 2, 0.5)
        says("labels must be a contiguous int32 tensor of 4 values on x's device", ops.rbf_svm_predict, q, x, bad, 2, 0.5, None, None)
        says("labels must be a contiguous int32 tensor of 4 values on x's device", ops.rbf_svm_decision, q, x, bad, 2, 0.5, None, None)


def test_float64_tensors(host_torch):
    """A host tensor of the right type and shape is still no CUDA tensor: each site's sentence, with its shape and its own ending.
    A wrong shape or type on a CUDA tensor needs a device: tests/test_identification_shared_gpu.py."""
    from hse_facerec_tf_amd import ops
    torch = host_torch
    x, q, labels = torch.zeros((4, 8)), torch.zeros((2, 8)), torch.zeros(4, dtype=torch.int32)

    def f64(*shape):
        return torch.zeros(shape, dtype=torch.float64)
    says("mean must be a contiguous float64 CUDA tensor of shape (8,)", ops.pca_transform, x, f64(8), f64(2, 8))
    says("coef must be a contiguous float64 CUDA tensor of shape (1, 8) on x's device", ops.linear_svm_decision, x, f64(1, 8), f64(1))
    says("dual_coef must be a contiguous float64 CUDA tensor of shape (2, 4) on x's device",
         ops.rbf_svm_predict, q, x, labels, 3, 0.5, f64(2, 4), f64(3))
    says("order must be a contiguous int32 CUDA tensor", ops.flat_cuts, torch.zeros(4, dtype=torch.int32), f64(3), f64(1))
    says("y_true must be a contiguous int32 CUDA tensor", ops.partition_scores, labels, labels)


def test_the_protocols_check_their_keywords_in_one_order():
    """n_neighbors, pca, classifier (with svm_C and svm_gamma), pca_components -- all before the library or a device is touched."""
    from hse_facerec_tf_amd import identification
    X, y = np.zeros((8, 8), np.float32), np.arange(8) % 2
    for fn in (lambda **kw: identification.gallery_probe_identification(X, y, X, y, **kw),
               lambda **kw: identification.one_nn_identification(X, y, **kw)):
        says("n_neighbors=0 must be in 1..16", fn, n_neighbors=0, pca="gpu", classifier="svm")
        says("pca='gpu' must be 'host' (scikit-learn on the CPU) or 'device' (ops.pca_fit / ops.pca_transform)",
             fn, pca="gpu", classifier="svm")
        says("classifier='svm' must be 'knn' (ops.nn1 / ops.knn), 'linear_svm' (ops.linear_svm_fit) or 'rbf_svm' (ops.rbf_svm_fit)",
             fn, classifier="svm", pca="device", pca_components=300)
        says("n_neighbors=3 has no meaning with classifier='linear_svm': leave it at 1", fn, classifier="linear_svm", n_neighbors=3, svm_C=0.0)
        says("C=0.0 must be positive and finite", fn, classifier="linear_svm", svm_C=0.0, pca="device", pca_components=300)
        says("svm_gamma='auto' must be 'scale' or a positive finite number", fn, classifier="rbf_svm", svm_gamma="auto", svm_C=0.0)
        says("gamma=0.0 must be positive and finite", fn, classifier="rbf_svm", svm_gamma=0.0, pca="device", pca_components=300)
        says("pca_components=300 must be in 1..256", fn, pca="device", pca_components=300)
    says("n_neighbors=9 exceeds the 8 gallery rows", identification.gallery_probe_identification, X, y, X, y, n_neighbors=9)
    says("pca_components=8 exceeds n - 1 for the 8 rows to fit on", identification.gallery_probe_identification, X, y, X, y,
         pca="device", pca_components=8)
    says("n_neighbors=0 must be in 1..16", identification.cross_validated_1nn, X, y, [], n_neighbors=0)
