"""CPU suite for the chi-square and KL nearest-neighbour searches: the fp64 oracle of tests/metric_knn_ref.py against scikit-learn's
KNeighborsClassifier(metric=callable) with the reference's two callables, the oracle's exactness on the {0, 1, 3} inputs of the GPU
suite, the two entry points' place in the ABI, and every argument check that comes before device work -- the C level's, ops' and the
protocols' metric keyword."""
import ctypes
import os

import numpy as np
import pytest

import metric_knn_ref as ref
from oracle import identification as oid

from conftest import GOLDEN


def protocol_split():
    z = np.load(os.path.join(GOLDEN, "protocols.npz"))
    X, y = oid.synthetic_gallery(int(z["n_classes"]), int(z["dim"]), int(z["seed"]), float(z["noise"]))
    Xn, y2, kept = oid.filter_and_encode(X, y)
    assert np.array_equal(y2, z["y"])
    return z, X[kept], Xn


@pytest.mark.parametrize("normalised", [False, True])
@pytest.mark.parametrize("k", [1, 3])
@pytest.mark.parametrize("metric", ref.METRICS)
def test_oracle_equals_sklearn_with_the_references_callables(metric, k, normalised):
    """146 probes x 170 gallery rows x 256 non-negative features, raw and L2-normalised: scikit-learn's neighbours under the callable are
    the oracle's on every probe, its distances within 1e-6 relative (it evaluates x + 0.001 in float64, the oracle the float32 sum)."""
    from sklearn.neighbors import KNeighborsClassifier
    z, Xraw, Xn = protocol_split()
    A = (Xn if normalised else Xraw).astype(np.float32)
    g, p = z["gallery"], z["probe"]
    assert (len(p), len(g), A.shape[1]) == (146, 170, 256) and A.min() >= 0
    clf = KNeighborsClassifier(n_neighbors=k, metric=ref.CALLABLES[metric]).fit(A[g], z["y"][g])
    want_dist, want_idx = clf.kneighbors(A[p])
    idx, dist, pred = ref.knn(A[p], A[g], k, metric, z["y"][g])
    assert np.array_equal(idx, want_idx)
    rel = np.abs(dist - want_dist).max() / np.abs(want_dist).max()
    print("%s k=%d normalised=%s: max relative difference %.2e" % (metric, k, normalised, rel))
    assert np.all(np.abs(dist - want_dist) <= 1e-6 * np.abs(want_dist))
    assert np.array_equal(pred, clf.predict(A[p]))


def test_oracle_is_the_callables_pair_by_pair_and_asymmetric():
    rs = np.random.RandomState(0)
    x = np.maximum(rs.randn(5, 12), 0).astype(np.float32)
    y = np.maximum(rs.randn(7, 12), 0).astype(np.float32)
    x[1] = 0
    y[2] = 0
    for metric in ref.METRICS:
        D, B = ref.dist_and_bound(x, y, metric)
        want = np.array([[ref.CALLABLES[metric](a.astype(np.float64), b.astype(np.float64)) for b in y] for a in x])
        assert np.abs(D - want).max() <= 1e-6 * np.abs(want).max()
        assert np.all(B >= 0) and np.all(ref.dist_and_bound(x, x, metric)[0].diagonal() == 0)
    kl = ref.dist(x, y, "kl")
    assert not np.allclose(kl, ref.dist(y, x, "kl").T)                       # the probe is the first argument
    assert ref.dist(np.full((1, 4), 5, np.float32), np.full((1, 4), 9, np.float32), "kl")[0, 0] < 0     # not clamped at 0
    bad = ref.dist(np.array([[-0.5, 1, 1, 1]], np.float32), y[:, :4], "kl")
    assert np.all(np.isposinf(bad))                                          # an entry <= -0.001: NaN, returned as +inf
    assert ref.dist(np.array([[-2, 1, 0, 0]], np.float32), np.array([[1, 1, 0, 0]], np.float32), "chi2")[0, 0] == 0.0   # a negative sum adds 0


def test_exact_inputs_have_integer_oracle_distances_full_of_ties():
    """The {0, 1, 3} features of the GPU suite: every chi2 term is 0, 1 or 3 ((3 - 1)^2 / 4 = 1), so the oracle is an integer below 2^24
    that float32 must reproduce, and a probe sees dozens of tied gallery rows."""
    rs = np.random.RandomState(33 + 65 + 64)
    g = rs.choice([0, 1, 3], (65, 64)).astype(np.float32)
    q = rs.choice([0, 1, 3], (33, 64)).astype(np.float32)
    D = ref.dist(q, g, "chi2")
    assert np.array_equal(D, np.round(D)) and D.max() < 2 ** 24
    ties = np.mean([65 - len(np.unique(row)) for row in D])
    print("ties per row: %.1f" % ties)
    assert ties > 20


def test_the_two_entry_points_are_declared_exported_and_bound():
    from hse_facerec_tf_amd import _lib
    header = open(os.path.join(os.path.dirname(GOLDEN), os.pardir, "include", "hsefr.h")).read()
    assert "#define HSEFR_METRIC_CHI2 1" in header and "#define HSEFR_METRIC_KL 2" in header
    assert "int hsefr_metric_dist(const float* x, const float* y, int n, int m, int d, int metric, float* out, hsefr_stream_t stream);" in header
    assert "int hsefr_knn_metric(const float* q, const float* g, int nq, int ng, int d, int k, int metric, int* nn_index, float* nn_dist," in header
    assert len(_lib.SIGNATURES["hsefr_metric_dist"][1]) == 8 and len(_lib.SIGNATURES["hsefr_knn_metric"][1]) == 12
    L = _lib.lib()
    assert hasattr(L, "hsefr_metric_dist") and hasattr(L, "hsefr_knn_metric")
    assert L.hsefr_version() == 141
    assert os.path.getsize(_lib.LIB_PATH) < 4_000_000


def test_knn_metric_rejects_bad_arguments_without_a_gpu():
    from hse_facerec_tf_amd import _lib
    L = _lib.lib()
    buf = ctypes.create_string_buffer(256)
    p = ctypes.cast(buf, ctypes.c_void_p).value
    ok = dict(q=p, g=p, nq=4, ng=6, d=8, k=3, metric=1, idx=p, dist=p, lab=p, pred=p)

    def call(**kw):
        a = dict(ok, **kw)
        rc = L.hsefr_knn_metric(a["q"], a["g"], a["nq"], a["ng"], a["d"], a["k"], a["metric"], a["idx"], a["dist"], a["lab"], a["pred"], None)
        return rc, _lib.last_error()

    for kw, words in ((dict(metric=0), ("metric=0",)),
                      (dict(metric=3), ("metric=3",)),
                      (dict(k=0), ("k=0", "ng=6")),
                      (dict(k=17, ng=40), ("k=17", "ng=40")),
                      (dict(k=7), ("k=7", "ng=6")),
                      (dict(d=10), ("d=10", "multiple of 4")),
                      (dict(d=0), ("d=0",)),
                      (dict(idx=None), ("null pointer",)),
                      (dict(q=None), ("null pointer",)),
                      (dict(g=None), ("null pointer",)),
                      (dict(pred=None), ("g_label and pred",)),
                      (dict(lab=None), ("g_label and pred",)),
                      (dict(ng=0, k=1), ("ng=0",)),
                      (dict(nq=-1), ("nq=-1",))):
        rc, msg = call(**kw)
        assert rc == _lib.ERR_INVALID, (kw, rc, msg)
        assert msg.startswith("knn_metric:") and all(w in msg for w in words), (kw, msg)
        with pytest.raises(ValueError, match="hsefr_knn_metric"):
            _lib.check(rc, "hsefr_knn_metric")
    for metric in (1, 2):
        assert call(nq=0, metric=metric)[0] == 0
        assert call(nq=0, metric=metric, q=None, g=None, idx=None, dist=None, lab=None, pred=None)[0] == 0
    assert call(nq=0, k=0)[0] == _lib.ERR_INVALID                            # an empty probe set does not excuse a bad k
    assert call(nq=0, metric=0)[0] == _lib.ERR_INVALID                       # nor a bad metric


def test_metric_dist_rejects_bad_arguments_without_a_gpu():
    from hse_facerec_tf_amd import _lib
    L = _lib.lib()
    buf = ctypes.create_string_buffer(256)
    p = ctypes.cast(buf, ctypes.c_void_p).value
    ok = dict(x=p, y=p, n=4, m=6, d=8, metric=2, out=p)

    def call(**kw):
        a = dict(ok, **kw)
        return L.hsefr_metric_dist(a["x"], a["y"], a["n"], a["m"], a["d"], a["metric"], a["out"], None), _lib.last_error()

    for kw, words in ((dict(metric=0), ("metric=0",)), (dict(metric=3), ("metric=3",)), (dict(d=6), ("d=6", "multiple of 4")),
                      (dict(d=-4), ("d=-4",)), (dict(x=None), ("null pointer",)), (dict(y=None), ("null pointer",)),
                      (dict(out=None), ("null pointer",)), (dict(n=-1), ("n=-1",)), (dict(m=-2), ("m=-2",)),
                      (dict(n=65535 * 64 + 1), ("n=4194241",))):
        rc, msg = call(**kw)
        assert rc == _lib.ERR_INVALID, (kw, rc, msg)
        assert msg.startswith("metric_dist:") and all(w in msg for w in words), (kw, msg)
    assert call(n=0)[0] == 0 and call(m=0, x=None, y=None, out=None)[0] == 0


def test_ops_check_the_metric_before_anything_is_loaded():
    import torch
    from hse_facerec_tf_amd import ops
    assert [ops.check_metric(m) for m in ("l2", "chi2", "kl")] == ["l2", "chi2", "kl"]
    for bad in ("cosine", "CHI2", "", None, 1, b"kl"):
        with pytest.raises(ValueError, match="metric="):
            ops.check_metric(bad)
    q, g = torch.zeros((2, 8)), torch.zeros((5, 8))
    for metric in ("chi2", "kl"):
        for k in (0, 17, 6, 2.0, True):
            with pytest.raises(ValueError, match="n_neighbors"):
                ops.knn(q, g, k, metric=metric)
    with pytest.raises(ValueError, match="metric='cosine'"):
        ops.knn(q, g, 1, metric="cosine")
    with pytest.raises(ValueError, match="metric="):
        ops.metric_distances(q, g, metric="euclid")
    with pytest.raises(ValueError, match="pairwise_distances"):
        ops.metric_distances(q, g, metric="l2")


def test_the_protocols_check_the_metric_keyword_after_the_others():
    from hse_facerec_tf_amd import identification
    X = np.zeros((6, 8), np.float32)
    y = np.array([0, 0, 1, 1, 2, 2])
    cv = [(np.arange(3), np.arange(3, 6))]
    protocols = (lambda **kw: identification.gallery_probe_identification(X, y, X, y, **kw),
                 lambda **kw: identification.one_nn_identification(X, y, **kw))
    for run in protocols + (lambda **kw: identification.cross_validated_1nn(X, y, cv, **kw),):
        with pytest.raises(ValueError, match="metric='cosine' must be"):
            run(metric="cosine")
        with pytest.raises(ValueError, match="n_neighbors"):                 # the earlier checks come first
            run(metric="cosine", n_neighbors=0)
    for run in protocols:
        for metric in ("chi2", "kl"):
            for classifier in ("linear_svm", "rbf_svm"):
                with pytest.raises(ValueError, match="metric='%s' is a k-NN distance" % metric):
                    run(metric=metric, classifier=classifier)
            with pytest.raises(ValueError, match="projections are signed"):
                run(metric=metric, pca_components=4)
            with pytest.raises(ValueError, match="pca="):
                run(metric=metric, pca="gpu", pca_components=4)
            with pytest.raises(ValueError, match="classifier="):
                run(metric=metric, classifier="forest")
            with pytest.raises(ValueError, match="C must be a number"):
                run(metric=metric, classifier="linear_svm", svm_C="big")
    kw = identification._check_keywords(n_neighbors=3, metric="kl")
    assert kw.metric == "kl" and kw.n_neighbors == 3 and identification._check_keywords().metric == "l2"
