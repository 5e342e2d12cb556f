"""CPU suite: hsefr_knn's neighbour order and vote, restated in tests/knn_ref.py, against scikit-learn's KNeighborsClassifier on the
gallery / probe fixture; the entry point's place in the ABI; and its argument checks and those of the Python entry points, which come
before any device work."""
import ctypes
import os

import numpy as np
import pytest

import knn_ref
from oracle import identification as oid

from conftest import GOLDEN


def protocol_split():
    z = np.load(os.path.join(GOLDEN, "protocols.npz"))
    X, y = oid.synthetic_gallery(int(z["n_classes"]), int(z["dim"]), int(z["seed"]), float(z["noise"]))
    Xn, y2, kept = oid.filter_and_encode(X, y)
    assert np.array_equal(y2, z["y"])
    return z, X[kept], Xn


@pytest.mark.parametrize("normalised", [False, True])
@pytest.mark.parametrize("k", [2, 3, 5, 8])
def test_restatement_equals_sklearn_on_the_gallery_probe_split(k, normalised):
    """No two distances of a probe are equal here, so scikit-learn's neighbours are the (dist2, index) order's; the vote does tie (a few
    dozen probes per case see every label once, or two labels equally often) and must go to the smallest label."""
    from sklearn.neighbors import KNeighborsClassifier
    z, Xraw, Xn = protocol_split()
    A = Xn if normalised else Xraw
    g, p = z["gallery"], z["probe"]
    assert (len(p), len(g), A.shape[1]) == (146, 170, 256)
    clf = KNeighborsClassifier(n_neighbors=k, p=2).fit(A[g], z["y"][g])
    _, want_idx = clf.kneighbors(A[p])
    idx, d2, pred = knn_ref.knn(A[p], A[g], k, z["y"][g])
    assert np.array_equal(idx, want_idx)
    assert np.array_equal(pred, clf.predict(A[p]))
    assert np.all(np.diff(d2, axis=1) > 0)
    votes = np.sort(z["y"][g][idx], axis=1)
    counts = np.array([np.unique(v, return_counts=True)[1] for v in votes], dtype=object)
    tied = sum(1 for c in counts if (c == c.max()).sum() > 1)
    assert tied >= 10, "the fixture no longer exercises the smallest-label rule"


def test_restatement_orders_ties_by_index_and_votes_for_the_smallest_label():
    d2 = np.array([[4.0, 1.0, 1.0, 0.0, 1.0, 4.0]])
    idx, near, pred = knn_ref.knn_from_dist2(d2, 3, np.array([9, 7, -2, 5, 1, 1]))
    assert idx.tolist() == [[3, 1, 2]] and near.tolist() == [[0.0, 1.0, 1.0]]          # the boundary tie (index 4) stays out
    assert pred.tolist() == [-2]                                                       # labels 5, 7, -2: the smallest, not the nearest's
    assert knn_ref.knn_from_dist2(d2, 4, np.array([9, 7, 5, 5, 7, 1]))[2].tolist() == [5]     # 2 - 2: the smaller label
    assert knn_ref.knn_from_dist2(d2, 3, np.array([9, 8, 8, 5, 1, 1]))[2].tolist() == [8]     # 2 - 1: the majority


def test_knn_is_declared_exported_and_bound():
    from hse_facerec_tf_amd import _lib
    header = open(os.path.join(os.path.dirname(GOLDEN), os.pardir, "include", "hsefr.h")).read()
    assert "int hsefr_knn(const float* q, const float* g, int nq, int ng, int d, int k, int* nn_index, float* nn_dist2," in header
    assert "hsefr_knn" in _lib.SIGNATURES and len(_lib.SIGNATURES["hsefr_knn"][1]) == 11
    L = _lib.lib()
    assert hasattr(L, "hsefr_knn")
    assert L.hsefr_version() == 141


def test_knn_rejects_bad_arguments_without_a_gpu():
    from hse_facerec_tf_amd import _lib
    L = _lib.lib()
    buf = ctypes.create_string_buffer(256)
    p = ctypes.cast(buf, ctypes.c_void_p).value
    ok = dict(q=p, g=p, nq=4, ng=6, d=8, k=3, idx=p, dist=p, lab=p, pred=p)

    def call(**kw):
        a = dict(ok, **kw)
        rc = L.hsefr_knn(a["q"], a["g"], a["nq"], a["ng"], a["d"], a["k"], a["idx"], a["dist"], a["lab"], a["pred"], None)
        return rc, _lib.last_error()

    for kw, code, words in ((dict(k=0), _lib.ERR_INVALID, ("k=0", "ng=6")),
                            (dict(k=17, ng=40), _lib.ERR_INVALID, ("k=17", "ng=40")),
                            (dict(k=7), _lib.ERR_INVALID, ("k=7", "ng=6")),
                            (dict(d=12), _lib.ERR_UNSUPPORTED, ("d=12", "multiple of 8")),
                            (dict(idx=None), _lib.ERR_INVALID, ("null pointer",)),
                            (dict(q=None), _lib.ERR_INVALID, ("null pointer",)),
                            (dict(pred=None), _lib.ERR_INVALID, ("g_label and pred",)),
                            (dict(lab=None), _lib.ERR_INVALID, ("g_label and pred",)),
                            (dict(ng=0, k=1), _lib.ERR_INVALID, ("ng=0",)),
                            (dict(nq=-1), _lib.ERR_INVALID, ("nq=-1",))):
        rc, msg = call(**kw)
        assert rc == code, (kw, rc, msg)
        assert all(w in msg for w in words), (kw, msg)
        with pytest.raises(NotImplementedError if code == _lib.ERR_UNSUPPORTED else ValueError):
            _lib.check(rc, "hsefr_knn")
    assert call(nq=0)[0] == 0
    assert call(nq=0, q=None, g=None, idx=None, dist=None, lab=None, pred=None)[0] == 0
    assert call(nq=0, k=0)[0] == _lib.ERR_INVALID                                      # an empty probe set does not excuse a bad k


def test_python_entry_points_reject_bad_n_neighbors_without_a_gpu():
    import torch
    from hse_facerec_tf_amd import identification, ops
    q, g = torch.zeros((2, 8)), torch.zeros((5, 8))
    for k in (0, -1, 17, 6, 2.0, True):
        with pytest.raises(ValueError, match="n_neighbors"):
            ops.knn(q, g, k)
    X = np.zeros((6, 8), np.float32)
    y = np.array([0, 0, 1, 1, 2, 2])
    cv = [(np.arange(3), np.arange(3, 6))]
    for k in (0, 17):
        with pytest.raises(ValueError, match="n_neighbors"):
            identification.gallery_probe_identification(X, y, X, y, n_neighbors=k)
        with pytest.raises(ValueError, match="n_neighbors"):
            identification.one_nn_identification(X, y, n_neighbors=k)
        with pytest.raises(ValueError, match="n_neighbors"):
            identification.cross_validated_1nn(X, y, cv, n_neighbors=k)
    with pytest.raises(ValueError, match="exceeds the 6 gallery rows"):
        identification.gallery_probe_identification(X, y, X, y, n_neighbors=7)
