"""CPU suite: the DBSCAN rule of csrc/dbscan.hip, restated in tests/dbscan_ref.py, against scikit-learn (labels_ and
core_sample_indices_) and, with min_samples = 1, against scipy's single-linkage cut; the argument checks of hsefr_dbscan and of the
Python entry points, which come before any device work."""
import ctypes

import numpy as np
import pytest
from scipy.cluster import hierarchy as hac
from scipy.spatial.distance import squareform
from sklearn.cluster import DBSCAN

import dbscan_ref as dref
import linkage_ref as ref


def symmetric(n, rs, kind):
    if kind == "rand":
        D = rs.rand(n, n)
    elif kind == "ties":
        D = rs.randint(0, rs.randint(2, 10), (n, n)).astype(np.float64)
    else:                                                       # points on a small integer grid: duplicates and exact ties
        X = rs.randint(0, 3, (n, 2)).astype(np.float64)
        D = np.sqrt(((X[:, None] - X[None]) ** 2).sum(-1))
    D = np.triu(D, 1)
    return D + D.T


def sklearn_dbscan(D, eps, min_samples):
    db = DBSCAN(eps=eps, min_samples=min_samples, metric="precomputed").fit(D)
    return db.core_sample_indices_.astype(np.int64), db.labels_.astype(np.int64)


def test_restatement_equals_sklearn_on_symmetric_matrices():
    rs = np.random.RandomState(0)
    cases = 0
    for trial in range(2500):
        n = [1, 2][trial % 2] if trial < 200 else int(rs.randint(3, 60))
        kind = ("rand", "ties", "grid")[trial % 3]
        D = symmetric(n, rs, kind)
        vals = D[np.triu_indices(n, 1)]
        eps = float(rs.choice(vals)) if len(vals) and rs.rand() < 0.7 and vals.max() > 0 else float(rs.uniform(0.05, 1.5))
        if eps <= 0:
            eps = 1.0
        min_samples = int(rs.randint(1, n + 3))
        want = sklearn_dbscan(D, eps, min_samples)
        got = dref.dbscan_dense(D, eps, min_samples)
        assert np.array_equal(got[0], want[0]), (trial, n, eps, min_samples)
        assert np.array_equal(got[1], want[1]), (trial, n, eps, min_samples)
        cases += 1
    assert cases == 2500


def test_min_samples_one_is_the_single_linkage_cut():
    rs = np.random.RandomState(1)
    for trial in range(200):
        n = int(rs.randint(2, 80))
        D = symmetric(n, rs, ("rand", "ties", "grid")[trial % 3])
        Z = hac.linkage(squareform(D, checks=False), "single")
        eps = float(rs.choice(Z[:, 2])) if trial % 2 else float(rs.uniform(0.05, 1.0))
        if eps <= 0:
            eps = 0.5
        core, labels = dref.dbscan_dense(D, eps, 1)
        assert np.array_equal(core, np.arange(n))
        assert np.array_equal(ref.canonical(labels), ref.canonical(hac.fcluster(Z, eps, "distance")))


def test_restatement_reads_the_upper_triangle():
    rs = np.random.RandomState(2)
    D = rs.rand(40, 40)                                         # asymmetric, nonzero diagonal
    U = np.triu(D, 1)
    for eps, m in ((0.1, 2), (0.2, 4), (0.05, 1)):
        assert all(np.array_equal(a, b) for a, b in zip(dref.dbscan_dense(D, eps, m), sklearn_dbscan(U + U.T, eps, m)))


def test_dbscan_rejects_bad_arguments_without_a_gpu():
    from hse_facerec_tf_amd import _lib
    L = _lib.lib()
    buf = ctypes.create_string_buffer(256)
    p = ctypes.cast(buf, ctypes.c_void_p).value
    ok = dict(x=p, n=4, d=8, born=None, year=None, dense=None, eps=0.5, m=2, labels=p, core=p)

    def call(**kw):
        a = dict(ok, **kw)
        return L.hsefr_dbscan(a["x"], a["n"], a["d"], a["born"], a["year"], a["dense"], a["eps"], a["m"], a["labels"], a["core"], None)
    cases = [dict(n=0), dict(n=-3), dict(x=None), dict(dense=p), dict(labels=None), dict(born=p), dict(year=p),
             dict(x=None, dense=p, born=p, year=p), dict(d=12), dict(d=0), dict(d=-8), dict(eps=0.0), dict(eps=-1.0),
             dict(eps=float("nan")), dict(eps=float("inf")), dict(m=0), dict(m=-5)]
    for kw in cases:
        assert call(**kw) == _lib.ERR_INVALID, kw
        assert _lib.last_error().startswith("dbscan:"), (kw, _lib.last_error())
    assert "hsefr_dbscan" in _lib.SIGNATURES


def test_python_entry_points_reject_bad_arguments_before_device_work():
    from hse_facerec_tf_amd import clustering
    X = np.ones((5, 8), np.float32)
    D = symmetric(5, np.random.RandomState(3), "rand")
    bad_eps = [0, 0.0, -1.0, float("nan"), float("inf"), "0.5", None, True]
    bad_min = [0, -1, 2.0, "3", None, True]
    for eps in bad_eps:
        for call in (lambda: clustering.dbscan(X, eps=eps), lambda: clustering.dbscan_dense(D, eps=eps),
                     lambda: clustering.get_facial_clusters(D, eps, method="dbscan"),
                     lambda: clustering.get_facial_clusters(D[:1, :1], eps, method="dbscan"),
                     lambda: clustering.cluster_faces(X, eps, method="dbscan")):
            with pytest.raises(ValueError):
                call()
    for m in bad_min:
        for call in (lambda: clustering.dbscan(X, 0.5, m), lambda: clustering.dbscan_dense(D, 0.5, m),
                     lambda: clustering.get_facial_clusters(D, 0.5, no_images_in_cluster=m, method="dbscan"),
                     lambda: clustering.cluster_faces(X, 0.5, min_cluster_size=m, method="dbscan")):
            with pytest.raises(ValueError):
                call()
    bad_matrices = [np.ones((3, 4)), np.ones((0, 0)), np.ones(5), np.where(np.eye(5, dtype=bool), np.nan, D), D - 0.5,
                    np.where(np.eye(5, dtype=bool), -1.0, D), np.full((5, 5), np.inf)]
    for M in bad_matrices:
        for call in (lambda: clustering.dbscan_dense(M, 0.5, 2), lambda: clustering.get_facial_clusters(M, 0.5, method="dbscan")):
            with pytest.raises(ValueError):
                call()
    bad_features = [np.ones((0, 8), np.float32), np.ones(8, np.float32), np.full((5, 8), np.nan, np.float32),
                    np.full((5, 8), np.inf)]
    for F in bad_features:
        for call in (lambda: clustering.dbscan(F, 0.5, 2), lambda: clustering.cluster_faces(F, 0.5, method="dbscan")):
            with pytest.raises(ValueError):
                call()
    born = np.full(5, 1990.0)
    for by, yr in ((born, None), (None, born), (born, born), (born[:4], born[:4] + 5), (born, np.full(5, np.nan))):
        with pytest.raises(ValueError):
            clustering.dbscan(X, 0.5, 2, by, yr)
        with pytest.raises(ValueError):
            clustering.cluster_faces(X, 0.5, by, yr, method="dbscan")


def test_linkage_entry_points_still_reject_dbscan():
    from hse_facerec_tf_amd import clustering
    D = symmetric(5, np.random.RandomState(4), "rand")
    for call in (lambda: clustering.linkage_dense(D, "dbscan"), lambda: clustering.linkage(np.ones((5, 8), np.float32), "dbscan")):
        with pytest.raises(ValueError) as e:
            call()
        assert "average" in str(e.value) and "complete" in str(e.value) and "weighted" in str(e.value)
    assert clustering.LINKAGE_METHODS == ("single", "average", "complete", "weighted")
    for bad in ("DBSCAN", "optics"):
        with pytest.raises(ValueError):
            clustering.get_facial_clusters(D, 0.5, method=bad)
