"""CPU suite: the rank-order rule of csrc/rank_order.hip, restated in tests/rank_order_ref.py, against the reference's recorded clusters
(tests/golden/rank_order_reference.npz, written by tools/record_rank_order_golden.py); the argument checks of hsefr_rank_order and of the
Python entry points, which come before any device work."""
import ctypes
import os

import numpy as np
import pytest

import rank_order_ref as ror

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "rank_order_reference.npz")
CASES = 37
MIN_MARGIN = 1e-9          # reordering an fp64 sum of <= 1e4 terms moves nd by ~1e-12 relative; the reference's own sum is that uncertain


def golden_cases():
    """-> [(kind, n, classes, seed, norm, rank, the reference's clusters as returned)]"""
    g = np.load(GOLDEN)
    out, at_size, at_member = [], 0, 0
    for i in range(len(g["n"])):
        clusters = []
        for s in g["sizes"][at_size:at_size + int(g["clusters"][i])]:
            clusters.append(g["members"][at_member:at_member + int(s)].tolist())
            at_member += int(s)
        at_size += int(g["clusters"][i])
        out.append((str(g["kind"][i]), int(g["n"][i]), int(g["classes"][i]), int(g["seed"][i]), float(g["norm"][i]), float(g["rank"][i]),
                    clusters))
    assert at_size == len(g["sizes"]) and at_member == len(g["members"])
    return out


def golden_matrix(kind, n, classes, seed):
    return (ror.coincident_case(n, seed) if kind == "coincident" else ror.integer_case(n, classes, seed))[1]


def test_restatement_returns_the_recorded_reference_clusters():
    """Cluster order included; the members of a cluster are compared as a sorted list (the reference lists them in set order)."""
    cases = 0
    sizes, kinds, thresholds = set(), set(), set()
    for kind, n, classes, seed, norm, rank, want in golden_cases():
        got, iters, margin = ror.rank_order(golden_matrix(kind, n, classes, seed), norm, rank)
        print("%s n=%d seed=%d (%g, %g): %d clusters, %d iterations, margin %.3g" % (kind, n, seed, norm, rank, len(got), iters, margin))
        assert got == [sorted(c) for c in want], (kind, n, seed, norm, rank)
        assert margin >= MIN_MARGIN, (kind, n, seed, norm, rank, margin)
        assert iters >= 1
        cases += 1
        sizes.add(n)
        kinds.add(kind)
        thresholds.add((norm, rank))
    assert cases == CASES
    assert {1, 2, 12, 13, 19, 20, 21, 1000} <= sizes and kinds == {"integer", "coincident"}
    assert thresholds == {(0.9, 14.0), (1.06, 16.0), (1.1, 20.0)}


def test_fixture_has_clusters_and_the_zero_guard_case():
    cases = golden_cases()
    assert sum(len(c[6]) > 0 for c in cases) >= 25
    for kind, n, classes, seed, norm, rank, want in cases:
        assert all(len(c) >= 2 for c in want)
        assert [len(c) for c in want] == sorted((len(c) for c in want), reverse=True)
        if n == 1:
            assert want == []
        if kind == "coincident":
            flat = sorted(c for c in map(sorted, want) if c[0] < 28)
            assert any(set(range(15)) <= set(c) for c in flat) and any(set(range(15, 28)) <= set(c) for c in flat)


def test_restatement_reads_the_upper_triangle_and_no_diagonal():
    rs = np.random.RandomState(2)
    _, D = ror.integer_case(120, 8, 11)
    A = np.triu(D, 1) + np.tril(rs.rand(120, 120), -1) + np.diag(rs.rand(120) + 1)
    assert ror.rank_order(A, 1.06, 16)[:2] == ror.rank_order(D, 1.06, 16)[:2]


def test_rank_order_rejects_bad_arguments_without_a_gpu():
    from hse_facerec_tf_amd import _lib
    L = _lib.lib()
    buf = ctypes.create_string_buffer(256)
    p = ctypes.cast(buf, ctypes.c_void_p).value
    iters = ctypes.c_int(0)
    ok = dict(x=p, n=4, d=8, born=None, year=None, dense=None, norm=0.9, rank=14.0, labels=p)

    def call(**kw):
        a = dict(ok, **kw)
        return L.hsefr_rank_order(a["x"], a["n"], a["d"], a["born"], a["year"], a["dense"], a["norm"], a["rank"], a["labels"],
                                  ctypes.byref(iters), None)
    cases = [dict(n=0), dict(n=-3), dict(x=None), dict(dense=p), dict(labels=None), dict(born=p), dict(year=p),
             dict(x=None, dense=p, born=p, year=p), dict(d=12), dict(d=0), dict(d=-8), dict(norm=0.0), dict(norm=-1.0),
             dict(norm=float("nan")), dict(norm=float("inf")), dict(rank=0.0), dict(rank=-5.0), dict(rank=float("nan")),
             dict(rank=float("inf"))]
    for kw in cases:
        assert call(**kw) == _lib.ERR_INVALID, kw
        assert _lib.last_error().startswith("rank_order:"), (kw, _lib.last_error())
    thr = (ctypes.c_double * 4)(0.9, 14.0, 1.06, 0.0)
    for pairs, t in ((2, thr), (0, thr), (-1, thr), (1, None)):
        assert L.hsefr_rank_order_sweep(p, 4, 8, None, None, None, t, pairs, p, None, None) == _lib.ERR_INVALID, pairs
        assert _lib.last_error().startswith("rank_order:")
    assert "hsefr_rank_order" in _lib.SIGNATURES and "hsefr_rank_order_sweep" in _lib.SIGNATURES


def test_python_entry_points_reject_bad_arguments_before_device_work():
    from hse_facerec_tf_amd import clustering
    X = np.ones((5, 8), np.float32)
    _, D = ror.integer_case(5, 2, 3)
    bad = [0, 0.0, -1.0, float("nan"), float("inf"), "0.5", None, True]
    for v in bad:
        for call in (lambda: clustering.rank_order(X, norm_threshold=v), lambda: clustering.rank_order(X, rank_threshold=v),
                     lambda: clustering.rank_order_dense(D, norm_threshold=v), lambda: clustering.rank_order_dense(D, rank_threshold=v),
                     lambda: clustering.rank_order_dense(D, thresholds=[(0.9, 14), (v, 14)]),
                     lambda: clustering.rank_order(X, thresholds=[(0.9, v)]),
                     lambda: clustering.get_facial_clusters(D, (v, 14), method="rankorder"),
                     lambda: clustering.get_facial_clusters(D, (0.9, v), method="rankorder"),
                     lambda: clustering.get_facial_clusters(D[:1, :1], (v, 14), method="rankorder"),
                     lambda: clustering.cluster_faces(X, (v, 14), method="rankorder"),
                     lambda: clustering.cluster_faces(X, (0.9, v), method="rankorder")):
            with pytest.raises(ValueError):
                call()
    for v in (0, -1.0, float("nan"), float("inf"), "0.5", None, True, (0.9,), (0.9, 14, 3), ()):
        for call in (lambda: clustering.get_facial_clusters(D, v, method="rankorder"),
                     lambda: clustering.cluster_faces(X, v, method="rankorder")):
            with pytest.raises(ValueError):
                call()
    for t in ([], 5, [0.9, 14], [(0.9, 14, 1)]):
        with pytest.raises(ValueError):
            clustering.rank_order_dense(D, thresholds=t)
    bad_matrices = [np.ones((3, 4)), np.ones((0, 0)), np.ones(5), np.where(np.eye(5, dtype=bool), np.nan, D), D - 50,
                    np.where(np.eye(5, dtype=bool), -1.0, D), np.full((5, 5), np.inf)]
    for M in bad_matrices:
        for call in (lambda: clustering.rank_order_dense(M), lambda: clustering.get_facial_clusters(M, (0.9, 14), method="rankorder")):
            with pytest.raises(ValueError):
                call()
    bad_features = [np.ones((0, 8), np.float32), np.ones(8, np.float32), np.full((5, 8), np.nan, np.float32), np.full((5, 8), np.inf)]
    for F in bad_features:
        for call in (lambda: clustering.rank_order(F), lambda: clustering.cluster_faces(F, (0.9, 14), method="rankorder")):
            with pytest.raises(ValueError):
                call()
    born = np.full(5, 1990.0)
    for by, yr in ((born, None), (None, born), (born, born), (born[:4], born[:4] + 5), (born, np.full(5, np.nan))):
        with pytest.raises(ValueError):
            clustering.rank_order(X, born_years=by, photo_years=yr)
        with pytest.raises(ValueError):
            clustering.cluster_faces(X, (0.9, 14), by, yr, method="rankorder")


def test_linkage_entry_points_reject_rankorder():
    from hse_facerec_tf_amd import clustering
    _, D = ror.integer_case(5, 2, 4)
    for call in (lambda: clustering.linkage_dense(D, "rankorder"), lambda: clustering.linkage(np.ones((5, 8), np.float32), "rankorder")):
        with pytest.raises(ValueError) as e:
            call()
        assert "average" in str(e.value) and "complete" in str(e.value) and "weighted" in str(e.value)
        assert "rankorder" not in str(e.value).split("supported methods")[1]
    assert clustering.LINKAGE_METHODS == ("single", "average", "complete", "weighted")
    assert clustering.CLUSTER_METHODS == clustering.LINKAGE_METHODS + ("dbscan", "rankorder")
    for bad in ("RankOrder", "rank-order", "rank_order"):
        with pytest.raises(ValueError):
            clustering.get_facial_clusters(D, (0.9, 14), method=bad)
