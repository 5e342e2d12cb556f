"""CPU suite: the host half of average / complete / weighted linkage (hse_facerec_tf_amd/clustering.py) -- Z assembly from merge
records against scipy through the NumPy restatement of the device's rounds (tests/hier_linkage_ref.py), the order of equal-height
merges, method-name validation -- and the argument checks of hsefr_hier_linkage, which come before any device call."""
import ctypes

import numpy as np
import pytest
from scipy.cluster import hierarchy as hac
from scipy.spatial.distance import squareform

import hier_linkage_ref as href
import linkage_ref as ref


def random_matrix(n, seed, ties=False):
    rs = np.random.RandomState(seed)
    D = rs.randint(0, 8, (n, n)).astype(np.float64) if ties else rs.rand(n, n)
    D = np.triu(D, 1)
    return D + D.T


def away_from(heights, ts, gap=1e-9):
    return [t for t in ts if np.abs(np.asarray(heights) - t).min() > gap]


@pytest.mark.parametrize("method", ["average", "complete", "weighted"])
@pytest.mark.parametrize("n", [2, 3, 7, 60, 250])
def test_rounds_and_z_assembly_equal_scipy(method, n):
    from hse_facerec_tf_amd import clustering
    D = random_matrix(n, 40 + n)
    a, b, h, r = href.rnn_rounds(D, method)
    perm = np.random.RandomState(n).permutation(n - 1)                 # the device leaves records unordered within a round
    Z = clustering.linkage_from_merges(a[perm], b[perm], h[perm], r[perm], n)
    Zs = hac.linkage(squareform(D, checks=False), method)
    assert hac.is_valid_linkage(Z)
    assert np.array_equal(Z[:, [0, 1, 3]], Zs[:, [0, 1, 3]])
    if method == "complete":
        assert np.array_equal(Z[:, 2], Zs[:, 2])
    else:
        assert np.allclose(Z[:, 2], Zs[:, 2], rtol=1e-12, atol=0)
    href.check_records(D, method, a, b, h, r)
    for t in away_from(Zs[:, 2], np.linspace(Zs[0, 2] - 0.05, Zs[-1, 2] + 0.05, 15)):
        assert np.array_equal(ref.canonical(clustering.fcluster_distance(Z, t)), ref.canonical(hac.fcluster(Zs, t, "distance")))


@pytest.mark.parametrize("method", ["average", "complete", "weighted"])
def test_rounds_on_ties_give_a_valid_hierarchy(method):
    from hse_facerec_tf_amd import clustering
    n = 120
    D = random_matrix(n, 9, ties=True)
    a, b, h, r = href.rnn_rounds(D, method)
    href.check_records(D, method, a, b, h, r)
    Z = clustering.linkage_from_merges(a, b, h, r, n)
    assert hac.is_valid_linkage(Z)
    assert np.all(np.diff(Z[:, 2]) >= 0)


def test_equal_height_child_precedes_parent():
    from hse_facerec_tf_amd import clustering
    # round 0 joins 2 and 3; round 1 joins 0 with that pair at the same height.  (height, lower, higher) would take (0, 2) first.
    # a last merge in round 2 completes the hierarchy
    Z = clustering.linkage_from_merges([0, 2, 0], [2, 3, 1], [1.0, 1.0, 1.0], [1, 0, 2], 4)
    assert Z.tolist() == [[2, 3, 1.0, 2], [0, 4, 1.0, 3], [1, 5, 1.0, 4]]
    assert hac.is_valid_linkage(Z)
    # within one round, equal heights go by the surviving point
    Z = clustering.linkage_from_merges([2, 0, 0], [3, 1, 2], [1.0, 1.0, 2.0], [0, 0, 1], 4)
    assert Z.tolist() == [[0, 1, 1.0, 2], [2, 3, 1.0, 2], [4, 5, 2.0, 4]]


def test_merge_records_are_checked():
    from hse_facerec_tf_amd import clustering
    with pytest.raises(ValueError):
        clustering.linkage_from_merges([0], [1], [1.0], [0], 4)
    with pytest.raises(RuntimeError):
        clustering.linkage_from_merges([0, 0, 1], [1, 2, 2], [1.0, 2.0, 3.0], [0, 1, 2], 4)     # a cycle: point 3 never joins
    with pytest.raises(RuntimeError):
        clustering.linkage_from_merges([0, 1, -1], [1, 2, 3], [1.0, 2.0, 3.0], [0, 1, 2], 4)


@pytest.mark.parametrize("bad", ["ward", "centroid", "median", "Average", "", None])
def test_unsupported_methods_raise_before_any_device_work(bad):
    from hse_facerec_tf_amd import clustering
    D = random_matrix(5, 1)
    for call in (lambda: clustering.linkage_dense(D, bad), lambda: clustering.linkage(np.ones((5, 8), np.float32), bad),
                 lambda: clustering.get_facial_clusters(D, 0.5, method=bad),
                 lambda: clustering.get_facial_clusters(D[:1, :1], 0.5, method=bad),
                 lambda: clustering.cluster_faces(np.ones((5, 8), np.float32), 0.5, method=bad)):
        with pytest.raises(ValueError) as e:
            call()
        assert "average" in str(e.value) and "complete" in str(e.value) and "weighted" in str(e.value)
    assert clustering.LINKAGE_METHODS == ("single", "average", "complete", "weighted")


def test_hier_linkage_rejects_bad_arguments_without_a_gpu():
    from hse_facerec_tf_amd import _lib
    L = _lib.lib()
    buf = ctypes.create_string_buffer(256)
    p = ctypes.cast(buf, ctypes.c_void_p).value
    ok = dict(x=p, n=4, d=8, born=None, year=None, dense=None, method=0, ma=p, mb=p, mh=p, mr=p)

    def call(**kw):
        a = dict(ok, **kw)
        return L.hsefr_hier_linkage(a["x"], a["n"], a["d"], a["born"], a["year"], a["dense"], a["method"], a["ma"], a["mb"], a["mh"],
                                    a["mr"], None)
    cases = [dict(n=0), dict(n=-3), dict(x=None), dict(dense=p), dict(d=12), dict(d=0), dict(born=p), dict(year=p), dict(method=3),
             dict(method=-1), dict(ma=None), dict(mb=None), dict(mh=None), dict(mr=None), dict(x=None, dense=p, born=p, year=p)]
    for kw in cases:
        assert call(**kw) == _lib.ERR_INVALID, kw
        assert "hier_linkage" in _lib.last_error()
    rc = L.hsefr_hier_linkage(p, 4, 8, None, None, None, 5, p, p, p, p, None)
    assert rc == _lib.ERR_INVALID and "method" in _lib.last_error()
