"""CPU suite: the host half of single-linkage clustering (hse_facerec_tf_amd/clustering.py) against scipy -- the fp64 restatement
of tests/linkage_ref.py, Z assembly from spanning-tree edges, flat cuts, the same-photo split's complete linkage, B-cubed -- and
the argument checks of hsefr_single_linkage, which come before any device call."""
import ctypes

import numpy as np
import pytest
from scipy.cluster import hierarchy as hac
from scipy.spatial.distance import squareform

import linkage_ref as ref
from hse_facerec_tf_amd import clustering


def random_matrix(n, seed, ties=False):
    rs = np.random.RandomState(seed)
    D = rs.randint(0, 6, (n, n)).astype(np.float64) if ties else rs.rand(n, n)
    D = np.triu(D, 1)
    return D + D.T


def scipy_labels(Z, t):
    return ref.canonical(hac.fcluster(Z, t, "distance"))


@pytest.mark.parametrize("n,seed,ties", [(2, 0, False), (3, 1, True), (17, 2, False), (64, 3, True), (150, 4, False), (200, 5, True)])
def test_restatement_equals_scipy(n, seed, ties):
    D = random_matrix(n, seed, ties)
    Z = hac.linkage(squareform(D, checks=False), "single")
    a, b, h = ref.prim_mst(D)
    assert np.array_equal(np.sort(h), Z[:, 2])
    for t in ref.cut_thresholds(h):
        assert np.array_equal(ref.flat_cut(n, a, b, h, t), scipy_labels(Z, t)), t


def test_restatement_reads_the_upper_triangle():
    D = random_matrix(40, 7)
    junk = np.tril(np.random.RandomState(8).rand(40, 40) * 5, -1)
    Za = hac.linkage(squareform(np.triu(D) + junk, checks=False), "single")
    a, b, h = ref.prim_mst(np.triu(D) + junk)
    assert np.array_equal(np.sort(h), Za[:, 2])


def test_z_from_a_hand_made_tree():
    #   0 -1.0- 1 -0.5- 2     3 -1.0- 4, joined 2 -2.0- 3, and 5 hanging on 0 at 2.0 (ties in height on purpose)
    a = [3, 1, 0, 2, 5]
    b = [4, 2, 1, 3, 0]
    h = [1.0, 0.5, 1.0, 2.0, 2.0]
    Z = clustering.linkage_from_edges(a, b, h, 6)
    assert hac.is_valid_linkage(Z)
    assert Z.shape == (5, 4) and (Z[:, 0] < Z[:, 1]).all()
    assert np.array_equal(Z[:, 2], [0.5, 1.0, 1.0, 2.0, 2.0])
    assert Z[-1, 3] == 6
    # sorted by (height, lower endpoint, higher endpoint): the 1.0 edges come as (0,1) then (3,4)
    assert Z[1].tolist() == [0.0, 6.0, 1.0, 3.0] and Z[2].tolist() == [3.0, 4.0, 1.0, 2.0]
    for t in [0.0, 0.5, 0.75, 1.0, 1.5, 2.0, 3.0]:
        assert np.array_equal(ref.canonical(clustering.fcluster_distance(Z, t)), scipy_labels(Z, t)), t
    with pytest.raises(RuntimeError):
        clustering.linkage_from_edges([0, 1, 0], [1, 0, 2], [1.0, 1.0, 1.0], 4)      # a cycle, no spanning tree


@pytest.mark.parametrize("n,seed,ties", [(5, 0, True), (33, 1, False), (120, 2, True), (257, 3, False)])
def test_z_and_cuts_from_spanning_tree_equal_scipy(n, seed, ties):
    D = random_matrix(n, seed, ties)
    a, b, h = ref.prim_mst(D)
    perm = np.random.RandomState(seed).permutation(n - 1)          # discovery order does not matter
    Z = clustering.linkage_from_edges(b[perm], a[perm], h[perm], n)
    Zs = hac.linkage(squareform(D, checks=False), "single")
    assert hac.is_valid_linkage(Z)
    assert np.array_equal(Z[:, 2], Zs[:, 2])
    ts = ref.cut_thresholds(h)
    got = clustering.fcluster_distance(Z, ts)
    assert got.shape == (len(ts), n)
    for t, lab in zip(ts, got):
        assert lab.min() == 1 and lab.max() == len(np.unique(lab))
        assert np.array_equal(ref.canonical(lab), scipy_labels(Zs, t)), t
        assert np.array_equal(ref.canonical(lab), ref.canonical(clustering.fcluster_distance(Z, float(t))))


def test_fcluster_distance_on_scipy_z():
    D = random_matrix(90, 11)
    for method in ("single", "complete"):
        Z = hac.linkage(squareform(D, checks=False), method)
        for t in ref.cut_thresholds(Z[:, 2]):
            assert np.array_equal(ref.canonical(clustering.fcluster_distance(Z, t)), scipy_labels(Z, t))


@pytest.mark.parametrize("k,seed", [(2, 0), (3, 1), (9, 2), (25, 3), (60, 4)])
def test_same_photo_complete_linkage_equals_scipy(k, seed):
    rs = np.random.RandomState(seed)
    D = rs.rand(k, k) * 1.5
    D = np.triu(D, 1)
    D = D + D.T
    photo = rs.randint(0, max(1, k // 2), k)
    same = (photo[:, None] == photo[None, :]) & ~np.eye(k, dtype=bool)
    P = D + 100.0 * same
    want = ref.canonical(hac.fcluster(hac.linkage(squareform(P), "complete"), 50.0, "distance"))
    assert np.array_equal(ref.canonical(clustering.complete_linkage_labels(P, 50.0)), want)
    parts = clustering._split_same_photo(D, photo)
    lab = np.empty(k, dtype=np.int64)
    for i, p in enumerate(parts):
        lab[p] = i
    assert np.array_equal(ref.canonical(lab), want)
    for p in parts:                                     # no photo twice in one part
        assert len(np.unique(photo[p])) == len(p)
    # complete linkage at every threshold, not only 50
    Zc = hac.linkage(squareform(D), "complete")
    for t in ref.cut_thresholds(Zc[:, 2]):
        assert np.array_equal(ref.canonical(clustering.complete_linkage_labels(D, t)), scipy_labels(Zc, t))


def bcubed_by_pairs(y_true, y_pred):
    n = len(y_true)
    prec, rec = [], []
    for i in range(n):
        same_t = [j for j in range(n) if y_true[j] == y_true[i]]
        same_p = [j for j in range(n) if y_pred[j] == y_pred[i]]
        prec.append(np.mean([float(y_pred[j] == y_pred[i]) for j in same_t]))
        rec.append(np.mean([float(y_true[j] == y_true[i]) for j in same_p]))
    p, r = float(np.mean(prec)), float(np.mean(rec))
    return p, r, 2 * p * r / (p + r)


@pytest.mark.parametrize("seed", range(4))
def test_bcubed_equals_the_pairwise_definition(seed):
    rs = np.random.RandomState(seed)
    n = 60 + 20 * seed
    y_true = rs.randint(0, 7, n)
    y_pred = np.where(rs.rand(n) < 0.7, y_true * 3 + 1, rs.randint(0, 30, n)).astype(np.float64)
    got = clustering.bcubed(y_true, y_pred)
    assert np.allclose(got, bcubed_by_pairs(y_true, y_pred), rtol=0, atol=1e-12)
    assert clustering.bcubed(y_true, y_true) == (1.0, 1.0, 1.0)


def test_single_linkage_rejects_bad_arguments_without_a_gpu():
    from hse_facerec_tf_amd import _lib
    L = _lib.lib()
    buf = ctypes.create_string_buffer(256)
    p = ctypes.cast(buf, ctypes.c_void_p).value
    ok = dict(x=p, n=4, d=8, born=None, year=None, dense=None, ea=p, eb=p, eh=p)

    def call(**kw):
        a = dict(ok, **kw)
        return L.hsefr_single_linkage(a["x"], a["n"], a["d"], a["born"], a["year"], a["dense"], a["ea"], a["eb"], a["eh"], None)
    cases = [dict(n=0, dense=None), dict(x=None), dict(dense=p), dict(d=12), dict(d=0), dict(born=p), dict(year=p),
             dict(ea=None), dict(eb=None), dict(eh=None), dict(x=None, dense=p, born=p, year=p)]
    for kw in cases:
        assert call(**kw) == _lib.ERR_INVALID, kw
        assert "single_linkage" in _lib.last_error()
