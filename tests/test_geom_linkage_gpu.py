"""GPU suite: centroid, median and Ward linkage on the device (libhsefr_geom.so through hse_facerec_tf_amd.clustering) against scipy and
the NumPy restatements of tests/geom_linkage_ref.py -- the dense path (centroid and median bit for bit, Ward's tree with its heights to
rounding) on both sides of the one-workgroup class, the records with and without ties, a chain, the features path on the device's own
matrix, the clamp, the drop-ins, and the two guards on the source."""
import functools

import numpy as np
import pytest
from scipy.cluster import hierarchy as hac
from scipy.spatial.distance import squareform

import geom_linkage_ref as gref
import linkage_ref as ref
from test_hier_linkage_gpu import reference_get_facial_clusters
from test_partition_scores_gpu import assert_sweep_row
from test_linkage_gpu import ages, as_partition, features, fp64_distances, random_matrix, scipy_labels

pytestmark = pytest.mark.gpu

SEQUENTIAL = ["centroid", "median"]


def merges(method, **source):
    """ops.geom_linkage_merges on host arrays -> (a, b, h, round, counts) as NumPy"""
    import torch
    from hse_facerec_tf_amd import ops
    if "dense" in source:
        source["dense"] = torch.from_numpy(np.ascontiguousarray(source["dense"], dtype=np.float64)).cuda()
    out = ops.geom_linkage_merges(method=method, return_counts=True, **source)
    return tuple(v.cpu().numpy() for v in out[:4]) + (out[4],)


def sorted_records(a, b, h, r):
    order = np.lexsort((a, r))
    return a[order], b[order], h[order], r[order]


@functools.lru_cache(maxsize=None)
def dense_case(n, d):
    D = gref.euclidean(n, d, gref.case_seed(n, d))
    D.setflags(write=False)
    return D


def six_cuts(Zs, min_gap):
    return ref.gap_thresholds(Zs[:, 2], np.quantile(Zs[:, 2], [0.1, 0.3, 0.5, 0.7, 0.9, 0.97]), min_gap)


def assert_cuts(Z, Zs, ts):
    from hse_facerec_tf_amd import clustering
    for t, lab in zip(ts, clustering.fcluster_distance(Z, ts)):
        assert np.array_equal(ref.canonical(lab), scipy_labels(Zs, t)), t


# ---- the dense path against scipy ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("method", SEQUENTIAL)
@pytest.mark.parametrize("d", gref.DENSE_DS)
@pytest.mark.parametrize("n", gref.DENSE_NS)
def test_centroid_and_median_dense_are_scipy_bit_for_bit(n, d, method):
    from hse_facerec_tf_amd import clustering
    D = dense_case(n, d)
    Z = clustering.linkage_geometric_dense(D, method)
    Zs = hac.linkage(squareform(D, checks=False), method)
    assert np.array_equal(Z, Zs)
    if n > 2:
        assert_cuts(Z, Zs, six_cuts(Zs, 1e-9))
    a, b, h, r, counts = merges(method, dense=D)
    assert counts.tolist() == [n - 1, 0]              # every step found its pair; no radicand of a real matrix is negative
    assert np.array_equal(r, np.arange(n - 1)) and (a < b).all()


@pytest.mark.parametrize("d", gref.DENSE_DS)
@pytest.mark.parametrize("n", gref.DENSE_NS + gref.WARD_EXTRA_NS)
def test_ward_dense_is_scipys_tree(n, d):
    from hse_facerec_tf_amd import clustering
    D = dense_case(n, d)
    Z = clustering.linkage_geometric_dense(D, "ward")
    Zs = hac.linkage(squareform(D, checks=False), "ward")
    assert hac.is_valid_linkage(Z)
    assert np.array_equal(Z[:, [0, 1, 3]], Zs[:, [0, 1, 3]])
    assert np.allclose(Z[:, 2], Zs[:, 2], rtol=1e-12, atol=0)
    if n > 2:
        assert_cuts(Z, Zs, six_cuts(Zs, 1e-9))
    assert merges("ward", dense=D)[4].tolist() == [n - 1, 0]


# ---- the records are the restatement's -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ties", [False, True])
@pytest.mark.parametrize("method", gref.METHODS)
@pytest.mark.parametrize("n", [65, 128, 129, 600])
def test_device_records_are_the_restated_records(n, method, ties):
    """Every record of the device -- the two slots, the height's bits, the step or round -- is the host restatement's, with and without
    ties; with ties the tree is valid and the same from run to run."""
    from hse_facerec_tf_amd import clustering
    D = random_matrix(n, 1100 + n, ties)
    a, b, h, r, counts = merges(method, dense=D)
    if method == "ward":
        want = gref.ward_rounds(D, return_clamps=True)
        for g, w in zip(sorted_records(a, b, h, r), sorted_records(*want[:4])):
            assert np.array_equal(g, w)
        Z = clustering.linkage_from_merges(a, b, h, r, n)
    else:
        want = gref.closest_pair_sequence(D, method, return_clamps=True)
        for g, w in zip((a, b, h), want[:3]):
            assert np.array_equal(g, w)
        assert np.array_equal(r, np.arange(n - 1))
        Z = clustering.linkage_from_sequence(a, b, h, n)
    assert counts.tolist() == [n - 1, want[-1]]
    if ties:
        assert hac.is_valid_linkage(Z)
        assert np.array_equal(clustering.linkage_geometric_dense(D, method), Z)
        for g, w in zip(sorted_records(*merges(method, dense=D)[:4]), sorted_records(a, b, h, r)):
            assert np.array_equal(g, w)


def test_a_chain():
    """Points on a line with doubling gaps: one reciprocal pair per round, so Ward's host loop reads the count over several batches;
    scipy's Z for all three."""
    from hse_facerec_tf_amd import clustering
    n = 130
    p = np.concatenate([[0.0], np.cumsum(2.0 ** np.arange(n - 1) / 2.0 ** 60)])
    D = np.abs(p[:, None] - p[None, :])
    assert sorted(merges("ward", dense=D)[3].tolist()) == list(range(n - 1))
    y = squareform(D, checks=False)
    for method in SEQUENTIAL:
        assert np.array_equal(clustering.linkage_geometric_dense(D, method), hac.linkage(y, method)), method
    Z, Zs = clustering.linkage_geometric_dense(D, "ward"), hac.linkage(y, "ward")
    assert np.array_equal(Z[:, [0, 1, 3]], Zs[:, [0, 1, 3]])
    assert np.allclose(Z[:, 2], Zs[:, 2], rtol=1e-12, atol=0)


# ---- the features path --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [100, 301])
@pytest.mark.parametrize("d,age", [(12, False), (12, True), (128, False), (128, True), (1024, False), (1024, True)])
def test_features_path_is_the_dense_path_on_the_devices_own_matrix(d, age, n):
    """There is one distance in the project: the working matrix of every method is the one the same-photo split builds for one group of
    all points, and the tree from the features is the tree from that matrix, bit for bit."""
    import torch
    from hse_facerec_tf_amd import clustering, ops
    X = features(n, d, 40 + d, classes=15)
    born, photo = ages(n, d) if age else (None, None)
    x, b, y = clustering._features(X, born, photo, None, True)
    members = torch.arange(n, dtype=torch.int32, device="cuda")
    P = ops.split_groups(members, [0, n], members, x=x, born=b, year=y, return_distances=True)[1].cpu().numpy().reshape(n, n)
    off = ~np.eye(n, dtype=bool)
    Zs = hac.linkage(squareform(fp64_distances(X, born, photo), checks=False), "ward")
    for method in gref.METHODS:
        out = ops.geom_linkage_merges(x=x, born=b, year=y, method=method, return_matrix=True, return_counts=True)
        W = out[4].cpu().numpy()
        assert np.array_equal(W, W.T) and np.isinf(np.diag(W)).all() and np.array_equal(W[off], P[off]), method
        assert out[5].tolist() == [n - 1, 0]
        Z = clustering.linkage_geometric(X, method, born, photo)
        np.fill_diagonal(W, 0.0)
        assert np.array_equal(Z, clustering.linkage_geometric_dense(W, method)), method
    assert hac.is_valid_linkage(Z)                                           # Ward's, the last of the loop
    assert_cuts(Z, Zs, six_cuts(Zs, 1e-3))
    assert clustering.linkage_geometric(X[:1], "ward").shape == (0, 4)
    assert clustering.linkage_geometric(X[:1], "centroid").shape == (0, 4)


# ---- the clamp ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("method", gref.METHODS)
@pytest.mark.parametrize("case", ["search", 130])
def test_a_negative_radicand_is_clamped_and_counted(case, method):
    """On the small matrix the seeded search finds (scipy's sqrt gives NaN there, tests/test_geom_linkage_cpu.py) and on a larger one of
    the same kind for the other size class, the device's records are finite, they are the restatement's, and the clamps are counted."""
    from hse_facerec_tf_amd import clustering
    D = gref.clamp_case() if case == "search" else gref.signed_symmetric(case, 3)
    n = D.shape[0]
    a, b, h, r, counts = merges(method, dense=D)
    assert np.isfinite(h).all()
    if method == "ward":
        want = gref.ward_rounds(D, return_clamps=True)
        for g, w in zip(sorted_records(a, b, h, r), sorted_records(*want[:4])):
            assert np.array_equal(g, w)
    else:
        want = gref.closest_pair_sequence(D, method, return_clamps=True)
        for g, w in zip((a, b, h), want[:3]):
            assert np.array_equal(g, w)
        Z = clustering.linkage_geometric_dense(D, method)
        assert np.isfinite(Z).all() and np.array_equal(Z, clustering.linkage_from_sequence(*want[:3], n))
    assert counts[0] == n - 1 and counts[1] == want[-1]
    if method == "centroid":
        assert counts[1] > 0


# ---- the drop-ins ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("method", gref.METHODS)
@pytest.mark.parametrize("with_photos", [False, True])
def test_get_facial_clusters_geometric_is_the_reference_branch(method, with_photos):
    from hse_facerec_tf_amd import clustering
    rs = np.random.RandomState(4)
    n = 400
    X = features(n, 64, 8, classes=25)
    D = fp64_distances(X)
    photos = rs.randint(0, 150, n) if with_photos else None
    Zs = hac.linkage(squareform(D, checks=False), method)
    for t in ref.gap_thresholds(Zs[:, 2], np.quantile(Zs[:, 2], [0.5, 0.8, 0.95, 0.99]), 1e-9):
        want = reference_get_facial_clusters(D, t, photos, method)
        for split in ("host", "device"):
            got = clustering.get_facial_clusters_geometric(D, t, method, photos, split=split)
            assert as_partition(got) == as_partition(want)
            assert [len(c) for c in got] == [len(c) for c in want]
            assert got == sorted(got, key=lambda c: (-len(c), c[0])) and all(c == sorted(c) for c in got)
            if with_photos:
                for c in got:
                    assert len(set(photos[c])) == len(c)
    assert clustering.get_facial_clusters_geometric(D[:1, :1], 0.96, method) == [[0]]


def test_cluster_faces_ward_equals_the_dense_route():
    from hse_facerec_tf_amd import clustering, identification
    rs = np.random.RandomState(12)
    n = 500
    X = features(n, 128, 10, classes=40)
    born, photo_year = ages(n, 13)
    photo_year = photo_year.astype(np.float64)
    photos = rs.randint(0, 200, n)
    D = identification.feature_distance_matrix(X, born, photo_year)
    Zs = hac.linkage(squareform(D, checks=False), "ward")
    for t in ref.gap_thresholds(Zs[:, 2], np.quantile(Zs[:, 2], [0.8, 0.95]), 1e-3):
        want = clustering.get_facial_clusters_geometric(D, t, "ward", photos)
        got = clustering.cluster_faces_geometric(X, t, "ward", born, photo_year, photos)
        assert as_partition(got) == as_partition(want)
    assert clustering.cluster_faces_geometric(X[:1], 1.0, "ward") == [[0]]


def test_threshold_sweep_takes_ward():
    from hse_facerec_tf_amd import clustering
    n = 300
    X = features(n, 64, 21, classes=12)
    y = np.random.RandomState(5).randint(0, 12, n)
    D = fp64_distances(X)
    Zs = hac.linkage(squareform(D, checks=False), "ward")
    ts = six_cuts(Zs, 1e-9)
    def check(method, Zm, tm):
        rows = clustering.threshold_sweep(D, y, method, tm, dense=True)
        assert rows.shape == (len(tm), 10)
        for t, row in zip(tm, rows):
            labels = hac.fcluster(Zm, t, "distance")
            # classes, clusters and ARI are exact; the sums lie within the scoring suite's derived bounds of the exact values
            assert np.array_equal(row[:3], clustering.clustering_scores(y, labels)[:3]), (method, t)
            assert_sweep_row((method, t), row, [np.flatnonzero(labels == v).tolist() for v in np.unique(labels)], y)
    check("ward", Zs, ts)
    for method in SEQUENTIAL:                                               # the other two names are taken as well
        Zm = hac.linkage(squareform(D, checks=False), method)
        check(method, Zm, six_cuts(Zm, 1e-9)[2:4])


# ---- the source -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("method", gref.METHODS)
@pytest.mark.parametrize("n", [100, 301])
def test_dense_path_reads_the_upper_triangle_and_leaves_it_alone(n, method):
    import torch
    from hse_facerec_tf_amd import clustering
    D = np.random.RandomState(6).rand(n, n) + 0.5                          # asymmetric, nonzero diagonal
    Dt = torch.from_numpy(D).cuda()
    keep = Dt.clone()
    Z = clustering.linkage_geometric_dense(Dt, method)
    assert torch.equal(Dt, keep)
    U = np.triu(D, 1)
    assert np.array_equal(clustering.linkage_geometric_dense(U + U.T, method), Z)
    if method == "ward":
        want = clustering.linkage_from_merges(*gref.ward_rounds(D), n)
    else:
        want = clustering.linkage_from_sequence(*gref.closest_pair_sequence(D, method), n)
    assert np.array_equal(Z, want)


@pytest.mark.parametrize("method", gref.METHODS)
def test_a_matrix_beyond_device_memory_is_refused_before_any_launch(method):
    import torch
    from hse_facerec_tf_amd import clustering, ops
    n = 200000                                                              # 8 n^2 = 320 GB of working matrix
    free, total = torch.cuda.mem_get_info()
    assert 8 * n * n > total
    x = torch.zeros((n, 8), dtype=torch.float32, device="cuda")
    with pytest.raises(MemoryError, match="working matrix"):
        ops.geom_linkage_merges(x=x, method=method)
    del x
    D = dense_case(64, 2)                                                   # the stream and the library still work
    assert np.array_equal(clustering.linkage_geometric_dense(D, "median"), hac.linkage(squareform(D, checks=False), "median"))
