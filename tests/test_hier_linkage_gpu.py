"""GPU suite: average, complete and weighted linkage on the device (csrc/hier_linkage.hip through hse_facerec_tf_amd.clustering)
against scipy and the NumPy restatement of tests/hier_linkage_ref.py -- the dense path (complete bit for bit, the two means to rounding),
tied integer matrices, a chain that needs n - 1 rounds, the features path with and without the age term, the get_facial_clusters
drop-in for the study's 'average' row, and an LFW-sized tree."""
import numpy as np
import pytest
from scipy.cluster import hierarchy as hac
from scipy.spatial.distance import squareform

import hier_linkage_ref as href
import linkage_ref as ref
from test_linkage_gpu import ages, as_partition, features, fp64_distances, random_matrix, scipy_labels

pytestmark = pytest.mark.gpu

METHODS = ["average", "complete", "weighted"]


def merges(D, method):
    import torch
    from hse_facerec_tf_amd import ops
    out = ops.hier_linkage_merges(dense=torch.from_numpy(np.ascontiguousarray(D, dtype=np.float64)).cuda(), method=method)
    return tuple(v.cpu().numpy() for v in out)


def sorted_records(a, b, h, r):
    order = np.lexsort((a, r))
    return a[order], b[order], h[order], r[order]


def away_from(heights, ts, gap):
    return [float(t) for t in ts if np.abs(np.asarray(heights) - t).min() > gap]


@pytest.mark.parametrize("n", [2, 3, 5, 64, 65, 257, 600])
def test_complete_dense_is_scipy_bit_for_bit(n):
    from hse_facerec_tf_amd import clustering
    D = random_matrix(n, 300 + n)
    Z = clustering.linkage_dense(D, "complete")
    Zs = hac.linkage(squareform(D, checks=False), "complete")
    assert np.array_equal(Z, Zs)


@pytest.mark.parametrize("method", ["average", "weighted"])
@pytest.mark.parametrize("n", [2, 3, 5, 64, 65, 257, 600])
def test_means_dense_match_scipy(method, n):
    from hse_facerec_tf_amd import clustering
    D = random_matrix(n, 500 + n)
    Z = clustering.linkage_dense(D, method)
    Zs = hac.linkage(squareform(D, checks=False), method)
    assert hac.is_valid_linkage(Z)
    assert np.array_equal(Z[:, [0, 1, 3]], Zs[:, [0, 1, 3]])
    assert np.allclose(Z[:, 2], Zs[:, 2], rtol=1e-12, atol=0)
    if n > 2:
        ts = ref.gap_thresholds(Zs[:, 2], np.linspace(Zs[0, 2], Zs[-1, 2], 12), 1e-9)
        got = clustering.fcluster_distance(Z, ts)
        for t, lab in zip(ts, got):
            assert np.array_equal(ref.canonical(lab), scipy_labels(Zs, t)), t


@pytest.mark.parametrize("method", METHODS)
@pytest.mark.parametrize("n", [65, 600])
def test_device_rounds_are_the_restated_rounds(method, n):
    """Every record of the device -- survivor, partner, height bits, round -- is the host restatement's (the same reciprocal pairs, the
    same Lance-Williams roundings), with and without ties."""
    for ties in (False, True):
        D = random_matrix(n, 700 + n, ties)
        got = sorted_records(*merges(D, method))
        want = sorted_records(*href.rnn_rounds(D, method))
        for g, w in zip(got, want):
            assert np.array_equal(g, w)


@pytest.mark.parametrize("method", METHODS)
@pytest.mark.parametrize("n", [2, 33, 300, 1000])
def test_ties_give_a_valid_deterministic_hierarchy(method, n):
    from hse_facerec_tf_amd import clustering
    D = random_matrix(n, 900 + n, ties=True)
    a, b, h, r = merges(D, method)
    href.check_records(D, method, a, b, h, r)
    Z = clustering.linkage_dense(D, method)
    assert hac.is_valid_linkage(Z)
    assert np.array_equal(clustering.linkage_dense(D, method), Z)


def test_dense_path_reads_the_upper_triangle_and_leaves_it_alone():
    import torch
    from hse_facerec_tf_amd import clustering
    rs = np.random.RandomState(6)
    D = rs.rand(301, 301)                                              # asymmetric, nonzero diagonal
    Dt = torch.from_numpy(D).cuda()
    keep = Dt.clone()
    Z = clustering.linkage_dense(Dt, "average")
    assert torch.equal(Dt, keep)
    Zs = hac.linkage(squareform(D, checks=False), "average")
    assert np.array_equal(Z[:, [0, 1, 3]], Zs[:, [0, 1, 3]])
    U = np.triu(D, 1)
    assert np.array_equal(clustering.linkage_dense(U + U.T, "average"), Z)


@pytest.mark.parametrize("method", METHODS)
def test_a_chain_takes_n_minus_one_rounds(method):
    """Points on a line with doubling gaps: one reciprocal pair per round, so the host reads the count over several batches."""
    from hse_facerec_tf_amd import clustering
    n = 130
    p = np.concatenate([[0.0], np.cumsum(2.0 ** np.arange(n - 1) / 2.0 ** 60)])
    D = np.abs(p[:, None] - p[None, :])
    a, b, h, r = merges(D, method)
    assert sorted(r.tolist()) == list(range(n - 1))
    Z = clustering.linkage_dense(D, method)
    Zs = hac.linkage(squareform(D, checks=False), method)
    assert np.array_equal(Z[:, [0, 1, 3]], Zs[:, [0, 1, 3]])
    assert np.allclose(Z[:, 2], Zs[:, 2], rtol=1e-12, atol=0)


@pytest.mark.parametrize("method", METHODS)
@pytest.mark.parametrize("d,age", [(12, False), (128, False), (128, True), (1024, False), (1024, True)])
def test_features_path_matches_scipy_on_fp64_distances(method, d, age):
    from hse_facerec_tf_amd import clustering
    n = 301
    X = features(n, d, 40 + d, classes=15)
    born, photo = ages(n, d) if age else (None, None)
    Z = clustering.linkage(X, method, born, photo)
    assert hac.is_valid_linkage(Z)
    Zs = hac.linkage(squareform(fp64_distances(X, born, photo), checks=False), method)
    assert np.abs(Z[:, 2] - Zs[:, 2]).max() < 1e-4
    ts = ref.gap_thresholds(Zs[:, 2], np.quantile(Zs[:, 2], [0.1, 0.3, 0.5, 0.7, 0.9, 0.97]), 1e-3)
    got = clustering.fcluster_distance(Z, ts)
    for t, lab in zip(ts, got):
        assert np.array_equal(ref.canonical(lab), scipy_labels(Zs, t)), t
    assert clustering.linkage(X[:1], method).shape == (0, 4)


@pytest.mark.parametrize("d,age", [(128, False), (128, True), (12, False), (12, True), (1024, True)])
def test_working_matrix_and_row_scan_hold_the_same_distances(d, age):
    """The one observable link between the two families of feature distances: the lowest merge of average, complete and weighted linkage
    (the least entry of the fp64 working matrix) and the lowest merge of single linkage (the least w(i,j) a row scan sees) are both the
    global minimum of w(i,j), so they are the same fp32 value widened -- bit for bit, whichever kernel computed it."""
    from hse_facerec_tf_amd import clustering
    n = 301
    X = features(n, d, 70 + d, classes=15)
    born, photo = ages(n, 7 + d) if age else (None, None)
    lowest = clustering.linkage_single(X, born, photo)[:, 2].min()
    assert lowest > 0 and lowest == np.float64(np.float32(lowest))
    for method in METHODS:
        assert clustering.linkage(X, method, born, photo)[:, 2].min() == lowest, method


def reference_get_facial_clusters(dist_matrix, distanceThreshold, all_indices=None, method="average"):
    """The scipy branch of facial_clustering.get_facial_clusters (:243-261, 284) with clusteringMethod = method, restated with scipy."""
    labels = hac.fcluster(hac.linkage(squareform(dist_matrix, checks=False), method=method), distanceThreshold, "distance")
    clusters = []
    for lbl in sorted(set(labels)):
        cluster = [i for i, v in enumerate(labels) if v == lbl]
        if all_indices is None or len(cluster) == 1:
            clusters.append(cluster)
            continue
        sub = dist_matrix[cluster][:, cluster].copy()
        sub += np.array([[100 * (all_indices[i] == all_indices[j] and i != j) for j in cluster] for i in cluster])
        lab = hac.fcluster(hac.linkage(squareform(sub), method="complete"), 50, "distance")
        clusters.extend([[cluster[k] for k, v in enumerate(lab) if v == m] for m in sorted(set(lab))])
    clusters.sort(key=len, reverse=True)
    return clusters


@pytest.mark.parametrize("method", METHODS)
@pytest.mark.parametrize("with_photos", [False, True])
def test_get_facial_clusters_is_the_reference_branch(method, with_photos):
    from hse_facerec_tf_amd import clustering
    rs = np.random.RandomState(4)
    n = 400
    X = features(n, 64, 8, classes=25)
    D = fp64_distances(X)
    photos = rs.randint(0, 150, n) if with_photos else None
    Zs = hac.linkage(squareform(D, checks=False), method)
    for t in ref.gap_thresholds(Zs[:, 2], [0.78, 0.96, 1.1, 1.3], 1e-9):
        got = clustering.get_facial_clusters(D, t, photos, method=method)
        want = reference_get_facial_clusters(D, t, photos, method)
        assert as_partition(got) == as_partition(want)
        assert [len(c) for c in got] == [len(c) for c in want]
        assert got == sorted(got, key=lambda c: (-len(c), c[0])) and all(c == sorted(c) for c in got)
        if with_photos:
            for c in got:
                assert len(set(photos[c])) == len(c)
    assert clustering.get_facial_clusters(D[:1, :1], 0.96, method=method) == [[0]]


def test_default_method_is_single():
    from hse_facerec_tf_amd import clustering
    X = features(200, 32, 3, classes=10)
    D = fp64_distances(X)
    assert clustering.get_facial_clusters(D, 0.8) == clustering.get_facial_clusters(D, 0.8, method="single")
    assert np.array_equal(clustering.linkage_dense(D, "single"), clustering.linkage_single_dense(D))
    assert np.array_equal(clustering.linkage(X, "single"), clustering.linkage_single(X))


def test_cluster_faces_average_equals_the_dense_route():
    from hse_facerec_tf_amd import clustering, identification
    rs = np.random.RandomState(12)
    n = 500
    X = features(n, 128, 10, classes=40)
    born, photo_year = ages(n, 13)
    photo_year = photo_year.astype(np.float64)
    photos = rs.randint(0, 200, n)
    D = identification.feature_distance_matrix(X, born, photo_year)
    Zs = hac.linkage(squareform(D, checks=False), "average")
    for t in ref.gap_thresholds(Zs[:, 2], [0.96, 1.1], 1e-3):
        want = clustering.get_facial_clusters(D, t, photos, method="average")
        got = clustering.cluster_faces(X, t, born, photo_year, photos, method="average")
        assert as_partition(got) == as_partition(want)


def test_argument_errors():
    from hse_facerec_tf_amd import clustering
    D = random_matrix(10, 2)
    with pytest.raises(ValueError, match="average, complete, weighted"):
        clustering.linkage_dense(D, "ward")
    with pytest.raises(ValueError):
        clustering.linkage_dense(np.ones((3, 4)), "average")
    bad = D.copy()
    bad[2, 3] = np.inf
    for m in METHODS:
        with pytest.raises(ValueError):
            clustering.linkage_dense(bad, m)
        with pytest.raises(ValueError):
            clustering.get_facial_clusters(bad, 1.0, method=m)
    X = features(10, 16, 1)
    X[3, 2] = np.nan
    with pytest.raises(ValueError):
        clustering.linkage(X, "average")


def test_lfw_sized_average_tree_matches_scipy_on_the_study_sweep():
    import torch
    from hse_facerec_tf_amd import clustering, gallery
    from oracle.identification import embeddings_for_labels
    y = gallery.lfw_like_labels()
    X = embeddings_for_labels(y, dim=1024)
    X = (X / np.linalg.norm(X, axis=1, keepdims=True)).astype(np.float32)
    assert X.shape == (9164, 1024)
    Xd = torch.from_numpy(X).cuda().double()
    sq = (Xd * Xd).sum(1)
    Dt = torch.sqrt(torch.clamp(sq[:, None] + sq[None, :] - 2 * Xd @ Xd.T, min=0))
    Dt = torch.triu(Dt, 1)
    Dt = (Dt + Dt.T).contiguous()
    Z = clustering.linkage_dense(Dt, "average")
    D = Dt.cpu().numpy()
    del Dt
    Zs = hac.linkage(squareform(D, checks=False), "average")
    assert np.array_equal(Z[:, [0, 1, 3]], Zs[:, [0, 1, 3]])
    assert np.allclose(Z[:, 2], Zs[:, 2], rtol=1e-12, atol=0)
    ts = away_from(Zs[:, 2], np.linspace(0.6, 1.3, 71), 1e-9)
    assert len(ts) > 60
    got = clustering.fcluster_distance(Z, ts)
    for t, lab in zip(ts, got):
        assert np.array_equal(ref.canonical(lab), scipy_labels(Zs, t)), t
    # the features path on the same points: an fp32 matrix, so the cuts agree away from the heights
    Zf = clustering.linkage(X, "average")
    assert hac.is_valid_linkage(Zf)
    for t in ref.gap_thresholds(Zs[:, 2], [0.78, 0.96], 1e-4):
        assert np.array_equal(ref.canonical(clustering.fcluster_distance(Zf, t)), scipy_labels(Zs, t)), t


def test_a_matrix_beyond_device_memory_is_refused_before_any_launch():
    import torch
    from hse_facerec_tf_amd import clustering, ops
    n = 200000                                                         # 8 n^2 = 320 GB of working matrix
    free, total = torch.cuda.mem_get_info()
    assert 8 * n * n > total
    x = torch.zeros((n, 8), dtype=torch.float32, device="cuda")
    with pytest.raises(MemoryError, match="hier_linkage"):
        ops.hier_linkage_merges(x=x, method="average")
    del x
    D = random_matrix(50, 3)                                           # the stream and the library still work
    assert np.array_equal(clustering.linkage_dense(D, "complete"), hac.linkage(squareform(D, checks=False), "complete"))
