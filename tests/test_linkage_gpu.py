"""GPU suite: single-linkage clustering on the device (csrc/linkage.hip through hse_facerec_tf_amd.clustering) against scipy and the
fp64 restatement of tests/linkage_ref.py -- the dense fp64 path bit for bit, the features path to fp32 round-off, the drop-ins for the
reference's get_facial_clusters / perform_clustering, and a 20 000-face tree."""
import numpy as np
import pytest
from scipy.cluster import hierarchy as hac
from scipy.spatial.distance import squareform

import linkage_ref as ref

pytestmark = pytest.mark.gpu


def random_matrix(n, seed, ties=False):
    rs = np.random.RandomState(seed)
    D = rs.randint(0, 8, (n, n)).astype(np.float64) if ties else rs.rand(n, n)
    D = np.triu(D, 1)
    return D + D.T


def scipy_labels(Z, t):
    return ref.canonical(hac.fcluster(Z, t, "distance"))


def features(n, d, seed, classes=None):
    """Unit-norm rows around a few centroids (the clustering study normalises its features)."""
    rs = np.random.RandomState(seed)
    classes = classes or max(2, n // 20)
    cent = rs.randn(classes, d)
    X = cent[rs.randint(0, classes, n)] + 0.6 * rs.randn(n, d)
    return (X / np.linalg.norm(X, axis=1, keepdims=True)).astype(np.float32)


def ages(n, seed):
    rs = np.random.RandomState(seed)
    born = rs.randint(1940, 2015, n).astype(np.float64)
    photo = born + rs.randint(1, 30, n)
    return born, photo


def fp64_distances(X, born=None, photo=None):
    """The feature distance of process_photos.py:46-56 in fp64 on the host (the oracle of the features path)."""
    X = np.asarray(X, dtype=np.float64)
    sq = (X * X).sum(1)
    D = np.sqrt(np.maximum(sq[:, None] + sq[None, :] - 2 * X @ X.T, 0))
    if born is not None:
        my = np.maximum(photo[:, None], photo[None, :])
        D = D + 0.1 * (born[None, :] - born[:, None]) ** 2 / (2 * my - born[:, None] - born[None, :])
    D = np.triu(np.maximum(D, 0), 1)
    return D + D.T                       # exactly symmetric (X @ X.T need not be), zero diagonal


def check_spanning_tree(Z, n):
    from hse_facerec_tf_amd import clustering
    assert Z.shape == (n - 1, 4)
    assert hac.is_valid_linkage(Z)
    assert Z[-1, 3] == n
    assert len(np.unique(clustering.fcluster_distance(Z, np.inf))) == 1


@pytest.mark.parametrize("n", [1, 2, 3, 65, 1000, 4097])
@pytest.mark.parametrize("ties", [False, True])
def test_dense_path_is_scipy_bit_for_bit(n, ties):
    from hse_facerec_tf_amd import clustering
    D = random_matrix(n, 100 + n, ties)
    Z = clustering.linkage_single_dense(D)
    if n == 1:
        assert Z.shape == (0, 4)
        assert clustering.get_facial_clusters(D) == [[0]]
        return
    Zs = hac.linkage(squareform(D, checks=False), "single")
    check_spanning_tree(Z, n)
    assert np.array_equal(Z[:, 2], Zs[:, 2])                          # bitwise: the MST of the same fp64 values
    ts = ref.cut_thresholds(Zs[:, 2])
    got = clustering.fcluster_distance(Z, ts)
    for t, lab in zip(ts, got):
        assert np.array_equal(ref.canonical(lab), scipy_labels(Zs, t)), t


def test_dense_path_reads_the_upper_triangle():
    from hse_facerec_tf_amd import clustering
    rs = np.random.RandomState(5)
    D = rs.rand(301, 301)                                              # asymmetric, nonzero diagonal
    Z = clustering.linkage_single_dense(D)
    Zs = hac.linkage(squareform(D, checks=False), "single")
    assert np.array_equal(Z[:, 2], Zs[:, 2])
    U = np.triu(D, 1)
    assert np.array_equal(clustering.linkage_single_dense(U + U.T), Z)


def test_dense_path_rejects_non_finite():
    from hse_facerec_tf_amd import clustering
    D = random_matrix(10, 1)
    D[2, 3] = np.nan
    with pytest.raises(ValueError):
        clustering.get_facial_clusters(D)
    with pytest.raises(ValueError):
        clustering.linkage_single_dense(np.ones((3, 4)))


@pytest.mark.parametrize("d", [8, 12, 128, 1024, 2048])
@pytest.mark.parametrize("age", [False, True])
def test_features_path_matches_the_fp64_restatement(d, age):
    from hse_facerec_tf_amd import clustering
    n = 203 if d >= 1024 else 1001
    X = features(n, d, d)
    born, photo = ages(n, d) if age else (None, None)
    Z = clustering.linkage_single(X, born, photo)
    check_spanning_tree(Z, n)
    a, b, h = ref.prim_mst(fp64_distances(X, born, photo))
    assert np.abs(Z[:, 2] - np.sort(h)).max() < 1e-5
    hs = np.sort(h)
    wide = np.flatnonzero(np.diff(hs) > 1e-4)
    ts = np.concatenate([[hs[0] - 1], (hs[wide] + hs[wide + 1]) / 2, [hs[-1] + 1]])
    got = clustering.fcluster_distance(Z, ts)
    for t, lab in zip(ts, got):
        assert np.array_equal(ref.canonical(lab), ref.flat_cut(n, a, b, h, t)), t


def test_lfw_sized_clustering_matches_scipy():
    import torch
    from hse_facerec_tf_amd import clustering, gallery
    from oracle.identification import embeddings_for_labels
    y = gallery.lfw_like_labels()
    X = embeddings_for_labels(y, dim=1024)
    X = (X / np.linalg.norm(X, axis=1, keepdims=True)).astype(np.float32)
    n = len(y)
    assert X.shape == (9164, 1024)
    Z = clustering.linkage_single(X)
    check_spanning_tree(Z, n)
    Xd = torch.from_numpy(X).cuda().double()
    sq = (Xd * Xd).sum(1)
    D = torch.sqrt(torch.clamp(sq[:, None] + sq[None, :] - 2 * Xd @ Xd.T, min=0)).cpu().numpy()
    np.fill_diagonal(D, 0)
    Zs = hac.linkage(squareform(D, checks=False), "single")
    assert np.abs(Z[:, 2] - Zs[:, 2]).max() < 1e-5
    for t in ref.gap_thresholds(Zs[:, 2], [0.78, 0.82], 1e-4):
        assert np.array_equal(ref.canonical(clustering.fcluster_distance(Z, t)), scipy_labels(Zs, t)), t


def reference_get_facial_clusters(dist_matrix, distanceThreshold, all_indices=None):
    """The scipy branch of facial_clustering.get_facial_clusters (:243-261, 284), restated with scipy."""
    labels = hac.fcluster(hac.linkage(squareform(dist_matrix, checks=False), method="single"), distanceThreshold, "distance")
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


def as_partition(clusters):
    return sorted(tuple(sorted(c)) for c in clusters)


@pytest.mark.parametrize("with_photos", [False, True])
def test_get_facial_clusters_is_the_reference_branch(with_photos):
    from hse_facerec_tf_amd import clustering
    rs = np.random.RandomState(3)
    n = 400
    X = features(n, 64, 7, classes=25)
    D = fp64_distances(X)
    photos = rs.randint(0, 150, n) if with_photos else None
    Zs = hac.linkage(squareform(D, checks=False), "single")
    for t in ref.gap_thresholds(Zs[:, 2], [0.6, 0.78, 0.82, 1.0], 1e-9):
        got = clustering.get_facial_clusters(D, t, photos, no_images_in_cluster=3)
        want = reference_get_facial_clusters(D, t, photos)
        assert as_partition(got) == as_partition(want)
        assert [len(c) for c in got] == [len(c) for c in want]            # the reference's order: longest first
        assert got == sorted(got, key=lambda c: (-len(c), c[0])) and all(c == sorted(c) for c in got)
        if with_photos:
            for c in got:
                assert len(set(photos[c])) == len(c)


def test_cluster_faces_equals_the_dense_route():
    from hse_facerec_tf_amd import clustering, identification
    rs = np.random.RandomState(11)
    n = 500
    X = features(n, 128, 9, classes=40)
    born, photo_year = ages(n, 12)
    photos = rs.randint(0, 200, n)
    photo_year = photo_year.astype(np.float64)
    D = identification.feature_distance_matrix(X, born, photo_year)
    Zs = hac.linkage(squareform(D, checks=False), "single")
    for t in ref.gap_thresholds(Zs[:, 2], [0.78, 0.82, 1.0], 1e-4):
        want = clustering.get_facial_clusters(D, t, photos)
        got = clustering.cluster_faces(X, t, born, photo_year, photos)
        assert as_partition(got) == as_partition(want)
        assert got == want
        assert clustering.cluster_faces(X, t, born, photo_year, photos, min_cluster_size=2) == [c for c in want if len(c) >= 2]
    with pytest.raises(ValueError):
        clustering.cluster_faces(X, 1.0, born, born)                  # photo year - born year must be > 0


def test_twenty_thousand_faces():
    import torch
    from hse_facerec_tf_amd import clustering
    n, d = 20000, 256
    X = features(n, d, 21, classes=500)
    Z = clustering.linkage_single(X)
    check_spanning_tree(Z, n)
    assert np.array_equal(clustering.linkage_single(X), Z)              # bit-identical reruns
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        Z2 = clustering.linkage_single(torch.from_numpy(X).cuda())
    torch.cuda.synchronize()
    assert np.array_equal(Z2, Z)
    # every face's lightest tree edge is its nearest-neighbour distance (fp64, on the device in blocks)
    from hse_facerec_tf_amd import ops
    ea, eb, eh = ops.single_linkage_edges(x=torch.from_numpy(X).cuda())
    ea, eb, eh = ea.cpu().numpy(), eb.cpu().numpy(), eh.cpu().numpy()
    low = np.full(n, np.inf)
    np.minimum.at(low, ea, eh)
    np.minimum.at(low, eb, eh)
    Xd = torch.from_numpy(X).cuda().double()
    sq = (Xd * Xd).sum(1)
    nn = np.empty(n)
    for i0 in range(0, n, 2048):
        blk = sq[i0:i0 + 2048, None] + sq[None, :] - 2 * Xd[i0:i0 + 2048] @ Xd.T
        blk[torch.arange(blk.shape[0]), torch.arange(i0, i0 + blk.shape[0])] = np.inf
        nn[i0:i0 + 2048] = torch.sqrt(torch.clamp(blk.min(1).values, min=0)).cpu().numpy()
    assert np.abs(low - nn).max() < 1e-5
