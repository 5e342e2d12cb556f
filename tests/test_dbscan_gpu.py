"""GPU suite: DBSCAN on the device (csrc/dbscan.hip through hse_facerec_tf_amd.clustering) against scikit-learn's labels_ and
core_sample_indices_ on the dense fp64 path, against the restatement of tests/dbscan_ref.py on the features path (exact on integer
features, at gap thresholds of the fp64 distances otherwise), against single linkage's cut with min_samples = 1, the drop-ins for the
reference's DBSCAN branch, and 20 000 faces without a dense host matrix."""
import numpy as np
import pytest
from sklearn.cluster import DBSCAN

import dbscan_ref as dref
import linkage_ref as ref
from test_linkage_gpu import ages, features, fp64_distances

pytestmark = pytest.mark.gpu


def sklearn_dbscan(D, eps, min_samples):
    db = DBSCAN(eps=eps, min_samples=min_samples, metric="precomputed").fit(D)
    return db.core_sample_indices_.astype(np.int64), db.labels_.astype(np.int64)


def assert_same(got, want, what=""):
    assert np.array_equal(got[0], want[0]), ("core_sample_indices", what)
    assert np.array_equal(got[1], want[1]), ("labels", what)


def tie_matrix(n, seed):
    rs = np.random.RandomState(seed)
    D = rs.randint(0, max(8, n // 4), (n, n)).astype(np.float64)
    D = np.triu(D, 1)
    return D + D.T


def rand_matrix(n, seed):
    rs = np.random.RandomState(seed)
    D = np.triu(rs.rand(n, n), 1)
    return D + D.T


def gap_eps(D, want, min_gap=1e-5):
    return ref.gap_thresholds(D[np.triu_indices(D.shape[0], 1)], want, min_gap)


@pytest.mark.parametrize("n", [1, 2, 31, 257, 1000, 4099])
@pytest.mark.parametrize("ties", [False, True])
def test_dense_path_is_sklearn(n, ties):
    from hse_facerec_tf_amd import clustering
    D = tie_matrix(n, 10 + n) if ties else rand_matrix(n, 20 + n)
    vals = np.sort(D[np.triu_indices(n, 1)])
    if ties:
        eps_list = [1.0, 2.0, 3.0]
    elif n > 1:
        eps_list = [float(vals[min(len(vals) - 1, k * n // 2)]) for k in (1, 4)] + [0.5]      # matrix entries: ties at eps
    else:
        eps_list = [0.5]
    for eps in eps_list:
        for m in (1, 2, 3, 5, 10, 50, n + 1):
            got = clustering.dbscan_dense(D, eps, m)
            assert_same(got, sklearn_dbscan(D, eps, m), (n, eps, m))
    assert clustering.get_facial_clusters(D[:1, :1], 0.5, no_images_in_cluster=1, method="dbscan") == [[0]]
    assert clustering.get_facial_clusters(D[:1, :1], 0.5, no_images_in_cluster=2, method="dbscan") == []


def test_dense_path_reads_the_upper_triangle():
    from hse_facerec_tf_amd import clustering
    rs = np.random.RandomState(5)
    n = 301
    D = rs.rand(n, n)                                                  # asymmetric, nonzero diagonal
    U = np.triu(D, 1)
    for eps, m in ((0.01, 2), (0.02, 4), (0.004, 1)):
        got = clustering.dbscan_dense(D, eps, m)
        assert_same(got, sklearn_dbscan(U + U.T, eps, m), (eps, m))
        assert_same(got, dref.dbscan_dense(D, eps, m))
        assert_same(clustering.dbscan_dense(D + 5 * np.eye(n), eps, m), got)       # the diagonal is never read


@pytest.mark.parametrize("d", [8, 16, 1024])
def test_features_path_is_exact_on_integer_features(d):
    from hse_facerec_tf_amd import clustering
    n = 300 if d == 1024 else 700
    rs = np.random.RandomState(d)
    X = rs.randint(-2, 3, (n, d)).astype(np.float64)
    X[rs.randint(0, n, 20)] = X[rs.randint(0, n, 20)]                   # duplicate points
    sq = (X * X).sum(1)
    K = sq[:, None] + sq[None, :] - 2 * X @ X.T                         # exact integer squared distances
    D = np.sqrt(K)
    ks = np.sort(K[np.triu_indices(n, 1)])
    for q in (0.002, 0.01, 0.05):
        k = float(ks[int(q * len(ks))])
        eps = float(np.sqrt(k + 0.5))
        for m in (1, 3, 8):
            got = clustering.dbscan(X.astype(np.float32), eps, m)
            assert_same(got, sklearn_dbscan(D, eps, m), (k, m))


def test_features_path_with_the_age_term():
    from hse_facerec_tf_amd import clustering
    n = 600
    X = features(n, 128, 31, classes=30)
    born, photo = ages(n, 32)
    D = fp64_distances(X, born, photo)
    for eps in gap_eps(D, [0.78, 0.82, 0.96]):
        for m in (2, 5, 10):
            got = clustering.dbscan(X, eps, m, born, photo)
            assert_same(got, sklearn_dbscan(D, eps, m), (eps, m))
            assert got[1].max() >= 0                                               # at least one cluster
    X_odd = np.ascontiguousarray(X[:, :100])                                # d padded to a multiple of 8
    D_odd = fp64_distances(X_odd, born, photo)
    eps = gap_eps(D_odd, [0.8])[0]
    assert_same(clustering.dbscan(X_odd, eps, 4, born, photo), sklearn_dbscan(D_odd, eps, 4))


def test_min_samples_one_is_single_linkage_on_the_same_distances():
    from hse_facerec_tf_amd import clustering
    n = 500
    X = features(n, 64, 41, classes=25)
    born, photo = ages(n, 42)
    Z = clustering.linkage_single(X, born, photo)
    hs = np.unique(Z[:, 2])
    picks = hs[np.linspace(0, len(hs) - 1, 30).astype(int)]
    ts = np.concatenate([picks, (hs[:-1] + hs[1:])[np.linspace(0, len(hs) - 2, 20).astype(int)] / 2])
    for t in ts:
        core, labels = clustering.dbscan(X, float(t), 1, born, photo)
        assert np.array_equal(core, np.arange(n))
        assert np.array_equal(ref.canonical(labels), ref.canonical(clustering.fcluster_distance(Z, t))), t


def reference_dbscan_branch(dist_matrix, distanceThreshold, no_images_in_cluster):
    """The sklearn branch of facial_clustering.get_facial_clusters (:260-265, 284), restated with scikit-learn."""
    labels = DBSCAN(eps=distanceThreshold, min_samples=no_images_in_cluster, metric="precomputed").fit(dist_matrix).labels_
    clusters = [[i for i, v in enumerate(labels) if v == lbl] for lbl in sorted(set(labels)) if lbl != -1]
    clusters.sort(key=len, reverse=True)
    return clusters


@pytest.mark.parametrize("with_photos", [False, True])
def test_get_facial_clusters_is_the_reference_branch(with_photos):
    from hse_facerec_tf_amd import clustering
    n = 400
    X = features(n, 64, 7, classes=25)
    D = fp64_distances(X)
    photos = np.random.RandomState(3).randint(0, 150, n) if with_photos else None
    for t in gap_eps(D, [0.6, 0.78, 0.82, 1.0], 1e-9):
        for m in (1, 3, 6):
            got = clustering.get_facial_clusters(D, t, photos, no_images_in_cluster=m, method="dbscan")
            want = reference_dbscan_branch(D, t, m)
            assert sorted(map(tuple, got)) == sorted(tuple(sorted(c)) for c in want)
            assert [len(c) for c in got] == [len(c) for c in want]
            assert got == sorted(got, key=lambda c: (-len(c), c[0])) and all(c == sorted(c) for c in got)


def test_cluster_faces_dbscan_is_perform_clustering_branch():
    from hse_facerec_tf_amd import clustering
    n = 500
    X = features(n, 128, 9, classes=40)
    born, photo = ages(n, 12)
    photos = np.random.RandomState(11).randint(0, 200, n)
    D = fp64_distances(X, born, photo)
    for t in gap_eps(D, [0.78, 0.82, 1.0]):
        for m in (1, 3, 5):
            want = [c for c in dref.clusters_of(sklearn_dbscan(D, t, m)[1]) if len(c) >= m]
            got = clustering.cluster_faces(X, t, born, photo, photos, min_cluster_size=m, method="dbscan")
            assert got == want, (t, m)
            assert got == clustering.cluster_faces(X, t, born, photo, None, min_cluster_size=m, method="dbscan")


def test_lfw_sized_dbscan():
    import torch
    from hse_facerec_tf_amd import clustering, gallery
    from oracle.identification import embeddings_for_labels
    y = gallery.lfw_like_labels()
    X = embeddings_for_labels(y, dim=1024)
    X = (X / np.linalg.norm(X, axis=1, keepdims=True)).astype(np.float32)
    assert X.shape == (9164, 1024)
    Xd = torch.from_numpy(X).cuda().double()
    sq = (Xd * Xd).sum(1)
    D = torch.sqrt(torch.clamp(sq[:, None] + sq[None, :] - 2 * Xd @ Xd.T, min=0)).cpu().numpy()
    D = np.triu(D, 1)
    D = D + D.T
    for t in gap_eps(D, [0.82, 0.85]):
        for m in (2, 5):
            want = sklearn_dbscan(D, t, m)
            assert want[1].max() >= 10
            assert_same(clustering.dbscan_dense(D, t, m), want, (t, m))
            assert_same(clustering.dbscan(X, t, m), dref.dbscan_dense(D, t, m), (t, m))


def test_twenty_thousand_faces():
    import torch
    from hse_facerec_tf_amd import clustering
    n, d = 20000, 256
    X = features(n, d, 21, classes=500)
    Xd = torch.from_numpy(X).cuda().double()
    sq = (Xd * Xd).sum(1)
    blocks = []
    for i0 in range(0, n, 2048):
        blk = torch.sqrt(torch.clamp(sq[i0:i0 + 2048, None] + sq[None, :] - 2 * Xd[i0:i0 + 2048] @ Xd.T, min=0))
        blk[torch.arange(blk.shape[0]), torch.arange(i0, i0 + blk.shape[0])] = np.inf
        r, c = torch.nonzero(blk <= 1.2, as_tuple=True)
        blocks.append(((r + i0).cpu().numpy(), c.cpu().numpy(), blk[r, c].cpu().numpy()))
    rows, cols, w = (np.concatenate(v) for v in zip(*blocks))
    # the blocks are symmetric only to fp64 round-off: every pair takes its upper-triangle value D[lo, hi], the entry of row lo (rows
    # come in ascending order)
    lo, hi = np.minimum(rows, cols), np.maximum(rows, cols)
    key = lo * n + hi
    order = np.argsort(key, kind="stable")
    first = order[np.r_[True, np.diff(key[order]) != 0]]
    first = first[rows[first] == lo[first]]
    ts = ref.gap_thresholds(w[first], [0.65, 1.0], 1e-5)
    for t, m in zip(ts, (3, 5)):
        sel = first[w[first] <= t]
        a, b = lo[sel], hi[sel]
        want = dref.dbscan_from_adjacency(n, np.concatenate([a, b]), np.concatenate([b, a]), m)
        got = clustering.dbscan(X, t, m)
        assert len(np.unique(want[1])) > 50
        assert_same(got, want, (t, m))
        assert_same(clustering.dbscan(X, t, m), got)                       # bit-identical reruns
        s = torch.cuda.Stream()
        with torch.cuda.stream(s):
            got_s = clustering.dbscan(torch.from_numpy(X).cuda(), t, m)
        torch.cuda.synchronize()
        assert_same(got_s, got)


def test_device_outputs_and_stream_order():
    import torch
    from hse_facerec_tf_amd import ops
    X = torch.from_numpy(features(3000, 64, 5, classes=60)).cuda()
    labels, core = ops.dbscan_labels(x=X, eps=0.8, min_samples=4)
    assert labels.is_cuda and labels.dtype == torch.int32 and core.dtype == torch.uint8 and labels.shape == core.shape == (3000,)
    D = torch.from_numpy(fp64_distances(X.cpu().numpy())).cuda()
    labels_d, core_d = ops.dbscan_labels(dense=D, eps=0.8, min_samples=4)
    assert labels_d.is_cuda and labels_d.dtype == torch.int32 and core_d.dtype == torch.uint8
    lab, is_core = labels.cpu().numpy(), core.cpu().numpy().astype(bool)
    assert lab.min() >= -1 and set(np.unique(lab[lab >= 0])) == set(range(lab.max() + 1))
    seeds = [int(np.flatnonzero((lab == v) & is_core)[0]) for v in range(lab.max() + 1)]
    assert seeds == sorted(seeds)                                          # clusters numbered by their smallest core index
    with pytest.raises(ValueError):
        ops.dbscan_labels(x=X, eps=0.0, min_samples=4)
    with pytest.raises(ValueError):
        ops.dbscan_labels(x=X, dense=D, eps=0.8, min_samples=4)
