"""GPU suite: rank-order clustering on the device (csrc/rank_order.hip through hse_facerec_tf_amd.clustering) against the reference's
recorded clusters (tests/golden/rank_order_reference.npz) and against the restatement of tests/rank_order_ref.py where the reference is
too slow to record: random and tied matrices up to n = 4099, the KN / NB edges, the upper-triangle reading, the features path on integer
features, threshold sequences, the drop-ins for the reference's branch, and an LFW-sized run.

The normalised distance nd of a merged cluster depends on the order its neighbour sums are added in (the reference's own order follows
Python set iteration), ~1e-12 relative.  Inputs whose sums are not exact are therefore used only where no tested pair lies within 1e-9
(relative) of the norm threshold -- 1e-5 on the features path, whose distances carry fp32 rounding."""
import numpy as np
import pytest

import rank_order_ref as ror
from test_dbscan_gpu import rand_matrix, tie_matrix
from test_linkage_gpu import ages, fp64_distances
from test_rank_order_cpu import CASES, golden_cases, golden_matrix

pytestmark = pytest.mark.gpu

THRESHOLDS = ((0.9, 14), (1.06, 16), (1.1, 20))


def safe_norm(D, norm, rank, min_margin, max_steps=5):
    """The first of norm, norm + 1e-3, ... whose restatement margin is >= min_margin -> (norm, clusters, iterations)."""
    for step in range(max_steps + 1):
        t = norm + 1e-3 * step
        clusters, iters, margin = ror.rank_order(D, t, rank)
        print("norm %.3f rank %g: margin %.3g after %d steps" % (t, rank, margin, step))
        if margin >= min_margin:
            return t, clusters, iters
    raise AssertionError("no norm threshold with margin >= %g within %d steps of %g" % (min_margin, max_steps, norm))


def test_dense_path_returns_the_recorded_reference_clusters():
    from hse_facerec_tf_amd import clustering
    cases = 0
    for kind, n, classes, seed, norm, rank, want in golden_cases():
        D = golden_matrix(kind, n, classes, seed)
        got, iters = clustering.rank_order_dense(D, norm, rank)
        assert got == [sorted(c) for c in want], (kind, n, seed, norm, rank)
        assert iters == ror.rank_order(D, norm, rank)[1], (kind, n, seed, norm, rank)
        cases += 1
    assert cases == CASES


@pytest.mark.parametrize("n", [1, 2, 12, 13, 19, 20, 21, 65, 257, 1000, 4099])
def test_dense_path_is_the_restatement_on_tied_matrices(n):
    """Integer distances with many ties (and zeros): the (value, index) order decides the lists.  Every sum is exact, so nd has no
    summation-order uncertainty and no margin is asked for."""
    from hse_facerec_tf_amd import clustering
    D = tie_matrix(n, 30 + n)
    for norm, rank in THRESHOLDS:
        want, iters, _ = ror.rank_order(D, norm, rank)
        assert clustering.rank_order_dense(D, norm, rank) == (want, iters), (n, norm, rank)
    X = np.random.RandomState(n).randint(0, 3, (n, 2)).astype(np.float64)     # a 3 x 3 grid: coincident faces, the zero guard
    G = ror.integer_distances(X)
    for norm, rank in THRESHOLDS:
        want, iters, _ = ror.rank_order(G, norm, rank)
        assert clustering.rank_order_dense(G, norm, rank) == (want, iters), ("grid", n, norm, rank)


def test_dense_path_is_the_restatement_on_random_matrices():
    from hse_facerec_tf_amd import clustering
    cases = skipped = 0
    for n in (1, 2, 12, 13, 19, 20, 21, 65, 257, 1000, 4099):
        for norm, rank in THRESHOLDS:
            cases += 1
            D = rand_matrix(n, 50 + n)
            want, iters, margin = ror.rank_order(D, norm, rank)
            print("n=%d (%g, %g): %d clusters, %d iterations, margin %.3g" % (n, norm, rank, len(want), iters, margin))
            if margin < 1e-9:
                skipped += 1
                continue
            assert clustering.rank_order_dense(D, norm, rank) == (want, iters), (n, norm, rank)
    assert cases == 33 and skipped * 20 <= cases


def test_clustered_matrices_merge_over_several_iterations():
    """Clustered faces at sizes between the fixture's and the LFW run: the in-place reduce runs several times."""
    from hse_facerec_tf_amd import clustering
    for n, classes, seed in ((700, 50, 21), (2500, 150, 22)):
        _, D = ror.integer_case(n, classes, seed)
        for norm, rank in THRESHOLDS:
            want, iters, margin = ror.rank_order(D, norm, rank)
            assert margin >= 1e-9 and iters >= 2 and len(want) >= classes // 2
            assert clustering.rank_order_dense(D, norm, rank) == (want, iters), (n, norm, rank)


def test_dense_path_reads_the_upper_triangle_and_no_diagonal():
    from hse_facerec_tf_amd import clustering
    rs = np.random.RandomState(5)
    n = 301
    _, S = ror.integer_case(n, 20, 9)
    A = np.triu(S, 1) + np.tril(rs.rand(n, n) * 40, -1) + np.diag(rs.rand(n) * 40 + 1)    # asymmetric, non-zero diagonal
    for norm, rank in THRESHOLDS:
        want, iters, margin = ror.rank_order(S, norm, rank)
        assert margin >= 1e-9 and len(want) > 3
        assert clustering.rank_order_dense(A, norm, rank) == (want, iters)
        assert clustering.rank_order_dense(S, norm, rank) == (want, iters)


@pytest.mark.parametrize("n", [64, 257, 500])
@pytest.mark.parametrize("with_age", [False, True])
def test_features_path_on_integer_features(n, with_age):
    """Squared distances of integer features are exact in fp32, so the order of distinct distances and every tie survive the fp32 root;
    nd carries its rounding (~1e-7 relative), hence thresholds with a restatement margin >= 1e-5."""
    from hse_facerec_tf_amd import clustering
    X, D = ror.integer_case(n, max(3, n // 12), 60 + n)
    born, photo = ages(n, 61 + n) if with_age else (None, None)
    if with_age:
        D = fp64_distances(X, born, photo)
    for norm0, rank in THRESHOLDS:
        norm, want, iters = safe_norm(D, norm0, rank, 1e-5)
        assert len(want) >= 2
        assert clustering.rank_order(X.astype(np.float32), norm, rank, born, photo) == (want, iters), (n, norm, rank)
        assert clustering.rank_order_dense(D, norm, rank) == (want, iters), (n, norm, rank)
        assert clustering.cluster_faces(X.astype(np.float32), (norm, rank), born, photo, method="rankorder") == want
    X30 = np.ascontiguousarray(X[:, :30])                                      # d padded to a multiple of 8
    D30 = fp64_distances(X30, born, photo)
    norm, want, _ = safe_norm(D30, 1.06, 16, 1e-5)
    assert clustering.cluster_faces(X30.astype(np.float32), (norm, 16), born, photo, method="rankorder") == want


def test_threshold_sequence_is_the_separate_calls():
    from hse_facerec_tf_amd import clustering
    n = 600
    X, D = ror.integer_case(n, 40, 77)
    pairs = [(0.9, 14), (1.1, 20), (1.06, 16), (0.9, 14), (0.7, 5)]
    got = clustering.rank_order_dense(D, thresholds=pairs)
    assert len(got) == len(pairs)
    for (norm, rank), res in zip(pairs, got):
        assert res == clustering.rank_order_dense(D, norm, rank), (norm, rank)
        want, iters, margin = ror.rank_order(D, norm, rank)
        assert margin >= 1e-9 and res == (want, iters)
    assert len({tuple(map(tuple, r[0])) for r in got}) >= 3                    # the pairs do give different clusterings
    assert clustering.rank_order_dense(D, thresholds=pairs[:1]) == [got[0]]
    Xf = X.astype(np.float32)
    born, photo = ages(n, 78)
    got_f = clustering.rank_order(Xf, born_years=born, photo_years=photo, thresholds=pairs)
    for (norm, rank), res in zip(pairs, got_f):
        assert res == clustering.rank_order(Xf, norm, rank, born, photo), (norm, rank)


def test_drop_ins_for_the_reference_branch():
    from hse_facerec_tf_amd import clustering
    n = 400
    X, D = ror.integer_case(n, 30, 88)
    Xf = X.astype(np.float32)
    photos = np.random.RandomState(3).randint(0, 150, n)
    want = clustering.rank_order_dense(D, 0.9, 14)[0]
    assert want == ror.rank_order(D, 0.9, 14)[0] and len(want) > 5
    assert clustering.get_facial_clusters(D, (0.9, 14), method="rankorder") == want
    assert clustering.get_facial_clusters(D, [0.9, 14], photos, no_images_in_cluster=7, method="rankorder") == want
    assert clustering.get_facial_clusters(D, 0.9, method="rankorder") == want              # a scalar is (scalar, 14)
    assert clustering.get_facial_clusters(D, 1.06, method="rankorder") == clustering.rank_order_dense(D, 1.06, 14)[0]
    want_f = clustering.rank_order(Xf, 1.06, 16)[0]
    assert clustering.cluster_faces(Xf, (1.06, 16), method="rankorder") == want_f
    assert clustering.cluster_faces(Xf, (1.06, 16), all_indices=photos, min_cluster_size=9, method="rankorder") == want_f
    assert clustering.cluster_faces(Xf, 1.06, method="rankorder") == clustering.rank_order(Xf, 1.06, 14)[0]
    assert want == sorted(want, key=lambda c: (-len(c), c[0])) and all(c == sorted(c) and len(c) >= 2 for c in want)
    # one face: no cluster of two
    assert clustering.get_facial_clusters(D[:1, :1], (0.9, 14), method="rankorder") == []
    assert clustering.cluster_faces(Xf[:1], (0.9, 14), method="rankorder") == []
    assert clustering.rank_order_dense(D[:1, :1]) == ([], 1) and clustering.rank_order(Xf[:1]) == ([], 1)


def unit_rows(n, d, seed):
    """The clustered unit-norm features of tools/linkage_time.py."""
    import torch
    g = torch.Generator(device="cuda").manual_seed(seed)
    c = torch.randn((max(2, n // 6), d), device="cuda", generator=g)
    x = c[torch.randint(0, c.shape[0], (n,), device="cuda", generator=g)] + 0.8 * torch.randn((n, d), device="cuda", generator=g)
    return (x / x.norm(dim=1, keepdim=True)).contiguous()


def test_lfw_sized_rank_order():
    """n = 9164, d = 1024: the features path finishes and repeats itself bit for bit; the dense path on the device's own fp32 distances
    (ops.pairwise_distances, widened) agrees with the restatement on the same matrix, which is vectorised enough to run at this size."""
    import torch
    from hse_facerec_tf_amd import clustering, ops
    n, d = 9164, 1024
    x = unit_rows(n, d, n + d)
    lab1, it1 = ops.rank_order_labels(x=x, norm_threshold=1.06, rank_threshold=16)
    lab2, it2 = ops.rank_order_labels(x=x, norm_threshold=1.06, rank_threshold=16)
    assert it1 == it2 and bool((lab1 == lab2).all())
    lab = lab1.cpu().numpy()
    assert np.array_equal(lab[lab], lab) and (lab <= np.arange(n)).all()       # every label is the smallest face of its cluster
    clusters, iters = clustering.rank_order(x, 1.06, 16)
    assert iters == it1 and clusters == ror.clusters_of(lab) and len(clusters) >= 100
    D = ops.pairwise_distances(x).double().cpu().numpy()
    D = np.triu(D, 1)
    D = D + D.T
    norm, want, want_iters = safe_norm(D, 1.06, 16, 1e-9)
    assert len(want) >= 100
    assert clustering.rank_order_dense(D, norm, 16) == (want, want_iters)
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        lab_s, it_s = ops.rank_order_labels(x=x, norm_threshold=1.06, rank_threshold=16)
    torch.cuda.synchronize()
    assert it_s == it1 and bool((lab_s == lab1).all())


def test_device_outputs():
    import torch
    from hse_facerec_tf_amd import ops
    X, D = ror.integer_case(900, 50, 5)
    x = torch.from_numpy(X.astype(np.float32)).cuda()
    labels, iters = ops.rank_order_labels(x=x)
    assert labels.is_cuda and labels.dtype == torch.int32 and labels.shape == (900,) and isinstance(iters, int) and iters >= 2
    Dd = torch.from_numpy(D).cuda()
    labels_s, iters_s = ops.rank_order_labels(dense=Dd, thresholds=[(0.9, 14), (1.06, 16)])
    assert labels_s.shape == (2, 900) and labels_s.dtype == torch.int32 and len(iters_s) == 2
    assert ror.clusters_of(labels_s[0].cpu().numpy()) == ror.rank_order(D, 0.9, 14)[0]
    with pytest.raises(ValueError):
        ops.rank_order_labels(x=x, norm_threshold=0.0)
    with pytest.raises(ValueError):
        ops.rank_order_labels(x=x, dense=Dd)
    with pytest.raises(ValueError):
        ops.rank_order_labels(dense=Dd, thresholds=[])
