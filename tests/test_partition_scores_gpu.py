"""GPU suite: flat cuts and partition scores on the device (csrc/partition_scores.hip through ops.flat_cuts / ops.partition_scores)
and the study's statistics built on them (clustering.clustering_scores, threshold_sweep, select_threshold).  The counts are NumPy's
as integers and ARI is scikit-learn's with ==; the six sums lie within the derived bounds (tests/partition_scores_ref.py) of the
mpmath goldens; results are bit-identical between calls, between a row of a 71-row call and a call on that row alone, and between
duplicate rows; the sweeps reproduce the host path (existing clustering, the study's y_pred, scikit-learn and bcubed)."""
import functools
import os

import numpy as np
import pytest
from sklearn import metrics

import partition_scores_ref as ref
from partition_cases import AMI_KINDS, CASES
from test_partition_scores_cpu import reference_rank_order_loop, reference_scalar_loop

pytestmark = pytest.mark.gpu
INT32_MAX = 2 ** 31 - 1

GOLDEN = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "partition_scores_exact.npz"))


def device_scores(y, labels):
    import torch
    from hse_facerec_tf_amd import ops
    counts, stats = ops.partition_scores(torch.from_numpy(np.ascontiguousarray(y)).cuda(), torch.from_numpy(np.ascontiguousarray(labels)).cuda())
    return counts.cpu().numpy(), stats.cpu().numpy()


@functools.lru_cache(maxsize=None)
def case_result(name):
    return device_scores(*CASES[name])


def tie_matrix(n, seed):
    rs = np.random.RandomState(seed)
    D = np.triu(rs.randint(1, max(8, n // 4), (n, n)).astype(np.float64), 1)
    return D + D.T


def rand_matrix(n, seed):
    D = np.triu(np.random.RandomState(seed).rand(n, n), 1)
    return D + D.T


@pytest.mark.parametrize("method", ["single", "average"])
@pytest.mark.parametrize("n", [2, 3, 65, 257, 1030])
def test_flat_cuts_is_fcluster_distance(n, method):
    import torch
    from hse_facerec_tf_amd import clustering, ops
    for D in (tie_matrix(n, 30 + n), rand_matrix(n, 40 + n)):
        Z = clustering.linkage_dense(D, method)
        order, gaps = clustering._cut_order(Z)
        exact = np.unique(gaps)
        ts = np.concatenate([exact[:: max(1, len(exact) // 12)], exact[-1:], [gaps.min() - 1.0, gaps.min() - 1e-9, gaps.max() + 1e-9,
                                                                            gaps.max() + 1.0, float(np.median(gaps)) + 1e-7]])
        got = ops.flat_cuts(torch.from_numpy(order.astype(np.int32)).cuda(), torch.from_numpy(gaps).cuda(),
                            torch.from_numpy(ts).cuda()).cpu().numpy()
        assert got.dtype == np.int32 and np.array_equal(got, clustering.fcluster_distance(Z, ts)), (n, method)
        assert got[len(ts) - 5].max() == n and got[len(ts) - 2].max() == 1     # below every gap: singletons; above: one cluster


def test_flat_cuts_of_one_leaf():
    import torch
    from hse_facerec_tf_amd import ops
    got = ops.flat_cuts(torch.zeros(1, dtype=torch.int32).cuda(), torch.zeros(0, dtype=torch.float64).cuda(),
                        torch.tensor([0.5, 2.0], dtype=torch.float64).cuda())
    assert got.cpu().tolist() == [[1], [1]]


@pytest.mark.parametrize("name", sorted(CASES))
def test_counts_ari_and_sums(name):
    from hse_facerec_tf_amd import clustering
    y, labels = CASES[name]
    n = len(y)
    counts, stats = case_result(name)
    assert counts.dtype == np.int64 and counts.shape == (len(labels), 8) and stats.dtype == np.float64 and stats.shape == (len(labels), 6)
    b_sum = ref.bound_sum(n)
    for r, row in enumerate(labels):
        a, b, nij, _, _, nonneg = ref.table(y, row)
        assert np.array_equal(counts[r], ref.counts_of(a, b, nij, nonneg)), (name, r)
        err = np.abs(stats[r] - GOLDEN[name][r])
        b_emi = ref.bound_emi(n, GOLDEN[name][r][3], ref.emi_terms_grouped(a, b, n))
        print("%s row %d: errors %s, bounds %.3g / EMI %.3g" % (name, r, err, b_sum, b_emi))
        assert (err[[0, 1, 2, 4, 5]] <= b_sum).all() and err[3] <= b_emi, (name, r, err, b_sum, b_emi)
        got = clustering.scores_from_counts(counts[r], stats[r], n)
        assert got[0] == metrics.adjusted_rand_score(y, ref.study_y_pred(row)), (name, r)
        if len(labels) <= 2 or r in (0, 5, 40, 70):
            ref.assert_scores(name, y, row, GOLDEN[name][r], got, name.split("_")[0] in AMI_KINDS and n >= 63)


def test_results_are_bit_identical():
    y, labels = CASES["random_n4099_rows71"]
    counts, stats = case_result("random_n4099_rows71")
    again = device_scores(y, labels)
    assert np.array_equal(again[0], counts) and again[1].tobytes() == stats.tobytes()
    assert np.array_equal(counts[5], counts[40]) and stats[5].tobytes() == stats[40].tobytes()          # the duplicate rows
    for r in (0, 5, 33, 70):
        alone = device_scores(y, labels[r:r + 1])
        assert np.array_equal(alone[0][0], counts[r]) and alone[1][0].tobytes() == stats[r].tobytes(), r
    # a merge of two clusters that share no class leaves the first B-cubed sum unchanged: the same bits, so that a selection sees a tie
    y, labels = CASES["random_n1000"]
    row = labels[0]
    ids = np.unique(row)
    classes = [set(y[row == c].tolist()) for c in ids]
    i, j = next((i, j) for i in range(len(ids)) for j in range(i + 1, len(ids)) if not classes[i] & classes[j])
    merged = np.where(row == ids[j], ids[i], row).astype(np.int32)
    relabelled = (INT32_MAX - merged).astype(np.int32)          # and another naming of the clusters, which reorders the cells
    pair = device_scores(y, np.stack([row, merged, relabelled]))
    assert pair[1][0][4].tobytes() == pair[1][1][4].tobytes() == pair[1][2][4].tobytes() and pair[0][0][1] == pair[0][1][1] + 1
    y, labels = CASES["negatives_n1000"]
    both, second = device_scores(y, labels), device_scores(y, labels[1:])
    assert np.array_equal(both[0][1], second[0][0]) and both[1][1].tobytes() == second[1][0].tobytes()


def zipf_album(n, classes, seed):
    rs = np.random.RandomState(seed)
    w = 1.0 / np.arange(1, classes + 1)
    y = rs.choice(classes, size=n, p=w / w.sum()).astype(np.int32)
    return rs, y


def test_lfw_size_counts_and_ari():
    """9164 faces pad to 16384 keys: the largest sort that runs in LDS"""
    from hse_facerec_tf_amd import clustering
    n, rows = 9164, 71
    rs, y = zipf_album(n, 1680, 11)
    labels = np.stack([np.where(rs.rand(n) < r / 80.0, rs.randint(0, 1680, n), y * (1 + r % 2) + rs.randint(0, 1 + r % 2, n))
                       for r in range(rows)]).astype(np.int32)
    labels[3][rs.rand(n) < 0.2] = -1
    counts, stats = device_scores(y, labels)
    for r in range(rows):
        assert np.array_equal(counts[r], ref.counts(y, labels[r])), r
        assert clustering.scores_from_counts(counts[r], stats[r], n)[0] == metrics.adjusted_rand_score(y, ref.study_y_pred(labels[r])), r
    assert np.isfinite(stats).all()


@pytest.mark.parametrize("n", [16384 + 4099, 65536])
def test_sort_in_global_memory_above_the_lds_tile(n):
    """more than 16384 keys sort in the row's workspace, up to HSEFR_SCORES_MAX_N; the sums against the NumPy restatement, each within
    the bound of the exact value, so within twice the bound of each other"""
    rs, y = zipf_album(n, 3000, 12)
    labels = np.stack([np.where(rs.rand(n) < 0.1, rs.randint(0, 3000, n), y), rs.randint(0, 40, n)]).astype(np.int32)
    labels[1][rs.rand(n) < 0.05] = -7
    counts, stats = device_scores(y, labels)
    for r in range(2):
        want_counts, want = ref.counts_stats(y, labels[r])
        assert np.array_equal(counts[r], want_counts), r
        a, b = ref.table(y, labels[r])[:2]
        err = np.abs(stats[r] - want)
        print("row %d: errors %s" % (r, err))
        assert (err[[0, 1, 2, 4, 5]] <= 2 * ref.bound_sum(n)).all() and err[3] <= 2 * ref.bound_emi(n, want[3], ref.emi_terms_grouped(a, b, n)), (r, err)
    assert device_scores(y, labels)[1].tobytes() == stats.tobytes()


def test_python_wrappers_check_their_arguments():
    import torch
    from hse_facerec_tf_amd import ops
    y = torch.zeros(5, dtype=torch.int32).cuda()
    for bad in (lambda: ops.partition_scores(y.long(), y), lambda: ops.partition_scores(y, y.long()), lambda: ops.partition_scores(y.cpu(), y),
                lambda: ops.partition_scores(y, y[:4]), lambda: ops.partition_scores(y[:0], y[:0]),
                lambda: ops.partition_scores(y, torch.zeros((2, 10), dtype=torch.int32).cuda()[:, ::2]),
                lambda: ops.flat_cuts(y, torch.zeros(5, dtype=torch.float64).cuda(), torch.zeros(1, dtype=torch.float64).cuda()),
                lambda: ops.flat_cuts(y, torch.zeros(4).cuda(), torch.zeros(1, dtype=torch.float64).cuda()),
                lambda: ops.flat_cuts(y, torch.zeros(4, dtype=torch.float64).cuda(), torch.zeros(0, dtype=torch.float64).cuda()),
                lambda: ops.flat_cuts(y.long(), torch.zeros(4, dtype=torch.float64).cuda(), torch.zeros(1, dtype=torch.float64).cuda())):
        with pytest.raises(ValueError):
            bad()


# ---- the study's statistics against the host path ------------------------------------------------------------------------------
def integer_album(n, seed):
    """integer features around integer centroids (their squared distances are exact in fp32) and the classes"""
    rs = np.random.RandomState(seed)
    classes = max(2, n // 12)
    y = rs.randint(0, classes, n)
    X = (3 * rs.randint(-2, 3, (classes, 8)))[y] + rs.randint(-1, 2, (n, 8))
    return X.astype(np.float32), y


def host_statistics(clusters, y_true):
    """get_clustering_results' y_pred (facial_clustering_test.py:402-409) and get_clustering_statistics' ten numbers (:416-423)"""
    from hse_facerec_tf_amd import clustering
    y_pred = -np.ones(len(y_true))
    for ind, cluster in enumerate(clusters):
        y_pred[cluster] = ind
    ind = len(clusters)
    for i in range(len(y_pred)):
        if y_pred[i] == -1:
            ind += 1
            y_pred[i] = ind
    return y_pred, (len(np.unique(y_true)), len(clusters), metrics.adjusted_rand_score(y_true, y_pred),
                    metrics.adjusted_mutual_info_score(y_true, y_pred, average_method="arithmetic"))


def assert_sweep_row(what, got, clusters, y_true):
    y_pred, (classes, count, ari, _) = host_statistics(clusters, y_true)
    assert (got[0], got[1]) == (classes, count), (what, got[:2], classes, count)
    assert got[2] == ari, what
    exact = ref.counts_stats(y_true, y_pred.astype(np.int64))[1]
    ref.assert_scores(what, y_true, y_pred.astype(np.int64), exact, tuple(float(v) for v in got[2:]), False)


SWEEPS = {"average": [0.5, 1.0, 2.0, 2.5, 3.7, 5.0, 100.0], "single": [0.5, 1.0, 1.5, 2.0, 2.3, 100.0],
          "dbscan": [0.5, 1.0, 1.5, 2.0, 2.3, 100.0], "rankorder": [(0.9, 14), (1.02, 12), (1.1, 20), (0.5, 5), (2.0, 30)]}


@pytest.mark.parametrize("method", ["average", "single", "dbscan", "rankorder"])
@pytest.mark.parametrize("n", [1, 2, 67, 257])
def test_threshold_sweep_is_the_host_path(n, method):
    from hse_facerec_tf_amd import clustering
    X, y = integer_album(n, 50 + n)
    D = np.sqrt(((X[:, None, :].astype(np.float64) - X[None, :, :]) ** 2).sum(-1))
    thresholds = SWEEPS[method]
    min_samples = 2 if method == "dbscan" else 1
    dense = clustering.threshold_sweep(D, y, method, thresholds, dense=True, min_samples=min_samples)
    feats = clustering.threshold_sweep(X, y, method, thresholds, min_samples=min_samples)
    assert dense.shape == feats.shape == (len(thresholds), 10) and dense.dtype == np.float64
    kinds = set()
    for r, t in enumerate(thresholds):
        if n == 1 and method in LINKAGE:
            clusters_d = clusters_f = [[0]]
        else:
            clusters_d = clustering.get_facial_clusters(D, t, no_images_in_cluster=min_samples, method=method)
            clusters_f = clustering.cluster_faces(X, t, min_cluster_size=min_samples, method=method)
        assert_sweep_row((n, method, t, "dense"), dense[r], clusters_d, y)
        if method != "dbscan":
            assert_sweep_row((n, method, t, "features"), feats[r], clusters_f, y)
        else:                   # cluster_faces also drops clusters a border point left short; the sweep scores dbscan's own labels
            labels = clustering.dbscan(X, t, min_samples)[1]
            assert_sweep_row((n, method, t, "features"), feats[r], clustering._clusters(labels), y)
        covered = sum(len(c) for c in clusters_d)
        kinds.add("all" if covered == n else "some")
    if n >= 67 and method in ("dbscan", "rankorder"):
        assert "some" in kinds                  # faces outside every cluster occur: 'clusters' is not the number of labels there


LINKAGE = ("single", "average", "complete", "weighted")


def test_clustering_scores_is_the_host_path():
    from hse_facerec_tf_amd import clustering
    rs = np.random.RandomState(9)
    for n in (1, 2, 65, 257):
        y = rs.randint(0, max(1, n // 10) + 1, n)
        for y_pred in (y.copy(), rs.randint(-3, max(2, n // 6), n), np.where(rs.rand(n) < 0.2, rs.randint(0, 5, n), y).astype(np.float64) - 0.5,
                       np.array(["c%d" % v for v in rs.randint(0, 4, n)])):
            got = clustering.clustering_scores(y, y_pred)
            dense = np.unique(y_pred, return_inverse=True)[1].reshape(-1)
            assert got.shape == (10,) and (got[0], got[1]) == (len(np.unique(y)), len(np.unique(y_pred)))
            assert got[2] == metrics.adjusted_rand_score(y, dense)
            ref.assert_scores((n, "scores"), y, dense, ref.counts_stats(y, dense)[1], tuple(float(v) for v in got[2:]), False)
    with pytest.raises(ValueError):
        clustering.clustering_scores([0, 1], [0, 1, 2])
    with pytest.raises(ValueError):
        clustering.clustering_scores([], [])


def test_select_threshold_is_the_reference_loop():
    from hse_facerec_tf_amd import clustering
    albums = [integer_album(120, 61), integer_album(90, 62)]

    def host_mean(method, threshold, column):
        total = 0
        for X, y in albums:
            y_pred = host_statistics(clustering.cluster_faces(X, threshold, method=method), y)[0]
            if column == "precision":
                total += clustering.bcubed(y, y_pred)[0]
            else:
                total += metrics.homogeneity_completeness_v_measure(y, y_pred)[2]
        return total / len(albums)
    grid = list(np.linspace(0.5, 7.5, 15))
    for method, ceiling in (("average", 0.85), ("single", 0.85), ("average", 2.0)):
        got = clustering.select_threshold(albums, method, thresholds=grid, ceiling=ceiling)
        want = reference_scalar_loop(grid, lambda t: host_mean(method, t, "precision"), ceiling=ceiling)
        assert got.threshold == want[0] and [p[0] for p in got.evaluated] == want[2], (method, got[:3], want)
        assert abs(got.statistic - want[1]) <= ref.bound_sum(120)
        rows = np.stack([clustering.threshold_sweep(X, y, method, [got.threshold])[0] for X, y in albums])
        assert np.array_equal(got.mean, rows.mean(0)) and np.array_equal(got.std, rows.std(0))
    norms, ranks = [0.8, 1.02, 1.1, 1.5], [4, 12, 20]
    got = clustering.select_threshold(albums, "rankorder", norm_thresholds=norms, rank_thresholds=ranks)
    want = reference_rank_order_loop(norms, ranks, lambda pair: host_mean("rankorder", pair, "v"))
    assert got.threshold == want[0] and [p[0] for p in got.evaluated] == want[2], (got[:3], want)
    bound = 0.0                                 # the V-measure's, propagated from the sums at the selected pair
    for X, y in albums:
        y_pred = host_statistics(clustering.cluster_faces(X, want[0], method="rankorder"), y)[0].astype(np.int64)
        h_true, h_pred, mi = ref.counts_stats(y, y_pred)[1][:3]
        bound += 2 * (ref.bound_ratio(len(y), mi, h_true) + ref.bound_ratio(len(y), mi, h_pred)) / len(albums)
    assert abs(got.statistic - want[1]) <= bound
