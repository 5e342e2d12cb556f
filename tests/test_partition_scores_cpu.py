"""CPU suite for the scoring of clustering sweeps: clustering.scores_from_counts against scikit-learn 1.7 on a NumPy restatement of
hsefr_partition_scores (tests/partition_scores_ref.py), the mpmath goldens against scikit-learn's own sums (which validates the fixture
and the bounds), the two selection loops of the clustering study against their literal restatement on synthetic score tables, and
the argument checks of the two C entry points."""
import ctypes
import os

import numpy as np
import pytest
from sklearn import metrics
from sklearn.metrics.cluster import contingency_matrix, entropy, expected_mutual_information, mutual_info_score

import partition_scores_ref as ref
from partition_cases import AMI_KINDS, CASES

GOLDEN = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "partition_scores_exact.npz"))


def rows_of(name, labels):
    """every row of a small case, a spread of rows of a 71-row one (the duplicate pair 5 / 40 included)"""
    return range(len(labels)) if len(labels) <= 2 else (0, 1, 5, 17, 40, 70)


def test_scores_from_counts_is_sklearn():
    from hse_facerec_tf_amd import clustering
    compared, special, skipped = [], 0, []
    for name, (y, labels) in CASES.items():
        for r in rows_of(name, labels):
            counts, stats = ref.counts_stats(y, labels[r])
            got = clustering.scores_from_counts(counts, stats, len(y))
            assert len(got) == 8 and all(type(v) is float for v in got)
            how, den = ref.assert_scores(name, y, labels[r], GOLDEN[name][r], got, name.split("_")[0] in AMI_KINDS and len(y) >= 63)
            if how == "quotient":
                compared.append(abs(den))
            elif how == "special":
                special += 1
            else:
                skipped.append((name, r, den))
    print("AMI: %d rows through the quotient (denominators %.2f .. %.2f), %d special values, not compared (denominator < 0.1): %s"
          % (len(compared), min(compared), max(compared), special, skipped))
    assert len(compared) >= 30 and min(compared) >= 0.1 and special >= 10
    assert all(len(CASES[name][0]) <= 3 for name, _, _ in skipped), skipped       # only the smallest albums are that ill-conditioned
    for kind in ("renamed", "singletons"):      # the kinds with a known AMI went through the quotient at their larger sizes
        assert not [s for s in skipped if s[0].startswith(kind) and len(CASES[s[0]][0]) >= 64]


def test_scores_from_counts_special_cases():
    """scikit-learn's own answers on the degenerate tables, by construction"""
    from hse_facerec_tf_amd import clustering
    one, two, four = np.zeros(4, int), np.array([0, 0, 1, 1]), np.arange(4)
    for y, p in ((one, one), (one, two), (two, one), (one, four), (four, one), (two, two), (two, 1 - two), (four, four), (two, four),
                 (four, two), (np.zeros(1, int), np.zeros(1, int))):
        counts, stats = ref.counts_stats(y, p)
        got = clustering.scores_from_counts(counts, stats, len(y))
        ref.assert_scores((y, p), y, p, stats, got, False)
        want = (metrics.adjusted_rand_score(y, p), metrics.adjusted_mutual_info_score(y, p)) \
            + metrics.homogeneity_completeness_v_measure(y, p)
        assert got[0] == want[0]
        if len(np.unique(y)) == 1 or len(np.unique(p)) == 1:
            assert got[:5] == want, (y, p, got, want)


def test_goldens_agree_with_sklearn_and_the_restatement():
    from hse_facerec_tf_amd import clustering
    assert sorted(GOLDEN.files) == sorted(CASES)
    for name, (y, labels) in CASES.items():
        n = len(y)
        assert GOLDEN[name].shape == (len(labels), 6)
        for r in rows_of(name, labels):
            g = GOLDEN[name][r]
            y_pred = ref.study_y_pred(labels[r])
            a, b = ref.table(y, labels[r])[:2]
            b_sum = ref.bound_sum(n)
            cont = contingency_matrix(y, y_pred, sparse=True)
            sk = [entropy(y), entropy(y_pred), mutual_info_score(None, None, contingency=cont) if min(len(a), len(b)) > 1 else g[2],
                  expected_mutual_information(cont, n)]
            p, rec, _ = clustering.bcubed(y, y_pred)
            for got, what, terms in ((sk + [p, rec], "scikit-learn", ref.emi_terms(a, b, n)),
                                     (list(ref.counts_stats(y, labels[r])[1]), "restatement", ref.emi_terms_grouped(a, b, n))):
                err, b_emi = np.abs(np.array(got) - g), ref.bound_emi(n, g[3], terms)
                assert (err[[0, 1, 2, 4, 5]] <= b_sum).all() and err[3] <= b_emi, (name, r, what, err, b_sum, b_emi)
            if labels[r].min() >= 0:           # the restated counts are the contingency table's
                counts = ref.counts_stats(y, labels[r])[0]
                dense = cont.toarray().astype(np.int64)
                assert list(counts) == [dense.shape[0], dense.shape[1], int((dense.sum(0) >= 2).sum()), dense.shape[1],
                                        int((dense > 0).sum()), int((dense ** 2).sum()), int((dense.sum(1) ** 2).sum()),
                                        int((dense.sum(0) ** 2).sum())]


# ---- the selection loops: facial_clustering_test.py:447-499 restated literally over a statistic that is looked up ------------------
def reference_scalar_loop(thresholds, stat_of, drop=0.01, ceiling=0.85):
    bestStatistic, prevStatistic = 0, 0
    bestThreshold = 0
    evaluated = []
    for distanceThreshold in thresholds:
        currentStatistic = stat_of(distanceThreshold)
        evaluated.append(distanceThreshold)
        if currentStatistic > bestStatistic:
            bestStatistic = currentStatistic
            bestThreshold = distanceThreshold
        if currentStatistic < prevStatistic - drop:
            break
        if currentStatistic > ceiling:
            break
        prevStatistic = currentStatistic
    return bestThreshold, bestStatistic, evaluated


def reference_rank_order_loop(norms, ranks, stat_of):
    bestStatistic, prevStatistic = 0, 0
    bestThreshold = (0, 0)
    evaluated = []
    for distanceThreshold in norms:
        prevStatistic = 0
        bestChanged = False
        for rankThreshold in ranks:
            currentStatistic = stat_of((distanceThreshold, rankThreshold))
            evaluated.append((distanceThreshold, rankThreshold))
            if currentStatistic > bestStatistic:
                bestStatistic = currentStatistic
                bestThreshold = (distanceThreshold, rankThreshold)
                bestChanged = True
            if currentStatistic <= prevStatistic:
                break
            prevStatistic = currentStatistic
        if not bestChanged:
            break
    return bestThreshold, bestStatistic, evaluated


CURVES = {
    "ceiling": [0.2, 0.5, 0.86, 0.9, 0.95],                     # stops at the first point above 0.85, which is the best
    "ceiling_is_strict": [0.2, 0.85, 0.85, 0.7, 0.1],           # 0.85 itself does not stop; the tie does not replace the best
    "drop": [0.5, 0.6, 0.58, 0.7, 0.5, 0.9],                    # a fall of 0.02 stops; 0.9 is never seen
    "drop_is_strict": [0.5, 0.49, 0.48, 0.47, 0.2, 0.8],        # falls of exactly-representable < 0.01 keep going
    "tie_keeps_the_first": [0.3, 0.6, 0.6, 0.6, 0.1],
    "all_zero": [0.0, 0.0, 0.0],
    "rises_to_the_end": [0.1, 0.2, 0.3, 0.4],
    "first_point_above": [0.99, 0.1],
}
GRIDS = {
    "equal_ends_a_row": [[0.2, 0.3, 0.3, 0.9, 0.9], [0.4, 0.5, 0.6, 0.7, 0.8], [0.1, 0.1, 0.1, 0.1, 0.1]],
    "row_without_a_new_best_ends_all": [[0.5, 0.6, 0.1, 0.9, 0.9], [0.5, 0.6, 0.6, 0.99, 0.99], [0.9, 0.95, 0.97, 0.98, 0.99]],
    "tie_keeps_the_first": [[0.5, 0.7, 0.6, 0.0, 0.0], [0.6, 0.7, 0.8, 0.7, 0.0], [0.8, 0.8, 0.9, 0.9, 0.9]],
    "zero_first_point": [[0.0, 0.9, 0.9, 0.9, 0.9], [0.9, 0.9, 0.9, 0.9, 0.9]],
    "all_rising": [[0.1, 0.2, 0.3, 0.4, 0.5], [0.2, 0.3, 0.4, 0.5, 0.6], [0.3, 0.4, 0.5, 0.6, 0.7]],
}


def test_selection_loops_are_the_reference_loops():
    from hse_facerec_tf_amd import clustering
    for name, curve in CURVES.items():
        ts = list(np.linspace(0.6, 1.3, 71)[:len(curve)])
        want = reference_scalar_loop(ts, dict(zip(ts, curve)).__getitem__)
        got = clustering.select_from_curve(ts, curve)
        assert (got[0], got[1], got[2]) == (want[0], want[1], len(want[2])), name
    assert clustering.select_from_curve([1, 2, 3], CURVES["drop"][:3], drop=0.05)[2] == 3          # the bounds are arguments
    assert clustering.select_from_curve([1, 2, 3], [0.1, 0.4, 0.5], ceiling=0.3)[:2] == (2, 0.4)
    for name, grid in GRIDS.items():
        norms, ranks = list(np.linspace(1.02, 1.1, 9)[:len(grid)]), list(range(12, 22, 2))
        table = {(a, b): grid[i][j] for i, a in enumerate(norms) for j, b in enumerate(ranks)}
        want = reference_rank_order_loop(norms, ranks, table.__getitem__)
        got = clustering.select_from_grid(norms, ranks, grid)
        assert (got[0], got[1]) == want[:2], name
        assert [(norms[i], ranks[j]) for i, j in got[2]] == want[2], name
    rs = np.random.RandomState(0)
    for _ in range(200):                        # and on random tables, coarse enough for ties
        curve = list(np.round(rs.rand(12) * rs.choice([0.5, 1.0]), 1))
        want = reference_scalar_loop(range(12), curve.__getitem__)
        assert clustering.select_from_curve(range(12), curve) == (want[0], want[1], len(want[2]))
        grid = np.round(rs.rand(4, 5), 1)
        want = reference_rank_order_loop(range(4), range(5), lambda ab: grid[ab])
        assert clustering.select_from_grid(range(4), range(5), grid) == want


def test_select_threshold_on_synthetic_albums(monkeypatch):
    """select_threshold with threshold_sweep replaced by tables: the albums' statistics are added in order and divided once, the
    stopping rules see that mean, and the ten statistics are averaged at the best threshold"""
    from hse_facerec_tf_amd import clustering
    rs = np.random.RandomState(1)
    col_p, col_v = clustering.STATS_NAMES.index("BCubed_precision"), clustering.STATS_NAMES.index("v-measure")
    assert (col_p, col_v) == (7, 6) and len(clustering.STATS_NAMES) == 10
    tables = {}

    def fake_sweep(source, y_true, method, thresholds, **kw):
        assert kw == dict(dense=False, min_samples=1, device=None)
        key = (source, len(thresholds))
        if key not in tables:
            tables[key] = rs.rand(len(thresholds), 10)
            if len(thresholds) == 71:
                tables[key][:, col_p] = np.clip(np.linspace(0.1, 0.8, 71) + 0.004 * rs.randn(71) + 0.05 * source, 0, 1)
        return tables[key]
    monkeypatch.setattr(clustering, "threshold_sweep", fake_sweep)
    albums = [(0, None), (1, None), (2, None)]
    for method, column in (("average", col_p), ("dbscan", col_p), ("rankorder", col_v)):
        tables.clear()
        got = clustering.select_threshold(albums, method)
        size = 45 if method == "rankorder" else 71
        stat = np.zeros(size)
        for a in range(3):
            stat = stat + tables[(a, size)][:, column]
        stat = stat / 3
        if method == "rankorder":
            norms, ranks = list(np.linspace(1.02, 1.1, 9)), list(range(12, 22, 2))
            grid = [(a, b) for a in norms for b in ranks]
            want = reference_rank_order_loop(norms, ranks, lambda ab: stat[grid.index(ab)])
        else:
            grid = list(np.linspace(0.6, 1.3, 71))
            want = reference_scalar_loop(grid, lambda t: stat[grid.index(t)])
        assert got.threshold == want[0] and got.statistic == want[1]
        assert [p[0] for p in got.evaluated] == want[2] and [p[1] for p in got.evaluated] == [stat[grid.index(t)] for t in want[2]]
        rows = np.stack([tables[(a, size)][grid.index(want[0])] for a in range(3)])
        assert np.array_equal(got.mean, np.mean(rows, axis=0)) and np.array_equal(got.std, np.std(rows, axis=0))
    # nothing scores above 0: the reference goes on with threshold 0 -- a linkage cut there; no DBSCAN or rank-order clustering
    calls = []

    def zero_sweep(source, y_true, method, thresholds, **kw):
        calls.append(list(thresholds))
        return np.zeros((len(thresholds), 10)) + (len(thresholds) == 1) * np.arange(10)
    monkeypatch.setattr(clustering, "threshold_sweep", zero_sweep)
    got = clustering.select_threshold(albums, "single")
    assert (got.threshold, got.statistic, len(got.evaluated)) == (0, 0.0, 71) and calls[-1] == [0]
    assert np.array_equal(got.mean, np.arange(10)) and np.array_equal(got.std, np.zeros(10))
    for method in ("dbscan", "rankorder"):
        with pytest.raises(ValueError, match="scored above 0"):
            clustering.select_threshold(albums, method)
    with pytest.raises(ValueError):
        clustering.select_threshold([], "average")
    with pytest.raises(ValueError):
        clustering.select_threshold(albums, "ward")


def test_entry_points_reject_bad_arguments_without_a_gpu():
    from hse_facerec_tf_amd import _lib
    L = _lib.lib()
    buf = ctypes.create_string_buffer(256)
    p = ctypes.cast(buf, ctypes.c_void_p).value
    assert len(_lib.SIGNATURES["hsefr_flat_cuts"][1]) == 7 and len(_lib.SIGNATURES["hsefr_partition_scores"][1]) == 7
    assert hasattr(L, "hsefr_flat_cuts") and hasattr(L, "hsefr_partition_scores")
    ok = dict(order=p, gaps=p, n=4, thr=p, rows=2, labels=p)
    for kw in (dict(order=None), dict(gaps=None), dict(thr=None), dict(labels=None), dict(n=0), dict(n=-1), dict(rows=0), dict(rows=-7)):
        a = dict(ok, **kw)
        assert L.hsefr_flat_cuts(a["order"], a["gaps"], a["n"], a["thr"], a["rows"], a["labels"], None) == _lib.ERR_INVALID, kw
        assert _lib.last_error().startswith("flat_cuts:"), (kw, _lib.last_error())
    ok = dict(y=p, labels=p, n=4, rows=2, counts=p, stats=p)
    for kw in (dict(y=None), dict(labels=None), dict(counts=None), dict(stats=None), dict(n=0), dict(n=-1), dict(rows=0), dict(rows=-7),
               dict(n=65537), dict(n=2 ** 31 - 1)):
        a = dict(ok, **kw)
        assert L.hsefr_partition_scores(a["y"], a["labels"], a["n"], a["rows"], a["counts"], a["stats"], None) == _lib.ERR_INVALID, kw
        assert _lib.last_error().startswith("partition_scores:"), (kw, _lib.last_error())
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "hsefr.h")).read()
    assert "#define HSEFR_SCORES_MAX_N 65536" in header
    from hse_facerec_tf_amd import ops
    assert ops.SCORES_MAX_N == 65536


def test_restated_flat_cuts_is_fcluster_distance():
    from hse_facerec_tf_amd import clustering
    import scipy.cluster.hierarchy as hac
    rs = np.random.RandomState(3)
    for n in (2, 3, 17, 64):
        D = rs.randint(1, 6, (n, n)).astype(np.float64)
        Z = hac.linkage(D[np.triu_indices(n, 1)], "average")
        order, gaps = clustering._cut_order(Z)
        ts = np.concatenate([np.unique(gaps), [0.0, 100.0, 2.5]])
        assert np.array_equal(ref.flat_cuts(order, gaps, ts), clustering.fcluster_distance(Z, ts))
