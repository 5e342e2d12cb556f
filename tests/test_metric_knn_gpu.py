"""GPU suite for hsefr_metric_dist / hsefr_knn_metric (ops.metric_distances, ops.knn(metric=)) and the metric keyword of the
identification protocols: exact chi2 answers on {0, 1, 3} features, every distance against fp64 within the header's bounds
(tests/metric_knn_ref.py), exact zeros for equal rows, position independence bit for bit, the query-slice walk, invalid values, and
scikit-learn's KNeighborsClassifier(metric=callable) with the reference's two callables through the protocol functions."""
import functools
import os

import numpy as np
import pytest

import metric_knn_ref as ref
from oracle import identification as oid

from conftest import GOLDEN

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def torch_():
    import torch
    assert torch.cuda.is_available()
    return torch


def run_knn(torch_, q, g, k, metric, labels=None):
    from hse_facerec_tf_amd import ops
    lab = None if labels is None else torch_.from_numpy(np.ascontiguousarray(labels, dtype=np.int32)).cuda()
    idx, dist, pred = ops.knn(torch_.from_numpy(q).cuda(), torch_.from_numpy(g).cuda(), k, lab, metric=metric)
    assert tuple(idx.shape) == (len(q), k) and tuple(dist.shape) == (len(q), k) and idx.dtype == torch_.int32
    return idx.cpu().numpy(), dist.cpu().numpy(), None if pred is None else pred.cpu().numpy()


def run_dist(torch_, x, y, metric):
    from hse_facerec_tf_amd import ops
    out = ops.metric_distances(torch_.from_numpy(x).cuda(), None if y is None else torch_.from_numpy(y).cuda(), metric=metric)
    assert out.dtype == torch_.float32 and tuple(out.shape) == (len(x), len(x if y is None else y))
    return out.cpu().numpy()


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


EXACT_SHAPES = [(1, 1, 4, 1), (5, 3, 8, 3), (33, 65, 64, 1), (33, 65, 64, 16), (70, 17, 8, 16), (37, 130, 24, 5), (65, 129, 260, 3)]


@pytest.mark.parametrize("nq,ng,d,k", EXACT_SHAPES)
def test_chi2_on_exact_inputs_gives_the_integers_and_the_oracles_neighbours(torch_, nq, ng, d, k):
    """Features in {0, 1, 3}: every term is 0, 1 or 3 where the division is exact, every sum an integer below 2^24, so the distances are
    full of exact ties and the answer is the oracle's and no other.  Identical gallery rows at 0, 31, 32, 63, 64 and ng - 1 with probe 0
    equal to them: its neighbours are the planted rows in index order, at distance 0."""
    rs = np.random.RandomState(nq + ng + d + k)
    g = rs.choice([0, 1, 3], (ng, d)).astype(np.float32)
    q = rs.choice([0, 1, 3], (nq, d)).astype(np.float32)
    planted = sorted({p for p in (0, 31, 32, 63, 64, ng - 1) if p < ng})
    g[planted] = g[planted[0]]
    q[0] = g[planted[0]]
    labels = (rs.randint(-3, 4, ng) * 100003).astype(np.int32)
    D = ref.dist(q, g, "chi2")
    assert np.array_equal(D, np.round(D)) and D.max() < 2 ** 24
    idx, dist, pred = run_knn(torch_, q, g, k, "chi2", labels)
    assert idx.min() >= 0 and idx.max() < ng
    assert np.array_equal(dist.astype(np.float64), np.take_along_axis(D, idx.astype(np.int64), axis=1))      # exactness itself, first
    want_idx, want_dist, want_pred = ref.knn_ref.knn_from_dist2(D, k, labels)
    assert np.array_equal(idx, want_idx)
    assert np.array_equal(dist.astype(np.float64), want_dist)
    assert np.array_equal(pred, want_pred)
    assert idx[0, :min(k, len(planted))].tolist() == planted[:k] and np.all(dist[0, :min(k, len(planted))] == 0)
    idx2, dist2, none = run_knn(torch_, q, g, k, "chi2")                     # without labels: the same neighbours, no prediction
    assert none is None and np.array_equal(idx2, idx) and np.array_equal(bits(dist2), bits(dist))
    full = run_dist(torch_, q, g, "chi2")                                   # the matrix entry point: the same integers
    assert np.array_equal(full.astype(np.float64), D)


def _rows(rs, n, d, scale=1.0):
    return (np.maximum(rs.randn(n, d), 0) * scale).astype(np.float32)


@pytest.mark.parametrize("metric", ref.METRICS)
@pytest.mark.parametrize("n,m,d", [(63, 65, 4), (64, 128, 36), (129, 127, 260), (65, 64, 10), (128, 129, 36)])
def test_metric_distances_are_within_the_bound_of_fp64(torch_, n, m, d, metric):
    """Every element against the exact value on the float32 inputs, n and m on both sides of 64 and 128, d below, across and beyond
    the 32-column chunk and one that ops pads (10); a zero probe, a zero gallery row and a pair of equal rows included."""
    rs = np.random.RandomState(n + m + d)
    x, y = _rows(rs, n, d), _rows(rs, m, d, 2.5)
    x[1] = 0
    y[2] = 0
    y[m - 1] = x[n - 1]
    D, B = ref.dist_and_bound(x, y, metric)
    got = run_dist(torch_, x, y, metric)
    assert np.isfinite(got).all()
    ratio = np.abs(got - D) / np.where(B > 0, B, 1.0)
    print("%s %dx%dx%d: max |dist - truth| / bound = %.3f" % (metric, n, m, d, ratio[B > 0].max()))
    assert np.all(np.abs(got - D) <= B)
    assert got[n - 1, m - 1] == 0 and got[1, 2] == 0                         # equal rows, the zero rows among them: exactly 0


@pytest.mark.parametrize("metric", ref.METRICS)
def test_equal_rows_are_at_exactly_zero(torch_, metric):
    rs = np.random.RandomState(7)
    for n, d, scale in ((130, 36, 1.0), (65, 260, 37.5), (70, 10, 3e-2)):
        x = _rows(rs, n, d, scale)
        same = run_dist(torch_, x, None, metric)
        copy = run_dist(torch_, x, x.copy(), metric)
        assert np.all(same.diagonal() == 0) and np.all(copy.diagonal() == 0)
        assert np.array_equal(bits(same), bits(copy))


@pytest.mark.parametrize("metric", ref.METRICS)
def test_a_distance_depends_on_its_two_rows_only(torch_, metric):
    """Permuting the gallery permutes the matrix bit for bit (rows change tile, lane and padding position), another n, m and row offset
    give the same bits, and a search over two halves of the probes is the search over all of them."""
    from hse_facerec_tf_amd import ops
    rs = np.random.RandomState(11)
    x, y = _rows(rs, 70, 36), _rows(rs, 130, 36)
    whole = run_dist(torch_, x, y, metric)
    perm = rs.permutation(130)
    assert np.array_equal(bits(run_dist(torch_, x, y[perm], metric)), bits(whole[:, perm]))
    assert np.array_equal(bits(run_dist(torch_, x[5:66], y[3:68], metric)), bits(whole[5:66, 3:68]))
    q, g = torch_.from_numpy(x).cuda(), torch_.from_numpy(y).cuda()
    labels = torch_.from_numpy(rs.randint(0, 9, 130).astype(np.int32)).cuda()
    for k in (1, 5):
        idx, dist, pred = ops.knn(q, g, k, labels, metric=metric)
        halves = [ops.knn(q[a:b].contiguous(), g, k, labels, metric=metric) for a, b in ((0, 35), (35, 70))]
        for i, t in enumerate((idx, dist, pred)):
            assert torch_.equal(t, torch_.cat([h[i] for h in halves]))
        picked = np.take_along_axis(whole, idx.cpu().numpy().astype(np.int64), axis=1)
        assert np.array_equal(bits(dist.cpu().numpy()), bits(picked))       # the search returns the matrix entry point's bits


FLOAT_CASES = [(300, 1000, 1024, 1.0), (70, 1000, 264, 37.5), (70, 1000, 264, 3e-2)]


@functools.lru_cache(maxsize=None)
def _float_case(nq, ng, d, scale, metric):
    """Clustered non-negative rows max(centre + 0.7 randn, 0) of any magnitude, a duplicated gallery row, a probe equal to it, a zero
    probe; the fp64 distances and bounds, once for every k."""
    rs = np.random.RandomState(nq + ng + d)
    centres = rs.randn(50, d)
    g = np.maximum(centres[rs.randint(0, 50, ng)] + 0.7 * rs.randn(ng, d), 0).astype(np.float32) * np.float32(scale)
    q = np.maximum(centres[rs.randint(0, 50, nq)] + 0.7 * rs.randn(nq, d), 0).astype(np.float32) * np.float32(scale)
    g[ng // 2] = g[3]
    q[5] = g[3]
    q[6] = 0.0
    D, B = ref.dist_and_bound(q, g, metric)
    for a in (q, g, D, B):
        a.setflags(write=False)
    return q, g, D, B


@pytest.mark.parametrize("metric", ref.METRICS)
@pytest.mark.parametrize("k", [3, 16])
@pytest.mark.parametrize("nq,ng,d,scale", FLOAT_CASES)
def test_float_inputs_vs_fp64(torch_, nq, ng, d, scale, k, metric):
    """Each of the k returned distances against the k-th smallest exact one, and the exact distance of each returned row against it, within
    the larger of the bounds of the rows involved (the oracle's k and the returned k).  No index equality: under the worst-case bounds
    up to a quarter of these rows are near-ties at k = 16."""
    q, g, D, B = _float_case(nq, ng, d, scale, metric)
    idx, dist, _ = run_knn(torch_, q.copy(), g.copy(), k, metric)          # the cached arrays are read-only
    assert idx.min() >= 0 and idx.max() < ng
    assert np.all(np.diff(dist, axis=1) >= 0)
    assert all(len(set(row)) == k for row in idx.tolist())
    idx = idx.astype(np.int64)
    order = np.argsort(D, axis=1, kind="stable")[:, :k]
    truth = np.take_along_axis(D, order, axis=1)
    bound = np.maximum(np.take_along_axis(B, order, axis=1).max(1), np.take_along_axis(B, idx, axis=1).max(1))[:, None]
    own = np.abs(dist - np.take_along_axis(D, idx, axis=1)) / np.maximum(np.take_along_axis(B, idx, axis=1), 1e-300)
    print("%s %dx%dx%d scale %g k=%d: max |dist - D[idx]| / bound = %.3f" % (metric, nq, ng, d, scale, k, own.max()))
    assert np.all(np.abs(dist - np.take_along_axis(D, idx, axis=1)) <= np.take_along_axis(B, idx, axis=1))
    assert np.all(np.abs(dist - truth) <= bound)
    assert np.all(np.abs(np.take_along_axis(D, idx, axis=1) - truth) <= bound)
    row = idx[5].tolist()                                                   # the exact duplicates: equal distances, the lower index first
    if metric == "chi2":
        assert row[:2] == [3, ng // 2] and np.all(dist[5, :2] == 0)
    if 3 in row[:-1]:
        assert row[row.index(3) + 1] == ng // 2
    if ng // 2 in row:
        assert row.index(ng // 2) >= 1 and row[row.index(ng // 2) - 1] == 3


@pytest.mark.parametrize("metric,seed", [("chi2", 5), ("kl", 5)])
def test_large_search_walks_query_slices(torch_, metric, seed):
    """16 500 x 4096 distances are more than one 256 MiB slice: two slices.  Rows are independent and a distance depends on its two rows
    only, so the search done in halves that fit one slice each gives the same bits; rows on both sides of the slice boundary against
    the oracle (clear rows, a property of the seeded inputs)."""
    from hse_facerec_tf_amd import ops
    nq, ng, d, k = 16500, 4096, 8, 3
    assert nq * ng * 4 > 256 << 20 and (256 << 20) // (ng * 4) == 16384
    rs = np.random.RandomState(seed)
    gal_h = np.maximum(rs.randn(ng, d), 0).astype(np.float32)
    q_h = np.maximum(gal_h[rs.randint(0, ng, nq)] + np.float32(0.3) * rs.randn(nq, d).astype(np.float32), 0)
    labels_h = rs.randint(0, 50, ng).astype(np.int32)
    gal, q, labels = (torch_.from_numpy(a).cuda() for a in (gal_h, q_h, labels_h))
    idx, dist, pred = ops.knn(q, gal, k, labels, metric=metric)
    halves = [ops.knn(q[a:b].contiguous(), gal, k, labels, metric=metric) for a, b in ((0, 8250), (8250, 16500))]
    for i, t in enumerate((idx, dist, pred)):
        assert torch_.equal(t, torch_.cat([h[i] for h in halves]))
    rows = np.array([0, 1, 8249, 8250, 16383, 16384, 16385, 16499])
    D, B = ref.dist_and_bound(q_h[rows], gal_h, metric)
    assert ref.clear_rows(D, B, k).all()                                    # a property of the seeded inputs
    want_idx, want_dist, want_pred = ref.knn_ref.knn_from_dist2(D, k, labels_h)
    got_idx = idx[rows].cpu().numpy().astype(np.int64)
    assert np.array_equal(got_idx, want_idx) and np.array_equal(pred[rows].cpu().numpy(), want_pred)
    assert np.all(np.abs(dist[rows].cpu().numpy() - want_dist) <= np.take_along_axis(B, got_idx, axis=1))


def test_invalid_values_sort_last_or_add_nothing(torch_):
    """A kl row with an entry <= -0.001 is at +inf from (or to) every row and such pairs sort last, in index order; a chi2 column whose
    sum is negative or zero adds 0."""
    rs = np.random.RandomState(3)
    g = _rows(rs, 9, 8) + np.float32(0.5)
    q = _rows(rs, 4, 8) + np.float32(0.5)
    g[2, 5] = -0.001                                                        # fl32(-0.001f + 0.001f) = 0: log b = -inf
    g[6, 0] = -3.0                                                          # b < 0: log b is NaN
    q[1, 7] = -0.5                                                          # a < 0: every pair of this probe
    got = run_dist(torch_, q, g, "kl")
    assert not np.isnan(got).any()
    assert np.all(np.isposinf(got[:, [2, 6]])) and np.all(np.isposinf(got[1]))
    fine = np.ones((4, 9), bool)
    fine[:, [2, 6]] = False
    fine[1] = False
    D, B = ref.dist_and_bound(q, g, "kl")
    assert np.isfinite(got[fine]).all() and np.all(np.abs(got[fine] - D[fine]) <= B[fine])
    idx, dist, _ = run_knn(torch_, q, g, 9, "kl")
    assert idx[0, 7:].tolist() == [2, 6] and np.all(np.isposinf(dist[0, 7:])) and np.isfinite(dist[0, :7]).all()
    assert idx[1].tolist() == list(range(9)) and np.all(np.isposinf(dist[1]))
    x = np.array([[-2, 1, 0, 3], [0, 0, 0, 0]], np.float32)
    y = np.array([[1, 1, 0, 1], [0, 0, 0, 0], [-1, -1, 5, -3]], np.float32)
    got = run_dist(torch_, x, y, "chi2")
    # row 0 against y[0]: sums (-1, 2, 0, 4), the first adds 0 | against y[2]: sums (-3, 0, 5, 0), only the third column counts
    assert got.tolist() == [[1.0, 4.0, 5.0], [3.0, 0.0, 5.0]]


def _protocol_fixture():
    z = np.load(os.path.join(GOLDEN, "protocols.npz"))
    X, y = oid.synthetic_gallery(int(z["n_classes"]), int(z["dim"]), int(z["seed"]), float(z["noise"]))
    Xn, y2, kept = oid.filter_and_encode(X, y)
    assert np.array_equal(y2, z["y"])
    return z, X[kept].astype(np.float32)


def _device_normalised(torch_, X):
    from hse_facerec_tf_amd import ops
    return ops.l2_normalize(torch_.from_numpy(X).cuda()).cpu().numpy()


def _sklearn(metric, k, A_gal, y_gal, A_probe):
    from sklearn.neighbors import KNeighborsClassifier
    clf = KNeighborsClassifier(n_neighbors=k, metric=ref.CALLABLES[metric]).fit(A_gal, y_gal)
    return clf.kneighbors(A_probe)[1], clf.predict(A_probe)


@pytest.mark.parametrize("metric", ref.METRICS)
@pytest.mark.parametrize("normalize", [False, True])
@pytest.mark.parametrize("k", [1, 3, 5])
def test_gallery_probe_protocol_matches_sklearn_with_the_callable(torch_, k, normalize, metric):
    """gallery_probe_identification(metric=) vs KNeighborsClassifier(k, metric=chi2dist | KL_dist) on the protocols.npz split (146 probes
    x 170 gallery rows x 256; the L2-normalised rows are the device's own, which both sides see).  A probe is clear when its first
    k + 1 oracle distances are further apart than the sum of their two bounds: every probe for k = 1 and 3, all but 3 at most for
    k = 5; on clear probes the neighbours, the predictions and with them the accuracy are scikit-learn's."""
    from hse_facerec_tf_amd import identification
    z, Xraw = _protocol_fixture()
    A = _device_normalised(torch_, Xraw) if normalize else Xraw
    g, p = z["gallery"], z["probe"]
    yg, yp = z["y"][g], z["y"][p]
    want_idx, want_pred = _sklearn(metric, k, A[g], yg, A[p])
    r = identification.gallery_probe_identification(Xraw[g], yg, Xraw[p], yp, normalize=normalize, n_neighbors=k, metric=metric)
    shape = (146,) if k == 1 else (146, k)
    assert r["nn_index"].shape == shape and r["nn_dist"].shape == shape and r["nn_dist"].dtype == np.float32
    D, B = ref.dist_and_bound(A[p], A[g], metric)
    clear = ref.clear_rows(D, B, k)
    unclear = int((~clear).sum())
    print("%s k=%d normalize=%s: %d unclear probes" % (metric, k, normalize, unclear))
    assert unclear <= (3 if k == 5 else 0)
    got_idx = r["nn_index"].reshape(146, k).astype(np.int64)
    assert np.array_equal(got_idx[clear], want_idx[clear])
    assert np.array_equal(r["y_pred"][clear], want_pred[clear])
    assert abs(r["accuracy"] - float((want_pred == yp).mean())) <= unclear / 146.0 + 1e-12
    assert np.all(np.abs(r["nn_dist"].reshape(146, k) - np.take_along_axis(D, got_idx, axis=1)) <= np.take_along_axis(B, got_idx, axis=1))


@pytest.mark.parametrize("metric", ref.METRICS)
def test_stratified_split_protocols_match_sklearn_with_the_callable(torch_, metric):
    """one_nn_identification and cross_validated_1nn (facerec_test.py:424-425: n_neighbors = 1 on X_norm) on the stratified half split."""
    from hse_facerec_tf_amd import identification
    z, Xraw = _protocol_fixture()
    y = z["y"]
    Xn = _device_normalised(torch_, Xraw)
    for k in (1, 3):
        r = identification.one_nn_identification(Xraw, y, n_neighbors=k, metric=metric)
        train, test = r["train"], r["test"]
        shape = (len(test),) if k == 1 else (len(test), k)
        assert np.array_equal(r["y"], y) and r["nn_index"].shape == shape and r["nn_dist"].shape == shape
        want_idx, want_pred = _sklearn(metric, k, Xn[train], y[train], Xn[test])
        D, B = ref.dist_and_bound(Xn[test], Xn[train], metric)
        clear = ref.clear_rows(D, B, k)
        unclear = int((~clear).sum())
        print("%s k=%d stratified split: %d probes, %d unclear" % (metric, k, len(test), unclear))
        assert unclear <= (0 if k == 1 else 2)                              # on the host: none but one probe of kl at k = 3
        assert np.array_equal(r["nn_index"].reshape(len(test), k)[clear], want_idx[clear])
        assert np.array_equal(r["y_pred"][clear], want_pred[clear])
        assert abs(r["accuracy"] - float((want_pred == y[test]).mean())) <= unclear / len(test) + 1e-12
        cv = identification.cross_validated_1nn(Xraw, y, [(train, test)], n_neighbors=k, metric=metric)
        assert cv["accuracies"].shape == (1,) and cv["accuracies"][0] == r["accuracy"] and np.array_equal(cv["y_pred"][0], r["y_pred"])


def test_metric_l2_is_the_path_it_was_and_string_labels_pass_through(torch_):
    from hse_facerec_tf_amd import identification
    z, Xraw = _protocol_fixture()
    y = z["y"]
    g, p = z["gallery"], z["probe"]
    for k in (1, 3):
        a = identification.one_nn_identification(Xraw, y, n_neighbors=k)
        b = identification.one_nn_identification(Xraw, y, n_neighbors=k, metric="l2")
        assert a.keys() == b.keys() and all(np.array_equal(a[key], b[key]) for key in a)
        a = identification.gallery_probe_identification(Xraw[g], y[g], Xraw[p], y[p], n_neighbors=k)
        b = identification.gallery_probe_identification(Xraw[g], y[g], Xraw[p], y[p], n_neighbors=k, metric="l2")
        assert a.keys() == b.keys() and all(np.array_equal(a[key], b[key]) for key in a)
    gal = np.zeros((6, 8), np.float32)
    gal[:, 1] = np.arange(6) / 10.0                                         # rows (1 - t, t, 0, ...): both distances to (1, 0, ...) grow with t
    gal[:, 0] = 1 - gal[:, 1]
    names = np.array(["carol", "alice", "bob", "dave", "dave", "dave"])
    for metric in ref.METRICS:
        assert np.all(np.diff(ref.dist(gal[:1], gal, metric)[0]) > 0)
        r = identification.gallery_probe_identification(gal, names, gal[:1], np.array(["carol"]), metric=metric)
        assert r["y_pred"].tolist() == ["carol"] and r["y_pred"].dtype.kind == "U" and r["accuracy"] == 1.0
        assert r["nn_index"].tolist() == [0] and r["nn_dist"].tolist() == [0.0]
        r = identification.gallery_probe_identification(gal, names, gal[:1], np.array(["alice"]), n_neighbors=3, metric=metric)
        assert r["nn_index"].tolist() == [[0, 1, 2]] and r["y_pred"].tolist() == ["alice"]      # three labels once each: the smallest
        r = identification.gallery_probe_identification(gal, names, gal[:1], np.array(["dave"]), n_neighbors=5, metric=metric)
        assert r["y_pred"].tolist() == ["dave"] and r["accuracy"] == 1.0
