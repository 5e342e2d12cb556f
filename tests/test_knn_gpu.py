"""GPU suite for hsefr_knn (ops.knn) and the n_neighbors keyword of the identification protocols: exact answers on exact inputs on both
search paths (tests/knn_ref.py), k = 1 against hsefr_nn1 bit for bit, float inputs against fp64, the query-block walk, scikit-learn's
KNeighborsClassifier through the protocol functions, and the vote rule on crafted rows."""
import os

import numpy as np
import pytest

import knn_ref
from oracle import identification as oid

from conftest import GOLDEN

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def torch_():
    import torch
    assert torch.cuda.is_available()
    return torch


def run_knn(torch_, q, g, k, labels=None):
    from hse_facerec_tf_amd import ops
    lab = None if labels is None else torch_.from_numpy(np.ascontiguousarray(labels, dtype=np.int32)).cuda()
    idx, dist, pred = ops.knn(torch_.from_numpy(q).cuda(), torch_.from_numpy(g).cuda(), k, lab)
    assert tuple(idx.shape) == (len(q), k) and tuple(dist.shape) == (len(q), k) and idx.dtype == torch_.int32
    return idx.cpu().numpy(), dist.cpu().numpy(), None if pred is None else pred.cpu().numpy()


def is_split_path(nq, ng, d):
    return d % 32 == 0 and nq * ng * d >= 1 << 28


FP32_SHAPES = [(1, 1, 8, 1), (5, 3, 8, 3), (33, 65, 64, 1), (33, 65, 64, 3), (33, 65, 64, 16), (70, 17, 8, 16), (37, 130, 24, 5)]
SPLIT_SHAPES = [(257, 2049, 512, 3), (257, 2049, 512, 16), (513, 1027, 512, 4)]


@pytest.mark.parametrize("low,high", [(0, 2), (-2, 2)])
@pytest.mark.parametrize("nq,ng,d,k", FP32_SHAPES + SPLIT_SHAPES)
def test_exact_inputs_give_exact_neighbours_and_votes(torch_, nq, ng, d, k, low, high):
    """Small-integer features: every product, every sum and |q|^2 + |g|^2 - 2 q.g is an exact integer in fp32, on the split-f16 path too
    (power-of-two scaling, a hi / lo split without remainder), so the distances are full of exact ties and the answer is knn_ref's and no
    other.  Identical gallery rows at 0, 31, 32, 63, 64 and ng - 1 -- on both sides of the lane, tile, wave and pad boundaries -- with
    probe 0 equal to them: its neighbours are the planted rows in index order."""
    assert is_split_path(nq, ng, d) == ((nq, ng, d, k) in SPLIT_SHAPES)
    rs = np.random.RandomState(nq + ng + d + k + high - low)
    g = rs.randint(low, high + 1, (ng, d)).astype(np.float32)
    q = rs.randint(low, high + 1, (nq, d)).astype(np.float32)
    planted = sorted({p for p in (0, 31, 32, 63, 64, ng - 1) if p < ng})
    g[planted] = g[planted[0]]
    q[0] = g[planted[0]]
    labels = (rs.randint(-3, 4, ng) * 100003).astype(np.int32)
    d2 = knn_ref.dist2(q, g)
    assert np.array_equal(d2, np.round(d2)) and d2.max() < 2 ** 24
    idx, dist, pred = run_knn(torch_, q, g, k, labels)
    assert idx.min() >= 0 and idx.max() < ng
    assert np.array_equal(dist.astype(np.float64), np.take_along_axis(d2, idx.astype(np.int64), axis=1))     # exactness itself, first
    want_idx, want_dist, want_pred = knn_ref.knn_from_dist2(d2, k, labels)
    assert np.array_equal(idx, want_idx)
    assert np.array_equal(dist.astype(np.float64), want_dist)
    assert np.array_equal(pred, want_pred)
    assert idx[0, :min(k, len(planted))].tolist() == planted[:k] and np.all(dist[0, :min(k, len(planted))] == 0)
    if k == 3 and ng > 32:
        assert idx[0].tolist() == [0, 31, 32]
    # without labels: the same neighbours, no prediction
    idx2, dist2, none = run_knn(torch_, q, g, k)
    assert none is None and np.array_equal(idx2, idx) and np.array_equal(dist2, dist)


@pytest.mark.parametrize("nq,ng,d", [(200, 1000, 1024), (300, 1000, 1024)])
def test_k1_is_nn1_bit_for_bit(torch_, nq, ng, d):
    """The invariant that ties the selection to hsefr_nn1, on the fp32 path and on the split-f16 path."""
    from hse_facerec_tf_amd import ops
    assert is_split_path(nq, ng, d) == (nq == 300)
    rs = np.random.RandomState(nq)
    q = torch_.from_numpy(rs.randn(nq, d).astype(np.float32)).cuda()
    g = torch_.from_numpy(rs.randn(ng, d).astype(np.float32)).cuda()
    idx, dist, pred = ops.knn(q, g, 1)
    nn_idx, nn_dist = ops.nn1(q, g)
    assert pred is None
    assert torch_.equal(idx[:, 0], nn_idx) and torch_.equal(dist[:, 0], nn_dist)


@pytest.mark.parametrize("k", [3, 16])
@pytest.mark.parametrize("nq,ng,d,scale", [(300, 1000, 1024, 1.0), (257, 2049, 512, 37.5), (257, 4100, 256, 3e-4), (70, 1000, 264, 1.0)])
def test_float_inputs_vs_fp64(torch_, nq, ng, d, scale, k):
    """The inputs of test_nn1_split_f16_gemm_path_vs_fp64 (clustered rows of any magnitude, a duplicated gallery row, a zero probe, a
    gallery row a thousand times smaller) and its error scale, unit = max|q| max|g| d 2^-20, for every one of the k neighbours; the
    last shape runs the fp32 tiles."""
    assert is_split_path(nq, ng, d) == (d != 264)
    rs = np.random.RandomState(nq + ng + d)
    centres = rs.randn(50, d)
    g = (centres[rs.randint(0, 50, ng)] + 0.7 * rs.randn(ng, d)).astype(np.float32) * np.float32(scale)
    q = (centres[rs.randint(0, 50, nq)] + 0.7 * rs.randn(nq, d)).astype(np.float32) * np.float32(scale)
    g[ng // 2] = g[3]
    q[5] = g[3]
    q[6] = 0.0
    g[7] *= np.float32(1e-3)
    d2 = knn_ref.dist2(q, g)
    idx, dist, _ = run_knn(torch_, q, g, k)
    unit = float((np.abs(q).max() * np.abs(g).max()) * d) * 2.0 ** -20
    truth = np.sort(d2, axis=1)[:, :k]
    assert np.all(np.diff(dist, axis=1) >= 0)
    assert idx.min() >= 0 and idx.max() < ng
    assert all(len(set(row)) == k for row in idx.tolist())
    print("max |dist - truth| / unit = %.3f" % (np.abs(dist - truth).max() / unit))
    assert np.abs(dist - truth).max() <= unit
    assert np.abs(np.take_along_axis(d2, idx.astype(np.int64), axis=1) - truth).max() <= unit
    assert idx[5, :2].tolist() == [3, ng // 2]               # the exact duplicates: equal distances, the lower index first


def _clear_rows(d2, k, unit):
    """Rows whose first k + 1 fp64-sorted distances are all further apart than the fp32 error scale."""
    first = np.sort(d2, axis=1)[:, :k + 1]
    return np.all(np.diff(first, axis=1) > unit, axis=1)


@pytest.mark.parametrize("d,seed", [(32, 5), (8, 7)])
def test_large_search_walks_query_blocks(torch_, d, seed):
    """16 500 x 4096 distances are more than the 256 MiB slice: two query blocks, on the split-f16 path (d = 32) and on the fp32 tiles
    (d = 8).  Rows are independent, so the search done in halves that fit one block each finds the same neighbours (on the split path
    each search scales its probes by one power of two of its own largest value, which can move a distance's last bit: see
    test_nn1_gemm_path_walks_large_searches_in_query_blocks); rows on both sides of the block boundary against fp64."""
    from hse_facerec_tf_amd import ops
    nq, ng, k = 16500, 4096, 3
    assert is_split_path(nq, ng, d) == (d == 32) and nq * ng * 4 > 256 << 20 and (256 << 20) // (ng * 4) == 16384
    rs = np.random.RandomState(seed)
    gal_h = rs.randn(ng, d).astype(np.float32)
    q_h = gal_h[rs.randint(0, ng, nq)] + np.float32(0.3) * rs.randn(nq, d).astype(np.float32)
    labels_h = rs.randint(0, 50, ng).astype(np.int32)
    gal, q, labels = (torch_.from_numpy(a).cuda() for a in (gal_h, q_h, labels_h))
    idx, dist, pred = ops.knn(q, gal, k, labels)
    halves = [ops.knn(q[a:b].contiguous(), gal, k, labels) for a, b in ((0, 8250), (8250, 16500))]
    assert torch_.equal(idx, torch_.cat([h[0] for h in halves]))
    assert float((dist - torch_.cat([h[1] for h in halves])).abs().max()) < 1e-4
    assert torch_.equal(pred, torch_.cat([h[2] for h in halves]))
    rows = np.array([0, 1, 8249, 8250, 16383, 16384, 16385, 16499])
    d2 = knn_ref.dist2(q_h[rows], gal_h)
    unit = float(np.abs(q_h).max() * np.abs(gal_h).max()) * d * 2.0 ** -20
    clear = _clear_rows(d2, k, unit)
    want_idx, want_dist, want_pred = knn_ref.knn_from_dist2(d2, k, labels_h)
    got_idx = idx[rows].cpu().numpy()
    assert clear.all()                                       # a property of the seeded inputs: none of these rows is an fp32 tie
    assert np.array_equal(got_idx[clear], want_idx[clear]) and np.array_equal(pred[rows].cpu().numpy()[clear], want_pred[clear])
    assert np.abs(dist[rows].cpu().numpy() - want_dist).max() <= unit
    assert np.abs(np.take_along_axis(d2, got_idx.astype(np.int64), axis=1) - want_dist).max() <= unit


def _protocol_fixture():
    z = np.load(os.path.join(GOLDEN, "protocols.npz"))
    X, y = oid.synthetic_gallery(int(z["n_classes"]), int(z["dim"]), int(z["seed"]), float(z["noise"]))
    Xn, y2, kept = oid.filter_and_encode(X, y)
    assert np.array_equal(y2, z["y"])
    return z, X[kept], Xn


@pytest.mark.parametrize("normalize", [False, True])
@pytest.mark.parametrize("k", [3, 5])
def test_gallery_probe_protocol_matches_sklearn(torch_, k, normalize):
    """gallery_probe_identification(n_neighbors=k) vs KNeighborsClassifier(k) on the protocols.npz split (146 probes x 170 gallery rows x
    256).  A probe is CLEAR when its first k + 1 fp64 distances are further apart than unit = max|q| max|g| d 2^-20; for k = 3 every
    probe is (unit 0.0122 against a smallest gap of 0.039 on the raw features, 3.2e-5 against 1.36e-4 normalised), for k = 5 at most two
    are not; on clear probes neighbours, predictions and with them the accuracy are scikit-learn's."""
    from sklearn.neighbors import KNeighborsClassifier
    from hse_facerec_tf_amd import identification
    z, Xraw, Xn = _protocol_fixture()
    A = Xn if normalize else Xraw
    g, p = z["gallery"], z["probe"]
    yg, yp = z["y"][g], z["y"][p]
    clf = KNeighborsClassifier(n_neighbors=k, p=2).fit(A[g], yg)
    want_dist, want_idx = clf.kneighbors(A[p])
    want_pred = clf.predict(A[p])
    r = identification.gallery_probe_identification(Xraw[g], yg, Xraw[p], yp, normalize=normalize, n_neighbors=k)
    assert r["nn_index"].shape == (146, k) and r["nn_dist"].shape == (146, k)
    unit = float(np.abs(A[p]).max() * np.abs(A[g]).max()) * A.shape[1] * 2.0 ** -20
    clear = _clear_rows(knn_ref.dist2(A[p], A[g]), k, unit)
    unclear = int((~clear).sum())
    print("k=%d normalize=%s: unit %.3e, %d unclear probes" % (k, normalize, unit, unclear))
    assert unclear <= (0 if k == 3 else 2)
    assert np.array_equal(r["nn_index"][clear], want_idx[clear])
    assert np.array_equal(r["y_pred"][clear], want_pred[clear])
    assert abs(r["accuracy"] - float((want_pred == yp).mean())) <= unclear / 146.0 + 1e-12
    assert np.abs(r["nn_dist"] ** 2 - want_dist ** 2).max() <= unit


def test_3nn_pca_matches_sklearn_pipeline(torch_):
    """The reference's '3-NN+PCA' (facerec_test.py:270, 16 components) at the bar of test_pca_variant_matches_sklearn_pipeline."""
    from sklearn.decomposition import PCA
    from sklearn.neighbors import KNeighborsClassifier
    from sklearn.pipeline import Pipeline
    from hse_facerec_tf_amd import identification
    z, Xraw, _ = _protocol_fixture()
    g, p = z["gallery"], z["probe"]
    pipe = Pipeline(steps=[('pca', PCA(n_components=16)), ('classifier', KNeighborsClassifier(n_neighbors=3, p=2))])
    want = pipe.fit(Xraw[g], z["y"][g]).predict(Xraw[p])
    r = identification.gallery_probe_identification(Xraw[g], z["y"][g], Xraw[p], z["y"][p], pca_components=16, n_neighbors=3)
    assert r["nn_index"].shape == (146, 3)
    assert (r["y_pred"] == want).mean() > 0.98            # PCA sign/rounding may flip a near-tie


def test_stratified_split_protocols_match_sklearn_cross_validate(torch_):
    """one_nn_identification and cross_validated_1nn with n_neighbors=3 on the stratified half split vs scikit-learn's cross_validate of
    KNeighborsClassifier(3): the same accuracy, up to the probes that are not clear (see test_gallery_probe_protocol_matches_sklearn)."""
    from sklearn import model_selection
    from sklearn.neighbors import KNeighborsClassifier
    from hse_facerec_tf_amd import identification
    z, Xraw, Xn = _protocol_fixture()
    y = z["y"]
    r = identification.one_nn_identification(Xraw, y, n_neighbors=3)
    train, test = r["train"], r["test"]
    assert np.array_equal(r["y"], y) and r["nn_index"].shape == (len(test), 3) and r["nn_dist"].shape == (len(test), 3)
    want = model_selection.cross_validate(KNeighborsClassifier(n_neighbors=3, p=2), Xn, y, scoring="accuracy", cv=[(train, test)])["test_score"][0]
    unit = float(np.abs(Xn[test]).max() * np.abs(Xn[train]).max()) * Xn.shape[1] * 2.0 ** -20
    unclear = int((~_clear_rows(knn_ref.dist2(Xn[test], Xn[train]), 3, unit)).sum())
    print("stratified split: %d probes, %d unclear" % (len(test), unclear))
    assert unclear <= 2
    assert abs(r["accuracy"] - want) <= unclear / len(test) + 1e-12
    cv = identification.cross_validated_1nn(Xraw, y, [(train, test)], n_neighbors=3)
    assert cv["accuracies"].shape == (1,) and abs(cv["accuracies"][0] - want) <= unclear / len(test) + 1e-12
    assert np.array_equal(cv["y_pred"][0], r["y_pred"])
    # n_neighbors=1 is the path it was: the same dictionary as without the keyword
    a, b = identification.one_nn_identification(Xraw, y), identification.one_nn_identification(Xraw, y, n_neighbors=1)
    assert a.keys() == b.keys() and all(np.array_equal(a[key], b[key]) for key in a) and a["nn_index"].ndim == 1


def test_vote_rule_on_crafted_rows(torch_):
    """Gallery row j lies at distance j + 1 from the probe, so the neighbour order is the row order and only the labels vary."""
    from hse_facerec_tf_amd import identification
    g = np.zeros((6, 8), np.float32)
    g[:, 0] = np.arange(1, 7)
    q = np.zeros((1, 8), np.float32)

    def vote(k, labels):
        idx, dist, pred = run_knn(torch_, q, g, k, np.array(labels, np.int32))
        assert idx.tolist() == [list(range(k))] and dist.tolist() == [[float((j + 1) ** 2) for j in range(k)]]
        return int(pred[0])
    assert vote(3, [7, -2, 5, -9, -9, -9]) == -2             # three different labels: the smallest, not the nearest row's
    assert vote(4, [9, 4, 4, 9, 1, 1]) == 4                  # 2 - 2: the smaller label
    assert vote(4, [4, 9, 9, 4, 1, 1]) == 4
    for labels in ([8, 8, 1], [8, 1, 8], [1, 8, 8]):         # 2 - 1: the majority, wherever it sits
        assert vote(3, labels + [1, 1, 1]) == 8
    assert vote(1, [7, -2, 5, 0, 0, 0]) == 7
    assert vote(6, [3, 2, 3, 2, 2, 3]) == 2                  # k == ng, 3 - 3
    assert vote(5, [2 ** 31 - 1, -2 ** 31, 2 ** 31 - 1, -2 ** 31, 2 ** 31 - 1, 0]) == 2 ** 31 - 1     # the ends of int32
    names = np.array(["carol", "alice", "bob", "dave", "dave", "dave"])
    r = identification.gallery_probe_identification(g, names, q, np.array(["alice"]), n_neighbors=3)
    assert r["y_pred"].tolist() == ["alice"] and r["y_pred"].dtype.kind == "U" and r["accuracy"] == 1.0
    r = identification.gallery_probe_identification(g, names, q, np.array(["alice"]), n_neighbors=5)
    assert r["y_pred"].tolist() == ["dave"] and r["accuracy"] == 0.0
