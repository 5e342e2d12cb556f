"""GPU suite for the random forest (hsefr_forest_fit / _predict through ops) and the classifier="random_forest" keyword of the
identification protocols: the device forest against tests/random_forest_ref.py bit for bit on the shapes of
tests/random_forest_cases.py, run-to-run and stream-to-stream equality, scikit-learn's recorded forests through
ops.random_forest_from_sklearn, the protocols against ops called by hand, and the fixture's accuracy against the recorded spread of
scikit-learn's own forests (tests/golden/random_forest.npz)."""
import numpy as np
import pytest

import pca_cases
import random_forest_cases as cases

pytestmark = pytest.mark.gpu

NODE_ARRAYS = ("feature", "threshold", "left", "right", "weight", "leaf_begin", "leaf_len")


@pytest.fixture(scope="module")
def torch_():
    import torch
    assert torch.cuda.is_available()
    return torch


def up(torch_, a, dtype=np.float32):
    return torch_.from_numpy(np.ascontiguousarray(a, dtype=dtype)).cuda()


@pytest.fixture(scope="module")
def fitted(torch_):
    """Every case fitted once on the device and shared, unchanged, by the tests below."""
    from hse_facerec_tf_amd import ops
    memo = {}

    def get(name):
        if name not in memo:
            X, y, C, kw, _, _, _ = cases.case(name)
            memo[name] = ops.random_forest_fit(up(torch_, X), up(torch_, y, np.int32), C, **kw)
        return memo[name]
    return get


def forest_bytes(forest):
    return [getattr(forest, name).cpu().numpy().tobytes() for name in forest.ARRAYS]


@pytest.mark.parametrize("name", list(cases.CASES))
def test_the_device_forest_is_the_restatement_bit_for_bit(torch_, fitted, name):
    from hse_facerec_tf_amd import ops
    X, y, C, kw, probes, want, proba_w = cases.case(name)
    got = fitted(name)
    n = len(X)
    assert got.n_trees == len(want) and got.node_capacity == ops.forest_node_capacity(n, kw["max_depth"]) and got.leaf_capacity == n
    assert np.array_equal(got.n_nodes.cpu().numpy(), [t["n_nodes"] for t in want])
    arrays = {k: getattr(got, k).cpu().numpy() for k in got.ARRAYS}
    for i, t in enumerate(want):
        m = t["n_nodes"]
        for k in NODE_ARRAYS:
            assert arrays[k][i, :m].tobytes() == t[k].tobytes(), (name, i, k)
            assert (arrays[k][i, m:] == (0.0 if k == "threshold" else -1)).all(), (name, i, k)
        assert np.array_equal(arrays["leaf_class"][i], t["leaf_class"]) and np.array_equal(arrays["leaf_count"][i], t["leaf_count"]), (name, i)
    proba, pred = ops.random_forest_predict_proba(got, up(torch_, probes))
    assert proba.cpu().numpy().tobytes() == proba_w.tobytes()
    assert np.array_equal(pred.cpu().numpy(), np.argmax(proba_w, axis=1))
    assert torch_.equal(ops.random_forest_predict(got, up(torch_, probes)), pred)
    if name == "duplicates":
        assert min(t["continued"] for t in want) > 0              # the visit past max_features was taken
    if name in ("tile_edge", "large_bootstrap", "large_leaves", "large_constant"):
        assert int((want[0]["weights"] > 0).sum()) > cases.SORT_TILE   # the root went through the global-memory sort
    if name == "large_leaves":                                         # and so did a leaf's class list
        assert want[0]["n_nodes"] == 3 and max(int(want[0]["weight"][1]), int(want[0]["weight"][2])) > cases.SORT_TILE
    if name == "large_constant":                                       # the root's visit went past max_features, in global memory
        assert want[0]["continued"] >= 1 and want[0]["feature"][0] >= 0


@pytest.mark.parametrize("name", ["n77", "large_bootstrap", "duplicates"])
def test_two_fits_are_bit_equal_on_any_stream(torch_, fitted, name):
    from hse_facerec_tf_amd import ops
    X, y, C, kw, probes, _, _ = cases.case(name)
    first = forest_bytes(fitted(name))
    xd, yd = up(torch_, X), up(torch_, y, np.int32)
    assert forest_bytes(ops.random_forest_fit(xd, yd, C, **kw)) == first
    s = torch_.cuda.Stream()
    with torch_.cuda.stream(s):
        again = ops.random_forest_fit(xd, yd, C, **kw)
        pred = ops.random_forest_predict(again, up(torch_, probes))
    torch_.cuda.synchronize()
    assert forest_bytes(again) == first
    assert torch_.equal(pred, ops.random_forest_predict(fitted(name), up(torch_, probes)))
    if torch_.cuda.device_count() > 1:
        other = ops.random_forest_fit(xd.to("cuda:1"), yd.to("cuda:1"), C, **kw)
        assert other.device.index == 1 and forest_bytes(other) == first


def test_bad_input_is_an_error(torch_):
    from hse_facerec_tf_amd import ops
    X, y, C, kw, _, _, _ = cases.case("n77")
    xd, yd = up(torch_, X), up(torch_, y, np.int32)
    for bad in (np.where(np.arange(len(y)) == 5, C, y), np.where(np.arange(len(y)) == 5, -1, y)):
        with pytest.raises(ValueError, match="outside 0..n_classes-1 = 4"):
            ops.random_forest_fit(xd, up(torch_, bad, np.int32), C, **kw)
    for value in (np.nan, np.inf, -np.inf):
        Xb = X.copy()
        Xb[40, 3] = value
        with pytest.raises(ValueError, match=r"x \(float32 \[77, 20\]\) holds a NaN or an infinity"):
            ops.random_forest_fit(up(torch_, Xb), yd, C, **kw)


def test_a_forest_built_by_hand_is_checked_before_it_runs(torch_, fitted):
    """dtype, shape, device and contiguity of every array of a RandomForest: what the kernel would otherwise read out of bounds."""
    from hse_facerec_tf_amd import ops
    good = fitted("n77")
    q = up(torch_, cases.case("n77")[4])

    def with_(**changed):
        return ops.RandomForest(good.n_classes, good.n_features, **dict({k: getattr(good, k) for k in good.ARRAYS}, **changed))
    assert torch_.equal(ops.random_forest_predict(with_(), q), ops.random_forest_predict(good, q))
    for changed, word in ((dict(threshold=good.threshold.float()), "forest.threshold must be a contiguous float64"),
                          (dict(left=good.left[:, :-1].contiguous()), "forest.left must be a contiguous int32"),
                          (dict(right=good.right.t().contiguous().t()), "not contiguous"),
                          (dict(weight=good.weight.long()), "forest.weight"), (dict(leaf_count=good.leaf_count[:, :5].contiguous()), "forest.leaf_count"),
                          (dict(leaf_len=good.leaf_len.cpu()), "forest.leaf_len"), (dict(n_nodes=good.n_nodes[:1]), "forest.n_nodes"),
                          (dict(feature=good.feature[0]), "forest.feature")):
        with pytest.raises(ValueError, match=word):
            ops.random_forest_predict(with_(**changed), q)


@pytest.mark.parametrize("prefix", ["sk0_", "sk1_", "sk2_"])
def test_scikit_learns_recorded_forests_run_on_the_device(torch_, prefix):
    """ops.random_forest_from_sklearn + predict_proba against scikit-learn's recorded predict_proba: within 1e-12 (about (n_trees + 5)
    2^-53 = 1.2e-14 for 100 trees, x 100 for scikit-learn's own renormalisation), equal labels wherever scikit-learn's two largest
    probabilities are more than 1e-12 apart, and at most 5 % of the probes left out by that rule."""
    from hse_facerec_tf_amd import ops
    g = cases.golden()
    forest = ops.random_forest_from_sklearn(cases.recorded_estimator(g, prefix))
    want = g[prefix + "proba"]
    proba, pred = ops.random_forest_predict_proba(forest, up(torch_, g[prefix + "probes"]))
    err = float(np.abs(proba.cpu().numpy() - want).max())
    top2 = np.sort(want, axis=1)[:, -2:]
    certain = top2[:, 1] - top2[:, 0] > 1e-12
    print("%s %d trees: max |dP| = %.2e, %d of %d probes certain" % (prefix, forest.n_trees, err, int(certain.sum()), len(want)))
    assert err <= 1e-12
    assert certain.mean() >= 0.95
    assert np.array_equal(pred.cpu().numpy()[certain], np.argmax(want, axis=1)[certain])
    assert (pred.cpu().numpy() >= 0).all()


def by_hand(torch_, gal, labels, qry, **kw):
    from hse_facerec_tf_amd import ops
    classes, codes = np.unique(labels, return_inverse=True)
    forest = ops.random_forest_fit(gal, up(torch_, codes, np.int32), len(classes), **kw)
    proba, pred = ops.random_forest_predict_proba(forest, qry)
    return classes[pred.cpu().numpy()], proba.max(dim=1).values.cpu().numpy(), forest.n_nodes.cpu().numpy()


# 12 components: padded to 16 columns by either PCA path, which the forest drops
@pytest.mark.parametrize("pca_components,pca", [(None, "device"), (12, "device"), (12, "host")])
def test_gallery_probe_protocol(torch_, pca_components, pca):
    from hse_facerec_tf_amd import identification, ops
    z, Xraw, _ = pca_cases.protocol_fixture()
    gi, pi = z["gallery"], z["probe"]
    yg, yp = z["y"][gi], z["y"][pi]
    kw = dict(classifier="random_forest", forest_trees=12, forest_depth=7, forest_seed=3)
    r = identification.gallery_probe_identification(Xraw[gi], yg, Xraw[pi], yp, pca_components=pca_components, pca=pca, **kw)
    assert sorted(r) == ["accuracy", "forest_nodes", "proba_max", "y_pred"]
    gal, qry = up(torch_, Xraw[gi]), up(torch_, Xraw[pi])
    if pca_components and pca == "device":
        mean, components, _, _ = ops.pca_fit(gal, pca_components, max_iter=identification.PCA_MAX_ITER)
        gal = ops.pca_transform(gal, mean, components)[:, :pca_components].contiguous()
        qry = ops.pca_transform(qry, mean, components)[:, :pca_components].contiguous()
    elif pca_components:
        from sklearn.decomposition import PCA
        fitted = PCA(n_components=pca_components).fit(Xraw[gi])
        gal, qry = (up(torch_, fitted.transform(a).astype(np.float32)) for a in (Xraw[gi], Xraw[pi]))
    assert gal.shape[1] == (pca_components or Xraw.shape[1])
    pred, pmax, nodes = by_hand(torch_, gal, yg, qry, n_trees=12, max_depth=7, seed=3)
    assert np.array_equal(r["y_pred"], pred) and np.array_equal(r["proba_max"], pmax) and np.array_equal(r["forest_nodes"], nodes)
    assert r["accuracy"] == float((pred == yp).mean()) and r["forest_nodes"].shape == (12,)
    with pytest.raises(ValueError, match="n_neighbors=3 has no meaning with classifier='random_forest'"):
        identification.gallery_probe_identification(Xraw[gi], yg, Xraw[pi], yp, n_neighbors=3, **kw)
    if pca == "device":                                        # scikit-learn's transform refuses an empty probe set
        empty = identification.gallery_probe_identification(Xraw[gi], yg, Xraw[:0], yp[:0], pca_components=pca_components, pca=pca, **kw)
        assert len(empty["y_pred"]) == 0 and np.isnan(empty["accuracy"]) and np.array_equal(empty["forest_nodes"], nodes)
        assert empty["proba_max"].shape == (0,)


@pytest.mark.parametrize("pca_components,pca", [(None, "host"), (12, "host"), (12, "device")])
def test_one_nn_protocol_with_the_random_forest(torch_, pca_components, pca):
    """one_nn_identification(classifier="random_forest") against the PCA, the fit and the predict called by hand; 12 components are
    padded to 16 columns by either PCA path -- on the host with zeros before the upload -- and the forest sees the 12."""
    from hse_facerec_tf_amd import identification, ops
    X, y, Xn, y2, train, test = pca_cases.golden_split()
    timings = {}
    r = identification.one_nn_identification(X, y, classifier="random_forest", forest_trees=10, forest_depth=8, timings=timings,
                                             pca_components=pca_components, pca=pca)
    assert sorted(r) == ["accuracy", "forest_nodes", "indices", "num_classes", "proba_max", "test", "train", "y", "y_pred"]
    assert np.array_equal(r["train"], train) and np.array_equal(r["test"], test)
    Xd = ops.l2_normalize(up(torch_, X))[torch_.from_numpy(np.asarray(r["indices"], dtype=np.int64)).cuda()]
    gal = Xd[torch_.from_numpy(np.asarray(train, dtype=np.int64)).cuda()].contiguous()
    qry = Xd[torch_.from_numpy(np.asarray(test, dtype=np.int64)).cuda()].contiguous()
    if pca_components and pca == "device":
        mean, components, _, _ = ops.pca_fit(gal, pca_components, max_iter=identification.PCA_MAX_ITER)
        gal = ops.pca_transform(gal, mean, components)[:, :pca_components].contiguous()
        qry = ops.pca_transform(qry, mean, components)[:, :pca_components].contiguous()
    elif pca_components:
        from sklearn.decomposition import PCA
        fitted = PCA(n_components=pca_components).fit(gal.cpu().numpy())
        gal, qry = (up(torch_, fitted.transform(t.cpu().numpy()).astype(np.float32)) for t in (gal, qry))
    assert gal.shape[1] == (pca_components or X.shape[1])
    pred, pmax, nodes = by_hand(torch_, gal, y2[train], qry, n_trees=10, max_depth=8)
    assert np.array_equal(r["y_pred"], pred) and np.array_equal(r["proba_max"], pmax) and np.array_equal(r["forest_nodes"], nodes)
    assert r["accuracy"] == float((pred == y2[test]).mean())
    assert timings["forest_fit_s"] > 0 and timings["forest_predict_s"] > 0 and "nn1_s" not in timings and "svm_fit_s" not in timings
    assert ("pca_s" in timings) == (pca_components is not None and pca == "device")


def test_fixture_accuracy_lies_in_scikit_learns_spread(torch_):
    """The default forest (100 trees, depth 10) on the fixture gallery over seeds 0..4 against the recorded accuracies of scikit-learn's
    RandomForestClassifier(100, max_depth=10, random_state=0..19): mean >= their mean - 3 of their standard deviations."""
    from hse_facerec_tf_amd import identification
    g = cases.golden()
    z, Xraw, _ = pca_cases.protocol_fixture()
    gi, pi = z["gallery"], z["probe"]
    acc = [identification.gallery_probe_identification(Xraw[gi], z["y"][gi], Xraw[pi], z["y"][pi], classifier="random_forest",
                                                       forest_seed=seed)["accuracy"] for seed in range(5)]
    theirs = g["fixture_sklearn_accuracy"]
    print("device %s mean %.4f; scikit-learn mean %.4f std %.4f over %d seeds" % (np.round(acc, 4), np.mean(acc), theirs.mean(), theirs.std(),
                                                                                 len(theirs)))
    assert len(theirs) == 20
    assert np.mean(acc) >= theirs.mean() - 3.0 * theirs.std()
