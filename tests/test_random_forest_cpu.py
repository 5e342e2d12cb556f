"""CPU suite: the random forest without a GPU -- the names libhsefr_forest.so exports and the limits its header shares with ops (what
holds for every library is in tests/test_libraries_cpu.py), every refused argument returns a status and a message before any device
work, tests/random_forest_ref.py against scikit-learn's recorded one-tree cases
(tests/golden/random_forest.npz) node for node, the restatement's own properties, and the keyword checks of the protocols."""
import ctypes
import os
import re

import numpy as np
import pytest

import random_forest_cases as cases
import random_forest_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "hsefr_forest.h")
NAMES = ["hsefr_forest_fit", "hsefr_forest_last_error_string", "hsefr_forest_predict", "hsefr_forest_version", "hsefr_forest_workspace_bytes"]


# ---- the library -----------------------------------------------------------------------------------------------------------------
def test_header_library_and_binding_agree():
    from hse_facerec_tf_amd import _lib
    assert sorted(_lib.FOREST_SIGNATURES) == NAMES
    assert "HSEFR_KNOB" not in open(os.path.join(ROOT, "hse_facerec_tf_amd", "csrc", "forest.hip")).read()
    # the limits stand once in the header and once in ops
    from hse_facerec_tf_amd import ops
    text = open(HEADER).read()
    for name, value in (("MAX_N", ops.FOREST_MAX_N), ("MAX_D", ops.FOREST_MAX_D), ("MAX_CLASSES", ops.FOREST_MAX_CLASSES),
                        ("MAX_TREES", ops.FOREST_MAX_TREES), ("MAX_DEPTH", ops.FOREST_MAX_DEPTH)):
        assert int(re.search(r"#define HSEFR_FOREST_%s (\d+)" % name, text).group(1)) == value, name
    assert "#define HSEFR_FOREST_MAX_SLAB_BYTES (1ll << 32)" in text and ops.FOREST_MAX_SLAB_BYTES == 1 << 32


def test_fit_and_predict_check_their_arguments_without_a_gpu():
    from hse_facerec_tf_amd import _lib, ops
    L = _lib.forest_lib()
    buf = ctypes.create_string_buffer(1 << 16)
    p = (ctypes.cast(buf, ctypes.c_void_p).value + 255) & ~255

    def fit(n=100, d=16, n_classes=5, n_trees=3, max_depth=4, max_features=4, bootstrap=1, seed=0, node_capacity=None, null=None, workspace=p,
            workspace_bytes=None):
        M = ops.forest_node_capacity(n, max_depth) if node_capacity is None and 1 <= max_depth <= 24 and n >= 1 else (node_capacity or 1)
        ptrs = [p] * 11
        if isinstance(null, int):
            ptrs[null] = None
        need = L.hsefr_forest_workspace_bytes(n, d, n_trees, max_depth, max_features) if workspace_bytes is None else workspace_bytes
        x, labels = (None if null == "x" else p), (None if null == "labels" else p)
        rc = L.hsefr_forest_fit(x, n, d, labels, n_classes, n_trees, max_depth, max_features, bootstrap, seed, M, *ptrs, workspace, need, None)
        return rc, _lib.forest_last_error()
    refused = [(dict(n=0), _lib.ERR_INVALID, "at least 1"), (dict(d=0, max_features=0), _lib.ERR_INVALID, "at least 1"),
               (dict(n_trees=0), _lib.ERR_INVALID, "at least 1"), (dict(max_depth=0), _lib.ERR_INVALID, "at least 1"),
               (dict(max_features=0), _lib.ERR_INVALID, "max_features = 0"), (dict(max_features=17), _lib.ERR_INVALID, "max_features = 17"),
               (dict(n_classes=1), _lib.ERR_INVALID, "n_classes = 1"), (dict(bootstrap=2), _lib.ERR_INVALID, "bootstrap = 2"),
               (dict(seed=-1), _lib.ERR_INVALID, "seed = -1"), (dict(node_capacity=30), _lib.ERR_INVALID, "node_capacity = 30"),
               (dict(null="x"), _lib.ERR_INVALID, "null pointer"), (dict(null="labels"), _lib.ERR_INVALID, "null pointer"),
               (dict(workspace=None), _lib.ERR_INVALID, "null pointer"), (dict(workspace_bytes=64), _lib.ERR_INVALID, "workspace of 64 bytes"),
               (dict(workspace=p + 8), _lib.ERR_INVALID, "16-byte aligned"),
               (dict(n=65536), _lib.ERR_UNSUPPORTED, "over the limits"), (dict(d=4097), _lib.ERR_UNSUPPORTED, "over the limits"),
               (dict(n_trees=1025), _lib.ERR_UNSUPPORTED, "over the limits"), (dict(max_depth=25), _lib.ERR_UNSUPPORTED, "over the limits"),
               (dict(n_classes=2049), _lib.ERR_UNSUPPORTED, "n_classes = 2049"),
               (dict(n=65535, d=4096, n_trees=1024, max_depth=20, max_features=4096), _lib.ERR_UNSUPPORTED, "candidates"),
               # few candidates (depth 1) but terabytes of sort space: refused by the library's own message, not by an allocation
               (dict(n=65535, d=4096, n_trees=1024, max_depth=1, max_features=4096), _lib.ERR_UNSUPPORTED, "bytes of sort space"),
               (dict(n=4097, d=4096, n_trees=1024, max_depth=1, max_features=4096), _lib.ERR_UNSUPPORTED, "bytes of sort space")]
    refused += [(dict(null=i), _lib.ERR_INVALID, "null pointer") for i in range(11)]
    for kw, status, word in refused:
        rc, msg = fit(**kw)
        assert rc == status and word in msg, (kw, rc, msg)
    assert L.hsefr_forest_workspace_bytes(0, 16, 3, 4, 4) == 0 and "at least 1" in _lib.forest_last_error()
    assert L.hsefr_forest_workspace_bytes(65536, 16, 3, 4, 4) == 0 and "over the limits" in _lib.forest_last_error()
    # LFW's gallery half lies inside the limits: 4582 x 1024, 100 trees, depth 10, sqrt(1024) features
    lfw = L.hsefr_forest_workspace_bytes(4582, 1024, 100, 10, 32)
    small = L.hsefr_forest_workspace_bytes(4096, 1024, 100, 10, 32)
    assert 0 < small < lfw and lfw - small > 100 * 32 * 2 * 4582 * 8 - (1 << 20)        # above one sort tile: the global-memory sort's slab
    with pytest.raises(ValueError, match="max_features = 17 outside 1..d = 16"):
        _lib.forest_check(fit(max_features=17)[0], "hsefr_forest_fit")
    with pytest.raises(NotImplementedError, match="over the limits"):
        _lib.forest_check(fit(n=65536)[0], "hsefr_forest_fit")

    def predict(nq=10, d=16, n_classes=5, n_trees=3, node_capacity=31, leaf_capacity=100, null=None, labels=p):
        ptrs = [p] * 9
        if isinstance(null, int):
            ptrs[null] = None
        rc = L.hsefr_forest_predict(None if null == "q" else p, nq, d, n_classes, n_trees, node_capacity, leaf_capacity, *ptrs, None, labels, None)
        return rc, _lib.forest_last_error()
    refused = [(dict(nq=0), _lib.ERR_INVALID, "at least 1"), (dict(d=0), _lib.ERR_INVALID, "at least 1"), (dict(n_trees=0), _lib.ERR_INVALID, "at least 1"),
               (dict(node_capacity=0), _lib.ERR_INVALID, "at least 1"), (dict(leaf_capacity=0), _lib.ERR_INVALID, "at least 1"),
               (dict(n_classes=1), _lib.ERR_INVALID, "n_classes = 1"), (dict(null="q"), _lib.ERR_INVALID, "null pointer"),
               (dict(labels=None), _lib.ERR_INVALID, "null pointer"), (dict(nq=(1 << 24) + 1), _lib.ERR_UNSUPPORTED, "over the limits"),
               (dict(n_classes=2049), _lib.ERR_UNSUPPORTED, "over the limits"), (dict(d=4097), _lib.ERR_UNSUPPORTED, "over the limits"),
               (dict(n_trees=1024, node_capacity=1 << 21), _lib.ERR_UNSUPPORTED, "2^31")]
    refused += [(dict(null=i), _lib.ERR_INVALID, "null pointer") for i in range(9)]
    for kw, status, word in refused:
        rc, msg = predict(**kw)
        assert rc == status and word in msg, (kw, rc, msg)


def test_ops_refuse_bad_arguments_before_the_library(monkeypatch):
    import torch
    from hse_facerec_tf_amd import _lib, ops
    monkeypatch.setattr(_lib, "forest_lib", lambda: pytest.fail("the library was reached"))
    x, labels = torch.zeros((10, 4)), torch.zeros((10,), dtype=torch.int32)
    for kw, word in ((dict(n_classes=1), "n_classes=1 must be at least 2"), (dict(n_trees=0), "n_trees=0 must be at least 1"),
                     (dict(max_depth=0), "max_depth=0 must be at least 1"), (dict(max_depth=25), "over the limits"),
                     (dict(max_features="log2"), "max_features='log2' must be 'sqrt' or an integer in 1..d"),
                     (dict(max_features=5), "max_features=5 must be 'sqrt' or an integer in 1..d=4"), (dict(max_features=0), "max_features=0"),
                     (dict(max_features=2.0), "max_features=2.0"), (dict(bootstrap=1), "bootstrap must be True or False, got 1"),
                     (dict(seed=-1), "seed=-1 must be in 0.."), (dict(seed=1.5), "seed must be an integer"), (dict(n_trees=1025), "over the limits"),
                     (dict(n_classes=2049), "over the limits")):
        with pytest.raises(ValueError, match=re.escape(word)):
            ops.random_forest_fit(x, labels, **dict(dict(n_classes=3), **kw))
    with pytest.raises(ValueError, match=r"x must be \[n, d\]"):
        ops.random_forest_fit(x[0], labels, 3)
    assert ops.check_random_forest_args(4582, 1024, 1680) == 32 and ops.check_random_forest_args(10, 3, 2) == 1
    with pytest.raises(ValueError, match="bytes of sort space, over the limit of %d" % ops.FOREST_MAX_SLAB_BYTES):
        ops.check_random_forest_args(65535, 4096, 2, n_trees=1024, max_depth=1, max_features=4096)
    assert ops.check_random_forest_args(4096, 4096, 2, n_trees=1024, max_depth=1, max_features=4096) == 4096      # one tile: no sort space
    assert ops.FOREST_SORT_TILE == cases.SORT_TILE
    assert ops.forest_node_capacity(4582, 10) == 2047 and ops.forest_node_capacity(5, 10) == 9
    with pytest.raises(ValueError, match="forest must be a RandomForest"):
        ops.random_forest_predict(None, x)
    with pytest.raises(ValueError, match="estimator must be a fitted single-output"):
        ops.random_forest_from_sklearn(object())


# ---- the restatement against scikit-learn ------------------------------------------------------------------------------------------
def node_counts(t, n_classes):
    counts = np.zeros((t["n_nodes"], n_classes), dtype=np.int64)
    for i in range(t["n_nodes"] - 1, -1, -1):                                           # children are stored after their parent
        if t["feature"][i] < 0:
            b, m = t["leaf_begin"][i], t["leaf_len"][i]
            counts[i, t["leaf_class"][b:b + m]] = t["leaf_count"][b:b + m]
        else:
            counts[i] = counts[t["left"][i]] + counts[t["right"][i]]
    return counts


@pytest.mark.parametrize("k", [0, 1, 2])
def test_the_restatement_is_scikit_learns_tree_where_that_is_a_function(k):
    """n_trees=1, bootstrap=False, max_features=d against the recorded DecisionTreeClassifier(max_depth=D, random_state=0), which the
    recorder accepted only where random_state 0..7 gave one tree: node count, every feature, every threshold (fp64 ==), every node's
    class counts -- and exactly one best candidate at every node, so that no tie hides behind an equal tree."""
    g = cases.golden()
    p = "t%d_" % k
    assert int(g["n_tree_cases"]) == 3 and [str(g["t%d_name" % i]) for i in range(3)] == ["plain", "ulp_gap", "duplicates"]
    X, y, C, D = g[p + "X"], g[p + "y"], int(g[p + "n_classes"]), int(g[p + "max_depth"])
    t = ref.fit(X, y, C, n_trees=1, max_depth=D, max_features=X.shape[1], bootstrap=False)[0]
    assert len(t["best_count"]) and t["best_count"].max() == 1
    order = ref.depth_first(t)
    assert len(order) == len(g[p + "feature"])
    counts = node_counts(t, C)
    for at, i in enumerate(order):
        leaf = g[p + "left"][at] < 0
        assert (t["feature"][i] < 0) == leaf, at
        if not leaf:
            assert t["feature"][i] == g[p + "feature"][at] and t["threshold"][i] == g[p + "threshold"][at], at
        assert np.array_equal(counts[i], g[p + "counts"][at]), at
    if str(g[p + "name"]) == "ulp_gap":
        # the case is what it claims: the root splits between two values 32 float32 ulps (6e-8 < 1e-7) apart at 0.03
        lo, hi = np.unique(X[:, 1])
        assert t["feature"][0] == 1 and 0 < float(hi) - float(lo) < 1e-7 and float(lo) < t["threshold"][0] < float(hi)
    if str(g[p + "name"]) == "duplicates":
        assert len(np.unique(X, axis=0)) <= len(X) // 2


def test_scikit_learns_splitter_compares_with_zero():
    """What FEATURE_THRESHOLD = 0.0 in the restatement rests on: the recorded node counts of DecisionTreeClassifier on two groups of
    rows 1, 32, 54 and 60 float32 ulps apart at 0.0, 0.03 and 1.0 -- a split (3 nodes) every time, also far below 1e-7."""
    assert cases.golden()["feature_threshold_splits"].tolist() == [3] * 12 and float(ref.FEATURE_THRESHOLD) == 0.0


# ---- properties of the restatement ---------------------------------------------------------------------------------------------------
def test_the_restatement_is_a_function_of_its_seed():
    X, y, C, kw, _, forest, _ = cases.case("n77")
    again = ref.fit(X, y, C, **kw)
    other = ref.fit(X, y, C, seed=1, **kw)
    keys = ("feature", "threshold", "left", "right", "weight", "leaf_begin", "leaf_len", "leaf_class", "leaf_count")
    assert all(a[k].tobytes() == b[k].tobytes() for a, b in zip(forest, again) for k in keys)
    assert any(a[k].tobytes() != b[k].tobytes() for a, b in zip(forest, other) for k in keys)
    assert len({t["feature"].tobytes() for t in forest}) == len(forest)                 # trees differ from each other
    for t in forest:
        assert int(t["weights"].sum()) == len(X) and t["weight"][0] == len(X)           # multiplicities sum to n
        assert 0 < (t["weights"] == 0).sum() < len(X)
    for name in ("no_bootstrap", "tile_edge"):
        assert all((t["weights"] == 1).all() for t in cases.case(name)[5])


def test_the_hash_is_splitmix64s_finaliser():
    # splitmix64 from state 0: its first output is mix(0 + G)
    assert int(ref._mix(np.asarray([0], dtype=np.uint64) + ref.G)[0]) == 0xE220A8397B1DCDAF
    h = ref.forest_hash(3, 1, 2, 5, np.arange(4))
    assert h.dtype == np.uint64 and len(set(h.tolist())) == 4
    order = ref.feature_order(20, 0, 1, 0)
    assert sorted(order.tolist()) == list(range(20)) and not np.array_equal(order, ref.feature_order(20, 0, 2, 0))


def test_one_class_gives_root_leaves_and_depth_is_respected():
    rs = np.random.RandomState(0)
    X = rs.rand(50, 6).astype(np.float32)
    for t in ref.fit(X, np.full(50, 2), 4, n_trees=3, max_depth=5):
        assert t["n_nodes"] == 1 and t["feature"][0] == -1 and t["leaf_len"][0] == 1 and t["leaf_class"][0] == 2 and t["leaf_count"][0] == 50
    y = rs.randint(0, 4, 50)
    for depth in (1, 2, 3):
        for t in ref.fit(X, y, 4, n_trees=3, max_depth=depth):
            assert t["deepest"] <= depth and t["n_nodes"] <= 2 ** (depth + 1) - 1
    assert all(t["deepest"] == 1 and t["n_nodes"] == 3 for t in cases.case("stump")[5])


def test_an_unbounded_tree_without_bootstrap_knows_its_training_rows():
    rs = np.random.RandomState(1)
    X = rs.rand(120, 5).astype(np.float32)
    y = rs.randint(0, 3, 120)
    forest = ref.fit(X, y, 3, n_trees=2, max_depth=24, max_features=5, bootstrap=False)
    for t in forest:
        assert np.array_equal(ref.predict([t], X, 3), y)
    proba = ref.predict_proba(forest, X, 3)
    assert np.array_equal(proba.max(axis=1), np.ones(120)) and np.array_equal(proba.sum(axis=1), np.ones(120))


def test_the_cases_reach_the_paths_they_are_there_for():
    assert min(t["continued"] for t in cases.case("duplicates")[5]) > 0
    assert int((cases.case("tile_edge")[5][0]["weights"] > 0).sum()) == cases.SORT_TILE + 1
    assert all(int((t["weights"] > 0).sum()) > cases.SORT_TILE and t["weights"].max() > 1 for t in cases.case("large_bootstrap")[5])
    stump = cases.case("large_leaves")[5][0]
    assert stump["n_nodes"] == 3 and max(int(stump["weight"][1]), int(stump["weight"][2])) > cases.SORT_TILE      # a leaf above one tile
    wide = cases.case("large_constant")[5][0]
    assert wide["weight"][0] > cases.SORT_TILE and wide["continued"] >= 1 and wide["feature"][0] >= 0            # a long visit above one tile
    X, y = cases.case("lonely_and_empty")[:2]
    assert (y == 4).sum() == 1 and (y == 2).sum() == 0
    assert np.diff(np.unique(cases.case("close_values")[0])).max() < 1e-7
    assert ref.resolve_max_features("sqrt", 3) == 1 and ref.resolve_max_features("sqrt", 1024) == 32
    assert "#define HSEFR_FOREST_MAX_N" in open(HEADER).read() and ("constexpr int TILE = %d;" % cases.SORT_TILE) in open(
        os.path.join(ROOT, "hse_facerec_tf_amd", "csrc", "forest.hip")).read()


# ---- the protocols' keywords -----------------------------------------------------------------------------------------------------------
def test_protocol_keywords_are_checked_before_the_library(monkeypatch):
    from hse_facerec_tf_amd import _lib, identification
    monkeypatch.setattr(_lib, "require_gpu", lambda: pytest.fail("a device was asked for"))
    monkeypatch.setattr(_lib, "forest_lib", lambda: pytest.fail("the library was reached"))
    X, y = np.zeros((8, 8), dtype=np.float32), np.arange(8) // 2

    def runs(**kw):
        return (lambda: identification.one_nn_identification(X, y, **kw)), (lambda: identification.gallery_probe_identification(X, y, X, y, **kw))
    for kw, word in ((dict(n_neighbors=3), "n_neighbors=3 has no meaning with classifier='random_forest': leave it at 1"),
                     (dict(metric="chi2"), "metric='chi2' is a k-NN distance: it has no meaning with classifier='random_forest'"),
                     (dict(metric="kl"), "metric='kl' is a k-NN distance"), (dict(forest_trees=0), "forest_trees=0 must be at least 1"),
                     (dict(forest_trees=1025), "over the limits"), (dict(forest_depth=0), "forest_depth=0 must be at least 1"),
                     (dict(forest_depth=25), "over the limits"), (dict(forest_seed=-1), "forest_seed=-1 must be at least 0"),
                     (dict(forest_trees=2.5), "forest_trees must be an integer"), (dict(pca="gpu"), "pca='gpu' must be")):
        for run in runs(classifier="random_forest", **kw):
            with pytest.raises(ValueError, match=re.escape(word)):
                run()
    for run in runs(classifier="forest"):                                               # still no name of a classifier
        with pytest.raises(ValueError, match=re.escape("classifier='forest' must be 'knn' (ops.nn1 / ops.knn), 'linear_svm' (ops.linear_svm_fit) "
                                                       "or 'rbf_svm' (ops.rbf_svm_fit)")):
            run()
    kw = identification._check_keywords(classifier="random_forest", forest_trees=7, forest_depth=3, forest_seed=11, pca_components=16, pca="device")
    assert (kw.classifier, kw.forest_trees, kw.forest_depth, kw.forest_seed, kw.pca_components) == ("random_forest", 7, 3, 11, 16)
    assert identification._check_keywords()[-3:] == (100, 10, 0)
    assert "random_forest" in identification.__doc__ and "forest_trees" in identification.__doc__
