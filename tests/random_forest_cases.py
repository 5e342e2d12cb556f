"""Inputs shared by the random forest suites (tests/test_random_forest_cpu.py, tests/test_random_forest_gpu.py): the small shapes that
reach every path of csrc/forest.hip, each with its restatement (tests/random_forest_ref.py) fitted once and kept, and the recorded
tests/golden/random_forest.npz (tools/record_random_forest_golden.py)."""
import functools
import os
import types

import numpy as np

import random_forest_ref as ref

from conftest import GOLDEN

SORT_TILE = 4096        # csrc/forest.hip's TILE: a node of more rows is sorted in global memory


def _continuous(rs, n, d):
    return rs.rand(n, d).astype(np.float32)


def _duplicated(rs, n, d):
    """Rows drawn from 12 prototypes whose columns hold 0 / 1 / 2, two thirds of the columns constant: nodes of identical rows, and
    nodes whose first max_features features are constant, so that the visit goes on past them."""
    proto = rs.randint(0, 3, (12, d)).astype(np.float32)
    proto[:, rs.permutation(d)[: 2 * d // 3]] = 1.0
    return proto[rs.randint(0, 12, n)]


def _close(rs, n, d):
    """Values a few float32 ulps apart around 0.03 (ulp 1.9e-9: all of them within 1e-7 of a neighbour), with repeats."""
    steps = rs.randint(0, 40, (n, d))
    return (np.float32(0.03) + steps.astype(np.float32) * np.float32(2.0 ** -29)).astype(np.float32)


def _leading_constant(rs, n, d):
    """Every column constant but the one that tree 0's root (heap node 1, seed 0) visits LAST: with max_features = 1 the root finds no
    candidate among its first features and goes on visiting, feature by feature, to the end of the order."""
    X = np.full((n, d), 0.25, dtype=np.float32)
    X[:, ref.feature_order(d, 0, 1, 0)[-1]] = rs.rand(n).astype(np.float32)
    return X


# name: (n, d, n_classes, kwargs of fit, data, labels) -- what each is there for stands in its name and beside it
CASES = {
    "n77": (77, 20, 5, dict(n_trees=3, max_depth=6), _continuous, None),                         # n no multiple of 64
    "tile_edge": (SORT_TILE + 1, 3, 3, dict(n_trees=1, max_depth=2, max_features=3, bootstrap=False), _continuous, None),
    # ^ the smallest root that takes the global-memory sort; max_features = d
    "large_bootstrap": (6700, 4, 4, dict(n_trees=2, max_depth=3, max_features=2), _continuous, None),
    # ^ about 0.632 n = 4235 distinct rows at the root: the large path with weights above 1, and its children on the tile path
    "large_leaves": (9000, 3, 5, dict(n_trees=1, max_depth=1, max_features=3, bootstrap=False), _continuous, None),
    # ^ a stump over 9000 rows: at least one of its two leaves holds more than one sort tile, so its class list is sorted in global memory
    "large_constant": (SORT_TILE + 204, 6, 3, dict(n_trees=1, max_depth=2, max_features=1, bootstrap=False), _leading_constant, None),
    # ^ a root above one sort tile whose visit goes past max_features: the search in global memory from the choosing kernel
    "d3": (100, 3, 4, dict(n_trees=4, max_depth=5), _continuous, None),                          # d < 8: sqrt gives 1 feature
    "all_features": (120, 7, 3, dict(n_trees=2, max_depth=10, max_features=7), _continuous, None),
    "duplicates": (90, 12, 3, dict(n_trees=4, max_depth=6), _duplicated, None),
    "close_values": (90, 6, 3, dict(n_trees=3, max_depth=8), _close, None),
    "lonely_and_empty": (80, 9, 6, dict(n_trees=3, max_depth=6), _continuous, "lonely"),          # class 4: one row, class 2: none
    "stump": (130, 9, 2, dict(n_trees=1, max_depth=1), _continuous, None),                       # n_trees = 1, max_depth = 1, 2 classes
    "classes300": (700, 16, 300, dict(n_trees=2, max_depth=8), _continuous, None),
    "no_bootstrap": (150, 10, 4, dict(n_trees=3, max_depth=10, bootstrap=False), _continuous, None),
}


@functools.lru_cache(maxsize=None)
def case(name):
    """(X, y, n_classes, kwargs, probes, restatement's forest, its probabilities): computed once, shared, never changed."""
    n, d, C, kw, data, labels = CASES[name]
    rs = np.random.RandomState(sum(map(ord, name)))
    X = data(rs, n, d)
    y = rs.randint(0, C, n).astype(np.int32)
    # a third of the labels follow the first column, so that trees have something to find
    lead = X[:, int(np.argmax(X.std(axis=0) > 0))]           # the first column that varies (the first of all, but for 'large_constant')
    y = np.where(rs.rand(n) < 0.33, np.minimum((np.argsort(np.argsort(lead)) * C // n), C - 1), y).astype(np.int32)
    if labels == "lonely":
        y[(y == 2) | (y == 4)] = 0
        y[7] = 4
        assert (y == 4).sum() == 1 and (y == 2).sum() == 0
    probes = np.concatenate([X[:: max(1, n // 40)], data(rs, 24, d)]).astype(np.float32)
    forest = ref.fit(X, y, C, **kw)
    return X, y, C, kw, probes, forest, ref.predict_proba(forest, probes, C)


@functools.lru_cache(maxsize=None)
def golden():
    return np.load(os.path.join(GOLDEN, "random_forest.npz"))


def recorded_estimator(g, prefix):
    """The stand-in for a fitted scikit-learn estimator that ops.random_forest_from_sklearn reads: the recorded attributes of its trees."""
    counts = g[prefix + "node_count"]
    at = np.concatenate([[0], np.cumsum(counts)])
    trees = []
    for i in range(len(counts)):
        s = slice(at[i], at[i + 1])
        tree = types.SimpleNamespace(node_count=int(counts[i]), children_left=g[prefix + "left"][s].astype(np.int64),
                                     children_right=g[prefix + "right"][s].astype(np.int64), feature=g[prefix + "feature"][s].astype(np.int64),
                                     threshold=g[prefix + "threshold"][s], value=g[prefix + "value"][s][:, None, :],
                                     weighted_n_node_samples=g[prefix + "weighted_n"][s])
        trees.append(types.SimpleNamespace(tree_=tree))
    shared = dict(n_classes_=int(g[prefix + "value"].shape[1]), n_features_in_=int(g[prefix + "probes"].shape[1]), n_outputs_=1)
    if bool(g[prefix + "is_tree"]):
        return types.SimpleNamespace(tree_=trees[0].tree_, **shared)
    return types.SimpleNamespace(estimators_=trees, **shared)
