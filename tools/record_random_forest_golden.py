#!/usr/bin/env python3
"""Records tests/golden/random_forest.npz (CPU only, scikit-learn 1.7.2):

one-tree cases  t<k>_*: inputs on which DecisionTreeClassifier(max_depth=D) is a function of its inputs -- the same tree for random_state
                0..7 -- and on which tests/random_forest_ref.py (n_trees=1, bootstrap=False, max_features=d) reports exactly one best
                candidate at every node; the recorder draws seeds until both hold, and asserts that the two trees are then equal node
                for node.  X, y, n_classes, max_depth and scikit-learn's tree (feature, threshold, children, class counts per node).
                'plain' 300 x 24; 'ulp_gap': the best split lies between two values 32 float32 ulps (6e-8) apart at 0.03, which a
                FEATURE_THRESHOLD of 1e-7 would skip; 'duplicates': every row twice or more, some with conflicting labels.
threshold       feature_threshold_splits: DecisionTreeClassifier's node count on two groups of rows k float32 ulps apart, for k in
                (1, 32, 54, 60) at 0.0, 0.03 and 1.0 -- 3 everywhere: scikit-learn 1.7.2's splitter compares with 0, not with 1e-7.
forests         sk<k>_*: fitted RandomForestClassifier / DecisionTreeClassifier objects as ops.random_forest_from_sklearn reads them
                (per tree: node_count, children, feature, threshold, value, weighted_n_node_samples, concatenated), probes and
                scikit-learn's predict_proba of them.  Few classes, deep trees, labels that follow the features: at most 5 % of the probes
                have their two largest probabilities within 1e-12 (asserted here).
fixture         fixture_sklearn_accuracy: the accuracy of RandomForestClassifier(100, max_depth=10, random_state=s), s = 0..19, on the
                gallery / probe fixture of tests/golden/protocols.npz.
usage: python tools/record_random_forest_golden.py [--out FILE]"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np


def plain(rs):
    return rs.randn(300, 24).astype(np.float32), rs.randint(0, 3, 300), 3, 4


def ulp_gap(rs):
    X = rs.randn(60, 3).astype(np.float32)
    y = (np.arange(60) >= 25).astype(np.int64)
    lo = np.float32(0.03)
    hi = lo
    for _ in range(32):
        hi = np.nextafter(hi, np.float32(1.0))
    X[:, 1] = np.where(y == 0, lo, hi)
    flip = rs.permutation(60)[:4]                       # a few labels that the rest of the tree has to find in the other columns
    y[flip] = 1 - y[flip]
    return X, y, 2, 3


def duplicates(rs):
    proto = rs.randn(120, 6).astype(np.float32)
    rows = np.concatenate([np.arange(120), np.arange(120), rs.randint(0, 120, 60)])
    y = (proto[rows, 0] > 0).astype(np.int64) + (proto[rows, 1] > 0.5)
    y[-12:] = (y[-12:] + 1) % 3                         # conflicting labels on identical rows
    return proto[rows], y, 3, 3


def sklearn_counts(tree):
    return np.rint(tree.value[:, 0, :] * tree.weighted_n_node_samples[:, None]).astype(np.int64)


def node_counts(t, n_classes):
    """Class counts of every node of a restated tree, from its leaves up."""
    counts = np.zeros((t["n_nodes"], n_classes), dtype=np.int64)
    for i in range(t["n_nodes"] - 1, -1, -1):
        if t["feature"][i] < 0:
            b, m = t["leaf_begin"][i], t["leaf_len"][i]
            counts[i, t["leaf_class"][b:b + m]] = t["leaf_count"][b:b + m]
        else:
            counts[i] = counts[t["left"][i]] + counts[t["right"][i]]
    return counts


def same_tree(t, sk, n_classes):
    import random_forest_ref as ref
    order = ref.depth_first(t)
    if len(order) != sk.node_count:
        return False
    counts = node_counts(t, n_classes)
    for k, i in enumerate(order):
        if (t["feature"][i] < 0) != (sk.children_left[k] < 0):
            return False
        if t["feature"][i] >= 0 and (t["feature"][i] != sk.feature[k] or t["threshold"][i] != sk.threshold[k]):
            return False
        if not np.array_equal(counts[i], sklearn_counts(sk)[k]):
            return False
    return True


def one_tree_cases(out):
    from sklearn.tree import DecisionTreeClassifier
    import random_forest_ref as ref
    for k, make in enumerate((plain, ulp_gap, duplicates)):
        for seed in range(200):
            X, y, C, D = make(np.random.RandomState(seed))
            trees = [DecisionTreeClassifier(max_depth=D, random_state=s).fit(X, y).tree_ for s in range(8)]
            if not all(np.array_equal(t.feature, trees[0].feature) and np.array_equal(t.threshold, trees[0].threshold) for t in trees):
                continue
            mine = ref.fit(X, y, C, n_trees=1, max_depth=D, max_features=X.shape[1], bootstrap=False)[0]
            if len(mine["best_count"]) and mine["best_count"].max() > 1:
                continue
            assert same_tree(mine, trees[0], C), (make.__name__, seed)
            sk = trees[0]
            p = "t%d_" % k
            out[p + "name"], out[p + "X"], out[p + "y"], out[p + "n_classes"], out[p + "max_depth"] = make.__name__, X, y.astype(np.int32), C, D
            out[p + "feature"], out[p + "threshold"] = sk.feature.astype(np.int32), sk.threshold
            out[p + "left"], out[p + "right"] = sk.children_left.astype(np.int32), sk.children_right.astype(np.int32)
            out[p + "counts"] = sklearn_counts(sk).astype(np.int32)
            print("%s: seed %d, %d nodes" % (make.__name__, seed, sk.node_count))
            break
        else:
            raise SystemExit("no seed gives a seed-invariant, tie-free %s case" % make.__name__)
    out["n_tree_cases"] = 3


def feature_threshold(out):
    from sklearn.tree import DecisionTreeClassifier
    y = (np.arange(40) >= 20).astype(int)
    nodes = []
    for base in (0.0, 0.03, 1.0):
        for k in (1, 32, 54, 60):
            a = b = np.float32(base)
            for _ in range(k):
                b = np.nextafter(b, np.float32(2))
            X = np.full((40, 1), a, np.float32)
            X[20:, 0] = b
            nodes.append(DecisionTreeClassifier(max_depth=2).fit(X, y).tree_.node_count)
    print("node counts over gaps of 1, 32, 54, 60 ulps at 0, 0.03, 1:", nodes)
    out["feature_threshold_splits"] = np.asarray(nodes, dtype=np.int32)


def forests(out):
    from sklearn.ensemble import RandomForestClassifier
    from sklearn.tree import DecisionTreeClassifier
    rs = np.random.RandomState(7)

    def data(n, d, C):
        X = rs.randn(n, d).astype(np.float32)
        centre = rs.randn(C, d) * 1.5
        y = rs.randint(0, C, n)
        return (X + centre[y]).astype(np.float32), y
    specs = [(RandomForestClassifier(n_estimators=100, random_state=0), data(150, 8, 3)),
             (RandomForestClassifier(n_estimators=10, max_depth=10, random_state=1), data(400, 12, 4)),
             (DecisionTreeClassifier(random_state=2), data(200, 5, 3))]
    for k, (est, (X, y)) in enumerate(specs):
        est.fit(X, y)
        probes = (X[: len(X) // 2] + rs.randn(len(X) // 2, X.shape[1]).astype(np.float32) * np.float32(0.7)).astype(np.float32)
        proba = est.predict_proba(probes)
        top2 = np.sort(proba, axis=1)[:, -2:]
        share = float((top2[:, 1] - top2[:, 0] <= 1e-12).mean())
        assert share <= 0.05, (k, share)
        trees = [est] if isinstance(est, DecisionTreeClassifier) else est.estimators_
        p = "sk%d_" % k
        out[p + "is_tree"] = isinstance(est, DecisionTreeClassifier)
        out[p + "node_count"] = np.asarray([t.tree_.node_count for t in trees], dtype=np.int32)
        out[p + "left"] = np.concatenate([t.tree_.children_left for t in trees]).astype(np.int32)
        out[p + "right"] = np.concatenate([t.tree_.children_right for t in trees]).astype(np.int32)
        out[p + "feature"] = np.concatenate([t.tree_.feature for t in trees]).astype(np.int32)
        out[p + "threshold"] = np.concatenate([t.tree_.threshold for t in trees])
        out[p + "value"] = np.concatenate([t.tree_.value[:, 0, :] for t in trees])
        out[p + "weighted_n"] = np.concatenate([t.tree_.weighted_n_node_samples for t in trees])
        out[p + "probes"], out[p + "proba"] = probes, proba
        print("sk%d: %d trees, %d nodes, %.1f %% of %d probes tied" % (k, len(trees), out[p + "node_count"].sum(), 100 * share, len(probes)))


def fixture(out):
    from sklearn.ensemble import RandomForestClassifier
    import pca_cases
    z, Xraw, _ = pca_cases.protocol_fixture()
    gi, pi = z["gallery"], z["probe"]
    acc = [float((RandomForestClassifier(n_estimators=100, max_depth=10, random_state=s).fit(Xraw[gi], z["y"][gi]).predict(Xraw[pi])
                  == z["y"][pi]).mean()) for s in range(20)]
    out["fixture_sklearn_accuracy"] = np.asarray(acc)
    print("fixture: gallery %s, %d probes, scikit-learn accuracy mean %.4f std %.4f min %.4f max %.4f"
          % (Xraw[gi].shape, len(pi), np.mean(acc), np.std(acc), np.min(acc), np.max(acc)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "random_forest.npz"))
    args = ap.parse_args()
    import sklearn
    out = {"sklearn_version": sklearn.__version__}
    one_tree_cases(out)
    feature_threshold(out)
    forests(out)
    fixture(out)
    np.savez_compressed(args.out, **out)
    print("wrote %s (%d bytes)" % (args.out, os.path.getsize(args.out)))


if __name__ == "__main__":
    main()
