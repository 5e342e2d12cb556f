"""The random forest of ops.random_forest_fit, restated in NumPy: integers and fp64 only, nothing shared with the package.  The forest is
a pure function of (X, y, n_trees, max_depth, max_features, bootstrap, seed); libhsefr_forest.so (include/hsefr_forest.h) equals it bit
for bit -- every node's feature, fp64 threshold, children, weight and leaf list, every probability and label.

The definition (scikit-learn 1.7.2's RandomForestClassifier(criterion="gini") with its sequential generator replaced by a hash):

hash      mix(z) is splitmix64's finaliser: z ^= z >> 30; z *= 0xBF58476D1CE4E5B9; z ^= z >> 27; z *= 0x94D049BB133111EB; z ^= z >> 31.
          hash(seed, tree, purpose, node, counter): h = mix(seed + G); then for v in (tree, purpose, node, counter): h = mix(h + v + G),
          G = 0x9E3779B97F4A7C15, all in uint64 with wrap-around.  purpose 1 = bootstrap, 2 = feature order.
bootstrap row j of tree t is ((hash(seed, t, 1, 0, j) >> 32) * n) >> 32; a row's multiplicity is its integer weight, rows with
          multiplicity 0 are not in the tree; without bootstrap every row has weight 1.
nodes     are numbered as a heap (root 1, children 2 i and 2 i + 1) for the hash, and STORED level by level: the root is node 0, and the
          children of a level's split nodes follow in that level's order, left before right.  A tree's rows stay partitioned: a node holds
          the segment [start, start + len) of the tree's distinct rows (ascending row index at the root), and a split moves the rows
          with (double) x <= threshold to the front of the segment, both halves keeping their order.
features  of a node are visited by ascending ((hash(seed, tree, 2, node, f) >> 12 << 12) | f): the hash's upper 52 bits, then f (d is
          at most 4096).  The first max_features are all visited; while no candidate has been seen the visit goes on, feature by
          feature, until one yields a candidate or all d are exhausted.
split     a feature's rows sorted by value; position p (1 <= p < len) is a candidate iff v[p] > v[p-1] + FEATURE_THRESHOLD in fp32, and
          FEATURE_THRESHOLD is 0.0: scikit-learn 1.7.2 declares it as 1e-7, but the splitter it ships compares with 0 -- two float32
          values one ulp apart are split at 0.0 (denormals), at 0.03 and at 1.0 (tools/record_random_forest_golden.py measures it and
          the one-tree case 'ulp_gap' pins it) -- so every pair of distinct values is a candidate.  This is the behaviour of the
          installed 1.7.2 build; should a later scikit-learn restore the 1e-7, the recorder stops reproducing the golden file's
          'feature_threshold_splits' and 'ulp_gap', and that is the reason.  Its score is S_L / N_L + S_R / N_R
          in fp64 (S: the sum of squared weighted class counts, N: the weighted count, both integers); the largest wins, equal scores go
          to the earlier feature of the visit, then the lower position.  threshold = lo / 2.0 + hi / 2.0 in fp64 (lo = v[p-1], hi = v[p]); lo if that equals hi
          or is not finite.
leaves    at max_depth, with fewer than 2 distinct rows, with one class only, or without a candidate.  A leaf keeps (class, weighted
          count) pairs by ascending class at [leaf_begin, leaf_begin + leaf_len) of the tree's list; leaf_begin is its segment's start
          (both are -1 at a split node).
predict   proba[c] = (sum_t count_t[c] / N_t) / n_trees in fp64, the terms added in tree order from 0.0; the label is the largest,
          equal values to the lowest class.
"""
import numpy as np

G = np.uint64(0x9E3779B97F4A7C15)
PURPOSE_BOOTSTRAP, PURPOSE_FEATURE = 1, 2
FEATURE_THRESHOLD = np.float32(0.0)     # what scikit-learn 1.7.2's splitter adds (see above), not the 1e-7 its source names


def _mix(z):
    z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
    z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    return z ^ (z >> np.uint64(31))


def forest_hash(seed, tree, purpose, node, counter):
    """uint64 array over ``counter`` (an integer array); the other arguments are scalars."""
    counter = np.atleast_1d(np.asarray(counter)).astype(np.uint64)
    h = _mix(np.full(counter.shape, seed, dtype=np.uint64) + G)
    for v in (tree, purpose, node):
        h = _mix(h + np.uint64(v) + G)
    return _mix(h + counter + G)


def bootstrap_weights(n, tree, seed, bootstrap=True):
    if not bootstrap:
        return np.ones(n, dtype=np.int64)
    u = forest_hash(seed, tree, PURPOSE_BOOTSTRAP, 0, np.arange(n)) >> np.uint64(32)
    rows = ((u * np.uint64(n)) >> np.uint64(32)).astype(np.int64)
    return np.bincount(rows, minlength=n).astype(np.int64)


def feature_order(d, tree, node_heap, seed):
    key = forest_hash(seed, tree, PURPOSE_FEATURE, node_heap, np.arange(d))
    assert d <= 4096
    return np.argsort(((key >> np.uint64(12)) << np.uint64(12)) | np.arange(d, dtype=np.uint64), kind="stable")


def resolve_max_features(max_features, d):
    if max_features == "sqrt":
        return max(1, int(np.sqrt(d)))
    assert 1 <= int(max_features) <= d
    return int(max_features)


def _scan_feature(v, c, w):
    """Candidates of one feature over a node's rows (values float32, classes, integer weights): (scores fp64, positions, sorted values)."""
    order = np.argsort(v, kind="stable")
    vs, cs, ws = v[order], c[order], w[order]
    with np.errstate(over="ignore"):
        pos = 1 + np.nonzero(vs[1:] > vs[:-1] + FEATURE_THRESHOLD)[0]              # float32 + float32: an fp32 sum
    if len(pos) == 0:
        return np.zeros(0), pos, vs
    _, inv = np.unique(cs, return_inverse=True)
    onehot = np.zeros((len(vs), inv.max() + 1), dtype=np.int64)
    onehot[np.arange(len(vs)), inv] = ws
    left = np.cumsum(onehot, axis=0)[pos - 1]                                       # counts of the rows at positions < p
    right = onehot.sum(axis=0)[None, :] - left
    s_l, s_r = (left * left).sum(axis=1), (right * right).sum(axis=1)
    n_l, n_r = left.sum(axis=1), right.sum(axis=1)
    return s_l.astype(np.float64) / n_l.astype(np.float64) + s_r.astype(np.float64) / n_r.astype(np.float64), pos, vs


def _threshold(lo, hi):
    with np.errstate(over="ignore", invalid="ignore"):
        t = np.float64(lo) / 2.0 + np.float64(hi) / 2.0
    return np.float64(lo) if (t == np.float64(hi) or not np.isfinite(t)) else t


def fit_tree(X, y, tree, max_depth, mf, bootstrap, seed):
    n, d = X.shape
    w = bootstrap_weights(n, tree, seed, bootstrap)
    rows = np.nonzero(w > 0)[0]
    feature, threshold, left, right, weight, leaf_begin, leaf_len, heap, start, length = ([] for _ in range(10))
    leaf_class, leaf_count = np.full(n, -1, dtype=np.int32), np.zeros(n, dtype=np.int32)
    best_count = []                                                                 # per split node: how many candidates had the best score
    continued = 0                                                                   # nodes whose visit went past max_features

    def new_node(s, m, h):
        feature.append(-1), threshold.append(0.0), left.append(-1), right.append(-1), weight.append(0)
        leaf_begin.append(-1), leaf_len.append(-1), heap.append(h), start.append(s), length.append(m)
        return len(feature) - 1
    level, deepest = [new_node(0, len(rows), 1)], 0
    for depth in range(max_depth + 1):
        for i in level:
            s, m = start[i], length[i]
            r = rows[s:s + m]
            c, ww = y[r], w[r]
            weight[i] = int(ww.sum())
            best = None
            if depth < max_depth and m >= 2 and len(np.unique(c)) > 1:
                visited, ties = 0, 0
                for f in feature_order(d, tree, heap[i], seed):
                    if visited >= mf and best is not None:
                        break
                    visited += 1
                    continued += visited == mf + 1
                    score, pos, vs = _scan_feature(X[r, f], c, ww)
                    if len(pos) == 0:
                        continue
                    k = int(np.argmax(score))                                        # the first of equal scores: the lower position
                    if best is None or score[k] > best[0]:
                        best, ties = (score[k], int(f), int(pos[k]), _threshold(vs[pos[k] - 1], vs[pos[k]])), int((score == score[k]).sum())
                    elif score[k] == best[0]:
                        ties += int((score == score[k]).sum())
            if best is None:
                cls, inv = np.unique(c, return_inverse=True)
                cnt = np.bincount(inv, weights=ww).astype(np.int64) if m else np.zeros(0, dtype=np.int64)
                leaf_begin[i], leaf_len[i] = s, len(cls)
                leaf_class[s:s + len(cls)], leaf_count[s:s + len(cls)] = cls, cnt
                continue
            _, f, p, thr = best
            feature[i], threshold[i] = f, thr
            best_count.append(ties)
            go_left = X[r, f].astype(np.float64) <= thr
            assert int(go_left.sum()) == p
            rows[s:s + m] = np.concatenate([r[go_left], r[~go_left]])
            left[i], right[i] = new_node(s, p, 2 * heap[i]), new_node(s + p, m - p, 2 * heap[i] + 1)
            deepest = depth + 1
        level = [j for i in level if feature[i] >= 0 for j in (left[i], right[i])]
    return {"feature": np.asarray(feature, dtype=np.int32), "threshold": np.asarray(threshold, dtype=np.float64),
            "left": np.asarray(left, dtype=np.int32), "right": np.asarray(right, dtype=np.int32),
            "weight": np.asarray(weight, dtype=np.int32), "leaf_begin": np.asarray(leaf_begin, dtype=np.int32),
            "leaf_len": np.asarray(leaf_len, dtype=np.int32), "leaf_class": leaf_class, "leaf_count": leaf_count,
            "n_nodes": len(feature), "best_count": np.asarray(best_count, dtype=np.int64), "deepest": deepest, "weights": w, "continued": int(continued)}


def fit(X, y, n_classes, n_trees=100, max_depth=10, max_features="sqrt", bootstrap=True, seed=0):
    """-> a list of trees (dicts of the node arrays in storage order, the leaf lists, and for the tests 'best_count' / 'weights')."""
    X = np.ascontiguousarray(X, dtype=np.float32)
    y = np.asarray(y).astype(np.int64)
    assert X.ndim == 2 and y.shape == (X.shape[0],) and y.min() >= 0 and y.max() < n_classes
    mf = resolve_max_features(max_features, X.shape[1])
    return [fit_tree(X, y, t, max_depth, mf, bootstrap, seed) for t in range(n_trees)]


def predict_proba(forest, Q, n_classes):
    Q = np.ascontiguousarray(Q, dtype=np.float32)
    out = np.zeros((Q.shape[0], n_classes), dtype=np.float64)
    for q in range(Q.shape[0]):
        acc = np.zeros(n_classes, dtype=np.float64)
        for t in forest:
            i = 0
            while t["feature"][i] >= 0:
                i = t["left"][i] if np.float64(Q[q, t["feature"][i]]) <= t["threshold"][i] else t["right"][i]
            b, m = t["leaf_begin"][i], t["leaf_len"][i]
            acc[t["leaf_class"][b:b + m]] += t["leaf_count"][b:b + m].astype(np.float64) / np.float64(t["weight"][i])
        out[q] = acc / np.float64(len(forest))
    return out


def predict(forest, Q, n_classes):
    return np.argmax(predict_proba(forest, Q, n_classes), axis=1).astype(np.int32)


def depth_first(tree):
    """The tree's node indices in scikit-learn's order: parent, left subtree, right subtree."""
    out, stack = [], [0]
    while stack:
        i = stack.pop()
        out.append(i)
        if tree["feature"][i] >= 0:
            stack.extend((int(tree["right"][i]), int(tree["left"][i])))
    return out
