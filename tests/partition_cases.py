"""Seeded cases for hsefr_partition_scores: name -> (y_true int32 [n], labels int32 [rows][n]).  Sizes around the wave (63, 64, 65),
past one 1024-thread chunk (1000 is below it, 4099 takes five and pads to 8192 keys), the smallest (1, 2, 3) and a middle one (257);
1, 2 and 71 rows.  The exact values of the six sums (mpmath, tools/record_partition_scores_golden.py) are in
tests/golden/partition_scores_exact.npz under the same names."""
import numpy as np

SIZES = (1, 2, 3, 63, 64, 65, 257, 1000, 4099)
INT_MAX = 2 ** 31 - 1


def _zipf_classes(rs, n):
    """class of each item: sizes fall off like 1 / rank, about n / 6 classes"""
    k = max(1, n // 6)
    w = 1.0 / np.arange(1, k + 1)
    return rs.choice(k, size=n, p=w / w.sum()).astype(np.int32)


def _noisy(rs, y, noise, spread):
    """clusters that follow the classes, split in ``spread`` parts, with a share ``noise`` of the items moved to a random cluster"""
    n = len(y)
    lab = y.astype(np.int64) * spread + rs.randint(0, spread, n)
    move = rs.rand(n) < noise
    lab[move] = rs.randint(0, max(1, int(lab.max()) + 1), int(move.sum()))
    return lab.astype(np.int32)


def _random(seed, n, rows):
    rs = np.random.RandomState(seed)
    y = _zipf_classes(rs, n)
    labels = np.stack([_noisy(rs, y, 0.02 + 0.9 * r / max(rows, 2), 1 + r % 3) for r in range(rows)])
    if rows >= 41:
        labels[40] = labels[5]                                  # a duplicate row
    return y, labels


def _negatives(seed, n):
    rs = np.random.RandomState(seed)
    y = _zipf_classes(rs, n)
    first = _noisy(rs, y, 0.1, 1)
    first[rs.rand(n) < 0.3] = -1                                # DBSCAN's noise
    second = -1 - rs.randint(0, 5, n).astype(np.int32)          # nothing but negative labels, repeated values included
    return y, np.stack([first, second])


def _sparse(seed, n):
    rs = np.random.RandomState(seed)
    values = np.array([INT_MAX, INT_MAX - 1, 0, 1, 2 ** 30, 2 ** 16, 65535, 123456789, 2 ** 31 - 1000], dtype=np.int64)
    lab = values[rs.randint(0, len(values), n)].astype(np.int32)
    tvals = np.array([-2 ** 31, -1, 0, INT_MAX, 7, 2 ** 24], dtype=np.int64)
    return tvals[rs.randint(0, len(tvals), n)].astype(np.int32), lab[None]


def _renamed(seed, n):
    rs = np.random.RandomState(seed)
    y = _zipf_classes(rs, n)
    return y, ((int(y.max()) - y) * 1000 + 17).astype(np.int32)[None]


def build():
    cases = {}
    for n in SIZES:
        cases["random_n%d" % n] = _random(100 + n, n, 2)
    cases["random_n257_rows71"] = _random(7, 257, 71)
    cases["random_n4099_rows71"] = _random(8, 4099, 71)
    for n in (3, 65, 1000):
        cases["renamed_n%d" % n] = _renamed(200 + n, n)
    for n in (2, 64, 1000):
        y = _zipf_classes(np.random.RandomState(300 + n), n)
        cases["singletons_n%d" % n] = (y, np.arange(n, dtype=np.int32)[::-1][None].copy())
    for n in (2, 63, 257):
        y = _zipf_classes(np.random.RandomState(400 + n), n)
        y[0], y[1] = 0, 1                                       # at least two classes
        cases["one_cluster_n%d" % n] = (y, np.full((1, n), 5, dtype=np.int32))
    for n in (3, 64, 257):
        rs = np.random.RandomState(500 + n)
        lab = rs.randint(0, max(2, n // 8), n).astype(np.int32)
        lab[0], lab[1] = 0, 1                                   # at least two clusters
        cases["one_class_n%d" % n] = (np.full(n, -3, dtype=np.int32), lab[None])
    for n in (1, 2, 65):
        cases["both_single_n%d" % n] = (np.full(n, 9, dtype=np.int32), np.full((1, n), INT_MAX, dtype=np.int32))
    for n in (1, 3, 65, 1000, 4099):
        cases["negatives_n%d" % n] = _negatives(600 + n, n)
    for n in (63, 257, 4099):
        cases["sparse_n%d" % n] = _sparse(700 + n, n)
    return cases


CASES = build()
# the kinds on which AMI goes through its quotient (the others end in one of scikit-learn's special cases or a zero numerator)
AMI_KINDS = ("random", "negatives", "sparse")
