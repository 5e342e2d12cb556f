"""The mean-shift cases of tests/golden/mean_shift.npz: the file holds each case's generator parameters and seed with scikit-learn's
answer, not the features -- this module makes the features again (tools/record_mean_shift_golden.py records with it, the CPU and GPU
suites replay it).

A case: ``ids`` identity centres on the unit sphere of R^d, identity i with 1 .. per faces at centre + noise * N(0, I) / sqrt(d),
every row normalised, float32."""
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "mean_shift.npz")

# (ids, per, d, bandwidth, noise): the four groups, seeds 0..2 each, and one larger case whose membership and means span several workgroups
GROUPS = ((12, 20, 64, 0.7, 0.5), (40, 16, 256, 0.7, 0.6), (30, 30, 128, 0.9, 0.8), (8, 40, 32, 0.7, 0.9))
SEEDS = (0, 1, 2)
LARGE = (90, 24, 64, 0.7, 0.5, 0)          # (ids, per, d, bandwidth, noise, seed): about 1100 faces
CASES = tuple(g + (s,) for g in GROUPS for s in SEEDS) + (LARGE,)
FIELDS = ("ids", "per", "d", "bandwidth", "noise", "seed")


def features(ids, per, d, noise, seed):
    rs = np.random.RandomState(seed)
    cen = rs.standard_normal((ids, d))
    cen /= np.linalg.norm(cen, axis=1, keepdims=True)
    sizes = rs.randint(1, per + 1, ids)
    rows = []
    for i, s in enumerate(sizes):
        v = cen[i] + noise * rs.standard_normal((s, d)) / np.sqrt(d)
        rows.append(v / np.linalg.norm(v, axis=1, keepdims=True))
    return np.concatenate(rows).astype(np.float32)


def case_features(case):
    ids, per, d, _, noise, seed = case
    return features(int(ids), int(per), int(d), float(noise), int(seed))


def case_id(case):
    return "ids%d-per%d-d%d-h%g-seed%d" % (case[0], case[1], case[2], case[3], case[5])


def load_golden():
    """[(case tuple, dict of the recorded answer)] in CASES' order"""
    z = np.load(GOLDEN)
    out = []
    for k in range(len(z["n"])):
        case = tuple(z[f][k].item() for f in FIELDS)
        out.append((case, dict(n=int(z["n"][k]), n_iter=int(z["n_iter"][k]), centers=int(z["centers"][k]),
                               labels=z["labels"][z["offset"][k]:z["offset"][k + 1]].astype(np.int64),
                               margins=tuple(float(v) for v in z["margins"][k]))))
    return out
