"""The affinity-propagation cases of tests/golden/affinity.npz: the file holds each case's generator parameters with scikit-learn's
answer, not the features -- this module makes the features again with the generator of the mean-shift cases
(tools/record_affinity_golden.py records with it, the CPU and GPU suites replay it).

A case is (ids, per, d, noise, seed, rows): mean_shift_cases.features(ids, per, d, noise, seed), its first ``rows`` rows when rows > 0."""
import os

import numpy as np

import mean_shift_cases

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "affinity.npz")

# the three groups the mean-shift cases use (at two seeds), boundary sizes of the 64-wide tiles and of one workgroup's 256 columns at
# d = 8, the mean-shift suite's large case and one near 1900 points
CASES = (
    (12, 20, 64, 0.5, 0, 0), (12, 20, 64, 0.5, 1, 0),
    (40, 16, 256, 0.6, 0, 0), (40, 16, 256, 0.6, 1, 0),
    (30, 30, 128, 0.8, 0, 0), (30, 30, 128, 0.8, 1, 0),
    (16, 30, 8, 0.5, 63, 63), (16, 30, 8, 0.5, 64, 64), (16, 30, 8, 0.5, 65, 65), (30, 30, 8, 0.5, 257, 257),
    (90, 24, 64, 0.5, 0, 0),
    (150, 24, 64, 0.5, 0, 0),
)
FIELDS = ("ids", "per", "d", "noise", "seed", "rows")
STEPS_CASE = 0                  # the case whose answers at max_iter 1, 5 and 16 are recorded too
STEPS = (1, 5, 16)


def case_features(case):
    ids, per, d, noise, seed, n = case
    X = mean_shift_cases.features(int(ids), int(per), int(d), float(noise), int(seed))
    if n:
        assert len(X) >= n
        X = np.ascontiguousarray(X[:int(n)])
    return X


def case_id(case):
    return "ids%d-per%d-d%d-noise%g-seed%d-n%d" % tuple(case)


def duplicated(X):
    """a third of the rows present twice (the copies at the end): the degeneracy scikit-learn's noise exists for"""
    return np.ascontiguousarray(np.concatenate([X, X[::3]]))


def load_golden():
    """[(case tuple, dict of the recorded answer)] in CASES' order, and the recorded steps of STEPS_CASE"""
    z = np.load(GOLDEN)
    out = []
    for k in range(len(z["n"])):
        case = tuple(z[f][k].item() for f in FIELDS)
        lo, hi = z["offset"][k], z["offset"][k + 1]
        clo, chi = z["cluster_offset"][k], z["cluster_offset"][k + 1]
        out.append((case, dict(n=int(z["n"][k]), n_iter=int(z["n_iter"][k]), clusters=int(z["clusters"][k]),
                               partition=z["partition"][lo:hi].astype(np.int64),
                               exemplars=z["exemplars"][clo:chi].astype(np.int64),
                               refinement_decidable=z["refinement_decidable"][clo:chi].astype(bool),
                               margin_diag=float(z["margin_diag"][k]), margin_assign=float(z["margin_assign"][k]))))
    steps = {}
    for m in STEPS:
        steps[m] = dict(labels=z["steps_labels_%d" % m].astype(np.int64), exemplars=z["steps_exemplars_%d" % m].astype(np.int64),
                        n_iter=int(z["steps_n_iter_%d" % m]), converged=int(z["steps_converged_%d" % m]),
                        margin_diag=float(z["steps_margin_diag_%d" % m]), margin_assign=float(z["steps_margin_assign_%d" % m]))
    return out, steps
