#!/usr/bin/env python3
"""Record tests/golden/affinity.npz on the CPU: for every case of tests/affinity_cases.py the generator's parameters (not the features),
scikit-learn's own answer at random_state=0 -- AffinityPropagation(random_state=0).fit(X.astype(float64)): the partition (relabelled in
order of first occurrence), n_iter_, the number of clusters and cluster_centers_indices_ -- the margins of the NumPy restatement
(tests/affinity_ref.py) and per cluster whether its refinement is decidable.

A case is recorded only if it is DECIDABLE: partition, n_iter_ and cluster count are equal over random_state 0..4, and equal to the
restatement's without noise, with the header's hash noise and with S perturbed by 1e-11 relative.  A case that is not is refused and
nothing is written: pick the next seed in tests/affinity_cases.py.

For the case affinity_cases.STEPS_CASE the restatement's answers at max_iter 1, 5 and 16 (no noise) are recorded as well.

    python tools/record_affinity_golden.py"""
import os
import sys
import time
import warnings

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import affinity_cases as cases  # noqa: E402
import affinity_ref as ref  # noqa: E402

REFINE_DECIDED = 1e-9           # a member-sum gap above this is no tie that rounding or noise could turn


def summary(labels, n_iter):
    part = ref.first_occurrence(labels)
    return part, int(n_iter), int(part.max()) + 1


def same(a, b):
    return np.array_equal(a[0], b[0]) and a[1:] == b[1:]


def exemplar_of(exemplars, labels, point):
    return int(exemplars[labels[point]])


def main():
    import sklearn
    from sklearn.cluster import AffinityPropagation
    warnings.simplefilter("ignore")
    cols = {f: [] for f in cases.FIELDS}
    out = dict(n=[], n_iter=[], clusters=[], margin_diag=[], margin_assign=[], partition=[], offset=[0], exemplars=[],
               refinement_decidable=[], cluster_offset=[0])
    for case in cases.CASES:
        name = cases.case_id(case)
        X = cases.case_features(case)
        X64 = X.astype(np.float64)
        t0 = time.time()
        fits = [AffinityPropagation(random_state=s).fit(X64) for s in range(5)]
        t1 = time.time()
        sk = [summary(f.labels_, f.n_iter_) for f in fits]
        S = ref.similarities(X)
        runs = dict(plain=ref.affinity_propagation(S), hashed=ref.affinity_propagation(S, seed=0),
                    perturbed=ref.affinity_propagation(S, perturb=1e-11))
        for s in range(1, 5):
            if not same(sk[0], sk[s]):
                raise SystemExit("%s is not decidable: random_state %d disagrees with 0 (%s / %s)" % (name, s, sk[0][1:], sk[s][1:]))
        for key, r in runs.items():
            if not (same(sk[0], summary(r.labels, r.n_iter)) and r.converged):
                raise SystemExit("%s is not decidable: the %s restatement disagrees (%s / %s)" % (name, key, sk[0][1:], (r.n_iter, len(r.exemplars))))
        r = runs["plain"]
        ex0 = fits[0].cluster_centers_indices_
        decidable = []
        for k, e in enumerate(ex0):
            ok = all(exemplar_of(f.cluster_centers_indices_, f.labels_, e) == e for f in fits[1:])
            ok = ok and all(exemplar_of(q.exemplars, q.labels, e) == e for q in runs.values())
            gaps = [q.margins.refine[q.first_labels[e]] for q in (runs["plain"], runs["hashed"])]
            decidable.append(bool(ok and min(gaps) > REFINE_DECIDED))
        print("%-40s n=%5d  n_iter=%3d  clusters=%3d  decidable refinements %3d  sklearn %.2f s / fit  margins diag %.1e assign %.1e"
              % (name, len(X), sk[0][1], sk[0][2], sum(decidable), (t1 - t0) / 5, r.margins.diag, r.margins.assign))
        for f, v in zip(cases.FIELDS, case):
            cols[f].append(v)
        out["n"].append(len(X))
        out["n_iter"].append(sk[0][1])
        out["clusters"].append(sk[0][2])
        out["margin_diag"].append(min(q.margins.diag for q in runs.values()))
        out["margin_assign"].append(min(q.margins.assign for q in runs.values()))
        out["partition"].append(sk[0][0].astype(np.int32))
        out["offset"].append(out["offset"][-1] + len(X))
        out["exemplars"].append(np.asarray(ex0, np.int32))
        out["refinement_decidable"].append(np.array(decidable, np.uint8))
        out["cluster_offset"].append(out["cluster_offset"][-1] + len(ex0))
    steps = {}
    S = ref.similarities(cases.case_features(cases.CASES[cases.STEPS_CASE]))
    for m in cases.STEPS:
        r = ref.affinity_propagation(S, max_iter=m)
        print("max_iter %2d: n_iter %d converged %d clusters %d margin diag %.1e" % (m, r.n_iter, r.converged, len(r.exemplars), r.margins.diag))
        steps["steps_labels_%d" % m] = r.labels.astype(np.int32)
        steps["steps_exemplars_%d" % m] = r.exemplars.astype(np.int32)
        steps["steps_n_iter_%d" % m] = np.array(r.n_iter, np.int64)
        steps["steps_converged_%d" % m] = np.array(int(r.converged), np.int64)
        steps["steps_margin_diag_%d" % m] = np.array(r.margins.diag)
        steps["steps_margin_assign_%d" % m] = np.array(r.margins.assign)
    np.savez_compressed(cases.GOLDEN, sklearn=np.array(sklearn.__version__),
                        **{k: np.array(v, np.float64 if k.startswith("margin") else np.int64) for k, v in out.items()
                           if k not in ("partition", "exemplars", "refinement_decidable")},
                        partition=np.concatenate(out["partition"]), exemplars=np.concatenate(out["exemplars"]),
                        refinement_decidable=np.concatenate(out["refinement_decidable"]), **steps,
                        **{f: np.array(v, np.float64 if f == "noise" else np.int64) for f, v in cols.items()})
    print("wrote", os.path.relpath(cases.GOLDEN, ROOT), os.path.getsize(cases.GOLDEN), "bytes")


if __name__ == "__main__":
    main()
