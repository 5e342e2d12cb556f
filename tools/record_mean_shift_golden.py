#!/usr/bin/env python3
"""Record tests/golden/mean_shift.npz on the CPU: for every case of tests/mean_shift_cases.py the generator's parameters and seed (not
the features), scikit-learn's own answer -- MeanShift(bandwidth=h).fit(X): labels_, n_iter_, the number of centres -- and the four
margins of the NumPy restatement (tests/mean_shift_ref.py), by which the suites prove a case decidable.  The restatement must give
scikit-learn's labels, n_iter_ and centres on every case, or nothing is written.

    python tools/record_mean_shift_golden.py"""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import mean_shift_cases as cases  # noqa: E402
import mean_shift_ref as ref  # noqa: E402


def main():
    import sklearn
    from sklearn.cluster import MeanShift
    cols = {f: [] for f in cases.FIELDS}
    ns, iters, centers, margins, labels, offset = [], [], [], [], [], [0]
    for case in cases.CASES:
        X = cases.case_features(case)
        h = case[3]
        t0 = time.time()
        ms = MeanShift(bandwidth=h).fit(X)
        t1 = time.time()
        r = ref.mean_shift(X, h)
        assert np.array_equal(ms.labels_, r.labels), cases.case_id(case)
        assert ms.n_iter_ == r.n_iter and len(ms.cluster_centers_) == len(r.centers), cases.case_id(case)
        err = float(np.abs(ms.cluster_centers_ - r.centers).max())          # scikit-learn keeps float32 inputs in float32
        assert err < 1e-6, (cases.case_id(case), err)
        print("%-34s n=%5d  n_iter=%d  means=%4d  centres=%3d  sklearn %.2f s  |centres - ref| %.1e  margins %s"
              % (cases.case_id(case), len(X), r.n_iter, r.distinct, len(r.centers), t1 - t0, err, " ".join("%.1e" % m for m in r.margins)))
        for f, v in zip(cases.FIELDS, case):
            cols[f].append(v)
        ns.append(len(X))
        iters.append(ms.n_iter_)
        centers.append(len(ms.cluster_centers_))
        margins.append(r.margins)
        labels.append(ms.labels_.astype(np.int32))
        offset.append(offset[-1] + len(X))
    np.savez_compressed(cases.GOLDEN, sklearn=np.array(sklearn.__version__), n=np.array(ns, np.int64), n_iter=np.array(iters, np.int64),
                        centers=np.array(centers, np.int64), margins=np.array(margins, np.float64), labels=np.concatenate(labels),
                        offset=np.array(offset, np.int64),
                        **{f: np.array(v, np.float64 if f in ("bandwidth", "noise") else np.int64) for f, v in cols.items()})
    print("wrote", os.path.relpath(cases.GOLDEN, ROOT), os.path.getsize(cases.GOLDEN), "bytes")


if __name__ == "__main__":
    main()
