#!/usr/bin/env python3
"""Records tests/golden/rbf_svm.npz (CPU only, scikit-learn): SVC(gamma='scale', tol=1e-12) -- libsvm at the optimum of every pair's dual,
which the default tol=1e-3 is not -- on every case of tests/rbf_svm_cases.py.  Per case c: c_gamma; c_votes and c_pred of every held-out
row (the votes taken from the pair decisions by libsvm's rule; libsvm's own predict is confirmed to be their first arg-max); c_rho; c_dec,
the pair decisions of the first 8 held-out rows in libsvm's sign and order (for the 44 850 pairs of the 'many pairs' case every 64th pair:
all of them would be 2.9 MB); c_tol_gap = max |dec(tol=1e-10) - dec(tol=1e-12)| and c_min_abs = the smallest |dec|, both over every
held-out row and pair.
usage: python tools/record_rbf_svm_golden.py [--out FILE]"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np


def libsvm_decisions(clf, rows, K):
    """decision_function in libsvm's sign (scikit-learn negates the binary case)."""
    dec = clf.decision_function(rows)
    return -dec[:, None] if K == 2 else dec


def record():
    from sklearn.svm import SVC
    import rbf_svm_cases as cases
    import rbf_svm_ref as ref
    out = {}
    for index in range(cases.N_CASES):
        name, X, labels, K, held = cases.case(index)
        X64, held64 = X.astype(np.float64), held.astype(np.float64)
        clf = SVC(C=1.0, gamma="scale", tol=1e-12, decision_function_shape="ovo").fit(X64, labels)
        loose = SVC(C=1.0, gamma="scale", tol=1e-10, decision_function_shape="ovo").fit(X64, labels)
        dec = libsvm_decisions(clf, held64, K)
        votes, first = ref.votes_of(dec, K)
        assert np.array_equal(clf.predict(held64), first), name          # libsvm's predict is the first arg-max of the votes
        rho = -clf._intercept_                                           # libsvm's sign, before scikit-learn's binary flip
        dual = np.zeros((K - 1, len(labels)))
        dual[:, clf.support_] = clf._dual_coef_
        assert np.abs(ref.decision(held, X, labels, K, clf._gamma, dual, rho) - dec).max() <= 1e-12, name      # the layouts are libsvm's
        c = "c%d_" % index
        out[c + "gamma"] = np.float64(clf._gamma)
        out[c + "votes"] = votes.astype(np.int16)
        out[c + "pred"] = first.astype(np.int16)
        out[c + "rho"] = rho.astype(np.float64)
        out[c + "dec"] = np.ascontiguousarray(dec[:cases.DECISION_ROWS][:, cases.recorded_pairs(dec.shape[1])])
        out[c + "tol_gap"] = np.float64(np.abs(libsvm_decisions(loose, held64, K) - dec).max())
        out[c + "min_abs"] = np.float64(np.abs(dec).min())
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "rbf_svm.npz"))
    args = ap.parse_args()
    out = record()
    np.savez_compressed(args.out, **out)
    for k, v in out.items():
        print(k, v.shape, v.dtype, v if v.ndim == 0 else "")
    print("wrote", args.out, os.path.getsize(args.out), "bytes")


if __name__ == "__main__":
    main()
