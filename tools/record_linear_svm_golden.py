#!/usr/bin/env python3
"""Records tests/golden/linear_svm.npz (CPU only, scikit-learn): LinearSVC(tol=1e-10, max_iter=10**6) -- the optimum of its objective to
about 1e-10 in decision values, which the default tol=1e-4 is not -- fitted on the gallery of tests/golden/protocols.npz, on the raw
and on the L2-normalised features; the file holds the probes' decision values and predicted labels (no coefficients: they are not
needed and would make the file eight times as large).
usage: python tools/record_linear_svm_golden.py [--out FILE]"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np

from oracle import identification as oid


def record():
    """{"decision_raw", "y_pred_raw", "decision_norm", "y_pred_norm"}: [146, 66] float64 and [146] labels."""
    from sklearn.svm import LinearSVC
    z = np.load(os.path.join(ROOT, "tests", "golden", "protocols.npz"))
    X, y = oid.synthetic_gallery(int(z["n_classes"]), int(z["dim"]), int(z["seed"]), float(z["noise"]))
    Xn, y2, kept = oid.filter_and_encode(X, y)
    g, p = z["gallery"], z["probe"]
    out = {}
    for name, A in (("raw", X[kept]), ("norm", Xn)):
        clf = LinearSVC(tol=1e-10, max_iter=10 ** 6, random_state=0).fit(A[g].astype(np.float32), y2[g])
        out["decision_" + name] = clf.decision_function(A[p].astype(np.float32)).astype(np.float64)
        out["y_pred_" + name] = clf.predict(A[p].astype(np.float32))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "linear_svm.npz"))
    args = ap.parse_args()
    out = record()
    np.savez_compressed(args.out, **out)
    for k, v in out.items():
        print(k, v.shape, v.dtype)
    print("wrote", args.out, os.path.getsize(args.out), "bytes")


if __name__ == "__main__":
    main()
