#!/usr/bin/env python3
"""GPU time of the device RBF SVM (hsefr_rbf_svm_gamma_scale / _fit / _predict through ops) next to scikit-learn's default SVC().fit +
predict on this machine's CPU, at four shapes: the 170 x 256 gallery of tests/golden/protocols.npz (66 classes), 2000 x 512 with 400
classes, LFW's gallery half after a 128-component device PCA (4582 x 128) and without it (4582 x 1024, 1680 classes:
gallery.lfw_like_labels' class histogram, oracle.identification.embeddings_for_labels, L2-normalised, the stratified half split).
Per shape: the pairs of classes, device-event time of one fit (gamma='scale' included, its host work too) and of one predict of the
probes (one warm-up, then the minimum of two), the most iterations of any pair, the wall seconds of ONE default SVC().fit and of its
predict, alternated with the device runs in this process, and the share of probes on which the two predict the same label.  Every row is
written as soon as it is measured.
usage: python tools/rbf_svm_time.py [--out FILE] [--rounds R] [--cases 0,1,2,3]"""
import argparse
import os
import sys
import threading
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import numpy as np
import torch

from hse_facerec_tf_amd import ops
from linear_svm_time import clusters, event_ms, fixture, lfw_half


def host_run(gal, codes, prb):
    """One default SVC().fit and one predict in a thread, a line of output a minute while they run."""
    from sklearn.svm import SVC
    box = {}

    def work():
        t0 = time.perf_counter()
        clf = SVC().fit(gal, codes)
        t1 = time.perf_counter()
        box["pred"] = clf.predict(prb)
        box["fit_s"], box["predict_s"] = t1 - t0, time.perf_counter() - t1
    th = threading.Thread(target=work)
    th.start()
    waited = 0
    while th.is_alive():
        th.join(60.0)
        waited += 60
        if th.is_alive():
            print("  ... SVC() on the host: %d s so far" % waited, flush=True)
    return box["pred"], box["fit_s"], box["predict_s"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rbf_svm_time.txt"))
    ap.add_argument("--rounds", type=int, default=2, help="timed repetitions of the device calls (the minimum is printed)")
    ap.add_argument("--cases", default="0,1,2,3", help="rows to measure, by index: protocols.npz, clusters, LFW half + PCA 128, LFW half")
    args = ap.parse_args()
    picked = sorted({int(c) for c in args.cases.split(",")})
    header = ["# device RBF SVM (tools/rbf_svm_time.py); %s; host: scikit-learn's libsvm on %d CPUs" % (torch.cuda.get_device_name(0),
                                                                                                         len(os.sched_getaffinity(0))),
              "# fit_ms: device-event time of ops.rbf_svm_gamma + ops.rbf_svm_fit(tol=1e-10), host work included; predict_ms: ops.rbf_svm_predict",
              "#   of the probes with votes (one warm-up, then the minimum of %d calls); iters: the most SMO iterations of any pair;" % args.rounds,
              "#   host_fit_s / host_predict_s: wall seconds of ONE default SVC().fit (tol=1e-3) and of its predict on the same rows;",
              "#   same: share of probes on which the device (every pair at its optimum) and the default fit predict one label",
              "%-18s %6s %5s %5s %8s %6s %10s %11s %6s %10s %14s %7s" % ("rows", "n", "d", "K", "pairs", "probes", "fit_ms", "predict_ms", "iters",
                                                                      "host_fit_s", "host_predict_s", "same")]
    with open(args.out, "w") as f:
        f.write("\n".join(header) + "\n")
    print("\n".join(header), flush=True)
    lfw = lfw_half() if picked[-1] >= 2 else None
    cases = [("protocols.npz", fixture, None), ("clusters", lambda: clusters(2000, 512, 400, 0), None), ("LFW half, PCA 128", lambda: lfw, 128),
             ("LFW half", lambda: lfw, None)]
    for name, make, k in [cases[i] for i in picked]:
        gal_h, y, prb_h = make()
        classes, codes = np.unique(y, return_inverse=True)
        K = len(classes)
        gal, prb = torch.from_numpy(np.ascontiguousarray(gal_h)).cuda(), torch.from_numpy(np.ascontiguousarray(prb_h)).cuda()
        if k:
            mean, comp, _, info = ops.pca_fit(gal, k)
            assert info["converged"]
            gal, prb = ops.pca_transform(gal, mean, comp), ops.pca_transform(prb, mean, comp)
        labels = torch.from_numpy(codes.astype(np.int32)).cuda()
        n, d = gal.shape

        def fit():
            gamma = ops.rbf_svm_gamma(gal, k)
            return (gamma,) + ops.rbf_svm_fit(gal, labels, K, gamma)
        fits, preds = [], []
        for r in range(args.rounds + 1):
            ms, (gamma, dual_coef, rho, info) = event_ms(fit)
            ms2, (pred, votes) = event_ms(lambda: ops.rbf_svm_predict(prb, gal, labels, K, gamma, dual_coef, rho))
            if r:                                               # round 0 warms up
                fits.append(ms)
                preds.append(ms2)
            print("%s round %d: fit %.1f ms, predict %.1f ms, gamma %.6g, %s" % (name, r, ms, ms2, gamma, info), flush=True)
            if r == 0:                                          # the host's run between the device's
                host_pred, host_fit_s, host_predict_s = host_run(gal.cpu().numpy()[:, :k or d], codes, prb.cpu().numpy()[:, :k or d])
        same = float((host_pred == pred.cpu().numpy()).mean())
        line = ("%-18s %6d %5d %5d %8d %6d %10.1f %11.1f %6d %10.2f %14.2f %7.4f%s"
                % (name, n, d, K, K * (K - 1) // 2, prb.shape[0], min(fits), min(preds), info["iterations"], host_fit_s, host_predict_s, same,
                   "" if info["converged"] else "  NOT CONVERGED"))
        with open(args.out, "a") as f:
            f.write(line + "\n")
        print(line, flush=True)


if __name__ == "__main__":
    main()
