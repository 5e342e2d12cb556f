#!/usr/bin/env python3
"""GPU time of the device linear SVM (hsefr_linear_svm_fit / _decision / _predict through ops) next to scikit-learn's default
LinearSVC().fit on this machine's CPU, at four shapes: LFW's gallery half (4582 x 1024, 1680 classes: gallery.lfw_like_labels'
class histogram, oracle.identification.embeddings_for_labels, L2-normalised, the stratified half split), the same rows after a
128-component device PCA (4582 x 128), 2000 x 512 with 400 classes, and the 170 x 256 gallery of tests/golden/protocols.npz (66 classes).
Per shape: device-event time of one fit (its host reads included), the Newton iterations and batched Hessian-vector products it used,
the time of decision + predict on the probes, the wall seconds of ONE default LinearSVC().fit, and the share of probes on which the two
predict the same label.  Last, the product kernel's achieved fp64 FLOP/s at the LFW shape: the decision call's rate (2 n d K flops; the fit's own
products are not timed separately).
usage: python tools/linear_svm_time.py [--out FILE] [--rounds R] [--cases 0,1,2,3] [--append]
(--cases picks rows by index; --append adds them to an existing file without the header, so that a slow host fit can have a run of its own)"""
import argparse
import os
import sys
import threading
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch

from hse_facerec_tf_amd import gallery, identification, ops
from oracle import identification as oid


def lfw_half():
    y = gallery.lfw_like_labels(9164, 1680)
    X = oid.embeddings_for_labels(y, dim=1024)
    X = X / np.linalg.norm(X, axis=1, keepdims=True)
    indices, y_enc = identification.filter_classes(y)
    train, test = identification.stratified_half_split(y_enc)
    X = X[indices].astype(np.float32)
    return X[train], y_enc[train], X[test]


def clusters(n, d, classes, seed):
    rs = np.random.RandomState(seed)
    cent = rs.randn(classes, d)
    y = np.repeat(np.arange(classes), n // classes)
    X = cent[np.concatenate([y, y])] + 0.8 * rs.randn(2 * len(y), d)
    X = (X / np.linalg.norm(X, axis=1, keepdims=True)).astype(np.float32)
    return X[:len(y)], y, X[len(y):]


def fixture():
    z = np.load(os.path.join(ROOT, "tests", "golden", "protocols.npz"))
    X, y = oid.synthetic_gallery(int(z["n_classes"]), int(z["dim"]), int(z["seed"]), float(z["noise"]))
    _, y2, kept = oid.filter_and_encode(X, y)
    X = X[kept]
    return X[z["gallery"]], y2[z["gallery"]], X[z["probe"]]


def event_ms(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    out = fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1), out


def host_fit(gal, codes):
    """One default LinearSVC().fit in a thread, a line of output a minute while it runs."""
    from sklearn.svm import LinearSVC
    box = {}

    def work():
        t0 = time.perf_counter()
        box["clf"] = LinearSVC().fit(gal, codes)
        box["s"] = time.perf_counter() - t0
    th = threading.Thread(target=work)
    th.start()
    waited = 0
    while th.is_alive():
        th.join(60.0)
        waited += 60
        if th.is_alive():
            print("  ... LinearSVC().fit on the host: %d s so far" % waited, flush=True)
    return box["clf"], box["s"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "linear_svm_time.txt"))
    ap.add_argument("--rounds", type=int, default=2, help="timed repetitions of the device calls (the minimum and the mean are printed)")
    ap.add_argument("--cases", default="0,1,2,3", help="rows to measure, by index: LFW half, LFW half + PCA 128, clusters, protocols.npz")
    ap.add_argument("--append", action="store_true", help="add the rows to --out instead of writing it anew (no header)")
    args = ap.parse_args()
    picked = sorted({int(c) for c in args.cases.split(",")})
    lines = ["# device linear SVM (tools/linear_svm_time.py); %s; host: scikit-learn's liblinear on %d CPUs" % (torch.cuda.get_device_name(0),
                                                                                                                 len(os.sched_getaffinity(0))),
             "# fit_ms: device-event time of one ops.linear_svm_fit(tol=1e-10) call, host reads included (one warm-up, then %d calls:" % args.rounds,
             "#   minimum / mean); newton: Newton iterations; hv: batched Hessian-vector products; predict_ms: ops.linear_svm_decision +",
             "#   ops.linear_svm_predict of the probes; host_s: wall seconds of ONE default LinearSVC().fit (tol=1e-4) on the same rows;",
             "#   speedup = host_s / fit; same: share of probes on which the device (the optimum) and the default fit predict one label",
             "%-18s %6s %5s %5s %6s %20s %6s %6s %18s %9s %8s %7s" % ("rows", "n", "d", "K", "probes", "fit_ms min/mean", "newton", "hv",
                                                                     "predict_ms", "host_s", "speedup", "same")]
    if args.append:
        lines = []
    lfw = lfw_half() if picked[0] < 2 else None
    cases = [("LFW half", lfw, None), ("LFW half, PCA 128", lfw, 128), ("clusters", clusters(2000, 512, 400, 0), None),
             ("protocols.npz", fixture(), None)]
    cases = [cases[i] for i in picked]
    flops = None
    for name, (gal_h, y, prb_h), k in cases:
        classes, codes = np.unique(y, return_inverse=True)
        gal, prb = torch.from_numpy(np.ascontiguousarray(gal_h)).cuda(), torch.from_numpy(np.ascontiguousarray(prb_h)).cuda()
        if k:
            mean, comp, _, info = ops.pca_fit(gal, k)
            assert info["converged"]
            gal, prb = ops.pca_transform(gal, mean, comp), ops.pca_transform(prb, mean, comp)
        labels = torch.from_numpy(codes.astype(np.int32)).cuda()
        n, d = gal.shape
        fits, preds = [], []
        for r in range(args.rounds + 1):
            ms, (coef, intercept, info) = event_ms(lambda: ops.linear_svm_fit(gal, labels, len(classes)))
            dec_ms, dec = event_ms(lambda: ops.linear_svm_decision(prb, coef, intercept))
            ms2, pred = event_ms(lambda: ops.linear_svm_predict(dec))
            if r:                                               # round 0 warms up
                fits.append(ms)
                preds.append(dec_ms + ms2)
                if name == "LFW half":
                    rate = 2.0 * prb.shape[0] * d * len(classes) / (dec_ms * 1e-3)
                    flops = rate if flops is None else max(flops, rate)
            print("%s round %d: fit %.1f ms, %s" % (name, r, ms, info), flush=True)
        clf, host = host_fit(gal.cpu().numpy(), codes)
        same = float((clf.predict(prb.cpu().numpy()) == pred.cpu().numpy()).mean())
        lines.append("%-18s %6d %5d %5d %6d %9.1f /%9.1f %6d %6d %8.3f /%8.3f %9.2f %8.1f %7.4f%s"
                     % (name, n, d, len(classes), prb.shape[0], min(fits), np.mean(fits), info["iterations"], info["hessian_products"],
                        min(preds), np.mean(preds), host, host * 1e3 / min(fits), same, "" if info["converged"] else "  NOT CONVERGED"))
        print(lines[-1], flush=True)
    if flops is not None:
        lines.append("# the product kernel at the LFW shape, as the DECISION call runs it (ops.linear_svm_decision of 4582 probes: 4582 result rows, fp32")
        lines.append("#   rows converted on load, the bias epilogue, the wrapper's host time inside the events; 2 n d K = %.1f GFLOP): %.2f TFLOP/s fp64."
                     % (2.0 * 4582 * 1024 * 1680 / 1e9, flops / 1e12))
        lines.append("#   The fit's own products (at most 512 class rows per block, a flag test per tile) are not timed on their own: hv counts the")
        lines.append("#   batched products LAUNCHED, tiles of finished classes that return at once included, so it gives no rate.")
    text = "\n".join(lines) + "\n"
    with open(args.out, "a" if args.append else "w") as f:
        f.write(text)
    print(text)


if __name__ == "__main__":
    main()
