#!/usr/bin/env python3
"""GPU time of the device random forest (hsefr_forest_fit / _predict through ops) next to scikit-learn's default
RandomForestClassifier(100, max_depth=10).fit + predict on this machine's CPU, at four shapes: the 170 x 256 gallery of
tests/golden/protocols.npz, 2000 x 512 with 400 classes, LFW's gallery half after a 128-component device PCA (4582 x 128) and without
it (4582 x 1024, 1680 classes: gallery.lfw_like_labels' class histogram, oracle.identification.embeddings_for_labels, L2-normalised,
the stratified half split).  Per shape: device-event time of one fit (its one read-back included) and of one predict_proba of the
probes (one warm-up, then the minimum of two), the nodes per tree and the deepest level of the device forest, the wall seconds of ONE
default scikit-learn fit and of its predict, and the accuracy of both on the probes.  Each shape runs in a child process of its own
under a time limit; its row is written as soon as it is measured.
usage: python tools/random_forest_time.py [--out FILE] [--rounds R] [--cases 0,1,2,3] [--append] [--limit SECONDS]"""
import argparse
import os
import subprocess
import sys
import threading
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import numpy as np

NAMES = ["protocols.npz", "clusters", "LFW half, PCA 128", "LFW half"]
ROW = "%-18s %6d %5d %5d %6d %9.1f %11.1f %10.1f %5d %8.4f %10.2f %14.2f %9.4f"


def lfw_half_with_probe_labels():
    from hse_facerec_tf_amd import gallery, identification
    from oracle import identification as oid
    y = gallery.lfw_like_labels(9164, 1680)
    X = oid.embeddings_for_labels(y, dim=1024)
    X = X / np.linalg.norm(X, axis=1, keepdims=True)
    indices, y_enc = identification.filter_classes(y)
    train, test = identification.stratified_half_split(y_enc)
    X = X[indices].astype(np.float32)
    return X[train], y_enc[train], X[test], y_enc[test]


def inputs(index):
    from linear_svm_time import clusters
    if index == 0:
        from oracle import identification as oid
        z = np.load(os.path.join(ROOT, "tests", "golden", "protocols.npz"))
        X, y = oid.synthetic_gallery(int(z["n_classes"]), int(z["dim"]), int(z["seed"]), float(z["noise"]))
        _, y2, kept = oid.filter_and_encode(X, y)
        X = X[kept]
        return X[z["gallery"]], y2[z["gallery"]], X[z["probe"]], y2[z["probe"]], None
    if index == 1:
        gal, y, prb = clusters(2000, 512, 400, 0)
        return gal, y, prb, y, None
    return lfw_half_with_probe_labels() + (128 if index == 2 else None,)


def host_run(gal, codes, prb):
    """One default fit and one predict in a thread, a line of output a minute while they run."""
    from sklearn.ensemble import RandomForestClassifier
    box = {}

    def work():
        t0 = time.perf_counter()
        clf = RandomForestClassifier(n_estimators=100, max_depth=10).fit(gal, codes)
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
            print("  ... RandomForestClassifier on the host: %d s so far" % waited, flush=True)
    return box["pred"], box["fit_s"], box["predict_s"]


def deepest_level(forest):
    left, right, feature = (getattr(forest, k).cpu().numpy() for k in ("left", "right", "feature"))
    deepest = 0
    for t in range(forest.n_trees):
        level, nodes = 0, [0]
        while nodes:
            nodes = [c for i in nodes if feature[t, i] >= 0 for c in (left[t, i], right[t, i])]
            level += bool(nodes)
        deepest = max(deepest, level)
    return deepest


def child(index, rounds):
    import torch
    from hse_facerec_tf_amd import ops
    from linear_svm_time import event_ms
    print("DEV " + torch.cuda.get_device_name(0), flush=True)
    gal_h, y, prb_h, y_prb, k = inputs(index)
    classes, codes = np.unique(y, return_inverse=True)
    K = len(classes)
    gal, prb = torch.from_numpy(np.ascontiguousarray(gal_h)).cuda(), torch.from_numpy(np.ascontiguousarray(prb_h)).cuda()
    if k:
        mean, comp, _, info = ops.pca_fit(gal, k)
        assert info["converged"]
        gal, prb = ops.pca_transform(gal, mean, comp)[:, :k].contiguous(), ops.pca_transform(prb, mean, comp)[:, :k].contiguous()
    labels = torch.from_numpy(codes.astype(np.int32)).cuda()
    n, d = gal.shape
    fits, preds = [], []
    for r in range(rounds + 1):
        ms, forest = event_ms(lambda: ops.random_forest_fit(gal, labels, K))
        ms2, (proba, pred) = event_ms(lambda: ops.random_forest_predict_proba(forest, prb))
        if r:                                               # round 0 warms up
            fits.append(ms)
            preds.append(ms2)
        print("%s round %d: fit %.1f ms, predict %.1f ms" % (NAMES[index], r, ms, ms2), flush=True)
        if r == 0:                                          # the host's run between the device's
            host_pred, host_fit_s, host_predict_s = host_run(gal.cpu().numpy(), codes, prb.cpu().numpy())
    nodes = forest.n_nodes.cpu().numpy()
    acc = float((classes[pred.cpu().numpy()] == y_prb).mean())
    host_acc = float((classes[host_pred] == y_prb).mean())
    print("ROW " + ROW % (NAMES[index], n, d, K, prb.shape[0], min(fits), min(preds), nodes.mean(), deepest_level(forest), acc, host_fit_s,
                          host_predict_s, host_acc), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "random_forest_time.txt"))
    ap.add_argument("--rounds", type=int, default=2, help="timed repetitions of the device calls (the minimum is printed)")
    ap.add_argument("--cases", default="0,1,2,3", help="rows to measure, by index: protocols.npz, clusters, LFW half + PCA 128, LFW half")
    ap.add_argument("--append", action="store_true", help="add rows to FILE instead of starting it")
    ap.add_argument("--limit", type=int, default=900, help="seconds a shape's child process may take")
    ap.add_argument("--child", type=int, default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child is not None:
        return child(args.child, args.rounds)
    if not args.append:                                     # the parent never touches the GPU: the children name it
        header = ["# device random forest (tools/random_forest_time.py); host: scikit-learn %s on %d CPUs (n_jobs unset: one)"
                  % (__import__("sklearn").__version__, len(os.sched_getaffinity(0))),
                  "# fit_ms: device-event time of ops.random_forest_fit (100 trees, depth 10, sqrt features; its read-back included);",
                  "#   predict_ms: ops.random_forest_predict_proba of the probes (one warm-up, then the minimum of %d calls); nodes: mean" % args.rounds,
                  "#   nodes per tree, deepest: the deepest level reached; acc: share of probes labelled right; host_*: wall seconds of ONE default",
                  "#   RandomForestClassifier(100, max_depth=10).fit and of its predict on the same rows, and its accuracy",
                  "%-18s %6s %5s %5s %6s %9s %11s %10s %5s %8s %10s %14s %9s" % ("rows", "n", "d", "K", "probes", "fit_ms", "predict_ms", "nodes",
                                                                             "deep", "acc", "host_fit_s", "host_predict_s", "host_acc")]
        with open(args.out, "w") as f:
            f.write("\n".join(header) + "\n")
        print("\n".join(header), flush=True)
    named = args.append
    for index in sorted({int(c) for c in args.cases.split(",")}):
        cmd = ["timeout", "-k", "10", str(args.limit), sys.executable, os.path.abspath(__file__), "--child", str(index), "--rounds", str(args.rounds)]
        p = subprocess.Popen(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
        row = None
        for line in p.stdout:
            print(line, end="", flush=True)
            if line.startswith("ROW "):
                row = line[4:]
            if line.startswith("DEV ") and not named:
                named = True
                with open(args.out, "a") as f:
                    f.write("# device: " + line[4:])
        rc = p.wait()
        with open(args.out, "a") as f:
            f.write(row if row else "%-18s not measured: the child ended with status %d\n" % (NAMES[index], rc))
        if rc != 0:                                         # a shape that failed or ran out of time ends the run: nothing more is started
            return rc
    return 0


if __name__ == "__main__":
    sys.exit(main())
