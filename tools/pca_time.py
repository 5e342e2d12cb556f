#!/usr/bin/env python3
"""GPU time of the device PCA (hsefr_pca_fit / hsefr_pca_transform through ops.pca_fit / ops.pca_transform) at LFW's gallery half
(4582 x 1024, k = 16 and 128), at 4582 x 2048 with k = 128 and on the 170 x 256 gallery of tests/golden/protocols.npz with k = 16:
device-event time of one fit and of one projection, the iterations the fit used, next to the host seconds of scikit-learn's
PCA(k).fit + transform on the same array; then the wall time of one_nn_identification(pca_components=128) on 9164 x 1024 synthetic
embeddings with pca="device" and with pca="host", alternated in one process.
usage: python tools/pca_time.py [--out FILE] [--rounds R]"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch

from hse_facerec_tf_amd import identification, ops

SHAPES = [(4582, 1024, 16), (4582, 1024, 128), (4582, 2048, 128)]


def clustered_rows(n, d, classes, seed):
    """Unit-norm rows around Gaussian class centres: a flat noise spectrum under the class directions, the slow case for the iteration."""
    g = torch.Generator(device="cuda").manual_seed(seed)
    c = torch.randn((classes, d), device="cuda", generator=g)
    y = torch.randint(0, classes, (n,), device="cuda", generator=g)
    x = c[y] + 0.8 * torch.randn((n, d), device="cuda", generator=g)
    return (x / x.norm(dim=1, keepdim=True)).contiguous(), y.cpu().numpy()


def fixture_gallery():
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from oracle import identification as oid
    z = np.load(os.path.join(ROOT, "tests", "golden", "protocols.npz"))
    X, y = oid.synthetic_gallery(int(z["n_classes"]), int(z["dim"]), int(z["seed"]), float(z["noise"]))
    _, _, kept = oid.filter_and_encode(X, y)
    return torch.from_numpy(np.ascontiguousarray(X[kept][z["gallery"]])).cuda()


def event_ms(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    out = fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1), out


def main():
    from sklearn.decomposition import PCA
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pca_time.txt"))
    ap.add_argument("--rounds", type=int, default=3, help="timed repetitions of every row (the minimum and the mean are printed)")
    args = ap.parse_args()
    lines = ["# device PCA (tools/pca_time.py); %s" % torch.cuda.get_device_name(0),
             "# fit_ms / transform_ms: device-event time of one ops.pca_fit / ops.pca_transform call (the fit includes its convergence",
             "#   checks' host reads), one warm-up, then %d calls: minimum / mean; iters: iterations the fit used; host_s: scikit-learn" % args.rounds,
             "#   PCA(k).fit(x) + transform(x) on the same float32 array, wall seconds of one call (its `auto` solver: randomized at the",
             "#   large shapes, so its coordinates are not the exact PCA's); speedup = host_s / (fit + transform)",
             "%6s %5s %4s %18s %18s %6s %5s %9s %8s" % ("n", "d", "k", "fit_ms min/mean", "transform_ms", "iters", "conv", "host_s", "speedup")]
    cases = [(clustered_rows(n, d, max(2, n // 6), n + d)[0], k) for n, d, k in SHAPES] + [(fixture_gallery(), 16)]
    for x, k in cases:
        n, d = x.shape
        ops.pca_fit(x, k)
        fits, trs = [], []
        for _ in range(args.rounds):
            ms, (mean, comp, _, info) = event_ms(lambda: ops.pca_fit(x, k))
            fits.append(ms)
            trs.append(event_ms(lambda: ops.pca_transform(x, mean, comp))[0])
        x_h = x.cpu().numpy()
        t0 = time.perf_counter()
        PCA(n_components=k).fit(x_h).transform(x_h)
        host = time.perf_counter() - t0
        lines.append("%6d %5d %4d %8.3f /%8.3f %8.3f /%8.3f %6d %5s %9.3f %8.1f"
                     % (n, d, k, min(fits), np.mean(fits), min(trs), np.mean(trs), info["iterations"], info["converged"], host,
                        host * 1e3 / (min(fits) + min(trs))))
        print(lines[-1], flush=True)
    # the protocol, end to end: LFW-sized embeddings, 128 components, the two PCA paths alternating
    X, y = clustered_rows(9164, 1024, 1500, 7)
    split = identification.start_split(y).result()[2:]
    wall = {"device": [], "host": []}
    acc = {}
    for r in range(args.rounds + 1):
        for mode in ("device", "host"):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            res = identification.one_nn_identification(X, y, split=split, pca_components=128, pca=mode)
            torch.cuda.synchronize()
            if r:                                                # round 0 warms both paths up
                wall[mode].append(time.perf_counter() - t0)
            acc[mode] = res["accuracy"]
    dev, host = min(wall["device"]), min(wall["host"])
    lines += ["# one_nn_identification(pca_components=128) on 9164 x 1024 synthetic embeddings (%d probes x %d gallery rows), wall seconds,"
              % (len(split[1]), len(split[0])),
              "#   minimum of %d alternated calls: pca=\"device\" %.4f s (accuracy %.4f), pca=\"host\" %.4f s (accuracy %.4f): %s"
              % (args.rounds, dev, acc["device"], host, acc["host"],
                 "the device path is %.1f x faster" % (host / dev) if dev < host else "THE DEVICE PATH DOES NOT WIN (%.2f x slower)" % (dev / host))]
    text = "\n".join(lines) + "\n"
    with open(args.out, "w") as f:
        f.write(text)
    print(text)


if __name__ == "__main__":
    main()
