#!/usr/bin/env python3
"""GPU time of k-nearest-neighbour identification (hsefr_knn through ops.knn, labels and vote included) for k in {1, 3, 5, 16} at LFW's
split (4582 probes x 4582 gallery rows x 1024: the split-f16 GEMM, then the selection kernel) and at one shape of the fp32 tile path
(1000 x 1000 x 256), next to ops.nn1 at the same shape -- timed in the same process, in rounds that alternate with the k-NN rounds --
and to the host seconds of scikit-learn's KNeighborsClassifier(k).fit(...).predict(...) on the same arrays.
usage: python tools/knn_time.py [--out FILE] [--seconds S]"""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from hse_facerec_tf_amd import ops

SHAPES = [(4582, 4582, 1024), (1000, 1000, 256)]
KS = [1, 3, 5, 16]
ROUNDS = 4


def clustered_unit_rows(n, d, classes, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    c = torch.randn((classes, d), device="cuda", generator=g)
    y = torch.randint(0, classes, (n,), device="cuda", generator=g)
    x = c[y] + 0.8 * torch.randn((n, d), device="cuda", generator=g)
    return (x / x.norm(dim=1, keepdim=True)).contiguous(), y.int().contiguous()


def event_ms(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def alternated_ms(fa, fb, seconds):
    """Mean device-event ms per call of fa and of fb: a warm-up of each, then ROUNDS rounds of each, alternating, sized from a first
    estimate so that each function's rounds fill ``seconds`` together."""
    for f in (fa, fb):
        f()
    torch.cuda.synchronize()
    reps = [max(3, int(seconds * 1e3 / ROUNDS / max(event_ms(f, 5), 1e-3))) for f in (fa, fb)]
    ta, tb = [], []
    for _ in range(ROUNDS):
        ta.append(event_ms(fa, reps[0]))
        tb.append(event_ms(fb, reps[1]))
    return float(np.mean(ta)), float(np.mean(tb)), reps


def main():
    from sklearn.neighbors import KNeighborsClassifier
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "knn_time.txt"))
    ap.add_argument("--seconds", type=float, default=0.5, help="device time each timed function is given per table row")
    args = ap.parse_args()
    lines = ["# k-NN identification from unit-norm features (tools/knn_time.py); %s" % torch.cuda.get_device_name(0),
             "# knn_ms: hsefr_knn with labels (neighbours, distances and the vote), device-event time per call: one warm-up, then the mean of",
             "#   %d rounds of `reps` calls; nn1_ms: hsefr_nn1 at the same shape, its rounds alternating with the k-NN rounds in one process" % ROUNDS,
             "# 4582 x 4582 x 1024 runs the split-f16 GEMM and then the selection kernel (nn1: the row arg-min kernel) over the same slice;",
             "#   1000 x 1000 x 256 runs fp32 distance tiles and the selection kernel (nn1: one kernel, no slice)",
             "# host_s: scikit-learn KNeighborsClassifier(k).fit(gallery, labels).predict(probes) on the same arrays, wall seconds of one call",
             "%6s %6s %5s %3s %10s %10s %8s %13s %10s %10s" % ("nq", "ng", "d", "k", "knn_ms", "nn1_ms", "knn/nn1", "reps", "host_s", "speedup")]
    for nq, ng, d in SHAPES:
        x, y = clustered_unit_rows(ng + nq, d, max(2, ng // 6), ng + d)
        gal, y, qry = x[:ng].contiguous(), y[:ng].contiguous(), x[ng:].contiguous()
        gal_h, qry_h, y_h = gal.cpu().numpy(), qry.cpu().numpy(), y.cpu().numpy()
        for k in KS:
            knn_ms, nn1_ms, reps = alternated_ms(lambda: ops.knn(qry, gal, k, y), lambda: ops.nn1(qry, gal), args.seconds)
            t0 = time.perf_counter()
            KNeighborsClassifier(n_neighbors=k, p=2).fit(gal_h, y_h).predict(qry_h)
            host = time.perf_counter() - t0
            lines.append("%6d %6d %5d %3d %10.4f %10.4f %8.2f %13s %10.3f %10.1f" % (nq, ng, d, k, knn_ms, nn1_ms, knn_ms / nn1_ms,
                                                                                 "%d/%d" % tuple(reps), host, host * 1e3 / knn_ms))
            print(lines[-1], flush=True)
    text = "\n".join(lines) + "\n"
    with open(args.out, "w") as f:
        f.write(text)
    print(text)


if __name__ == "__main__":
    main()
