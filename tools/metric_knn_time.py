#!/usr/bin/env python3
"""GPU time of k-nearest-neighbour identification under the study's chi-square and KL distances (hsefr_knn_metric through
ops.knn(metric=), labels and vote included) for k in {1, 3} at LFW's split (4582 probes x 4582 gallery rows x 1024) and at
1000 x 1000 x 256, next to hsefr_knn (squared L2) at the same shape -- timed in the same process, in rounds that alternate -- and to
the host seconds of scikit-learn's KNeighborsClassifier(k, metric=callable).fit(...).predict(...) with the reference's two callables
(facerec_test.py:157-164), which it calls pair by pair: run once at 1000 x 1000 x 256, at LFW size only with --host-lfw (minutes).
usage: python tools/metric_knn_time.py [--out FILE] [--seconds S] [--host-lfw]"""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from hse_facerec_tf_amd import ops

SHAPES = [(4582, 4582, 1024), (1000, 1000, 256)]
KS = [1, 3]
METRICS = ["chi2", "kl"]
ROUNDS = 4


def chi2dist(x, y):
    total = x + y
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(total > 0, (x - y) ** 2 / total, 0).sum()


def KL_dist(x, y):
    return ((x + 0.001) * np.log((x + 0.001) / (y + 0.001))).sum()


CALLABLES = {"chi2": chi2dist, "kl": KL_dist}


def clustered_nonnegative_unit_rows(n, d, classes, seed):
    """Non-negative like GAP features after ReLU6, L2-normalised as the reference's X_norm."""
    g = torch.Generator(device="cuda").manual_seed(seed)
    c = torch.randn((classes, d), device="cuda", generator=g)
    y = torch.randint(0, classes, (n,), device="cuda", generator=g)
    x = (c[y] + 0.8 * torch.randn((n, d), device="cuda", generator=g)).clamp_(min=0)
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
    reps = [max(3, int(seconds * 1e3 / ROUNDS / max(event_ms(f, 3), 1e-3))) for f in (fa, fb)]
    ta, tb = [], []
    for _ in range(ROUNDS):
        ta.append(event_ms(fa, reps[0]))
        tb.append(event_ms(fb, reps[1]))
    return float(np.mean(ta)), float(np.mean(tb)), reps


def main():
    from sklearn.neighbors import KNeighborsClassifier
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "metric_knn_time.txt"))
    ap.add_argument("--seconds", type=float, default=0.5, help="device time each timed function is given per table row")
    ap.add_argument("--host-lfw", action="store_true", help="run scikit-learn with the callables at 4582 x 4582 x 1024 too (minutes per row)")
    args = ap.parse_args()
    lines = ["# k-NN identification under chi2dist / KL_dist from non-negative unit-norm features (tools/metric_knn_time.py); %s"
             % torch.cuda.get_device_name(0),
             "# metric_ms: hsefr_knn_metric with labels (distance tiles, selection, vote), device-event time per call: one warm-up, then the",
             "#   mean of %d rounds of `reps` calls; l2_ms: hsefr_knn at the same shape and k, its rounds alternating in one process" % ROUNDS,
             "# Gpair-el/s: nq * ng * d pair elements per second of metric_ms",
             "# host_s: scikit-learn KNeighborsClassifier(k, metric=callable).fit(gallery, labels).predict(probes) with the reference's callable",
             "#   on the same arrays, wall seconds of ONE call (- : not run; --host-lfw runs it); same: share of probes with scikit-learn's label",
             "%6s %6s %5s %5s %3s %10s %10s %9s %11s %11s %9s %9s %6s"
             % ("nq", "ng", "d", "metric", "k", "metric_ms", "l2_ms", "metric/l2", "Gpair-el/s", "reps", "host_s", "speedup", "same")]
    for nq, ng, d in SHAPES:
        x, y = clustered_nonnegative_unit_rows(ng + nq, d, max(2, ng // 6), ng + d)
        gal, y, qry = x[:ng].contiguous(), y[:ng].contiguous(), x[ng:].contiguous()
        gal_h, qry_h, y_h = gal.cpu().numpy(), qry.cpu().numpy(), y.cpu().numpy()
        for metric in METRICS:
            for k in KS:
                m_ms, l2_ms, reps = alternated_ms(lambda: ops.knn(qry, gal, k, y, metric=metric), lambda: ops.knn(qry, gal, k, y), args.seconds)
                host, speedup, same = "-", "-", "-"
                if args.host_lfw or nq * ng <= 1000 * 1000:
                    t0 = time.perf_counter()
                    want = KNeighborsClassifier(n_neighbors=k, metric=CALLABLES[metric]).fit(gal_h, y_h).predict(qry_h)
                    t = time.perf_counter() - t0
                    got = ops.knn(qry, gal, k, y, metric=metric)[2].cpu().numpy()
                    host, speedup, same = "%.2f" % t, "%.0f" % (t * 1e3 / m_ms), "%.4f" % float((got == want).mean())
                lines.append("%6d %6d %5d %5s %3d %10.4f %10.4f %9.2f %11.1f %11s %9s %9s %6s"
                             % (nq, ng, d, metric, k, m_ms, l2_ms, m_ms / l2_ms, nq * ng * d / m_ms / 1e6, "%d/%d" % tuple(reps), host, speedup, same))
                print(lines[-1], flush=True)
    text = "\n".join(lines) + "\n"
    with open(args.out, "w") as f:
        f.write(text)
    print(text)


if __name__ == "__main__":
    main()
