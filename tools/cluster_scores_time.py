#!/usr/bin/env python3
"""GPU time of scoring a clustering sweep on the device (hsefr_flat_cuts + hsefr_partition_scores through ops.flat_cuts /
ops.partition_scores) for the study's 71 thresholds at n = 2048 and n = 9164 (LFW's size; about 1680 Zipf-sized classes there, the same
density at 2048), next to the host path it replaces -- clustering.fcluster_distance, scikit-learn's adjusted_rand_score,
adjusted_mutual_info_score and homogeneity_completeness_v_measure, and clustering.bcubed, per row and in total; then
clustering.select_threshold(method="average") end to end against the same sweep scored on the host, alternated in one process.
Also writes the largest error of the device's six sums and of scikit-learn's own against the mpmath goldens of
tests/golden/partition_scores_exact.npz (profiles/cluster_scores_accuracy.txt).
usage: python tools/cluster_scores_time.py [--out FILE] [--accuracy-out FILE] [--rounds R] [--reps K]"""
import argparse
import os
import sys
import time
import warnings

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import torch
from sklearn import metrics

from hse_facerec_tf_amd import clustering, ops

warnings.filterwarnings("ignore", category=UserWarning, module="sklearn")      # "y could represent a regression problem"
STATS = ("H_true", "H_pred", "MI", "EMI", "sum nij^2/a/N", "sum nij^2/b/N")


def album(n, classes, seed, d=128):
    """unit-norm features around class centres, Zipf-like class sizes"""
    rs = np.random.RandomState(seed)
    w = 1.0 / np.arange(1, classes + 1)
    y = rs.choice(classes, size=n, p=w / w.sum())
    X = rs.randn(classes, d)[y] + 0.55 * rs.randn(n, d)
    return (X / np.linalg.norm(X, axis=1, keepdims=True)).astype(np.float32), y


def host_scores(y, y_pred, clocks=None):
    """the ten statistics of get_clustering_statistics on the host, adding each part's seconds to clocks"""
    out, t = [], time.perf_counter()
    for name, fn in (("ARI", lambda: (metrics.adjusted_rand_score(y, y_pred),)),
                     ("AMI", lambda: (metrics.adjusted_mutual_info_score(y, y_pred, average_method="arithmetic"),)),
                     ("h/c/v", lambda: metrics.homogeneity_completeness_v_measure(y, y_pred)),
                     ("bcubed", lambda: clustering.bcubed(y, y_pred))):
        out += list(fn())
        now = time.perf_counter()
        if clocks is not None:
            clocks[name] = clocks.get(name, 0.0) + now - t
        t = now
    return [len(np.unique(y)), len(np.unique(y_pred))] + out


def host_select(X, y, thresholds):
    """select_threshold's work with the sweep cut and scored on the host (the linkage itself runs on the device either way)"""
    Z = clustering.linkage(X, "average")
    labels = clustering.fcluster_distance(Z, thresholds)
    table = np.array([host_scores(y, row) for row in labels])
    best, stat, count = clustering.select_from_curve(thresholds, table[:, clustering.STATS_NAMES.index("BCubed_precision")])
    return best, stat, count


def time_sweep(n, classes, reps, lines):
    X, y = album(n, classes, n)
    thresholds = clustering.SWEEP_THRESHOLDS
    Z = clustering.linkage(X, "average")
    order, gaps = clustering._cut_order(Z)
    d_order, d_gaps = torch.from_numpy(order.astype(np.int32)).cuda(), torch.from_numpy(gaps).cuda()
    d_thr = torch.from_numpy(thresholds).cuda()
    d_y = torch.from_numpy(np.unique(y, return_inverse=True)[1].reshape(-1).astype(np.int32)).cuda()

    def device():
        return ops.partition_scores(d_y, ops.flat_cuts(d_order, d_gaps, d_thr))
    device()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        counts, stats = device()
        e1.record()
        torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1))
    t0 = time.perf_counter()
    labels = clustering.fcluster_distance(Z, thresholds)
    clocks = {"fcluster_distance": time.perf_counter() - t0}
    table = np.array([host_scores(y, row, clocks) for row in labels])
    host_total = sum(clocks.values())
    # the same numbers both ways (ARI exactly, the rest to rounding)
    counts, stats = counts.cpu().numpy(), stats.cpu().numpy()
    dev = np.array([clustering.scores_from_counts(counts[r], stats[r], n) for r in range(len(thresholds))])
    assert np.array_equal(dev[:, 0], table[:, 2]), "ARI differs between the device and scikit-learn"
    worst = float(np.abs(dev - table[:, 2:]).max())
    clusters = counts[:, 1]
    lines.append("n = %d, %d classes, 71 thresholds (%d .. %d clusters a row): device flat_cuts + partition_scores %.3f ms min / %.3f ms mean of %d"
                 % (n, len(np.unique(y)), clusters.max(), clusters.min(), min(ms), np.mean(ms), reps))
    lines.append("    host, all 71 rows: %.3f s = %s" % (host_total, ", ".join("%s %.3f s" % kv for kv in clocks.items())))
    lines.append("    host per row: %s" % ", ".join("%s %.2f ms" % (k, v * 1e3 / (1 if k == "fcluster_distance" else 71)) for k, v in clocks.items())
                 + " (fcluster_distance: all rows)")
    lines.append("    host / device = %.0f; largest difference between the two paths' eight scores: %.2e" % (host_total * 1e3 / min(ms), worst))
    print("\n".join(lines[-4:]), flush=True)
    return X, y


def accuracy(path):
    from partition_cases import CASES
    from sklearn.metrics.cluster import contingency_matrix, entropy, expected_mutual_information, mutual_info_score
    import partition_scores_ref as ref
    golden = np.load(os.path.join(ROOT, "tests", "golden", "partition_scores_exact.npz"))
    worst = {"device": np.zeros(6), "scikit-learn": np.zeros(6)}
    worst_rel_emi = {"device": 0.0, "scikit-learn": 0.0}
    rows = 0
    for name, (y, labels) in CASES.items():
        stats = ops.partition_scores(torch.from_numpy(y).cuda(), torch.from_numpy(labels).cuda())[1].cpu().numpy()
        for r, row in enumerate(labels):
            g = golden[name][r]
            y_pred = ref.study_y_pred(row)
            cont = contingency_matrix(y, y_pred, sparse=True)
            single = min(cont.shape) == 1
            p, rec, _ = clustering.bcubed(y, y_pred)
            sk = np.array([entropy(y), entropy(y_pred), g[2] if single else mutual_info_score(None, None, contingency=cont),
                           expected_mutual_information(cont, len(y)), p, rec])
            for who, got in (("device", stats[r]), ("scikit-learn", sk)):
                worst[who] = np.maximum(worst[who], np.abs(got - g))
                if g[3] > 0:
                    worst_rel_emi[who] = max(worst_rel_emi[who], abs(got[3] - g[3]) / g[3])
            rows += 1
    lines = ["# largest error of hsefr_partition_scores' six sums, and of scikit-learn 1.7's own (entropy, mutual_info_score,",
             "# expected_mutual_information; clustering.bcubed for the last two), against the mpmath values of",
             "# tests/golden/partition_scores_exact.npz over the %d rows of the %d cases of tests/partition_cases.py (n = 1 .. 4099)" % (rows, len(CASES)),
             "# (tools/cluster_scores_time.py); %s" % torch.cuda.get_device_name(0),
             "%-16s %12s %12s" % ("sum", "device", "scikit-learn")]
    for k, name in enumerate(STATS):
        lines.append("%-16s %12.3e %12.3e" % (name, worst["device"][k], worst["scikit-learn"][k]))
    lines.append("%-16s %12.3e %12.3e" % ("EMI, relative", worst_rel_emi["device"], worst_rel_emi["scikit-learn"]))
    lines.append("# the bounds the tests hold them to at n = 4099: %.2e for the sums, 40 eps N ln N = %.2e relative for EMI plus its summation term"
                 % (ref.bound_sum(4099), 40 * ref.EPS * 4099 * np.log(4099)))
    with open(path, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cluster_scores_time.txt"))
    ap.add_argument("--accuracy-out", default=os.path.join(ROOT, "profiles", "cluster_scores_accuracy.txt"))
    ap.add_argument("--rounds", type=int, default=2, help="alternated end-to-end repetitions after one warm-up round")
    ap.add_argument("--reps", type=int, default=20, help="timed device calls per size")
    args = ap.parse_args()
    accuracy(args.accuracy_out)
    lines = ["# scoring a 71-threshold clustering sweep (tools/cluster_scores_time.py); %s" % torch.cuda.get_device_name(0),
             "# device: CUDA-event time of ops.flat_cuts + ops.partition_scores for all 71 rows in one call each, after one warm-up call;",
             "# host: wall seconds on this machine's CPU of what they replace, scikit-learn %s" % __import__("sklearn").__version__]
    X, y = None, None
    for n, classes in ((2048, 375), (9164, 1680)):
        X, y = time_sweep(n, classes, args.reps, lines)
    # the largest album the call takes: its keys sort in global memory (above 16384 faces), one workgroup per row
    rs = np.random.RandomState(65536)
    big_y = torch.from_numpy(rs.randint(0, 12000, 65536).astype(np.int32)).cuda()
    big = torch.from_numpy(np.stack([rs.randint(0, c, 65536) for c in np.linspace(400, 40000, 71).astype(int)]).astype(np.int32)).cuda()
    ops.partition_scores(big_y, big)
    torch.cuda.synchronize()
    ms = []
    for _ in range(5):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        ops.partition_scores(big_y, big)
        e1.record()
        torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1))
    lines.append("n = 65536 (HSEFR_SCORES_MAX_N), 12000 random classes, 71 random labellings of 400 .. 40000 clusters: device partition_scores "
                 "%.3f ms min / %.3f ms mean of 5 (global-memory sort)" % (min(ms), np.mean(ms)))
    print(lines[-1], flush=True)
    wall = {"device": [], "host": []}
    answer = {}
    for r in range(args.rounds + 1):
        for mode in ("device", "host"):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            if mode == "device":
                sel = clustering.select_threshold([(X, y)], "average")
                answer[mode] = (sel.threshold, sel.statistic, len(sel.evaluated))
            else:
                answer[mode] = host_select(X, y, clustering.SWEEP_THRESHOLDS)
            torch.cuda.synchronize()
            if r:
                wall[mode].append(time.perf_counter() - t0)
    dev, host = min(wall["device"]), min(wall["host"])
    lines += ["# clustering.select_threshold([album], 'average') on the 9164-face album, wall seconds, minimum of %d alternated calls after a" % args.rounds,
              "#   warm-up round: %.3f s (threshold %.2f, statistic %.6f, %d points); the same sweep cut and scored on the host: %.3f s"
              % (dev, answer["device"][0], answer["device"][1], answer["device"][2], host),
              "#   (threshold %.2f, statistic %.6f, %d points): %s.  Both include the device linkage and the host's"
              % (answer["host"][0], answer["host"][1], answer["host"][2],
                 "the device path is %.1f x faster" % (host / dev) if dev < host else "THE DEVICE PATH DOES NOT WIN (%.2f x slower)" % (dev / host)),
              "#   union-find and leaf-order pass over Z, which the scoring does not touch."]
    text = "\n".join(lines) + "\n"
    with open(args.out, "w") as f:
        f.write(text)
    print(text)


if __name__ == "__main__":
    main()
