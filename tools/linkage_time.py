#!/usr/bin/env python3
"""GPU time of single-linkage clustering from features (hsefr_single_linkage, csrc/linkage.hip: Boruvka rounds, no N x N matrix) for
n in {2048, 9164, 32768} x d in {1024, 2048}, with the rounds the tree actually needed and the time per round, next to the host path it
replaces (identification.feature_distance_matrix + scipy's single linkage on the dense matrix, up to n = 9164).
With --method average / complete / weighted: hsefr_hier_linkage (csrc/hier_linkage.hip: the fp64 n x n matrix, then reciprocal
nearest-neighbour rounds) for n in {2048, 9164}, against the host matrix + scipy's linkage of the same method.
With --method dbscan: hsefr_dbscan (csrc/dbscan.hip: degree scan, filtered Boruvka rounds, border scan; no N x N matrix) for the same
n x d as single linkage at --eps / --min-samples, with the rounds used, clusters and noise, against the host matrix + scikit-learn's
DBSCAN on it (up to n = 9164).
With --method rankorder: hsefr_rank_order (csrc/rank_order.hip: the fp64 n x n matrix, top-20 lists, pair tests and an in-place cluster
reduce per iteration) for n in {2048, 9164} at --norm / --rank, with the iterations, clusters and faces left single, and a three-pair
threshold sequence next to three single calls, against the host matrix + the NumPy restatement of tests/rank_order_ref.py.
With --method centroid / median / ward: hsefr_geom_linkage (libhsefr_geom.so; csrc/geom_linkage.hip's closest-pair engine, or
csrc/hier_linkage.hip's rounds with Ward's rule) for n in {128, 129, 2048, 9164} at d = 1024 -- 128 is the one-workgroup class of
centroid / median, 129 the smallest n of their two-launches-per-step class -- against the host matrix + scipy's linkage of the same
method, with hsefr_hier_linkage 'average' on the same features alternated in the same run.  Every size runs in a child process under
its own time limit.
usage: python tools/linkage_time.py [--method M] [--eps E] [--min-samples K] [--norm T] [--rank R] [--out FILE]"""
import argparse
import os
import subprocess
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from hse_facerec_tf_amd import identification, ops

SIZES = [2048, 9164, 32768]
DIMS = [1024, 2048]
HOST_MAX_N = 9164


def unit_rows(n, d, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    c = torch.randn((max(2, n // 6), d), device="cuda", generator=g)
    x = c[torch.randint(0, c.shape[0], (n,), device="cuda", generator=g)] + 0.8 * torch.randn((n, d), device="cuda", generator=g)
    return (x / x.norm(dim=1, keepdim=True)).contiguous()


def rounds_used(n, a, b, h):
    """Boruvka on the tree (or forest) itself under the same total order (height, lower, higher): the lightest edge leaving a component
    of the full graph is a tree edge, so this replays the device's rounds."""
    lo, hi = np.minimum(a, b), np.maximum(a, b)
    m = len(lo)
    rank = np.empty(m, dtype=np.int64)
    rank[np.lexsort((hi, lo, h))] = np.arange(m)
    label = np.arange(n)
    rounds = 0
    while (label[lo] != label[hi]).any():
        rounds += 1
        la, lb = label[lo], label[hi]
        out = la != lb
        best = np.full(n, m, dtype=np.int64)          # per component root: rank of its lightest outgoing edge
        np.minimum.at(best, la[out], rank[out])
        np.minimum.at(best, lb[out], rank[out])
        chosen = np.flatnonzero(best < m)
        e = np.argsort(rank)[best[chosen]]
        # union the chosen edges (a forest plus mutual picks), then relabel
        uf = np.arange(n)

        def find(v):
            while uf[v] != v:
                uf[v] = uf[uf[v]]
                v = uf[v]
            return v
        for x, y in zip(label[lo[e]], label[hi[e]]):
            rx, ry = find(x), find(y)
            if rx != ry:
                uf[max(rx, ry)] = min(rx, ry)
        parent = np.array([find(v) for v in range(n)])
        label = parent[label]
    return rounds


def gpu_ms(x, reps):
    ops.single_linkage_edges(x=x)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        out = ops.single_linkage_edges(x=x)
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps, out


def host_s(xh, method="single"):
    from scipy.cluster import hierarchy as hac
    from scipy.spatial.distance import squareform
    t0 = time.perf_counter()
    D = identification.feature_distance_matrix(xh)
    t1 = time.perf_counter()
    hac.linkage(squareform(D, checks=False), method)
    t2 = time.perf_counter()
    return t1 - t0, t2 - t1


def hier_ms(x, method, reps):
    ops.hier_linkage_merges(x=x, method=method)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        out = ops.hier_linkage_merges(x=x, method=method)
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps, out


def main_hier(method, out):
    lines = ["# %s-linkage clustering from unit-norm features, fp32 distances in an fp64 matrix (tools/linkage_time.py --method %s); %s"
             % (method, method, torch.cuda.get_device_name(0)),
             "# GPU: hsefr_hier_linkage, CUDA-event time per call (mean of reps after one warm-up): matrix build + reciprocal-NN rounds",
             "# rounds = rounds the tree needed (launched in batches of 32); ms_per_round = gpu_ms / rounds, the matrix build included",
             "# host: identification.feature_distance_matrix (GPU distances + copy to a host float64 matrix) + scipy linkage '%s'" % method,
             "%7s %5s %11s %9s %13s %12s %12s %10s" % ("n", "d", "gpu_ms", "rounds", "ms_per_round", "host_D_s", "host_link_s",
                                                      "speedup")]
    for n in (2048, 9164):
        for d in DIMS:
            x = unit_rows(n, d, n + d)
            ms, (a, b, h, r) = hier_ms(x, method, 3)
            rounds = int(r.max().item()) + 1
            hd, hl = host_s(x.cpu().numpy(), method)
            lines.append("%7d %5d %11.2f %9d %13.3f %12.3f %12.3f %10.1f" % (n, d, ms, rounds, ms / rounds, hd, hl,
                                                                            (hd + hl) * 1e3 / ms))
            print(lines[-1], flush=True)
    text = "\n".join(lines) + "\n"
    if out:
        with open(out, "w") as f:
            f.write(text)
    print(text)


GEOM_SIZES = (128, 129, 2048, 9164)
GEOM_SECTION_TIMEOUT_S = 240


def replay_rescans(W, method, a, b, h):
    """The closest-pair engine replayed on the host from the device's own working matrix, with the cached row minima: checks the
    device's records bit for bit and counts the rows whose minimum had to be rescanned (row y of every step included)."""
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
    import geom_linkage_ref as gref
    n = W.shape[0]
    alive = np.ones(n, dtype=bool)
    size = np.ones(n, dtype=np.int64)
    nn = np.argmin(W, axis=1)
    nnd = W[np.arange(n), nn]
    rescans = 0
    for step in range(n - 1):
        d = nnd.min()
        cand = np.flatnonzero(nnd == d)
        lo, hi = np.minimum(cand, nn[cand]), np.maximum(cand, nn[cand])
        k = np.lexsort((hi, lo))[0]
        x, y = int(lo[k]), int(hi[k])
        assert (x, y, d) == (int(a[step]), int(b[step]), h[step]), (step, x, y, d, a[step], b[step], h[step])
        alive[x] = False
        idx = np.flatnonzero(alive)
        idx = idx[idx != y]
        if method == "centroid":
            v = gref.centroid(W[x, idx], W[y, idx], d, int(size[x]), int(size[y]))[0]
        else:
            v = gref.median(W[x, idx], W[y, idx], d)[0]
        W[y, idx] = v
        W[idx, y] = v
        W[x, :] = np.inf
        W[:, x] = np.inf
        nnd[x] = np.inf
        size[y] += size[x]
        gone = (nn[idx] == x) | (nn[idx] == y)
        take = ~gone & ((v < nnd[idx]) | ((v == nnd[idx]) & (y < nn[idx])))
        nn[idx[take]] = y
        nnd[idx[take]] = v[take]
        rows = np.append(idx[gone], y)
        for r in rows:
            nn[r] = int(np.argmin(W[r]))
            nnd[r] = W[r, nn[r]]
        rescans += len(rows)
    return rescans


def geom_ms(x, method, reps):
    """Device-event ms per call of ops.geom_linkage_merges and, alternated with it in the same loop, of hsefr_hier_linkage 'average'"""
    ops.geom_linkage_merges(x=x, method=method)
    ops.hier_linkage_merges(x=x, method="average")
    torch.cuda.synchronize()
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2 * reps + 1)]
    ev[0].record()
    for k in range(reps):
        out = ops.geom_linkage_merges(x=x, method=method)
        ev[2 * k + 1].record()
        ops.hier_linkage_merges(x=x, method="average")
        ev[2 * k + 2].record()
    torch.cuda.synchronize()
    ms = sum(ev[2 * k].elapsed_time(ev[2 * k + 1]) for k in range(reps)) / reps
    avg = sum(ev[2 * k + 1].elapsed_time(ev[2 * k + 2]) for k in range(reps)) / reps
    return ms, avg, out


def geom_section(method, n):
    """One size, in a process of its own: prints the table's row"""
    d = 1024
    x = unit_rows(n, d, n + d)
    ms, avg_ms, (a, b, h, r) = geom_ms(x, method, 3)
    hd, hl = host_s(x.cpu().numpy(), method)
    if method == "ward":
        rounds = int(r.max().item()) + 1
        detail = "%9d %13.3f" % (rounds, ms / rounds)
    else:
        W, counts = ops.geom_linkage_merges(x=x, method=method, return_matrix=True, return_counts=True)[4:]
        assert counts.tolist() == [n - 1, 0], counts
        rescans = replay_rescans(W.cpu().numpy(), method, a.cpu().numpy(), b.cpu().numpy(), h.cpu().numpy())
        detail = "%9.2f %13.2f" % (ms * 1e3 / (n - 1), rescans / (n - 1))
    print("ROW %7d %5d %11.2f %s %14.2f %12.3f %12.3f %10.1f  # %s" % (n, d, ms, detail, avg_ms, hd, hl, (hd + hl) * 1e3 / ms,
                                                                     torch.cuda.get_device_name(0)), flush=True)


def main_geom(method, out):
    if method == "ward":
        what = ["# GPU: hsefr_geom_linkage, device-event time per call (mean of 3 after one warm-up): matrix build + reciprocal-NN rounds with",
                "# Ward's three-term rule; rounds = rounds the tree needed (launched in batches of 32); ms_per_round = gpu_ms / rounds"]
        cols = ("rounds", "ms_per_round")
    else:
        what = ["# GPU: hsefr_geom_linkage, device-event time per call (mean of 3 after one warm-up): matrix build + n - 1 closest-pair steps",
                "# (n <= 128: one launch of one workgroup, the matrix in LDS; above: two launches per step, no host synchronisation)",
                "# us_per_step = gpu_ms / (n - 1), the matrix build included; rescans_per_step = rows whose cached minimum was rescanned per",
                "# step (row y included), from a host replay of the engine on the device's matrix that also checks every record's bits"]
        cols = ("us_per_step", "rescans_per_step")
    lines = ["# %s-linkage clustering from unit-norm features, fp32 distances in an fp64 matrix (tools/linkage_time.py --method %s)"
             % (method, method)] + what + [
             "# average_ms = hsefr_hier_linkage 'average' on the same features, alternated with it in the same loop",
             "# host: identification.feature_distance_matrix (GPU distances + copy to a host float64 matrix) + scipy linkage '%s'" % method,
             "# every row ran in a child process of its own under a %d s limit" % GEOM_SECTION_TIMEOUT_S,
             "%7s %5s %11s %9s %13s %14s %12s %12s %10s" % (("n", "d", "gpu_ms") + cols + ("average_ms", "host_D_s", "host_link_s", "speedup"))]
    device, failed = None, False
    for n in GEOM_SIZES:
        try:
            res = subprocess.run([sys.executable, os.path.abspath(__file__), "--method", method, "--section", str(n)], capture_output=True,
                                 text=True, timeout=GEOM_SECTION_TIMEOUT_S)
        except subprocess.TimeoutExpired:
            lines.append("%7d  -- no result within %d s; the sizes after it were not run" % (n, GEOM_SECTION_TIMEOUT_S))
            failed = True
            break
        rows = [l for l in res.stdout.splitlines() if l.startswith("ROW ")]
        if res.returncode != 0 or not rows:
            lines.append("%7d  -- the section ended with status %d; the sizes after it were not run" % (n, res.returncode))
            sys.stderr.write(res.stderr[-2000:])
            failed = True
            break
        row, _, device = rows[0][4:].partition("  # ")
        lines.append(row)
        print(lines[-1], flush=True)
    lines[0] += "; %s" % device
    text = "\n".join(lines) + "\n"
    if out:
        with open(out, "w") as f:
            f.write(text)
    print(text)
    if failed:
        sys.exit(1)                                  # nothing more is started on a GPU that a section may have left in a bad state


def dbscan_ms(x, eps, min_samples, reps):
    ops.dbscan_labels(x=x, eps=eps, min_samples=min_samples)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        out = ops.dbscan_labels(x=x, eps=eps, min_samples=min_samples)
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps, out


def dbscan_rounds(x, core, eps):
    """The filtered rounds are Boruvka on the core points' spanning forest of edges w <= eps: the core points' minimum spanning tree
    (single linkage on them, the same w and the same order under their increasing renumbering) cut at eps."""
    idx = torch.nonzero(core, as_tuple=True)[0]
    if len(idx) < 2:
        return 0
    a, b, h = (t.cpu().numpy() for t in ops.single_linkage_edges(x=x[idx].contiguous()))
    keep = h <= eps
    return rounds_used(len(idx), a[keep], b[keep], h[keep])


def main_dbscan(eps, min_samples, out):
    from sklearn.cluster import DBSCAN
    lines = ["# DBSCAN from unit-norm features, fp32 (tools/linkage_time.py --method dbscan --eps %g --min-samples %d); %s"
             % (eps, min_samples, torch.cuda.get_device_name(0)),
             "# GPU: hsefr_dbscan, CUDA-event time per call (mean of reps after one warm-up): degree scan, Boruvka rounds filtered to",
             "# core-core edges w <= eps (ceil(log2 n) launched; the round after the last that hooks ends the rest), border scan",
             "# used = rounds that hooked; row scans = degree + min(used + 1, launched) rounds + border; ms_per_scan = gpu_ms / row scans",
             "# host: identification.feature_distance_matrix (GPU distances + copy to a host float64 matrix) + sklearn DBSCAN (precomputed)",
             "%7s %5s %11s %9s %6s %9s %7s %12s %12s %12s %10s" % ("n", "d", "gpu_ms", "launched", "used", "clusters", "noise",
                                                               "ms_per_scan", "host_D_s", "host_db_s", "speedup")]
    for n in SIZES:
        for d in DIMS:
            x = unit_rows(n, d, n + d)
            ms, (labels, core) = dbscan_ms(x, eps, min_samples, 3 if n <= 9164 else 2)
            used = dbscan_rounds(x, core, eps)
            launched = int(np.ceil(np.log2(n)))
            lab = labels.cpu().numpy()
            hd = hb = float("nan")
            if n <= HOST_MAX_N:
                t0 = time.perf_counter()
                D = identification.feature_distance_matrix(x.cpu().numpy())
                t1 = time.perf_counter()
                DBSCAN(eps=eps, min_samples=min_samples, metric="precomputed").fit(D)
                hd, hb = t1 - t0, time.perf_counter() - t1
            sp = (hd + hb) * 1e3 / ms if n <= HOST_MAX_N else float("nan")
            scans = min(used + 1, launched) + 2
            lines.append("%7d %5d %11.2f %9d %6d %9d %7d %12.2f %12.3f %12.3f %10.1f" % (n, d, ms, launched, used, lab.max() + 1,
                                                                                   (lab < 0).sum(), ms / scans, hd, hb, sp))
            print(lines[-1], flush=True)
    text = "\n".join(lines) + "\n"
    if out:
        with open(out, "w") as f:
            f.write(text)
    print(text)


def rank_order_ms(x, reps, **kw):
    ops.rank_order_labels(x=x, **kw)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        out = ops.rank_order_labels(x=x, **kw)
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps, out


def main_rankorder(norm, rank, out):
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
    import rank_order_ref as ror
    sweep = [(norm, rank), (norm - 0.1, rank), (norm + 0.04, rank + 4)]
    lines = ["# rank-order clustering from unit-norm features, fp32 distances in an fp64 matrix (tools/linkage_time.py --method rankorder "
             "--norm %g --rank %g); %s" % (norm, rank, torch.cuda.get_device_name(0)),
             "# GPU: hsefr_rank_order, CUDA-event time per call (mean of reps after one warm-up): matrix build, top-20 lists, and per",
             "# iteration the pair tests, components, in-place reduce and new lists; the host reads one count per iteration",
             "# single = faces left in no cluster of two; sweep3_ms = one call with the three pairs %s (matrix and" % (sweep,),
             "# first lists built once, restored by device copies), three_ms = the same pairs as three calls",
             "# host: identification.feature_distance_matrix (GPU distances + copy to a host float64 matrix) + the NumPy restatement of",
             "# tests/rank_order_ref.py (the reference's own find_clusters is interpreted Python over face objects: 5-18 s for ONE",
             "# threshold pair at n = 1000 on a development CPU, measured there and not on this machine -- context, not a speed-up)",
             "%7s %5s %11s %6s %9s %7s %11s %11s %12s %12s %10s" % ("n", "d", "gpu_ms", "iters", "clusters", "single", "sweep3_ms",
                                                                "three_ms", "host_D_s", "host_ro_s", "speedup")]
    for n in (2048, 9164):
        for d in DIMS:
            x = unit_rows(n, d, n + d)
            ms, (labels, iters) = rank_order_ms(x, 3, norm_threshold=norm, rank_threshold=rank)
            sweep_ms, _ = rank_order_ms(x, 2, thresholds=sweep)
            three_ms = sum(rank_order_ms(x, 2, norm_threshold=a, rank_threshold=b)[0] for a, b in sweep)
            clusters = ror.clusters_of(labels.cpu().numpy())
            t0 = time.perf_counter()
            D = identification.feature_distance_matrix(x.cpu().numpy())
            t1 = time.perf_counter()
            host, host_iters, _ = ror.rank_order(D, norm, rank)
            hd, hr = t1 - t0, time.perf_counter() - t1
            lines.append("%7d %5d %11.2f %6d %9d %7d %11.2f %11.2f %12.3f %12.3f %10.1f"
                         % (n, d, ms, iters, len(clusters), n - sum(map(len, clusters)), sweep_ms, three_ms, hd, hr, (hd + hr) * 1e3 / ms))
            print(lines[-1], flush=True)
    text = "\n".join(lines) + "\n"
    if out:
        with open(out, "w") as f:
            f.write(text)
    print(text)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--method", default="single", choices=["single", "average", "complete", "weighted", "dbscan", "rankorder", "centroid", "median", "ward"])
    ap.add_argument("--section", type=int, default=None, help="--method centroid / median / ward: run this one size (the tool's own child)")
    ap.add_argument("--eps", type=float, default=0.9, help="--method dbscan: the neighbourhood radius")
    ap.add_argument("--min-samples", type=int, default=4, help="--method dbscan: points within eps (itself included) that make a core")
    ap.add_argument("--norm", type=float, default=1.06, help="--method rankorder: the normalised-distance threshold")
    ap.add_argument("--rank", type=float, default=16, help="--method rankorder: the rank-order threshold")
    args = ap.parse_args()
    if args.method in ("centroid", "median", "ward"):
        return geom_section(args.method, args.section) if args.section else main_geom(args.method, args.out)
    if args.method == "rankorder":
        return main_rankorder(args.norm, args.rank, args.out)
    if args.method == "dbscan":
        return main_dbscan(args.eps, args.min_samples, args.out)
    if args.method != "single":
        return main_hier(args.method, args.out)
    lines = ["# single-linkage clustering from unit-norm features, fp32 (tools/linkage_time.py); %s" % torch.cuda.get_device_name(0),
             "# GPU: hsefr_single_linkage, CUDA-event time per call (mean of reps after one warm-up); rounds launched = ceil(log2 n)",
             "# host: identification.feature_distance_matrix (GPU distances + copy to a host float64 matrix) + scipy linkage 'single'",
             "%7s %5s %11s %9s %9s %13s %12s %12s %10s" % ("n", "d", "gpu_ms", "launched", "used", "ms_per_round", "host_D_s",
                                                        "host_link_s", "speedup")]
    for n in SIZES:
        for d in DIMS:
            x = unit_rows(n, d, n + d)
            ms, (a, b, h) = gpu_ms(x, 3 if n <= 9164 else 2)
            used = rounds_used(n, a.cpu().numpy(), b.cpu().numpy(), h.cpu().numpy())
            launched = int(np.ceil(np.log2(n)))
            hd = hl = float("nan")
            if n <= HOST_MAX_N:
                hd, hl = host_s(x.cpu().numpy())
            sp = (hd + hl) * 1e3 / ms if n <= HOST_MAX_N else float("nan")
            lines.append("%7d %5d %11.2f %9d %9d %13.2f %12.3f %12.3f %10.1f" % (n, d, ms, launched, used, ms / used, hd, hl, sp))
            print(lines[-1], flush=True)
    text = "\n".join(lines) + "\n"
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)
    print(text)


if __name__ == "__main__":
    main()
