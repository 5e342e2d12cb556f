#!/usr/bin/env python3
"""Device time of mean-shift clustering (hsefr_shift_fit, libhsefr_shift.so, through ops.mean_shift_fit) on synthetic unit-norm features
at 328 x 256, 2048 x 1024 and 9164 x 1024 -- class sizes falling as a power of the rank (tools/same_photo_split_time.py's profile), one
centroid per identity plus noise, the faces of an identity not neighbours -- at the clustering study's bandwidth 0.7:

  * the device-event time of the whole fit, the minimum of REPS repetitions, with its centres and n_iter;
  * per iteration the seeds active in it and its milliseconds.  The library does not time itself: the fit is run with max_iter = 0, 1, ..
    n_iter, each the minimum of REPS repetitions; run t stops every seed after iteration t, so its info[3] (seeds stopped by max_iter)
    is the number of seeds active in iteration t + 1, and an iteration's time is the difference of two runs (each run also holds the
    start and the finish, whose cost differs a little from run to run with the means they order: the first row holds them);
  * ONE sklearn.cluster.MeanShift(bandwidth=0.7).fit(X) on the host, in a process of its own under a time limit; where it does not end
    inside it the record says "not finished in N s", and a larger size is then not attempted.

Each size runs in a child process of its own under `timeout -k 10`; a section that fails or runs out of time ends the run.
usage: python tools/mean_shift_time.py [--out FILE] [--limit SECONDS_PER_SECTION] [--host-limit SECONDS]"""
import argparse
import json
import os
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import numpy as np

from same_photo_split_time import class_sizes

REPS = 5
BANDWIDTH = 0.7
# name -> (faces, d, identities, the largest identity): the gallery's profile, scaled
SECTIONS = {"328x256": (328, 256, 60, 19), "2048x1024": (2048, 1024, 375, 118), "9164x1024": (9164, 1024, 1680, 530)}


def faces(name):
    n, d, classes, largest = SECTIONS[name]
    rs = np.random.RandomState(n)
    ident = np.repeat(np.arange(classes), class_sizes(n, classes, largest))
    cent = rs.standard_normal((classes, d)).astype(np.float32)
    cent /= np.linalg.norm(cent, axis=1, keepdims=True)
    X = cent[ident] + (0.45 / np.sqrt(d)) * rs.standard_normal((n, d)).astype(np.float32)
    X /= np.linalg.norm(X, axis=1, keepdims=True)
    return np.ascontiguousarray(X[rs.permutation(n)], dtype=np.float32)


def event_min(fn):
    import torch
    fn()
    out = []
    for _ in range(REPS):
        start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        start.record()
        fn()
        end.record()
        torch.cuda.synchronize()
        out.append(start.elapsed_time(end))
    return min(out)


def device_section(name):
    import torch
    from hse_facerec_tf_amd import _lib, ops
    x = torch.from_numpy(faces(name)).cuda()
    n, d = x.shape
    ws = torch.empty((_lib.shift_lib().hsefr_shift_workspace_bytes(n, d),), dtype=torch.uint8, device="cuda")
    centers, intensity, labels, dist, info = ops.mean_shift_fit(x, BANDWIDTH, workspace=ws)
    whole = event_min(lambda: ops.mean_shift_fit(x, BANDWIDTH, workspace=ws))
    rows, active = [], n
    for t in range(info["n_iter"] + 1):
        words = ops.mean_shift_fit(x, BANDWIDTH, max_iter=t, workspace=ws)[4]
        rows.append(dict(iteration=t, active=active, ms=event_min(lambda: ops.mean_shift_fit(x, BANDWIDTH, max_iter=t, workspace=ws))))
        active = words["max_iter"]
    print(name, "fit %.3f ms, n_iter %d, centres %d" % (whole, info["n_iter"], info["centers"]), flush=True)
    return dict(device=torch.cuda.get_device_name(0), n=n, d=d, ms=whole, info=info, rows=rows, workspace=ws.numel(),
                labels=labels.cpu().numpy().tolist(), left=active)


def host_section(name):
    from sklearn.cluster import MeanShift
    X = faces(name)
    t0 = time.perf_counter()
    ms = MeanShift(bandwidth=BANDWIDTH).fit(X)
    return dict(seconds=time.perf_counter() - t0, n_iter=int(ms.n_iter_), centers=len(ms.cluster_centers_), labels=ms.labels_.tolist())


def child(kind, name, limit, tmp):
    path = os.path.join(tmp, "%s_%s.json" % (kind, name))
    cmd = ["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__), "--" + kind, name, "--json", path]
    rc = subprocess.run(cmd).returncode
    if rc != 0:
        return rc, None
    with open(path) as f:
        return 0, json.load(f)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mean_shift_time.txt"))
    ap.add_argument("--limit", type=int, default=150, help="time limit of one size's device process, seconds")
    ap.add_argument("--host-limit", type=int, default=60, help="time limit of one size's scikit-learn fit, seconds")
    ap.add_argument("--device", choices=list(SECTIONS), help="(internal) run one size on the device in this process and write --json")
    ap.add_argument("--host", choices=list(SECTIONS), help="(internal) run one size's scikit-learn fit in this process and write --json")
    ap.add_argument("--json")
    args = ap.parse_args()
    if args.device or args.host:
        res = device_section(args.device) if args.device else host_section(args.host)
        with open(args.json, "w") as f:
            json.dump(res, f)
        return
    lines, unfinished = [], None
    with tempfile.TemporaryDirectory() as tmp:
        for name in SECTIONS:
            rc, r = child("device", name, args.limit, tmp)
            if rc != 0:
                sys.exit("size %s ended with status %d on the device: nothing written, nothing further run" % (name, rc))
            if not lines:
                lines += ["# Mean-shift clustering on the device (tools/mean_shift_time.py); %s, %s" % (r["device"], time.strftime("%Y-%m-%d")),
                          "# ops.mean_shift_fit(x, %.1f): hsefr_shift_fit, every face a seed, fp64; device events around the call, the minimum of %d"
                          % (BANDWIDTH, REPS),
                          "#   repetitions.  Per iteration: the seeds active in it, and the difference between the fits with max_iter = t and t - 1",
                          "#   (the first row is the fit with max_iter = 0: the start, one iteration of every seed and the finish).",
                          "#   host: ONE sklearn.cluster.MeanShift(bandwidth=%.1f).fit(X) in a process of its own, limit %d s" % (BANDWIDTH, args.host_limit)]
            info = r["info"]
            lines.append("# %s: %d faces x %d, %d centres of %d distinct means, n_iter %d, %d seed-iterations, workspace %.1f MB"
                         % (name, r["n"], r["d"], info["centers"], info["distinct"], info["n_iter"], info["work"], r["workspace"] / 1e6))
            lines.append("%-12s %14s" % ("fit", "%.3f ms" % r["ms"]))
            prev = 0.0
            for row in r["rows"]:
                lines.append("%-12s %14s   active seeds %6d   fit with max_iter=%d: %.3f ms"
                             % ("iteration %d" % row["iteration"], "%.3f ms" % (row["ms"] - prev), row["active"], row["iteration"], row["ms"]))
                prev = row["ms"]
            if r["left"]:
                lines.append("#   (%d seeds were still moving when the last run stopped them)" % r["left"])
            if unfinished:
                lines.append("%-12s %14s" % ("host", "not attempted: the %s fit did not finish in %d s" % (unfinished, args.host_limit)))
                continue
            rc, h = child("host", name, args.host_limit, tmp)
            if rc in (124, 137):
                unfinished = name
                lines.append("%-12s %14s" % ("host", "not finished in %d s" % args.host_limit))
            elif rc != 0:
                sys.exit("size %s ended with status %d on the host: nothing written" % (name, rc))
            else:
                same = h["labels"] == r["labels"] and h["n_iter"] == info["n_iter"] and h["centers"] == info["centers"]
                lines.append("%-12s %14s   n_iter %d, %d centres, labels %s the device's; host / device = %.0f"
                             % ("host", "%.2f s" % h["seconds"], h["n_iter"], h["centers"], "equal to" if same else "NOT equal to",
                                h["seconds"] * 1e3 / r["ms"]))
    text = "\n".join(lines) + "\n"
    with open(args.out, "w") as f:
        f.write(text)
    print(text)


if __name__ == "__main__":
    main()
