#!/usr/bin/env python3
"""Device time of affinity-propagation clustering (hsefr_affinity_fit, libhsefr_affinity.so, through ops.affinity_propagation_fit) on
the synthetic unit-norm features of tools/mean_shift_time.py at 328 x 256, 2048 x 1024 and 9164 x 1024, scikit-learn's defaults
(damping 0.5, max_iter 200, convergence_iter 15, the median preference), noise seed 0:

  * the device-event time of the whole fit, the minimum of REPS repetitions, with its clusters and n_iter;
  * milliseconds per iteration: (the fit - the fit with max_iter = 1) / (n_iter - 1), both the minimum of REPS repetitions -- the start
    (similarities, median, noise) and the finish are in both;
  * the bytes an iteration must move, 5 n^2 x 8 (A, R and S read, A and R written), over that time, as a share of the MI355X's HBM3E rates:
    8.0 TB/s peak, 6.3 TB/s achievable (measured with a float4 copy);
  * ONE sklearn.cluster.AffinityPropagation(random_state=0).fit(X.astype(float64)) on the host, in a process of its own under a time
    limit, and whether its partition, n_iter_ and cluster count are the device's; the last line is the share of equal partitions.

With --alternative LIB every size is also run on another build of the library (HSEFR_AFFINITY_LIB), for the schedule that lost: the
same kernel with the row's similarities read again in sweep 2 instead of kept in LDS, built beside the product with
    hipcc $(bash hse_facerec_tf_amd/csrc/build.sh --list | grep '^name=affinity' | tr '\t' '\n' | sed -n 's/^flags=//p') \
          -DHSEFR_AFFINITY_ROW_IN_LDS=0 -shared hse_facerec_tf_amd/csrc/affinity.hip -o LIB

Each size runs in a child process of its own under `timeout -k 10`; a section that fails or runs out of time ends the run.
usage: python tools/affinity_time.py [--out FILE] [--limit SECONDS_PER_SECTION] [--host-limit SECONDS] [--alternative LIB]"""
import argparse
import json
import os
import subprocess
import sys
import tempfile
import time
import warnings

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np

from mean_shift_time import REPS, SECTIONS, event_min, faces

HBM_PEAK, HBM_ACHIEVABLE = 8.0e12, 6.3e12
# written before the first run on the device: what the schedule should cost if an iteration is its five n^2 sweeps and nothing else
ESTIMATE = ("# estimate before measuring: an iteration is 5 n^2 x 8 bytes -- 3.36 GB at 9164 faces, 0.53 ms at the achievable 6.3 TB/s; with a\n"
            "#   barrier pair per row, two workgroups a CU and the partial sums, 0.8 - 1.2 ms (45 - 65 %) was expected.  At 2048 faces the three\n"
            "#   matrices (101 MB) lie in the Infinity Cache and at 328 in L2: there an iteration is its three launches and the host's read,\n"
            "#   40 - 100 us, whatever the bytes.")


def partition(labels):
    import affinity_ref
    return affinity_ref.first_occurrence(np.asarray(labels)).tolist()


def device_section(name):
    import torch
    from hse_facerec_tf_amd import _lib, ops
    x = torch.from_numpy(faces(name)).cuda()
    n, d = x.shape
    ws = torch.empty((_lib.affinity_lib().hsefr_affinity_workspace_bytes(n, d),), dtype=torch.uint8, device="cuda")
    exemplars, labels, diag, pref, info = ops.affinity_propagation_fit(x=x, workspace=ws)
    whole = event_min(lambda: ops.affinity_propagation_fit(x=x, workspace=ws))
    first = event_min(lambda: ops.affinity_propagation_fit(x=x, max_iter=1, workspace=ws))
    print(name, "fit %.3f ms, n_iter %d, clusters %d" % (whole, info["n_iter"], info["clusters"]), flush=True)
    return dict(device=torch.cuda.get_device_name(0), n=n, d=d, ms=whole, first=first, info=info, preference=pref, workspace=ws.numel(),
                partition=partition(labels.cpu().numpy()))


def host_section(name):
    from sklearn.cluster import AffinityPropagation
    X = faces(name).astype(np.float64)
    t0 = time.perf_counter()
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        ap = AffinityPropagation(random_state=0).fit(X)
    return dict(seconds=time.perf_counter() - t0, n_iter=int(ap.n_iter_), clusters=len(ap.cluster_centers_indices_),
                partition=partition(ap.labels_))


def child(kind, name, limit, tmp, library=None):
    path = os.path.join(tmp, "%s_%s%s.json" % (kind, name, "_alt" if library else ""))
    cmd = ["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__), "--" + kind, name, "--json", path]
    rc = subprocess.run(cmd, env=dict(os.environ, HSEFR_AFFINITY_LIB=os.path.abspath(library)) if library else None).returncode
    if rc != 0:
        return rc, None
    with open(path) as f:
        return 0, json.load(f)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "affinity_time.txt"))
    ap.add_argument("--limit", type=int, default=150, help="time limit of one size's device process, seconds")
    ap.add_argument("--host-limit", type=int, default=120, help="time limit of one size's scikit-learn fit, seconds")
    ap.add_argument("--alternative", help="another build of libhsefr_affinity.so to time beside the product (see above)")
    ap.add_argument("--device", choices=list(SECTIONS), help="(internal) run one size on the device in this process and write --json")
    ap.add_argument("--host", choices=list(SECTIONS), help="(internal) run one size's scikit-learn fit in this process and write --json")
    ap.add_argument("--json")
    args = ap.parse_args()
    if args.device or args.host:
        res = device_section(args.device) if args.device else host_section(args.host)
        with open(args.json, "w") as f:
            json.dump(res, f)
        return
    lines, unfinished, compared, equal = [], None, 0, 0
    with tempfile.TemporaryDirectory() as tmp:
        for name in SECTIONS:
            rc, r = child("device", name, args.limit, tmp)
            if rc != 0:
                sys.exit("size %s ended with status %d on the device: nothing written, nothing further run" % (name, rc))
            if not lines:
                lines += ["# Affinity-propagation clustering on the device (tools/affinity_time.py); %s, %s" % (r["device"], time.strftime("%Y-%m-%d")),
                          "# ops.affinity_propagation_fit(x): hsefr_affinity_fit, scikit-learn's defaults, noise seed 0, fp64; device events around the",
                          "#   call, the minimum of %d repetitions.  per iteration = (fit - fit with max_iter=1) / (n_iter - 1); an iteration moves" % REPS,
                          "#   5 n^2 x 8 bytes (A, R, S read; A, R written): its share of the HBM's 8.0 TB/s peak and 6.3 TB/s achievable rate.",
                          "#   host: ONE sklearn.cluster.AffinityPropagation(random_state=0).fit(X.astype(float64)) in a process of its own, limit %d s"
                          % args.host_limit, ESTIMATE]
            info = r["info"]
            per = (r["ms"] - r["first"]) / max(info["n_iter"] - 1, 1)
            moved = 5.0 * r["n"] * r["n"] * 8
            rate = moved / (per * 1e-3)
            lines.append("# %s: %d faces x %d, %d clusters, n_iter %d, converged %d, preference %.6f, workspace %.1f MB"
                         % (name, r["n"], r["d"], info["clusters"], info["n_iter"], info["converged"], r["preference"], r["workspace"] / 1e6))
            lines.append("%-14s %12s   fit with max_iter=1 (start, one iteration, finish): %.3f ms" % ("fit", "%.3f ms" % r["ms"], r["first"]))
            lines.append("%-14s %12s   %.1f MB an iteration, %.2f TB/s: %.0f %% of the peak, %.0f %% of the achievable rate"
                         % ("per iteration", "%.4f ms" % per, moved / 1e6, rate / 1e12, 100 * rate / HBM_PEAK, 100 * rate / HBM_ACHIEVABLE))
            if args.alternative:
                rc, a = child("device", name, args.limit, tmp, args.alternative)
                if rc != 0:
                    sys.exit("size %s ended with status %d on the alternative build: nothing written, nothing further run" % (name, rc))
                a_per = (a["ms"] - a["first"]) / max(a["info"]["n_iter"] - 1, 1)
                lines.append("%-14s %12s   S read again in sweep 2, no LDS row: fit %.3f ms, n_iter %d, partition %s the product's"
                             % ("alternative", "%.4f ms" % a_per, a["ms"], a["info"]["n_iter"],
                                "equal to" if a["partition"] == r["partition"] else "NOT equal to"))
            if unfinished:
                lines.append("%-14s %12s" % ("host", "not attempted: the %s fit did not finish in %d s" % (unfinished, args.host_limit)))
                continue
            rc, h = child("host", name, args.host_limit, tmp)
            if rc in (124, 137):
                unfinished = name
                lines.append("%-14s %12s" % ("host", "not finished in %d s" % args.host_limit))
            elif rc != 0:
                sys.exit("size %s ended with status %d on the host: nothing written" % (name, rc))
            else:
                same = h["partition"] == r["partition"]
                compared += 1
                equal += int(same)
                lines.append("%-14s %12s   n_iter %d, %d clusters; partition %s the device's, n_iter %s, clusters %s; host / device = %.0f"
                             % ("host", "%.2f s" % h["seconds"], h["n_iter"], h["clusters"], "equal to" if same else "NOT equal to",
                                "equal" if h["n_iter"] == info["n_iter"] else "NOT equal", "equal" if h["clusters"] == info["clusters"] else "NOT equal",
                                h["seconds"] * 1e3 / r["ms"]))
    lines.append("# equal partitions: %d of the %d sizes scikit-learn finished" % (equal, compared))
    text = "\n".join(lines) + "\n"
    with open(args.out, "w") as f:
        f.write(text)
    print(text)


if __name__ == "__main__":
    main()
