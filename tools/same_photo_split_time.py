#!/usr/bin/env python3
"""Wall time of clustering.cluster_faces(all_indices=..., split="device") -- the same-photo split of every cluster in one device pass
(libhsefr_split.so, ops.split_groups) -- against split="host", the split cluster by cluster in NumPy, on synthetic unit-norm features:

  gallery : 9164 x 1024 features of 1680 identities, class sizes falling as a power of the rank from 530 (synthetic, not LFW's real
            profile), about 5 % of the faces in one photo with another face of their identity
  album   : 129 faces of 6 identities with born / photo years, a dozen photos with two faces of one identity
  one     : ONE identity of 4096 faces, 5 % of them paired in photos: the longest sequential chain

Per section: cluster_faces both ways (wall, both sides end on the host), the split alone -- device events around ops.split_groups against
the wall time of clustering._split_groups on the same clusters -- and the call's counts (ops.SPLIT_STATS).

The host side is measured in the same process, never taken from a record: after a warm-up of both, REPS repetitions of each, alternating
(tools/mtcnn_ragged_time.py's method); per side the minimum and the median; `spread` is the larger of the two sides' max - min; a side
wins where the other's minimum exceeds its minimum by more than that spread.

The last line applies the rule of album.SPLIT_DEVICE_DEFAULT: True if the device side wins on the gallery and is not slower than the host
side by more than the spread on the album; otherwise False.

Each section runs in a child process of its own under `timeout -k 10`; a section that fails or runs out of time ends the run.
usage: python tools/same_photo_split_time.py [--out FILE] [--seconds S] [--limit SECONDS_PER_SECTION]"""
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

import mtcnn_ragged_time as base      # the alternation and the spread: one method for every record
from mixed_device_time import event_ms

REPS = base.REPS
SECTIONS = ("gallery", "album", "one")
THRESHOLD = 0.9                       # between the distances inside an identity (about 0.6) and between two (about 1.4)
D = 1024


def class_sizes(total, classes, largest):
    """`classes` sizes from `largest` down, falling as a power of the rank, summing to `total`."""
    lo, hi = 0.0, 4.0
    for _ in range(60):
        a = (lo + hi) / 2
        s = np.maximum(1, np.floor(largest * np.arange(1, classes + 1) ** -a)).astype(np.int64)
        lo, hi = (a, hi) if s.sum() > total else (lo, a)
    s = np.maximum(1, np.floor(largest * np.arange(1, classes + 1) ** -hi)).astype(np.int64)
    rest = total - int(s.sum())                        # what the floor left: one more face for the classes after the largest
    s[1:1 + rest] += 1
    assert s.sum() == total and s[0] == largest and len(s) == classes
    return s


def faces(sizes, seed, shared=0.05):
    """-> (X float32 [n, D] unit rows around one centroid per identity, identity of every face, photo of every face): every face in its
    own photo, except that about `shared` of the faces are in a photo with another face of their identity."""
    rs = np.random.RandomState(seed)
    ident = np.repeat(np.arange(len(sizes)), sizes)
    n = len(ident)
    cent = rs.standard_normal((len(sizes), D)).astype(np.float32)
    cent /= np.linalg.norm(cent, axis=1, keepdims=True)
    X = cent[ident] + (0.45 / np.sqrt(D)) * rs.standard_normal((n, D)).astype(np.float32)
    X /= np.linalg.norm(X, axis=1, keepdims=True)
    order = rs.permutation(n)                          # the faces of an identity are not neighbours in the album
    X, ident = np.ascontiguousarray(X[order]), ident[order]
    photo = np.arange(n)
    for c in np.flatnonzero(np.asarray(sizes) >= 2):
        m = rs.permutation(np.flatnonzero(ident == c))
        pairs = rs.binomial(len(m) // 2, shared)
        for a, b in zip(m[:pairs], m[pairs:2 * pairs]):
            photo[b] = photo[a]
    return X, ident, photo


def section(name, seconds):
    import torch
    from hse_facerec_tf_amd import clustering, ops
    born = year = None
    if name == "gallery":
        X, ident, photo = faces(class_sizes(9164, 1680, 530), 1)
    elif name == "album":
        X, ident, photo = faces([40, 30, 25, 20, 10, 4], 2, shared=0.2)
        born = 1950.0 + 11 * ident + np.random.RandomState(3).rand(len(ident))
        year = np.full(len(ident), 2019.0)
    else:
        X, ident, photo = faces([4096], 4)
    n = len(ident)
    kw = dict(born_years=born, photo_years=year, all_indices=photo)
    new = lambda: clustering.cluster_faces(X, THRESHOLD, split="device", **kw)      # noqa: E731
    old = lambda: clustering.cluster_faces(X, THRESHOLD, split="host", **kw)        # noqa: E731
    got, want = new(), old()
    same = got == want
    tn, to, calls = base.alternated(new, old, seconds)
    rows = [dict(what="cluster_faces", new=tn, old=to, calls=calls)]
    print(name, "cluster_faces device min %.2f host min %.2f ms, same clusters: %s" % (min(tn), min(to), same), flush=True)
    # the split alone, on the clusters the linkage gives
    x, bt, yt = clustering._features(X, born, year, None, finite=False)
    by, yr = clustering._age_arrays(born, year, n)
    labels = clustering.fcluster_distance(clustering.linkage_single(x, by, yr), THRESHOLD)
    groups = clustering._groups(labels)
    members, offsets = clustering.group_table(labels)
    mt = torch.from_numpy(members).cuda()
    pt = torch.from_numpy(np.unique(photo, return_inverse=True)[1].reshape(-1).astype(np.int32)).cuda()
    split = lambda **k: ops.split_groups(mt, offsets, pt, x=x, born=bt, year=yt, penalty=clustering.SAME_PHOTO_PENALTY,      # noqa: E731
                                         cut=clustering.SAME_PHOTO_PENALTY / 2, **k)
    stats = split(return_stats=True)[1]
    dev_ms = [event_ms(split, 5) for _ in range(REPS)]

    def sub_dist(g):                                   # cluster_faces' own, written out: the host side's G launches and read-backs
        rows_g = x[torch.from_numpy(g).to(x.device)].contiguous()
        Dg = ops.pairwise_distances(rows_g).cpu().numpy().astype(np.float64)
        if by is not None:
            b, y = by[g], yr[g]
            max_year = np.maximum(y[:, None], y[None, :])
            ai, aj = max_year - b[:, None], max_year - b[None, :]
            Dg = Dg + 0.1 * (ai - aj) ** 2 / (ai + aj)
        return np.clip(Dg, 0, None)
    host_ms = []
    for _ in range(REPS):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        clustering._split_groups(groups, photo, n, sub_dist)
        host_ms.append((time.perf_counter() - t0) * 1e3)
    rows.append(dict(what="the split alone", new=dev_ms, old=host_ms, calls=[5, 1]))
    print(name, "split alone device min %.3f host min %.2f ms, stats %s" % (min(dev_ms), min(host_ms), stats.tolist()), flush=True)
    sizes = np.diff(offsets)
    return dict(device=torch.cuda.get_device_name(0), rows=rows, stats=[int(v) for v in stats], same=bool(same), faces=n, clusters=len(sizes),
                largest=int(sizes.max()), after=len(want), shared=int(n - len(np.unique(photo))))


TITLES = {"gallery": "(a) gallery: 9164 x 1024 features of 1680 identities, largest 530",
          "album": "(b) album: 129 faces of 6 identities, with the age term",
          "one": "(c) one identity of 4096 faces: the longest chain"}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "same_photo_split_time.txt"))
    ap.add_argument("--seconds", type=float, default=0.3, help="wall time one repetition of one side is sized to")
    ap.add_argument("--limit", type=int, default=200, help="time limit of one section's process, seconds")
    ap.add_argument("--section", choices=SECTIONS, help="(internal) run one section in this process and write --json")
    ap.add_argument("--json")
    args = ap.parse_args()
    if args.section:
        res = section(args.section, args.seconds)
        with open(args.json, "w") as f:
            json.dump(res, f)
        return
    results = {}
    with tempfile.TemporaryDirectory() as tmp:
        for name in SECTIONS:
            path = os.path.join(tmp, name + ".json")
            cmd = ["timeout", "-k", "10", str(args.limit), sys.executable, os.path.abspath(__file__), "--section", name, "--json", path,
                   "--seconds", str(args.seconds)]
            rc = subprocess.run(cmd).returncode
            if rc != 0:
                sys.exit("section %s ended with status %d: nothing written, nothing further run" % (name, rc))
            with open(path) as f:
                results[name] = json.load(f)
    lines = ["# The same-photo split of every cluster in one device pass (tools/same_photo_split_time.py); %s, %s"
             % (results["gallery"]["device"], time.strftime("%Y-%m-%d")),
             "# device: clustering.cluster_faces(X, %.2f, all_indices=photos, split=\"device\") -- one ops.split_groups call for all clusters;" % THRESHOLD,
             "#   host: the same call with split=\"host\" (the default) -- one distance launch, one read-back and one NumPy chain per cluster.",
             "#   ms (wall) per call, %d repetitions of each side, alternating; 'the split alone': device events around ops.split_groups against" % REPS,
             "#   the wall time of clustering._split_groups on the same clusters.  ratio = host_min / device_min; spread = the larger of the two",
             "#   sides' max - min; faster = the side whose minimum is below the other's by more than the spread, '-' where neither is"]
    verdict = {}
    for name in SECTIONS:
        r = results[name]
        lines.append("# %s: %d faces in %d clusters (largest %d), %d faces share a photo with an earlier one, %d clusters after the split; "
                     "the two sides' clusters are %s" % (TITLES[name], r["faces"], r["clusters"], r["largest"], r["shared"], r["after"],
                                                         "the same" if r["same"] else "NOT the same"))
        lines.append("%-18s %12s %12s %12s %12s %10s %8s %7s %7s" % ("", "device_min", "device_med", "host_min", "host_med", "spread", "ratio", "faster",
                                                                     "calls"))
        for row in r["rows"]:
            tn, to, spread = row["new"], row["old"], base.spread_of(row)
            faster = "device" if min(to) - min(tn) > spread else ("host" if min(tn) - min(to) > spread else "-")
            lines.append("%-18s %12.3f %12.3f %12.3f %12.3f %10.3f %8.2f %7s %7s" % (row["what"], min(tn), float(np.median(tn)), min(to),
                                                                                     float(np.median(to)), spread, min(to) / min(tn), faster,
                                                                                     "%d/%d" % tuple(row["calls"])))
            if row["what"] == "cluster_faces":
                verdict[name] = (min(to) - min(tn) > spread, min(tn) - min(to) <= spread)
        lines.append("#   stats: " + ", ".join("%s %d" % (k, v) for k, v in zip(("answered without a chain", "chains in LDS", "chains on the slab",
                                                                                   "merges", "members out of range"), r["stats"])))
    wins, not_slower = verdict["gallery"][0], verdict["album"][1]
    lines.append("# rule: album.SPLIT_DEVICE_DEFAULT = %s  (split=\"device\" faster than split=\"host\" by more than the spread on the gallery: %s; "
                 "not slower by more than the spread on the album: %s)" % (wins and not_slower, "yes" if wins else "no", "yes" if not_slower else "no"))
    text = "\n".join(lines) + "\n"
    with open(args.out, "w") as f:
        f.write(text)
    print(text)


if __name__ == "__main__":
    main()
