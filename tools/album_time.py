#!/usr/bin/env python3
"""Wall time of the album organiser's device path against the paths it replaces, on the reference photo (tests/golden/test_image.jpg,
784 x 588) and same-size variants of it:

  crops : FacialImageProcessing.process_images(frames, max_frames=B, device_crops=True)   against   the same call with
          device_crops=False (the host crops: the yardstick), at B = 1, 2, 8, 16, 32 frames per call; next to them the detector alone
          (detect_batch on the RGB frames) and the BGR -> RGB copy alone, which say where a frame's time goes;
          and the same call with device_frames=True (the frames uploaded as decoded, converted on the device)   against   the
          device_crops=True side, with the np.stack of the raw frames alone next to them
  album : album.process_album on a 64-photo album (every fourth photo stored a quarter turn off, every eighth blank)   against   the
          loop a user stitches by hand from process_image, the rotation retries, cluster_faces, the filters and the summaries;
          and with device_frames=True   against   device_frames=False
  kernel: hsefr_frames_prepare alone on 16 frames of that size at each rotation, by device events
The last line is the rule for album.DEVICE_FRAMES_DEFAULT applied to these numbers.

All sides of a section run in ONE process: after a warm-up of each, REPS repetitions of each, alternating; a repetition is as many calls
as fill --seconds, timed with a host clock (every side ends in a device-to-host copy of its results, so the clock sees finished work).
Per side the minimum and the median of the repetitions; `spread` is the largest max - min among the sides of a row.

Each section runs in a child process of its own under `timeout -k 10`; a section that fails or runs out of time ends the run.
usage: python tools/album_time.py [--out FILE] [--seconds S] [--limit SECONDS_PER_SECTION]"""
import argparse
import calendar
import json
import os
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np

from mtcnn_batch_time import make_frames, wall_ms

BATCHES = [1, 2, 8, 16, 32]
ALBUM_PHOTOS = 64
REPS = 5
KERNEL_REPS = 30


def alternated(sides, seconds):
    """sides: [callable] -> (ms per call of each repetition, per side; calls per repetition, per side)."""
    for f in sides:                                  # warm-up: every shape the timed window uses, code objects, work tensors
        f()
        f()
    calls = [max(2, int(seconds * 1e3 / max(wall_ms(f, 2), 1e-3))) for f in sides]
    times = [[] for _ in sides]
    for _ in range(REPS):
        for t, f, c in zip(times, sides, calls):
            t.append(wall_ms(f, c))
    return times, calls


def sequential_album(fip, photos, mdates, config):
    """The album organiser stitched by hand from the calls the package had before album.py (process_photos.py:238-346)."""
    import torch
    from hse_facerec_tf_amd import album, clustering, ops, preprocess

    def one(draw):
        bboxes, _, ages, genders, feats = fip.process_image(draw)
        rgb = draw[..., ::-1]
        images = [preprocess.resize_linear_u8(rgb[y1:y2, x1:x2], 224, 224) for (x1, y1, x2, y2) in bboxes]
        return images, ages, genders, feats, album.has_center_face(bboxes, draw.shape[1], config)
    images, genders, feats, born, all_indices, private = [], [], [], [], [], []
    for i, photo in enumerate(photos):
        r = one(photo)
        if not r[0]:
            r = one(np.ascontiguousarray(np.rot90(photo, -1)))
            if not r[0]:
                r = one(np.ascontiguousarray(np.rot90(photo, 1)))
        if r[4]:
            private.append(i)
        images.extend(r[0])
        genders.extend(float(g[0]) for g in r[2])
        feats.extend(r[3])
        all_indices.extend([i] * len(r[1]))
        year = mdates[i].tm_year + (mdates[i].tm_mon - 1) / 12
        born.extend(year - (a - 0.5) for a in r[1])
    x = ops.l2_normalize(torch.from_numpy(np.stack(feats)).cuda())
    clusters = clustering.cluster_faces(x, config.distance_threshold, born_years=born, photo_years=[mdates[i].tm_year for i in all_indices],
                                        all_indices=all_indices, min_cluster_size=config.min_photos)
    posix = [calendar.timegm(m) for m in mdates]
    clusters = [c for c in clusters
                if (max(posix[all_indices[i]] for i in c) - min(posix[all_indices[i]] for i in c)) // 86400 >= config.min_days_difference]
    summary = album.summarize_clusters(clusters, genders, born, feats)
    return clusters, summary, album.split_private_public(clusters, all_indices, private, len(photos)), images


def section(name, seconds):
    import torch
    from hse_facerec_tf_amd import FacialImageProcessing, album
    fip = FacialImageProcessing(mtcnn_detector=True, minsize=32, latency_plan=False)
    rows = []
    if name == "crops":
        rgb = make_frames(max(BATCHES))
        bgr = [np.ascontiguousarray(f[..., ::-1]) for f in rgb]           # BGR, as cv2.imread gives them
        for b in BATCHES:
            fs, fr = bgr[:b], rgb[:b]
            sides = [lambda: fip.process_images(fs, max_frames=b, device_crops=True),
                     lambda: fip.process_images(fs, max_frames=b),
                     lambda: fip.detector.detect_batch(fr, max_frames=b),
                     lambda: [fip._bgr_to_rgb(f) for f in fs],
                     lambda: fip.process_images(fs, max_frames=b, device_frames=True),
                     lambda: np.stack(fs)]
            faces = sum(len(r[0]) for r in sides[0]())
            assert faces == sum(len(r[0]) for r in sides[1]()) == sum(len(r[0]) for r in sides[4]())
            times, calls = alternated(sides, seconds)
            rows.append(dict(b=b, faces=faces, calls=calls, times=[[t / b for t in side] for side in times]))
            print(name, b, "frames min %.3f device min %.3f host min %.3f ms/frame"
                  % (min(rows[-1]["times"][4]), min(rows[-1]["times"][0]), min(rows[-1]["times"][1])), flush=True)
    elif name == "kernel":
        # the launch alone, by device events: 16 frames of the photo's size, each rotation, out of place and (rotation 0) in place
        from hse_facerec_tf_amd import preprocess_device
        n, (h, w) = 16, make_frames(1)[0].shape[:2]
        src = torch.randint(0, 256, (n, h, w, 3), dtype=torch.uint8, device="cuda")
        for rotation, in_place in ((0, False), (0, True), (90, False), (270, False)):
            work = src.clone()
            out = work if in_place else torch.empty((n, h, w, 3) if rotation == 0 else (n, w, h, 3), dtype=torch.uint8, device="cuda")
            for _ in range(5):
                preprocess_device.prepare_frames(work, rotation, True, out=out)
            ms = []
            for _ in range(KERNEL_REPS):
                a, z = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                preprocess_device.prepare_frames(work, rotation, True, out=out)
                z.record()
                z.synchronize()
                ms.append(a.elapsed_time(z))
            rows.append(dict(rotation=rotation, in_place=in_place, n=n, h=h, w=w, bytes=2 * n * h * w * 3, ms=ms))
            print(name, rotation, "in place" if in_place else "", "min %.4f ms" % min(ms), flush=True)
    else:
        base = make_frames(ALBUM_PHOTOS)
        photos = []
        for i, f in enumerate(base):
            f = np.zeros_like(f) if i % 8 == 7 else (np.rot90(f, 1) if i % 4 == 1 else f)
            photos.append(np.ascontiguousarray(f[..., ::-1]))
        mdates = [time.gmtime(1551693600 + i * 11 * 3600) for i in range(ALBUM_PHOTOS)]
        config = album.AlbumConfig()
        sides = [lambda: album.process_album(fip, photos, mdates, config=config, device_crops=True, device_frames=False),
                 lambda: album.process_album(fip, photos, mdates, config=config, device_crops=False, device_frames=False),
                 lambda: sequential_album(fip, photos, mdates, config),
                 lambda: album.process_album(fip, photos, mdates, config=config, device_frames=True)]
        got, want = sides[0](), sides[2]()
        assert got.clusters == want[0] and (got.private_photos, got.public_photos) == want[2], "the two albums differ"
        third = sides[3]()
        assert (third.clusters, third.all_indices, third.private_photos, third.public_photos) == \
            (got.clusters, got.all_indices, got.private_photos, got.public_photos), "the device-frames album differs"
        times, calls = alternated(sides, seconds)
        rows.append(dict(b=ALBUM_PHOTOS, faces=len(got.all_indices), clusters=len(got.clusters), calls=calls, times=times))
    return dict(device=torch.cuda.get_device_name(0), host_fallbacks=int(fip.detector.host_fallbacks), rows=rows)


def stats(side):
    return min(side), float(np.median(side))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "album_time.txt"))
    ap.add_argument("--seconds", type=float, default=0.3, help="wall time one repetition of one side is sized to")
    ap.add_argument("--limit", type=int, default=240, help="time limit of one section's process, seconds")
    ap.add_argument("--section", choices=["crops", "album", "kernel"], help="(internal) run one section in this process and write --json")
    ap.add_argument("--json")
    args = ap.parse_args()
    if args.section:
        res = section(args.section, args.seconds)
        with open(args.json, "w") as f:
            json.dump(res, f)
        return
    results = {}
    with tempfile.TemporaryDirectory() as tmp:
        for name in ("crops", "album", "kernel"):
            path = os.path.join(tmp, name + ".json")
            cmd = ["timeout", "-k", "10", str(args.limit), sys.executable, os.path.abspath(__file__), "--section", name, "--json", path,
                   "--seconds", str(args.seconds)]
            rc = subprocess.run(cmd).returncode
            if rc != 0:
                sys.exit("section %s ended with status %d: nothing written, nothing further run" % (name, rc))
            with open(path) as f:
                results[name] = json.load(f)
    lines = ["# the album organiser's device path against the paths it replaces (tools/album_time.py); %s, %s"
             % (results["crops"]["device"], time.strftime("%Y-%m-%d")),
             "# frames: tests/golden/test_image.jpg (784 x 588, 4 faces) and same-size variants (mirrored, upside down, dimmed, shifted)",
             "# %d repetitions of each side, alternating in one process; min / median over the repetitions; spread = the largest max - min" % REPS,
             "#   among the sides of a row; calls = calls per repetition of each side",
             "# crops: process_images(frames, max_frames=B) with device_crops=True (device) and False (host: the yardstick), ms per FRAME;",
             "#   detect = detect_batch alone on the RGB frames, bgr2rgb = the channel copy alone; slower = device_min - host_min > spread.",
             "#   At B = 1 the frame takes the single-frame call and both sides cut it on the host: the row shows the bookkeeping alone",
             "%3s %6s %11s %11s %10s %10s %11s %12s %8s %7s %7s %15s"
             % ("B", "faces", "device_min", "device_med", "host_min", "host_med", "detect_min", "bgr2rgb_min", "spread", "ratio", "slower", "calls")]
    for r in results["crops"]["rows"]:
        dev, host, det, copy = r["times"][:4]
        spread = max(max(s) - min(s) for s in (dev, host))
        lines.append("%3d %6d %11.3f %11.3f %10.3f %10.3f %11.3f %12.3f %8.3f %7.2f %7s %15s"
                     % (r["b"], r["faces"], *stats(dev), *stats(host), min(det), min(copy), spread, min(host) / min(dev),
                        "yes" if min(dev) - min(host) > spread else "no", "/".join(str(c) for c in r["calls"][:4])))
    lines += ["# frames: the same call with device_frames=True (frames) against the device_crops=True side above (device: the parent path), ms per",
              "#   FRAME; stack = np.stack of the raw frames alone (the host work device_frames keeps); spread = the largest max - min of the",
              "#   two sides; faster = device_min - frames_min > spread.  At B = 1 the frame is alone in its group: the host path on both sides",
              "%3s %11s %11s %11s %11s %10s %8s %7s %7s %9s"
              % ("B", "frames_min", "frames_med", "device_min", "device_med", "stack_min", "spread", "ratio", "faster", "calls")]
    faster_at = {}
    for r in results["crops"]["rows"]:
        dev, fra, stk = r["times"][0], r["times"][4], r["times"][5]
        spread = max(max(s) - min(s) for s in (dev, fra))
        faster_at[r["b"]] = min(dev) - min(fra) > spread
        lines.append("%3d %11.3f %11.3f %11.3f %11.3f %10.3f %8.3f %7.2f %7s %9s"
                     % (r["b"], *stats(fra), *stats(dev), min(stk), spread, min(dev) / min(fra), "yes" if faster_at[r["b"]] else "no",
                        "%d/%d" % (r["calls"][4], r["calls"][0])))
    lines.append("# frames redone on the host in this section: %d" % results["crops"]["host_fallbacks"])
    r = results["album"]["rows"][0]
    dev, host, loop, fra = r["times"]
    lines += ["# album: process_album on %d photos (every fourth a quarter turn off: found in the retry pass; every eighth blank: all three passes),"
              % r["b"],
              "#   %d faces, %d clusters, ms per ALBUM; loop = process_image per photo, the retries, cluster_faces, filters and summaries by hand"
              % (r["faces"], r["clusters"]),
              "%12s %12s %10s %10s %10s %10s %8s %11s %9s"
              % ("device_min", "device_med", "host_min", "host_med", "loop_min", "loop_med", "spread", "loop/device", "calls"),
              "%12.1f %12.1f %10.1f %10.1f %10.1f %10.1f %8.1f %11.2f %9s"
              % (*stats(dev), *stats(host), *stats(loop), max(max(s) - min(s) for s in (dev, host, loop)), min(loop) / min(dev),
                 "/".join(str(c) for c in r["calls"][:3])),
              "# the same album with device_frames=True (frames) against device_frames=False (device, the columns above); slower = frames_min -",
              "#   device_min > spread of the two",
              "%12s %12s %8s %7s %7s %6s" % ("frames_min", "frames_med", "spread", "ratio", "slower", "calls")]
    album_spread = max(max(s) - min(s) for s in (dev, fra))
    album_slower = min(fra) - min(dev) > album_spread
    lines += ["%12.1f %12.1f %8.1f %7.2f %7s %6d" % (*stats(fra), album_spread, min(dev) / min(fra), "yes" if album_slower else "no", r["calls"][3]),
              "# frames redone on the host in this section: %d" % results["album"]["host_fallbacks"],
              "# kernel: hsefr_frames_prepare alone, %d frames of %d x %d, swap_rb = 1, device events around one launch, %d launches each;"
              % (results["kernel"]["rows"][0]["n"], results["kernel"]["rows"][0]["w"], results["kernel"]["rows"][0]["h"], KERNEL_REPS),
              "#   GB/s = bytes read + bytes written over the minimum (both stacks, 22 MB each, fit the Infinity Cache: not an HBM rate)",
              "%9s %9s %9s %9s %9s" % ("rotation", "in_place", "min_us", "med_us", "GB/s")]
    for k in results["kernel"]["rows"]:
        lines.append("%9d %9s %9.1f %9.1f %9.0f" % (k["rotation"], "yes" if k["in_place"] else "no", 1e3 * min(k["ms"]), 1e3 * float(np.median(k["ms"])),
                                                    k["bytes"] / (min(k["ms"]) * 1e-3) / 1e9))
    decided = all(faster_at[b] for b in (8, 16, 32)) and not album_slower
    lines.append("# album.DEVICE_FRAMES_DEFAULT: %s (rule: faster by more than the spread at B = 8, 16 and 32 -- %s -- and the album not slower by more"
                 " than its spread -- %s)" % (decided, "/".join("yes" if faster_at[b] else "no" for b in (8, 16, 32)), "no" if not album_slower else "yes: slower"))
    text = "\n".join(lines) + "\n"
    with open(args.out, "w") as f:
        f.write(text)
    print(text)


if __name__ == "__main__":
    main()
