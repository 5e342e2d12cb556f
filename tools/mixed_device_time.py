#!/usr/bin/env python3
"""Wall time of process_images / process_album with the device stages of the mixed-size passes (mixed_device=True: libhsefr_mixed.so,
preprocess_device.prepare_packed and face_crops_packed, MTCNNDetector.detect_packed) against the same calls without the flag, on the
cut-outs of tools/mtcnn_ragged_time.py (tests/golden/test_image.jpg, 784 x 588, every frame of a different size):

  rot0, rot90 : process_images(frames, mixed_sizes=True, device_frames=True, rotation=R, mixed_device=True) against the same call without
                mixed_device, at B = 2, 4, 8, 16, 32 frames per call
  album       : process_album on 64 photos of 64 different sizes (a quarter of them turned, an eighth empty), mixed_device=True against False
  launches    : the two launches alone, by device events: prepare_packed (rotation 0 in place, 90 and 270) and face_crops_packed on the
                32 frames, with the bytes they move per second.  Information only

The side without the flag is measured in the same process, never taken from a record: after a warm-up of both, REPS repetitions of each,
alternating; a repetition is as many calls as fill --seconds, timed with a host clock (both sides end in a device-to-host copy of their
results).  Per side the minimum and the median of the repetitions; `spread` is the larger of the two sides' max - min; a side wins where
the other's minimum exceeds its minimum by more than that spread.

The last line of the output applies the rule of album.MIXED_DEVICE_DEFAULT: True if mixed_device wins at 4, 8 and 16 frames per call at
both rotations and its album is not slower by more than the album's spread; otherwise False.

Each section runs in a child process of its own under `timeout -k 10`; a section that fails or runs out of time ends the run.
usage: python tools/mixed_device_time.py [--out FILE] [--seconds S] [--limit SECONDS_PER_SECTION]"""
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

import mtcnn_ragged_time as base      # the frames, the alternation and the spread: one method for both records

BATCHES = base.MIXED_BATCHES
RULE_BATCHES = base.RULE_BATCHES
ALBUM_PHOTOS = base.ALBUM_PHOTOS
REPS = base.REPS
SECTIONS = ("rot0", "rot90", "album", "launches")


def same_results(got, want):
    return len(got) == len(want) and all(g[0] == w[0] and np.array_equal(np.asarray(g[1]), np.asarray(w[1])) and g[2] == w[2]
                                         and all(np.array_equal(a, b) for k in (3, 4) for a, b in zip(g[k], w[k])) for g, w in zip(got, want))


def event_ms(fn, calls):
    import torch
    fn()
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    start.record()
    for _ in range(calls):
        fn()
    end.record()
    torch.cuda.synchronize()
    return start.elapsed_time(end) / calls


def section(name, seconds):
    import torch
    from hse_facerec_tf_amd import FacialImageProcessing, album, preprocess_device
    fip = FacialImageProcessing(mtcnn_detector=True, minsize=32, latency_plan=False)
    det = fip.detector
    rows = []
    if name in ("rot0", "rot90"):
        rotation = 0 if name == "rot0" else 90
        frames = [np.ascontiguousarray(f[..., ::-1]) for f in base.mixed_frames(max(BATCHES))]       # BGR, as cv2.imread gives them
        for b in BATCHES:
            fs = frames[:b]
            new = lambda fs=fs: fip.process_images(fs, mixed_sizes=True, device_frames=True, rotation=rotation, mixed_device=True)      # noqa: E731
            old = lambda fs=fs: fip.process_images(fs, mixed_sizes=True, device_frames=True, rotation=rotation)                         # noqa: E731
            got, want = new(), old()
            assert same_results(got, want), "the two sides differ at %d frames, rotation %d" % (b, rotation)
            tn, to, calls = base.alternated(new, old, seconds)
            rows.append(dict(b=b, new=[t / b for t in tn], old=[t / b for t in to], calls=calls, faces=sum(len(r[0]) for r in want)))
            print(name, b, "new min %.3f old min %.3f ms/frame" % (min(rows[-1]["new"]), min(rows[-1]["old"])), flush=True)
    elif name == "album":
        photos = []
        for i, f in enumerate(base.mixed_frames(ALBUM_PHOTOS, step=(4, 6))):
            f = np.zeros_like(f) if i % 8 == 7 else (np.rot90(f, 1) if i % 4 == 1 else f)
            photos.append(np.ascontiguousarray(f[..., ::-1]))
        mdates = [time.gmtime(1551693600 + i * 11 * 3600) for i in range(ALBUM_PHOTOS)]
        config = album.AlbumConfig()
        new = lambda: album.process_album(fip, photos, mdates, config=config, mixed_sizes=True, mixed_device=True)       # noqa: E731
        old = lambda: album.process_album(fip, photos, mdates, config=config, mixed_sizes=True, mixed_device=False)      # noqa: E731
        got, want = new(), old()
        assert (got.clusters, got.all_indices, got.private_photos, got.public_photos) == \
            (want.clusters, want.all_indices, want.private_photos, want.public_photos), "the two albums differ"
        assert all(np.array_equal(a, b) for a, b in zip(got.facial_images, want.facial_images)), "the two albums' faces differ"
        tn, to, calls = base.alternated(new, old, seconds)
        rows.append(dict(b=ALBUM_PHOTOS, new=tn, old=to, calls=calls, faces=len(want.all_indices)))
        print(name, "new min %.1f old min %.1f ms/album" % (min(tn), min(to)), flush=True)
    else:
        frames = base.mixed_frames(max(BATCHES))
        shapes = [f.shape[:2] for f in frames]
        packed = torch.from_numpy(np.concatenate([f.reshape(-1) for f in frames])).cuda()
        out = torch.empty_like(packed)
        n_bytes = int(packed.shape[0])
        for what, fn in (("prepare_packed, rotation 0, in place", lambda: preprocess_device.prepare_packed(packed, shapes, 0, True, out=packed)),
                         ("prepare_packed, rotation 90", lambda: preprocess_device.prepare_packed(packed, shapes, 90, True, out=out)),
                         ("prepare_packed, rotation 270", lambda: preprocess_device.prepare_packed(packed, shapes, 270, True, out=out))):
            ms = [event_ms(fn, 50) for _ in range(REPS)]
            rows.append(dict(what=what, ms=ms, bytes=2 * n_bytes))
        boxes, rs = [], np.random.RandomState(0)
        for f, (h, w) in enumerate(shapes):                                                 # three faces of 120 to 260 pixels per frame
            for _ in range(3):
                s = int(rs.randint(120, 261))
                x, y = int(rs.randint(0, w - s + 1)), int(rs.randint(0, h - s + 1))
                boxes.append((f, x, y, x + s, y + s))
        faces = torch.empty((len(boxes), 224, 224, 3), dtype=torch.uint8, device="cuda")
        ms = [event_ms(lambda: preprocess_device.face_crops_packed(packed, shapes, boxes, (224, 224), out=faces), 50) for _ in range(REPS)]
        moved = int(faces.numel()) + sum((x2 - x1) * (y2 - y1) * 3 for _, x1, y1, x2, y2 in boxes)
        rows.append(dict(what="face_crops_packed, %d faces to 224 x 224" % len(boxes), ms=ms, bytes=moved))
        for r in rows:
            print(name, r["what"], "min %.4f ms" % min(r["ms"]), flush=True)
    res = dict(device=torch.cuda.get_device_name(0), host_fallbacks=int(det.host_fallbacks), ragged_passes=int(det.ragged_passes), rows=rows)
    fip.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mixed_device_time.txt"))
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
    lines = ["# The device stages of the mixed-size passes (tools/mixed_device_time.py); %s, %s" % (results["rot0"]["device"], time.strftime("%Y-%m-%d")),
             "# frames: cut-outs of tests/golden/test_image.jpg (784 x 588, 4 faces), every other one transposed, every one of a different size",
             "# device: process_images / process_album with mixed_sizes=True, device_frames=True AND mixed_device=True (a ragged pass's frames",
             "#   uploaded as decoded, turned and converted by one launch, its faces cut by one launch from that buffer);",
             "#   host: the same call without mixed_device -- those frames turned and converted, and their faces cut, on the host.",
             "#   ratio = host_min / device_min; spread = the larger of the two sides' max - min over the repetitions; faster = the side whose",
             "#   minimum is below the other's by more than the spread, '-' where neither is"]
    for name, rotation in (("rot0", 0), ("rot90", 90)):
        lines += base.table("process_images(mixed_sizes=True, device_frames=True, rotation=%d), mixed_device=True vs absent" % rotation, results[name],
                            "device", "host", "ms per frame")
    lines += base.table("album: process_album on %d photos of %d sizes, mixed_device=True vs False" % (ALBUM_PHOTOS, ALBUM_PHOTOS), results["album"],
                        "device", "host", "ms per album")
    lines.append("# the two launches alone on the %d frames (device events, 50 launches per repetition, %d repetitions): bytes = read + written"
                 % (max(BATCHES), REPS))
    lines.append("%-48s %10s %10s %12s %10s" % ("launch", "min_us", "med_us", "bytes", "GB/s"))
    for r in results["launches"]["rows"]:
        lines.append("%-48s %10.1f %10.1f %12d %10.1f" % (r["what"], min(r["ms"]) * 1e3, float(np.median(r["ms"])) * 1e3, r["bytes"],
                                                           r["bytes"] / (min(r["ms"]) * 1e-3) / 1e9))
    wins = []
    for name in ("rot0", "rot90"):
        by_b = {r["b"]: r for r in results[name]["rows"]}
        wins += [min(by_b[b]["old"]) - min(by_b[b]["new"]) > base.spread_of(by_b[b]) for b in RULE_BATCHES]
    al = results["album"]["rows"][0]
    album_ok = min(al["new"]) - min(al["old"]) <= base.spread_of(al)
    lines.append("# rule: album.MIXED_DEVICE_DEFAULT = %s  (mixed_device faster by more than the spread at B = %s, rotation 0 then 90: %s; its album not "
                 "slower by more than the album's spread: %s)" % (all(wins) and album_ok, ", ".join(str(b) for b in RULE_BATCHES),
                                                                  ", ".join("yes" if w else "no" for w in wins), "yes" if album_ok else "no"))
    text = "\n".join(lines) + "\n"
    with open(args.out, "w") as f:
        f.write(text)
    print(text)


if __name__ == "__main__":
    main()
