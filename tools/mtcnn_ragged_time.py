#!/usr/bin/env python3
"""Wall time of the mixed-size MTCNN pass (MTCNNDetector.detect_ragged, libhsefr_ragged.so) against the paths it can replace, on cut-outs
and transposes of the reference photo (tests/golden/test_image.jpg, 784 x 588):

  mixed   : B = 2, 4, 8, 16, 32 frames, EVERY ONE OF A DIFFERENT SIZE (between about 300 x 400 and 784 x 588)
              detect : detect_batch(frames, mixed_sizes=True)    against  detect_batch(frames)    -- one single-frame call per frame
              process: process_images(frames, mixed_sizes=True)  against  process_images(frames)
  same    : B = 8, 16, 32 frames of 784 x 588:  detect_ragged(frames) against detect_batch(frames).  Information only: whether one
            launch per P-Net layer beats one per pyramid level where both paths share a pass
  album   : process_album on 64 photos of 64 different sizes (a quarter of them turned, an eighth empty), with and without
            mixed_sizes

The side without the flag is the code of before, unchanged, measured in the same process: after a warm-up of both, REPS repetitions of
each, alternating; a repetition is as many calls as fill --seconds, timed with a host clock (both sides end in a device-to-host copy of
their results).  Per side the minimum and the median of the repetitions; `spread` is the larger of the two sides' max - min; a side wins
where the other's minimum exceeds its minimum by more than that spread.

The last line of the output applies the rule of album.MIXED_SIZES_DEFAULT: True if the mixed pass wins `detect` at 4, 8 and 16 frames per
call and the mixed album is not slower by more than its spread; otherwise False.

Each section runs in a child process of its own under `timeout -k 10`; a section that fails or runs out of time ends the run.
usage: python tools/mtcnn_ragged_time.py [--out FILE] [--seconds S] [--limit SECONDS_PER_SECTION]"""
import argparse
import json
import os
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np

MIXED_BATCHES = [2, 4, 8, 16, 32]
SAME_BATCHES = [8, 16, 32]
ALBUM_PHOTOS = 64
REPS = 5
RULE_BATCHES = (4, 8, 16)
TEST_IMAGE = os.path.join(ROOT, "tests", "golden", "test_image.jpg")
SECTIONS = ("detect", "process", "same", "album")


def mixed_frames(n, step=(9, 12)):
    """n RGB frames of n different sizes: cut-outs of the photo that shrink by `step` pixels per frame (784 x 588 down to about 300 x 400
    at n = 32), every other one transposed."""
    from hse_facerec_tf_amd import preprocess
    img = preprocess.imread_rgb(TEST_IMAGE)
    out = []
    for i in range(n):
        f = img[(i * 5) % 40:, (i * 7) % 60:][:img.shape[0] - step[0] * i, :img.shape[1] - step[1] * i]
        out.append(np.ascontiguousarray(np.transpose(f, (1, 0, 2)) if i % 2 else f))
    assert len({f.shape for f in out}) == n
    return out


def same_frames(n):
    from hse_facerec_tf_amd import preprocess
    img = preprocess.imread_rgb(TEST_IMAGE)
    base = [img, img[:, ::-1], img[::-1], (img * 0.6).astype(np.uint8)]
    return [np.ascontiguousarray(np.roll(base[i % 4], 37 * (i // 4), axis=1)) for i in range(n)]


def wall_ms(fn, calls):
    import torch
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(calls):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / calls


def alternated(new, old, seconds):
    """-> (ms per call of each repetition of `new`, the same of `old`, calls per repetition of each)."""
    for f in (new, old):                         # warm-up: every shape the timed window uses, code objects, work tensors, the plan's tables
        f()
        f()
    calls = [max(2, int(seconds * 1e3 / max(wall_ms(f, 2), 1e-3))) for f in (new, old)]
    tn, to = [], []
    for _ in range(REPS):
        tn.append(wall_ms(new, calls[0]))
        to.append(wall_ms(old, calls[1]))
    return tn, to, calls


def same_detections(a, b):
    return len(a) == len(b) and all(x[0].shape == y[0].shape and np.array_equal(x[0], y[0]) and np.array_equal(x[1], y[1]) for x, y in zip(a, b))


def section(name, seconds):
    import torch
    from hse_facerec_tf_amd import FacialImageProcessing, album
    from hse_facerec_tf_amd.mtcnn import MTCNNDetector
    rows = []
    if name in ("detect", "same"):
        det = MTCNNDetector(minsize=32)
        for b in (MIXED_BATCHES if name == "detect" else SAME_BATCHES):
            if name == "detect":
                fs = mixed_frames(max(MIXED_BATCHES))[:b]
                new, old = (lambda fs=fs: det.detect_batch(fs, mixed_sizes=True)), (lambda fs=fs: det.detect_batch(fs))
            else:
                fs = same_frames(b)
                new, old = (lambda fs=fs: det.detect_ragged(fs)), (lambda fs=fs: det.detect_batch(fs))
            got, want = new(), old()
            assert same_detections(got, want), "the two sides differ at %d frames" % b
            tn, to, calls = alternated(new, old, seconds)
            rows.append(dict(b=b, new=[t / b for t in tn], old=[t / b for t in to], calls=calls, faces=sum(r[0].shape[0] for r in want)))
            print(name, b, "new min %.3f old min %.3f ms/frame" % (min(rows[-1]["new"]), min(rows[-1]["old"])), flush=True)
    elif name == "process":
        fip = FacialImageProcessing(mtcnn_detector=True, minsize=32, latency_plan=False)
        det = fip.detector
        frames = [np.ascontiguousarray(f[..., ::-1]) for f in mixed_frames(max(MIXED_BATCHES))]       # BGR, as cv2.imread gives them
        for b in MIXED_BATCHES:
            fs = frames[:b]
            new, old = (lambda fs=fs: fip.process_images(fs, mixed_sizes=True)), (lambda fs=fs: fip.process_images(fs))
            got, want = new(), old()
            assert [g[0] for g in got] == [w[0] for w in want], "the two sides differ at %d frames" % b
            tn, to, calls = alternated(new, old, seconds)
            rows.append(dict(b=b, new=[t / b for t in tn], old=[t / b for t in to], calls=calls, faces=sum(len(r[0]) for r in want)))
            print(name, b, "new min %.3f old min %.3f ms/frame" % (min(rows[-1]["new"]), min(rows[-1]["old"])), flush=True)
    else:
        fip = FacialImageProcessing(mtcnn_detector=True, minsize=32, latency_plan=False)
        det = fip.detector
        photos = []
        for i, f in enumerate(mixed_frames(ALBUM_PHOTOS, step=(4, 6))):
            f = np.zeros_like(f) if i % 8 == 7 else (np.rot90(f, 1) if i % 4 == 1 else f)
            photos.append(np.ascontiguousarray(f[..., ::-1]))
        mdates = [time.gmtime(1551693600 + i * 11 * 3600) for i in range(ALBUM_PHOTOS)]
        config = album.AlbumConfig()
        new = lambda: album.process_album(fip, photos, mdates, config=config, mixed_sizes=True)
        old = lambda: album.process_album(fip, photos, mdates, config=config, mixed_sizes=False)
        got, want = new(), old()
        assert (got.clusters, got.all_indices, got.private_photos, got.public_photos) == \
            (want.clusters, want.all_indices, want.private_photos, want.public_photos), "the two albums differ"
        tn, to, calls = alternated(new, old, seconds)
        rows.append(dict(b=ALBUM_PHOTOS, new=tn, old=to, calls=calls, faces=len(want.all_indices)))
        print(name, "new min %.1f old min %.1f ms/album" % (min(tn), min(to)), flush=True)
    return dict(device=torch.cuda.get_device_name(0), host_fallbacks=int(det.host_fallbacks), ragged_passes=int(det.ragged_passes), rows=rows)


def spread_of(r):
    return max(max(r["new"]) - min(r["new"]), max(r["old"]) - min(r["old"]))


def table(title, res, new_name, old_name, unit):
    lines = ["# %s: %s (wall), %d repetitions of each side, alternating; calls = calls per repetition (%s/%s)" % (title, unit, REPS, new_name, old_name),
             "%3s %12s %12s %10s %10s %8s %7s %6s %9s %6s" % ("B", new_name + "_min", new_name + "_med", old_name + "_min", old_name + "_med", "spread",
                                                              "ratio", "faster", "calls", "faces")]
    for r in res["rows"]:
        tn, to = r["new"], r["old"]
        spread = spread_of(r)
        faster = new_name if min(to) - min(tn) > spread else (old_name if min(tn) - min(to) > spread else "-")
        lines.append("%3d %12.3f %12.3f %10.3f %10.3f %8.3f %7.2f %6s %9s %6d"
                     % (r["b"], min(tn), float(np.median(tn)), min(to), float(np.median(to)), spread, min(to) / min(tn), faster,
                        "%d/%d" % tuple(r["calls"]), r["faces"]))
    lines.append("# frames redone on the host in this section: %d; ragged passes run: %d" % (res["host_fallbacks"], res["ragged_passes"]))
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mtcnn_ragged_time.txt"))
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
    lines = ["# MTCNN, frames of different sizes in one pass (tools/mtcnn_ragged_time.py); %s, %s" % (results["detect"]["device"], time.strftime("%Y-%m-%d")),
             "# frames: cut-outs of tests/golden/test_image.jpg (784 x 588, 4 faces), every other one transposed, every one of a different size",
             "# mixed: detect_batch / process_images / process_album with mixed_sizes=True (the lone frames share ragged passes of up to 32);",
             "#   loop: the same call without the flag -- one single-frame detector call per frame, the path of before, unchanged.",
             "#   ratio = old_min / new_min; spread = the larger of the two sides' max - min over the repetitions; faster = the side whose",
             "#   minimum is below the other's by more than the spread, '-' where neither is"]
    lines += table("detect: detect_batch(mixed_sizes=True) vs detect_batch()", results["detect"], "mixed", "loop", "ms per frame")
    lines += table("process: process_images(mixed_sizes=True) vs process_images() (detection + age/gender/features)", results["process"], "mixed", "loop",
                   "ms per frame")
    lines += table("same size, information only: detect_ragged vs detect_batch on frames of 784 x 588 (one launch per P-Net layer vs one per level)",
                   results["same"], "ragged", "batch", "ms per frame")
    lines += table("album: process_album on %d photos of %d sizes, mixed_sizes=True vs False" % (ALBUM_PHOTOS, ALBUM_PHOTOS), results["album"], "mixed", "loop",
                   "ms per album")
    by_b = {r["b"]: r for r in results["detect"]["rows"]}
    wins = [min(by_b[b]["old"]) - min(by_b[b]["new"]) > spread_of(by_b[b]) for b in RULE_BATCHES]
    al = results["album"]["rows"][0]
    album_ok = min(al["new"]) - min(al["old"]) <= spread_of(al)
    lines.append("# rule: album.MIXED_SIZES_DEFAULT = %s  (mixed faster than the loop by more than the spread at B = %s: %s; the mixed album not slower by "
                 "more than its spread: %s)" % (all(wins) and album_ok, ", ".join(str(b) for b in RULE_BATCHES),
                                                ", ".join("yes" if w else "no" for w in wins), "yes" if album_ok else "no"))
    text = "\n".join(lines) + "\n"
    with open(args.out, "w") as f:
        f.write(text)
    print(text)


if __name__ == "__main__":
    main()
