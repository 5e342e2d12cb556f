#!/usr/bin/env python3
"""Wall time per frame of the batched MTCNN cascade against the per-frame loop it replaces, on the reference photo
(tests/golden/test_image.jpg, 784 x 588) and same-size variants of it:

  detect : MTCNNDetector.detect_batch(frames, max_frames=B)          against  [det(f) for f in frames]
  process: FacialImageProcessing.process_images(frames, max_frames=B) against  [fip.process_image(f) for f in frames]

at B = 1, 2, 4, 8, 16, 32, 64 frames per call.  The loop is the code of before the batched path, unchanged, so it is the baseline, measured
in the same process: after a warm-up of both, REPS repetitions of each, alternating; a repetition is as many calls as fill --seconds, timed
with a host clock (both sides end in a device-to-host copy of their results, so the clock sees finished work).  Per side the minimum and
the median of the repetitions; `spread` is the larger of the two sides' max - min; batching counts as a win at a B only where the loop's
minimum exceeds the batched minimum by more than that spread.

Each section runs in a child process of its own under `timeout -k 10`; a section that fails or runs out of time ends the run.
usage: python tools/mtcnn_batch_time.py [--out FILE] [--seconds S] [--limit SECONDS_PER_SECTION]"""
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

BATCHES = [1, 2, 4, 8, 16, 32, 64]
REPS = 5
TEST_IMAGE = os.path.join(ROOT, "tests", "golden", "test_image.jpg")


def make_frames(n):
    """n distinct RGB frames of the photo's size: the photo, its mirror images and a dimmed copy, each shifted sideways a little further
    every fourth frame."""
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


def alternated(batched, loop, seconds):
    """-> (ms per call of each repetition of `batched`, the same of `loop`, calls per repetition of each)."""
    for f in (batched, loop):                    # warm-up: every shape the timed window uses, code objects, work tensors
        f()
        f()
    calls = [max(2, int(seconds * 1e3 / max(wall_ms(f, 2), 1e-3))) for f in (batched, loop)]
    tb, tl = [], []
    for _ in range(REPS):
        tb.append(wall_ms(batched, calls[0]))
        tl.append(wall_ms(loop, calls[1]))
    return tb, tl, calls


def section(name, seconds):
    import torch
    from hse_facerec_tf_amd import FacialImageProcessing
    from hse_facerec_tf_amd.mtcnn import MTCNNDetector
    frames = make_frames(max(BATCHES))
    rows = []
    if name == "detect":
        det = MTCNNDetector(minsize=32)
        batched_of = lambda fs, b: (lambda: det.detect_batch(fs, max_frames=b))
        loop_of = lambda fs: (lambda: [det(f) for f in fs])
        faces_of = lambda out: sum(r[0].shape[0] for r in out)
    else:
        fip = FacialImageProcessing(mtcnn_detector=True, minsize=32)
        det = fip.detector
        frames = [np.ascontiguousarray(f[..., ::-1]) for f in frames]       # BGR, as cv2.imread gives them
        batched_of = lambda fs, b: (lambda: fip.process_images(fs, max_frames=b))
        loop_of = lambda fs: (lambda: [fip.process_image(f) for f in fs])
        faces_of = lambda out: sum(len(r[0]) for r in out)
    for b in BATCHES:
        fs = frames[:b]
        batched, loop = batched_of(fs, b), loop_of(fs)
        faces = (faces_of(batched()), faces_of(loop()))
        tb, tl, calls = alternated(batched, loop, seconds)
        rows.append(dict(b=b, batched=[t / b for t in tb], loop=[t / b for t in tl], calls=calls, faces=faces))
        print(name, b, "batched min %.3f loop min %.3f ms/frame" % (min(rows[-1]["batched"]), min(rows[-1]["loop"])), flush=True)
    return dict(device=torch.cuda.get_device_name(0), host_fallbacks=int(det.host_fallbacks), rows=rows)


def table(name, res):
    lines = ["# %s: ms per frame (wall), %d repetitions of each side, alternating; calls = calls per repetition (batched/loop)" % (name, REPS),
             "%3s %12s %12s %10s %10s %8s %7s %5s %9s %11s"
             % ("B", "batched_min", "batched_med", "loop_min", "loop_med", "spread", "ratio", "win", "calls", "faces(b/l)")]
    for r in res["rows"]:
        tb, tl = r["batched"], r["loop"]
        spread = max(max(tb) - min(tb), max(tl) - min(tl))
        win = min(tl) - min(tb) > spread
        lines.append("%3d %12.3f %12.3f %10.3f %10.3f %8.3f %7.2f %5s %9s %11s"
                     % (r["b"], min(tb), float(np.median(tb)), min(tl), float(np.median(tl)), spread, min(tl) / min(tb), "yes" if win else "no",
                        "%d/%d" % tuple(r["calls"]), "%d/%d" % tuple(r["faces"])))
    lines.append("# frames redone on the host in this section: %d" % res["host_fallbacks"])
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mtcnn_batch_time.txt"))
    ap.add_argument("--seconds", type=float, default=0.3, help="wall time one repetition of one side is sized to")
    ap.add_argument("--limit", type=int, default=240, help="time limit of one section's process, seconds")
    ap.add_argument("--section", choices=["detect", "process"], help="(internal) run one section in this process and write --json")
    ap.add_argument("--json")
    args = ap.parse_args()
    if args.section:
        res = section(args.section, args.seconds)
        with open(args.json, "w") as f:
            json.dump(res, f)
        return
    results = {}
    with tempfile.TemporaryDirectory() as tmp:
        for name in ("detect", "process"):
            path = os.path.join(tmp, name + ".json")
            cmd = ["timeout", "-k", "10", str(args.limit), sys.executable, os.path.abspath(__file__), "--section", name, "--json", path,
                   "--seconds", str(args.seconds)]
            rc = subprocess.run(cmd).returncode
            if rc != 0:
                sys.exit("section %s ended with status %d: nothing written, nothing further run" % (name, rc))
            with open(path) as f:
                results[name] = json.load(f)
    lines = ["# MTCNN, many frames per pass against one frame per call (tools/mtcnn_batch_time.py); %s, %s"
             % (results["detect"]["device"], time.strftime("%Y-%m-%d")),
             "# frames: tests/golden/test_image.jpg (784 x 588, 4 faces) and same-size variants (mirrored, upside down, dimmed, shifted)",
             "# batched: detect_batch / process_images with max_frames = B, one pass; loop: the single-frame call per frame (the path of before,",
             "#   unchanged).  ratio = loop_min / batched_min; spread = the larger of the two sides' max - min over the repetitions;",
             "#   win = loop_min - batched_min > spread.  At B = 1 detect_batch hands its one frame to the single-frame call: that row",
             "#   compares the same launches and shows what the list bookkeeping (and, for process, the bulk age/gender plan) costs"]
    lines += table("detect: MTCNNDetector.detect_batch vs [det(f) for f in frames]", results["detect"])
    lines += table("process: FacialImageProcessing.process_images vs [process_image(f) for f in frames] (detection + age/gender/features)",
                   results["process"])
    text = "\n".join(lines) + "\n"
    with open(args.out, "w") as f:
        f.write(text)
    print(text)


if __name__ == "__main__":
    main()
