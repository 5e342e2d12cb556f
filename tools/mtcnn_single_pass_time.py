#!/usr/bin/env python3
"""Wall time of ONE frame through the same-size pass against the single-frame call, `det(f)`, on the reference photo
(tests/golden/test_image.jpg, 784 x 588): the measurement that decides whether the single-frame call may run as a pass of one.  Two
forms of the pass: `det._detect_pass([f])[0]`, which stacks its frames on the host first (np.stack: a copy of the frame), and
`det._detect_stack_body(upload(f)[None])[0]`, the pass over a view of the one uploaded frame -- what the single-frame call runs.  All
sides upload the frame and end in their read-backs.  Measured as tools/mtcnn_batch_time.py measures (its `alternated`): in one process,
after a warm-up of both, REPS repetitions of each side, alternating; a repetition is as many calls as fill --seconds.  Per side the
minimum and the median; `spread` is the larger of the two sides' max - min; a pass of one counts as slower only where its minimum
exceeds the call's by more than that spread.

usage: python tools/mtcnn_single_pass_time.py [--out FILE] [--seconds S]"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import numpy as np

from mtcnn_batch_time import REPS, TEST_IMAGE, alternated


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mtcnn_single_pass_time.txt"))
    ap.add_argument("--seconds", type=float, default=1.0, help="wall time one repetition of one side is sized to")
    args = ap.parse_args()
    import torch
    from hse_facerec_tf_amd import preprocess
    from hse_facerec_tf_amd.mtcnn import MTCNNDetector
    f = preprocess.imread_rgb(TEST_IMAGE)
    det = MTCNNDetector(minsize=32)
    upload = lambda: torch.from_numpy(np.ascontiguousarray(f)).to(det.device)
    call = lambda: det(f)
    lines = ["# MTCNN, one frame as a pass of one against the single-frame call (tools/mtcnn_single_pass_time.py); %s, %s"
             % (torch.cuda.get_device_name(0), time.strftime("%Y-%m-%d")),
             "# frame: tests/golden/test_image.jpg (784 x 588); ms per call (wall), %d repetitions of each side, alternating;" % REPS,
             "#   spread = the larger of the two sides' max - min; slower = pass_min - call_min > spread"]
    for name, one in (("det._detect_pass([f])[0]", lambda: det._detect_pass([f])[0]),
                      ("det._detect_stack_body(upload(f)[None])[0]", lambda: det._detect_stack_body(upload()[None])[0])):
        (bp, pp), (bc, pc) = one(), call()
        assert bp.shape[0] > 0 and np.array_equal(bp, bc) and np.array_equal(pp, pc)
        tp, tc, calls = alternated(one, call, args.seconds)
        spread = max(max(tp) - min(tp), max(tc) - min(tc))
        lines += ["%-44s %8s %8s %8s %7s" % ("side", "min", "median", "max", "calls"),
                  "%-44s %8.3f %8.3f %8.3f %7d" % (name, min(tp), float(np.median(tp)), max(tp), calls[0]),
                  "%-44s %8.3f %8.3f %8.3f %7d" % ("det(f)", min(tc), float(np.median(tc)), max(tc), calls[1]),
                  "spread %.3f  pass_min - call_min %+.3f  this pass of one is slower than the call: %s"
                  % (spread, min(tp) - min(tc), "yes" if min(tp) - min(tc) > spread else "no")]
    lines.append("# frames redone on the host: %d" % det.host_fallbacks)
    text = "\n".join(lines) + "\n"
    with open(args.out, "w") as out:
        out.write(text)
    print(text)


if __name__ == "__main__":
    main()
