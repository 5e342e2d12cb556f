#!/usr/bin/env python3
"""Same-box A/B of the 24 x 24 depthwise-pointwise block's launch between two builds of the library: MobileNet-192 at batch 256, the
engine's op-event times of the conv_dw_5 + conv_pw_5 launch (dwpw3_f16s_kernel) and of the plan's first launch (the stem), and the whole
forward's ms / step, 20 profiled forwards
each.  A process loads one library, so every measurement is a child process with HSEFR_LIB set; the two builds alternate over ROUNDS rounds.
  python tools/dwpw_strip_ab.py PARENT_LIB [ROUNDS=4] [BATCH=256]     PARENT_LIB: a libhsefr.so of the parent commit (path relative to the
                                                                      package directory, or absolute)"""
import os, subprocess, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def child(B):
    import time
    import numpy as np, torch
    from hse_facerec_tf_amd import lowering
    from hse_facerec_tf_amd.engine import Engine
    from hse_facerec_tf_amd.graphdef import read_graph
    from hse_facerec_tf_amd.tf_inference import AGE_GENDER_PB
    hw = 192
    x = torch.from_numpy(np.random.RandomState(1).uniform(-128, 128, (B, hw, hw, 3)).astype(np.float32)).cuda()
    plan = lowering.lower_graph(read_graph(AGE_GENDER_PB), "input_1:0", {0: "global_pooling/Mean:0"}, (hw, hw), input_bound=256.0)
    i = [k for k, L in enumerate(plan.layers) if L.kind == lowering.OP_DWPW_F16S and tuple(L.in_shape) == (24, 24, 256)][0]
    kernel = plan.describe(B)[i]["kernels"]
    eng = Engine(plan, max_batch=B)
    for _ in range(10):
        feat = eng.forward(x, (0,))["features"].clone()
    torch.cuda.synchronize(); t0 = time.perf_counter()
    for _ in range(20): eng.forward(x, (0,))
    torch.cuda.synchronize(); dt = (time.perf_counter() - t0) / 20
    eng.set_profiling(20)
    for _ in range(20): eng.forward(x, (0,))
    per = np.median([eng.op_times_ms(s) for s in range(20)], axis=0) * 1e3
    eng.close()
    print("RESULT %.2f %.2f %.4f %08x %s" % (per[i], per[0], dt * 1e3, int(feat.cpu().numpy().view(np.uint32).sum(dtype=np.uint64)) & 0xFFFFFFFF, kernel[0]))


if __name__ == "__main__":
    if sys.argv[1] == "--child":
        child(int(sys.argv[2]))
        sys.exit(0)
    parent_lib = sys.argv[1]
    rounds = int(sys.argv[2]) if len(sys.argv) > 2 else 4
    B = sys.argv[3] if len(sys.argv) > 3 else "256"
    print("round  build   block us  stem us  forward ms  feature bits  kernel")
    table = {"parent": [], "this": []}
    for r in range(rounds):
        for name, lib in (("parent", parent_lib), ("this", "libhsefr.so")):
            out = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", B], env=dict(os.environ, HSEFR_LIB=lib), capture_output=True,
                                 text=True, timeout=300)
            line = [l for l in out.stdout.splitlines() if l.startswith("RESULT ")]
            if out.returncode != 0 or not line:
                sys.exit("child failed (%d): %s" % (out.returncode, out.stderr[-2000:]))
            us, stem, ms, bits, kernel = line[0].split(" ", 5)[1:]
            table[name].append(float(us))
            print("%5d  %-6s  %8.1f  %7.1f  %10.4f  %s      %s" % (r, name, float(us), float(stem), float(ms), bits, kernel), flush=True)
    import numpy as np
    a, b = np.array(table["this"]), np.array(table["parent"])
    print("this: median %.1f us (min %.1f, max %.1f); parent: median %.1f us (min %.1f, max %.1f, spread %.1f); saved %.1f us; "
          "smallest per-round gain %.1f us" % (np.median(a), a.min(), a.max(), np.median(b), b.min(), b.max(), b.max() - b.min(),
                                             np.median(b) - np.median(a), (b - a).min()))
