#!/usr/bin/env python3
"""Same-box A/B of cache-policy candidates on the edges of the MobileNet-192 plan (DESIGN.md lesson 76): one build of the library per
candidate (build.sh with HSEFR_EXTRA_FLAGS), each measured in a process of its own (a process loads one library: HSEFR_LIB), the parent
build and the candidates alternating over ROUNDS rounds.  Per child: batch 256, 10 warm forwards, 20 timed, then the engine's op events
over 20 profiled forwards (medians).  A candidate is judged on the launch it changes plus the launch behind it.
  python tools/edge_policy_ab.py [--rounds 4] [--batch 256] [--out FILE] parent=PATH name=PATH[:OP[:COUNT]] ...
      PATH: a libhsefr.so (relative to the package directory, or absolute); OP: index of the plan's LAUNCH the candidate changes (it is
      judged on launches OP .. OP + COUNT - 1, COUNT = 2 unless given: a set of candidates spans more); the first library named is the parent.
A candidate is KEPT only if its launches' sum is below the parent's in EVERY round and the median gain exceeds the parent's own spread."""
import json, os, subprocess, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
NOPS = 6          # launches printed per child: the stem, the three fused blocks, conv_dw_6, conv_pw_6


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
    rows = plan.describe(B)
    kernels = [d["kernels"][0] for d in rows if d["kernels"]]
    eng = Engine(plan, max_batch=B)
    for _ in range(10):
        feat = eng.forward(x, (0,))["features"].clone()
    torch.cuda.synchronize(); t0 = time.perf_counter()
    for _ in range(20): eng.forward(x, (0,))
    torch.cuda.synchronize(); dt = (time.perf_counter() - t0) / 20
    eng.set_profiling(20)
    for _ in range(20): eng.forward(x, (0,))
    per_op = np.median([eng.op_times_ms(s) for s in range(20)], axis=0) * 1e3
    eng.close()
    per = []          # per LAUNCH: an op that runs inside the launch in front of it has no kernel of its own
    for d, v in zip(rows, per_op):
        if d["kernels"]: per.append(float(v))
        else: per[-1] += float(v)
    bits = int(feat.cpu().numpy().view(np.uint32).sum(dtype=np.uint64)) & 0xFFFFFFFF
    print("RESULT " + json.dumps({"ops": [round(float(v), 2) for v in per], "ms": round(dt * 1e3, 4), "bits": "%08x" % bits, "kernels": kernels}))


def main(argv):
    rounds, B, out_path, libs = 4, "256", None, []
    while argv:
        a = argv.pop(0)
        if a == "--rounds": rounds = int(argv.pop(0))
        elif a == "--batch": B = argv.pop(0)
        elif a == "--out": out_path = argv.pop(0)
        else:
            name, path = a.split("=", 1)
            op = None
            if ":" in path:
                path, op = path.split(":", 1)
                op = tuple(int(v) for v in op.split(":")) if ":" in op else (int(op), 2)
            libs.append((name, path, op))
    out = open(out_path, "w") if out_path else None

    def say(line):
        print(line, flush=True)
        if out: out.write(line + "\n"); out.flush()
    table = {name: [] for name, _, _ in libs}
    say("round  build       " + "".join("   op%d us" % i for i in range(NOPS)) + "  ops sum us  forward ms  feature bits")
    for r in range(rounds):
        for name, lib, _ in libs:
            res = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", B], env=dict(os.environ, HSEFR_LIB=lib), capture_output=True,
                                 text=True, timeout=300)
            line = [l for l in res.stdout.splitlines() if l.startswith("RESULT ")]
            if res.returncode != 0 or not line:
                say("child %s failed (%d): %s" % (name, res.returncode, res.stderr[-2000:]))
                return 1       # nothing more is started on the GPU after a failed child
            d = json.loads(line[0][7:])
            if r == 0 and name == libs[0][0]:
                say("kernels: " + " | ".join("op%d %s" % (i, k) for i, k in enumerate(d["kernels"][:NOPS])))
            table[name].append(d)
            say("%5d  %-10s  " % (r, name) + "".join("%8.1f" % v for v in d["ops"][:NOPS]) + "  %10.1f  %10.4f  %s" % (sum(d["ops"]), d["ms"], d["bits"]))
    import numpy as np
    pname = libs[0][0]
    say("")
    say("candidate   pair     parent us per round            candidate us per round         gain per round            median gain  parent spread  verdict")
    for name, _, op in libs[1:]:
        if op is None: continue
        op, cnt = op
        a = np.array([sum(d["ops"][op:op + cnt]) for d in table[pname]])
        b = np.array([sum(d["ops"][op:op + cnt]) for d in table[name]])
        gain = a - b
        keep = bool((gain > 0).all() and np.median(gain) > a.max() - a.min())
        same = all(d["bits"] == table[pname][0]["bits"] for d in table[name])
        fmt = lambda v: " ".join("%6.1f" % x for x in v)
        say("%-10s  op%d-%d  %s    %s    %s   %8.1f  %11.1f    %s%s" % (name, op, op + cnt - 1, fmt(a), fmt(b), fmt(gain), np.median(gain), a.max() - a.min(),
                                                                      "KEEP" if keep else "reject", "" if same else "  (BITS DIFFER)"))
    ms = {name: [d["ms"] for d in table[name]] for name in table}
    say("")
    say("forward ms per round (20 forwards, wall clock): " + "; ".join("%s %s" % (n, " ".join("%.4f" % v for v in ms[n])) for n in ms))
    return 0


if __name__ == "__main__":
    if sys.argv[1] == "--child":
        child(int(sys.argv[2]))
        sys.exit(0)
    sys.exit(main(sys.argv[1:]))
