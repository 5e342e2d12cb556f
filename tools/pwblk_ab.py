#!/usr/bin/env python3
"""Same-box A/B of the conv_pw_2 + block launch (lower_graph pw_block_fusion): MobileNet-192 at batch 256, the plan with the one
row-streaming launch and the plan with the two launches alternating over ROUNDS rounds (default 4), 20 profiled forwards each.  Per round:
the engine's op-event times of conv_pw_2 and the block (fused: the block's own interval is empty), and the whole forward's ms / step."""
import os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np, torch
from hse_facerec_tf_amd import lowering
from hse_facerec_tf_amd.engine import Engine
from hse_facerec_tf_amd.graphdef import read_graph
from hse_facerec_tf_amd.tf_inference import AGE_GENDER_PB

rounds = int(sys.argv[1]) if len(sys.argv) > 1 else 4
B, hw = 256, 192
x = torch.from_numpy(np.random.RandomState(1).uniform(-128, 128, (B, hw, hw, 3)).astype(np.float32)).cuda()
engines, feats = {}, {}
for mode in ("auto", "none"):
    plan = lowering.lower_graph(read_graph(AGE_GENDER_PB), "input_1:0", {0: "global_pooling/Mean:0"}, (hw, hw), input_bound=256.0,
                                pw_block_fusion=mode)
    i = [k for k, L in enumerate(plan.layers) if L.name.startswith("conv_pw_2")][0]
    engines[mode] = (Engine(plan, max_batch=B), i)
    for _ in range(5):
        feats[mode] = engines[mode][0].forward(x, (0,))["features"].clone()
assert torch.equal(feats["auto"], feats["none"]), "the two plans differ"
print("round  plan   conv_pw_2 us  block us   sum us   forward ms")
table = {"auto": [], "none": []}
for r in range(rounds):
    for mode in ("none", "auto"):
        eng, i = engines[mode]
        eng.set_profiling(0)
        torch.cuda.synchronize(); t0 = time.perf_counter()
        for _ in range(20): eng.forward(x, (0,))
        torch.cuda.synchronize(); dt = (time.perf_counter() - t0) / 20
        eng.set_profiling(20)
        for _ in range(20): eng.forward(x, (0,))
        per = np.median([eng.op_times_ms(s) for s in range(20)], axis=0) * 1e3
        table[mode].append(per[i] + per[i + 1])
        print("%5d  %-5s  %12.1f  %8.1f  %7.1f  %10.4f" % (r, mode, per[i], per[i + 1], per[i] + per[i + 1], dt * 1e3))
a, n = np.array(table["auto"]), np.array(table["none"])
print("one launch: median %.1f us (min %.1f, max %.1f); two launches: median %.1f us (min %.1f, max %.1f); saved %.1f us"
      % (np.median(a), a.min(), a.max(), np.median(n), n.min(), n.max(), np.median(n) - np.median(a)))
for eng, _ in engines.values():
    eng.close()
