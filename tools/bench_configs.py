#!/usr/bin/env python3
"""Throughput of the other BASELINE configs on one MI355X (parity-test cases, not the headline bench line):
    python tools/bench_configs.py resnet50      # config 3: ResNet-50, batch 128, 224x224x3, bf16 MFMA
    python tools/bench_configs.py agegender     # config 4: age/gender MobileNet multi-head, batch 512, 224x224x3
    python tools/bench_configs.py mobilenet192  # config 2 (the headline): MobileNet-192 embeddings, batch 256 -- for its per-LAYER table
    python tools/bench_configs.py mobilenet_f32 # config 2 with every product on the fp32 pipes (pw_math='f32')
    python tools/bench_configs.py mobilenetv2   # MobileNetV2 alpha 1.0 at 192 and alpha 1.4 at 224, batch 256: default plan, pad_channels' bound at 3 / 2 /
                                                # 1.5, no channel padding and the fp32-grade general mode, alternated (profiles/mobilenetv2_time.txt)
Every run prints a per-LAYER table (the engine's HIP-event ring) and `forwards N`, the number of forwards it launched -- what
tools/make_profile_summary.py stores next to a PMC profile of the same command so that bench.py can turn bytes per launch into bytes per forward.
"""
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from hse_facerec_tf_amd import lowering, resnet50
from hse_facerec_tf_amd.engine import Engine
from hse_facerec_tf_amd.graphdef import read_graph
from hse_facerec_tf_amd.tf_inference import AGE_GENDER_PB

STEPS, WARM = int(os.environ.get("BC_STEPS", "20")), 5


def run(eng, x, want, label, flops_per_img, bytes_per_img):
    for _ in range(WARM):
        out = eng.forward(x, want)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(STEPS):
        out = eng.forward(x, want)
    torch.cuda.synchronize()
    dt = (time.perf_counter() - t0) / STEPS
    n = x.shape[0]
    print("%s: %.3f ms/step  %.0f faces/s  (%.1f TFLOP/s, %.0f GB/s algorithmic)" %
          (label, dt * 1e3, n / dt, flops_per_img * n / dt / 1e12, bytes_per_img * n / dt / 1e9))
    eng.set_profiling(STEPS)
    for _ in range(STEPS):
        eng.forward(x, want)
    per = np.mean([eng.op_times_ms(s) for s in range(STEPS)], axis=0)
    eng.set_profiling(0)
    print("forwards %d" % (WARM + 2 * STEPS))
    for i, L in enumerate(eng.plan.layers):
        oh, ow, co = L.out_shape
        fl = float(lowering.Plan.layer_flops(L)) * n
        print("  %2d kind %2d %-26s %-16s -> %-16s %8.1f us %7.1f TF" % (i, L.kind, L.name[:26], L.in_shape, L.out_shape, per[i] * 1e3,
                                                                          fl / (per[i] * 1e-3) / 1e12 if per[i] > 0 else 0))
    return out


def mobilenetv2(B, rs, reps=5):
    """MobileNetV2 (tests/keras_mobilenetv2_graph.py: seeded weights) alpha 1.0 at 192 and alpha 1.4 at 224.  The sides of one model are timed
    ALTERNATELY, `reps` repetitions of STEPS forwards each, the minimum and the spread (max - min) of the repetitions reported:
      default    the Keras-style graph (Pad + VALID), lower_graph's defaults: channel padding, MFMA GEMMs, fused residuals
      bound N    the same with channel_padding=N: pad_channels' bound at 3, 2 and 1.5 in place of lowering.CHANNEL_PAD_MAX_RATIO -- the
                 sweep the constant is set from (a class above the bound stays on the general kernel)
      unpadded   the same with channel_padding="none": every odd-width 1x1 layer on the general kernel
      baseline   the SAME-padded graph under dtype="f32g": what the engine could run before it lowered MobileNetV2
    then the default plan's per-layer table, the padded-over-real FLOP ratio and the expanded tensors' bytes."""
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
    import keras_mobilenetv2_graph as kg
    out = "global_average_pooling2d_1/Mean:0"
    for alpha, size in ((1.0, 192), (1.4, 224)):
        keras, slim = (read_graph(kg.build(alpha, size, 0, style)[0]) for style in ("keras", "slim"))
        plans = {"default": lowering.lower_graph(keras, "input_1:0", {0: out})}
        for bound in (3.0, 2.0, 1.5):
            plans["bound %.1f" % bound] = lowering.lower_graph(keras, "input_1:0", {0: out}, channel_padding=bound)
        plans.update({"unpadded": lowering.lower_graph(keras, "input_1:0", {0: out}, channel_padding="none"),
                      "baseline": lowering.lower_graph(slim, "input_1:0", {0: out}, dtype="f32g")})
        x = torch.from_numpy(rs.uniform(-1, 1, (B, size, size, 3)).astype(np.float32)).cuda()
        engines = {k: Engine(p, max_batch=B) for k, p in plans.items()}
        feats = {k: e.forward(x, (0,))["features"].clone() for k, e in engines.items()}
        for k in ("unpadded", "baseline"):      # (the keras and slim graphs hold the same weights and compute the same function)
            print("MobileNetV2 alpha %.1f %d: default vs %s max-norm %.2e" %
                  (alpha, size, k, float((feats["default"] - feats[k]).abs().max() / feats[k].abs().max())))
        times = {k: [] for k in engines}
        for _ in range(reps):
            for k, e in engines.items():
                for _ in range(2):
                    e.forward(x, (0,))
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(STEPS):
                    e.forward(x, (0,))
                torch.cuda.synchronize()
                times[k].append((time.perf_counter() - t0) / STEPS * 1e3)
        for k, t in times.items():
            print("MobileNetV2 alpha %.1f %d batch %d %-9s: min %.3f ms/step  %.0f faces/s  %.1f MFLOP per image  (spread of %d repetitions %.3f ms; %s)" %
                  (alpha, size, B, k, min(t), B / min(t) * 1e3, plans[k].flops_per_image() / 1e6, reps, max(t) - min(t), " ".join("%.3f" % v for v in t)))
        real, padded = plans["unpadded"].flops_per_image(), plans["default"].flops_per_image()
        print("MobileNetV2 alpha %.1f %d: %.1f MFLOP per image real, %.1f padded: ratio %.3f" % (alpha, size, real / 1e6, padded / 1e6, padded / real))
        eng = engines["default"]
        eng.set_profiling(STEPS)
        for _ in range(STEPS):
            eng.forward(x, (0,))
        per = np.mean([eng.op_times_ms(s) for s in range(STEPS)], axis=0)
        eng.set_profiling(0)
        rows = plans["default"].describe(B)
        total = float(per.sum())
        block_ms = expanded_bytes = 0.0
        for i, L in enumerate(plans["default"].layers):
            inside = any(s in L.name for s in ("expand", "depthwise", "project"))
            block_ms += per[i] if inside else 0.0
            if "expand/" in L.name or "depthwise/" in L.name:      # the expanded tensor: written by this layer, read by the next
                expanded_bytes += 2.0 * L.out_bytes
            print("  %2d kind %2d %-34s %-16s -> %-16s %8.1f us %6.1f TF  %s" %
                  (i, L.kind, L.name[:34], L.in_shape, L.out_shape, per[i] * 1e3,
                   float(lowering.Plan.layer_flops(L)) * B / (per[i] * 1e-3) / 1e12 if per[i] > 0 else 0, " + ".join(rows[i]["family"])))
        print("MobileNetV2 alpha %.1f %d: layers sum to %.3f ms; the inverted residual blocks take %.3f ms (%.0f%%); their expanded tensors are "
              "%.1f MB per image written and read back, %.2f GB per step" %
              (alpha, size, total, block_ms, 100 * block_ms / total, expanded_bytes / 1e6, expanded_bytes * B / 1e9))
        for e in engines.values():
            e.close()


if __name__ == "__main__":
    what = sys.argv[1] if len(sys.argv) > 1 else "resnet50"
    rs = np.random.RandomState(123)
    if what == "resnet50f32":
        B = int(os.environ.get("BC_BATCH", "32"))
        plan = resnet50.build_plan(resnet50.synthetic_weights(123), (224, 224), "caffe", dtype="f32")
        eng = Engine(plan, max_batch=B)
        x = torch.from_numpy(rs.uniform(-128, 128, (B, 224, 224, 3)).astype(np.float32)).cuda()
        run(eng, x, (0,), "ResNet-50 fp32-grade batch %d" % B, resnet50.flops_per_image(plan), 2 * resnet50.activation_bytes_per_image(plan))
    elif what == "resnet50":
        B = int(os.environ.get("BC_BATCH", "128"))
        plan = resnet50.build_plan(resnet50.synthetic_weights(123), (224, 224), "caffe")
        eng = Engine(plan, max_batch=B)
        x = torch.from_numpy(rs.uniform(-128, 128, (B, 224, 224, 3)).astype(np.float32)).cuda()
        run(eng, x, (0,), "ResNet-50 bf16 batch %d" % B, resnet50.flops_per_image(plan), resnet50.activation_bytes_per_image(plan))
    elif what in ("mobilenet192", "mobilenet_f32"):
        B = int(os.environ.get("BC_BATCH", "256"))
        f32 = what == "mobilenet_f32"
        plan = lowering.lower_graph(read_graph(AGE_GENDER_PB), "input_1:0", {0: "global_pooling/Mean:0"}, (192, 192),
                                    **({"pw_math": "f32"} if f32 else {"input_bound": 256.0}))
        eng = Engine(plan, max_batch=B)
        x = torch.from_numpy(rs.uniform(-128, 128, (B, 192, 192, 3)).astype(np.float32)).cuda()
        run(eng, x, (0,), "MobileNet-192 batch %d%s" % (B, " (pw_math='f32')" if f32 else ""), plan.flops_per_image(), plan.bytes_per_image())
    elif what == "mobilenetv2":
        mobilenetv2(int(os.environ.get("BC_BATCH", "256")), rs)
    else:
        B = int(os.environ.get("BC_BATCH", "512"))
        plan = lowering.lower_graph(read_graph(AGE_GENDER_PB), "input_1:0",
                                    {0: "global_pooling/Mean:0", 1: "age_pred/Softmax:0", 2: "gender_pred/Sigmoid:0"}, input_bound=256.0)
        eng = Engine(plan, max_batch=B)
        x = torch.from_numpy(rs.uniform(-128, 128, (B, 224, 224, 3)).astype(np.float32)).cuda()
        run(eng, x, (0, 1, 2), "age/gender MobileNet-224 batch %d (3 outputs)" % B, plan.flops_per_image(), plan.bytes_per_image())
