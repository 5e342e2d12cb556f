"""One line per plan of a fixed matrix of lowerings: the options and a SHA-256 of everything the plan says.  CPU only.

The instrument for a change to hse_facerec_tf_amd/lowering.py that must not change a plan: run it before and after and diff the two
listings.  The matrix makes every graph-to-plan pass fire, and makes every pass decline because its tensor is a requested output.
usage: python tools/plan_digest.py > listing.txt

--describe adds, per plan, a SHA-256 of plan.describe(n) at n = 1, 4 and 256: the instrument for a change to the engine's host code
that must not change a route.  It asks the loaded library (HSEFR_LIB selects the file; no GPU needed); the product library refuses
round 1's stem, so there the stem_fusion="stem" rows are left out, as are the requests the lowering refuses.  Every hash of such a listing is cut to its first 12 hex digits:
enough to tell two listings apart, and a listing that is kept stays small."""
import hashlib
import itertools
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
from hse_facerec_tf_amd import graphdef, lowering, resnet50     # noqa: E402
import keras_mobilenet_graph                                      # noqa: E402
import mini_resnet_graph                                          # noqa: E402

MODEL_PB = os.path.join(ROOT, "models", "age_gender_tf2_new-01-0.14-0.92_quantized.pb")
FEATURES = "global_pooling/Mean:0"
ALL_OUTS = {0: FEATURES, 1: "age_pred/Softmax:0", 2: "gender_pred/Sigmoid:0"}
MEAN_BGR = (103.939, 116.779, 123.68)
OPTION_SETS = [{}, {"fuse": False}, {"input_bound": 256.0}, {"input_bound": 256.0, "u8_mean_bgr": MEAN_BGR}, {"stem_fusion": "stem"},
               {"stem_fusion": "none"}, {"fuse_stem_block": False}, {"block_fusion": "all"}, {"block_fusion": "none"}, {"presplit": "none"},
               {"pwdw_fusion": "none"}, {"pw_math": "f32"}, {"launch_fusion": False}]
# tensors a pass would fuse away, requested next to the features: the pass has to decline.  The first six are the intermediate
# outputs tests/test_lowering_cpu.py asks for; the rest reach the passes those leave out (fuse_pwgap, presplit_activations).
KEPT = ["conv_dw_1_relu/clip_by_value:0", "conv1_relu/clip_by_value:0", "conv_dw_3_relu/clip_by_value:0", "conv_pw_8_relu/clip_by_value:0",
        "conv_pw_3_relu/clip_by_value:0", "conv_pw_3_bn/batchnorm_1/add_1:0", "conv_pw_1_relu/clip_by_value:0", "conv_dw_8_relu/clip_by_value:0",
        "conv_pw_13_relu/clip_by_value:0"]
KEPT_OPTION_SETS = [{}, {"input_bound": 256.0}, {"stem_fusion": "stem"}, {"stem_fusion": "none"}, {"block_fusion": "none"},
                    {"block_fusion": "all"}, {"pwdw_fusion": "none"}]
# ... and of the ResNet passes: conv1 (fuse_stem_pool), a projection (fuse_proj), a stage's last block and its 3x3 layer
# (subsample_stage_tails), a paired increase layer (compact_pair_outputs)
MINI_KEPT = [None, "conv1/relu:0", "conv2_1_1x1_proj/bn:0", "conv2_2/relu:0", "conv2_2_3x3/relu:0", "conv2_1/relu:0"]
MINI_PARAMS = [("SAME", "fused", "avgpool", 40), ("PADVALID", "muladd", "mean", 38), ("SAME", "fused", "avgpool", 38)]


def digest(plan) -> str:
    h = hashlib.sha256(plan.serialize())
    text = [repr(sorted((int(s), int(li), int(e)) for s, (li, e) in plan.outputs.items())),
            repr(sorted((str(n), int(li)) for n, li in plan.tensor_layer.items()))]
    for L in plan.layers:
        hw = None if L.graph_hw is None else tuple(int(v) for v in L.graph_hw)
        text.append(repr((str(L.name), int(L.kind), [str(t) for t in L.tensors], hw, int(L.out_buf))))
    h.update("\n".join(text).encode())
    return h.hexdigest()


DESCRIBE_BATCHES = (1, 4, 256)
describe_routes = False          # --describe
dev_library = False


def routes(plan) -> str:
    """`n1,n4=... n256=...`: batch sizes with one result share an entry."""
    results = {}
    for n in DESCRIBE_BATCHES:
        try:
            r = hashlib.sha256(repr(plan.describe(n)).encode()).hexdigest()[:12]
        except (ValueError, NotImplementedError) as e:          # the library's refusal (_lib.check)
            r = "%s:%s" % (type(e).__name__, hashlib.sha256(str(e).encode()).hexdigest()[:12])      # (its message, hashed)
        results.setdefault(r, []).append("n%d" % n)
    return " ".join("%s=%s" % (",".join(ns), r) for r, ns in results.items())


def show(what: str, opts: dict, make) -> None:
    """`make` builds the plan; a request the lowering refuses is listed with its refusal."""
    if describe_routes and not dev_library and opts.get("stem_fusion") == "stem":
        return
    try:
        plan = make()
        result = digest(plan)
        if describe_routes:
            result = result[:12] + " " + routes(plan)
    except lowering.LoweringError as e:
        if describe_routes:          # no plan, no routes
            return
        result = "LoweringError: %s" % e
    print("%s %s %s" % (what, " ".join("%s=%r" % kv for kv in sorted(opts.items())) or "defaults", result))


def main() -> None:
    global describe_routes, dev_library
    if "--describe" in sys.argv[1:]:
        from hse_facerec_tf_amd import _lib
        describe_routes, dev_library = True, hasattr(_lib.lib(), "hsefr_debug_set")
    g = graphdef.read_graph(MODEL_PB)
    for size, opts in itertools.product((96, 98, 100, 192, 224), OPTION_SETS):
        show("mobilenet %d" % size, opts, lambda: lowering.lower_graph(g, "input_1:0", ALL_OUTS, (size, size), **opts))
    for size, kept, opts in itertools.product((64, 192), KEPT, KEPT_OPTION_SETS):
        for outs in ({0: kept}, {0: FEATURES, 1: kept}):
            show("mobilenet %d out %s" % (size, ",".join(outs.values())), opts,
                 lambda: lowering.lower_graph(g, "input_1:0", outs, (size, size), **opts))
    feeds = {"conv1_bn/keras_learning_phase:0": 0}
    for size in (64, 192):
        kg = graphdef.read_graph(keras_mobilenet_graph.build(MODEL_PB, size))
        for opts in OPTION_SETS:
            show("keras %d" % size, opts, lambda: lowering.lower_graph(kg, "input_1:0", {0: "reshape_1/Reshape:0"}, None, feeds, **opts))
    w = resnet50.synthetic_weights(7)
    for (size, pool), dtype, fuse, pair, sub in itertools.product(((64, "caffe"), (70, "valid"), (224, "caffe")), ("bf16", "f32"),
                                                                  (True, False), (True, False), (True, False)):
        opts = {"dtype": dtype, "fuse": fuse, "pair": pair, "subsample": sub}
        show("resnet50 %d %s" % (size, pool), opts, lambda: resnet50.build_plan(w, (size, size), pool, **opts))
    for pool, bn, head, hw in MINI_PARAMS:
        mg = graphdef.read_graph(mini_resnet_graph.build(3, hw, pool, bn, 64, head)[0])
        for kept, dtype, fuse, launch in itertools.product(MINI_KEPT, ("bf16", "f32g"), (True, False), (True, False)):
            outs = {0: "pool5_7x7_s1:0"} if kept is None else {0: "pool5_7x7_s1:0", 1: kept}
            opts = {"dtype": dtype, "fuse": fuse, "launch_fusion": launch}
            show("mini_resnet %s %s %s %d out %s" % (pool, bn, head, hw, ",".join(outs.values())), opts,
                 lambda: lowering.lower_graph(mg, "input:0", outs, **opts))


if __name__ == "__main__":
    main()
