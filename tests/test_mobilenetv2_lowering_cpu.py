"""Lowering of MobileNetV2 graphs (tests/keras_mobilenetv2_graph.py: the shape of the reference's facerec_test.py:216-217 files) -- CPU.

What is new next to MobileNet-v1: Keras's ZeroPadding2D(correct_pad) + VALID stride-2 layers, the residual Add of an inverted residual
block in the MobileNet mode, and pointwise layers of widths (16, 24, 96, 144 ... / 24, 48, 88, 136 ...) the MFMA GEMMs do not take:
zero channel padding (lowering.pad_channels) or the general kernel.  Shapes come from oracle/tf_graph.py's GraphOracle, values from the
same oracle through tests/plan_ref.py's CPU execution of the serialized plan."""
import importlib.util
import os

import numpy as np
import pytest

import gb
import keras_mobilenetv2_graph as kg
import plan_ref
from hse_facerec_tf_amd import graphdef, lowering
from oracle import tf_graph as tfo

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = "global_average_pooling2d_1/Mean:0"
MODES = [{}, {"channel_padding": "none"}, {"dtype": "f32g"}]
_GRAPHS = {}


def graph(alpha, size, style="keras", blocks=None, bn="fused"):
    key = (alpha, size, style, blocks, bn)
    if key not in _GRAPHS:
        data, info = kg.build(alpha, size, 7, style, blocks=blocks, bn=bn)
        _GRAPHS[key] = (data, info, graphdef.read_graph(data))
    return _GRAPHS[key]


def feeds_of(info):
    return {info["learning_phase"] + ":0": 0} if info["learning_phase"] else None


def test_make_divisible_gives_the_widths_of_keras_applications():
    assert [c for _, _, c, _ in kg.block_table(1.0)] == [16, 24, 24, 32, 32, 32, 64, 64, 64, 64, 96, 96, 96, 160, 160, 160, 320]
    assert sorted({c for _, _, c, _ in kg.block_table(1.4)}) == [24, 32, 48, 88, 136, 224, 448]
    assert kg.make_divisible(32 * 1.4) == 48 and kg.last_width(1.4) == 1792 and kg.last_width(1.0) == 1280 and kg.last_width(0.5) == 1280
    assert kg.correct_pad(16) == (0, 1) and kg.correct_pad(5) == (1, 1)


@pytest.mark.parametrize("opts", MODES)
@pytest.mark.parametrize("bn", ["fused", "switch"])
def test_toy_graph_lowers_and_computes_what_the_graph_does(opts, bn):
    """conv1, expanded_conv, a stride-2 block, residual blocks, Conv_1, Mean at 36 x 36: the second stride-2 depthwise sees a 9 x 9 map
    (correct_pad's odd branch), the first an 18 x 18 one.  The serialized plan, executed by tests/plan_ref.py in fp64, gives the
    oracle's features."""
    data, info, g = graph(1.0, 36, blocks=5, bn=bn)
    plan = lowering.lower_graph(g, "input_1:0", {0: OUT}, None, feeds_of(info), **opts)
    x = np.random.RandomState(0).uniform(-1, 1, (2, 36, 36, 3)).astype(np.float32)
    fd = {"input_1:0": x}
    fd.update(feeds_of(info) or {})
    want = tfo.GraphOracle(tfo.parse_graphdef(data)).run(OUT, fd)
    got = plan_ref.run(plan.serialize(), x)["features"]
    assert got.shape == (2, 1280)
    assert np.abs(got - want).max() < 1e-6 * np.abs(want).max()        # fp32 constants folded on the host, fp64 arithmetic
    kinds = [L.kind for L in plan.layers]
    if opts.get("dtype") != "f32g":
        assert kinds[0] == lowering.OP_CONV_C3 and sum(L.res >= 0 for L in plan.layers) == 2
        assert all(L.kind == lowering.OP_CONV_F32 for L in plan.layers if L.res >= 0)


def _oracle_shapes(data, info, size, names):
    x = np.zeros((1, size, size, 3), np.float32)
    fd = {"input_1:0": x}
    fd.update(feeds_of(info) or {})
    outs = tfo.GraphOracle(tfo.parse_graphdef(data), np.float32).run([n + ":0" for n in names], fd)
    return {n: tuple(o.shape[1:]) for n, o in zip(names, outs)}


@pytest.mark.parametrize("alpha,size", [(1.0, 96), (1.0, 80), (1.4, 64)])
def test_every_layer_has_the_shape_tensorflow_gives_its_tensor(alpha, size):
    """Full graphs, Keras style (Pad + VALID on Conv1 and every stride-2 depthwise).  96: even maps 48 ... 3; 80: the last stride-2
    depthwise sees a 5 x 5 map; alpha 1.4: the widths no MFMA multiple fits.  In the default mode and in f32g; with channel padding
    the height and width are TensorFlow's and the channels at least its."""
    data, info, g = graph(alpha, size)
    shapes = None
    for opts in MODES:
        plan = lowering.lower_graph(g, "input_1:0", {0: OUT}, None, **opts)
        names = sorted(n for n in plan.tensor_layer if not n.endswith("/Pad"))      # (a Pad's own tensor is listed under its producer)
        if shapes is None:
            shapes = _oracle_shapes(data, info, size, names)
        assert {plan.tensor_layer[n] for n in names} == set(range(len(plan.layers))) and len(plan.layers) > 50      # no layer goes unchecked
        for n in names:
            L = plan.layers[plan.tensor_layer[n]]
            want = shapes[n] if len(shapes[n]) == 3 else (1, 1) + shapes[n]
            if opts:
                assert tuple(L.out_shape) == want, (opts, n, L.out_shape, want)
            else:
                assert tuple(L.out_shape[:2]) == want[:2] and want[2] <= L.out_shape[2] < want[2] + 64, (n, L.out_shape, want)
        assert plan.outputs[0][1] == info["features"]
    if size == 80:
        assert shapes["block_13_depthwise_relu/Relu6"] == (3, 3, 576) and shapes["block_12_add/add"] == (5, 5, 96)


def test_keras_padded_depthwise_is_8x8_in_both_fp32_modes():
    """The depthwise branch used to drop a Pad in front of it: 7 x 7 where TensorFlow gives 8 x 8, every later layer wrong."""
    data, info, g = graph(1.0, 32, blocks=3)
    for dtype in ("f32", "f32g"):
        plan = lowering.lower_graph(g, "input_1:0", {0: OUT}, None, dtype=dtype)
        dw = plan.layers[plan.tensor_layer["block_1_depthwise_relu/Relu6"]]
        assert tuple(dw.in_shape[:2]) == (16, 16) and tuple(dw.out_shape[:2]) == (8, 8) and (dw.pad_t, dw.pad_l, dw.stride) == (0, 0, 2)
        assert lowering.same_geometry(dw)


def _pad_graph(consumer, pads=((0, 1), (0, 1)), c=8):
    b = gb.GraphBuilder()
    b.placeholder("x", [-1, 8, 8, 3])
    rs = np.random.RandomState(3)
    b.const("c/k", rs.randn(3, 3, 3, c).astype(np.float32))
    b.node("c", "Conv2D", ["x", "c/k"], strides=[1, 1, 1, 1], padding="SAME", data_format="NHWC")
    b.node("r", "Relu6", ["c"])
    b.const("p/paddings", np.array([[0, 0], list(pads[0]), list(pads[1]), [0, 0]], np.int32))
    b.node("p", "Pad", ["r", "p/paddings"])
    if consumer == "dw":
        b.const("d/k", rs.randn(3, 3, c, 1).astype(np.float32))
        b.node("out", "DepthwiseConv2dNative", ["p", "d/k"], strides=[1, 2, 2, 1], padding="VALID", data_format="NHWC")
    elif consumer == "dw_same":
        b.const("d/k", rs.randn(3, 3, c, 1).astype(np.float32))
        b.node("out", "DepthwiseConv2dNative", ["p", "d/k"], strides=[1, 2, 2, 1], padding="SAME", data_format="NHWC")
    elif consumer == "dw_behind_identity":
        b.node("i", "Identity", ["p"])
        b.const("d/k", rs.randn(3, 3, c, 1).astype(np.float32))
        b.node("out", "DepthwiseConv2dNative", ["i", "d/k"], strides=[1, 2, 2, 1], padding="VALID", data_format="NHWC")
    elif consumer == "pw":
        b.const("d/k", rs.randn(1, 1, c, 64).astype(np.float32))
        b.node("out", "Conv2D", ["p", "d/k"], strides=[1, 1, 1, 1], padding="VALID", data_format="NHWC")
    elif consumer == "mean":
        b.const("m/axes", np.array([1, 2], np.int32))
        b.node("out", "Mean", ["p", "m/axes"])
    elif consumer == "relu":
        b.node("out", "Relu", ["p"])
    elif consumer == "nobody":
        b.node("out", "Identity", ["p"])
    return b.serialize()


@pytest.mark.parametrize("dtype", ["f32", "f32g"])
def test_a_pad_is_honoured_or_refused_never_dropped(dtype):
    for pads, hw, pt in ((((0, 1), (0, 1)), 4, 0), (((1, 1), (1, 1)), 4, 1), (((2, 0), (1, 2)), 4, 2)):
        data = _pad_graph("dw", pads)
        plan = lowering.lower_graph(graphdef.read_graph(data), "x:0", {0: "out:0"}, None, dtype=dtype)
        L = plan.layers[-1]
        x = np.random.RandomState(1).uniform(-1, 1, (2, 8, 8, 3)).astype(np.float32)
        want = tfo.GraphOracle(tfo.parse_graphdef(data)).run("out:0", {"x:0": x})
        assert tuple(L.out_shape) == want.shape[1:] and (L.pad_t, L.pad_l) == (pt, pads[1][0])
        got = plan_ref.run(plan.serialize(), x)["features"].reshape(want.shape)
        assert np.abs(got - want).max() < 1e-6 * np.abs(want).max()
    # (the general convolution of f32g takes a Pad in front of any VALID kernel, a 1x1 one included; the MobileNet mode's GEMMs do not)
    for consumer in ("dw_same", "dw_behind_identity", "mean", "relu", "nobody") + (("pw",) if dtype == "f32" else ()):
        with pytest.raises(lowering.LoweringError):
            lowering.lower_graph(graphdef.read_graph(_pad_graph(consumer)), "x:0", {0: "out:0"}, None, dtype=dtype)
    with pytest.raises(lowering.LoweringError):      # a left pad the depthwise kernel's column mask does not take
        lowering.lower_graph(graphdef.read_graph(_pad_graph("dw", ((1, 1), (3, 0)))), "x:0", {0: "out:0"}, None, dtype=dtype)


def _pad_graph_bf16(consumer):
    """A graph the bf16 mode takes: Pad + VALID 7x7 / 2 stem (3 -> 64), ReLU, then a Pad ((0, 1), (0, 1)) on the 16 x 16 x 64 map
    in front of `consumer`."""
    b = gb.GraphBuilder()
    b.placeholder("x", [-1, 32, 32, 3])
    rs = np.random.RandomState(5)
    b.const("s/paddings", np.array([[0, 0], [3, 3], [3, 3], [0, 0]], np.int32))
    b.node("s/pad", "Pad", ["x", "s/paddings"])
    b.const("s/k", (rs.randn(7, 7, 3, 64) * 0.1).astype(np.float32))
    b.node("s", "Conv2D", ["s/pad", "s/k"], strides=[1, 2, 2, 1], padding="VALID", data_format="NHWC")
    b.node("r", "Relu", ["s"])
    b.const("p/paddings", np.array([[0, 0], [0, 1], [0, 1], [0, 0]], np.int32))
    b.node("p", "Pad", ["r", "p/paddings"])
    if consumer in ("dw", "dw_same", "dw_behind_identity"):
        b.const("d/k", rs.randn(3, 3, 64, 1).astype(np.float32))
        if consumer == "dw_behind_identity":
            b.node("i", "Identity", ["p"])
        b.node("out", "DepthwiseConv2dNative", ["i" if consumer == "dw_behind_identity" else "p", "d/k"], strides=[1, 2, 2, 1],
               padding="SAME" if consumer == "dw_same" else "VALID", data_format="NHWC")
    elif consumer == "conv":
        b.const("d/k", (rs.randn(3, 3, 64, 64) * 0.1).astype(np.float32))
        b.node("out", "Conv2D", ["p", "d/k"], strides=[1, 2, 2, 1], padding="VALID", data_format="NHWC")
    elif consumer == "pool":
        b.node("out", "MaxPool", ["p"], ksize=[1, 3, 3, 1], strides=[1, 2, 2, 1], padding="VALID", data_format="NHWC")
    elif consumer == "mean":
        b.const("m/axes", np.array([1, 2], np.int32))
        b.node("out", "Mean", ["p", "m/axes"])
    elif consumer == "relu":
        b.node("out", "Relu", ["p"])
    elif consumer == "nobody":
        b.node("out", "Identity", ["p"])
    return b.serialize()


def test_a_pad_is_honoured_or_refused_in_the_bf16_mode_too():
    """dtype="bf16": the general convolution and the pool take a Pad as before; the depthwise branch, which bf16 graphs share with the
    other modes, used to drop it there too (7 x 7 where TensorFlow gives 8 x 8 on a 16 x 16 map); everything else refuses."""
    x = np.zeros((1, 32, 32, 3), np.float32)
    for consumer in ("dw", "conv", "pool"):
        data = _pad_graph_bf16(consumer)
        plan = lowering.lower_graph(graphdef.read_graph(data), "x:0", {0: "out:0"}, None, dtype="bf16", fuse=False)      # (layer by layer)
        want = tfo.GraphOracle(tfo.parse_graphdef(data), np.float32).run("out:0", {"x:0": x})
        L = plan.layers[-1]
        assert want.shape[1:] == (8, 8, 64) and tuple(L.out_shape) == (8, 8, 64) and tuple(L.in_shape) == (16, 16, 64), consumer
        assert (L.pad_t, L.pad_l, L.stride) == (0, 0, 2)
    for consumer in ("dw_same", "dw_behind_identity", "mean", "relu", "nobody"):
        with pytest.raises(lowering.LoweringError):
            lowering.lower_graph(graphdef.read_graph(_pad_graph_bf16(consumer)), "x:0", {0: "out:0"}, None, dtype="bf16")


@pytest.mark.parametrize("dtype", ["f32", "f32g", "bf16"])
def test_a_pad_tensor_itself_is_refused_as_an_output(dtype):
    """No layer materialises the padded tensor: requested next to the layer that consumes the Pad, it used to come back as the
    UNPADDED tensor in front of it."""
    g = graphdef.read_graph(_pad_graph_bf16("dw") if dtype == "bf16" else _pad_graph("dw"))
    lowering.lower_graph(g, "x:0", {0: "out:0", 1: "r:0"}, None, dtype=dtype)
    with pytest.raises(lowering.LoweringError, match="Pad's own tensor"):
        lowering.lower_graph(g, "x:0", {0: "out:0", 1: "p:0"}, None, dtype=dtype)


def test_no_requested_output_is_a_padded_tensor():
    """Every block's output of a blocks=6 graph requested, three at a time: 16, 24, 24, 32, 32, 32 channels wide, none a multiple of
    64.  The plan hands out the real width, and what it computes is the oracle's tensor."""
    data, info, g = graph(1.0, 32, blocks=6)
    x = np.random.RandomState(2).uniform(-1, 1, (1, 32, 32, 3)).astype(np.float32)
    orc = tfo.GraphOracle(tfo.parse_graphdef(data))
    for i in range(0, 6, 3):
        names = info["block_outputs"][i:i + 3]
        plan = lowering.lower_graph(g, "input_1:0", {s: n + ":0" for s, n in enumerate(names)})
        want = orc.run([n + ":0" for n in names], {"input_1:0": x})
        got = plan_ref.run(plan.serialize(), x)
        for s, key in enumerate(("features", "age_probs", "gender")):
            li, elems = plan.outputs[s]
            assert elems == want[s].size and tuple(plan.layers[li].out_shape) == want[s].shape[1:]
            assert np.abs(got[key].reshape(want[s].shape) - want[s]).max() < 1e-6 * np.abs(want[s]).max()
    # ... while the tensors in between are widened
    plan = lowering.lower_graph(g, "input_1:0", {0: OUT})
    assert plan.layers[plan.tensor_layer["block_1_project_BN/FusedBatchNorm_1"]].out_shape[2] == 64


def _effective_kernel(L):
    """Kernel times the per-output-channel scale, wherever the layer keeps it: folded into the kernel (OP_CONV_C3, OP_PWCONV_F32),
    or next to it (OP_CONV_F32; a depthwise layer's is [3, 3, C, 1], so its scale runs along axis 2)."""
    w = L.w.astype(np.float64)
    if L.scale is None:
        return w
    s = L.scale.astype(np.float64)
    return w * (s.reshape(1, 1, -1, 1) if L.kind == lowering.OP_DWCONV3X3 else s.reshape(1, 1, 1, -1))


@pytest.mark.parametrize("alpha", [1.0, 1.4])
def test_padding_on_and_off_the_real_channel_weights_are_the_graphs(alpha):
    data, info, g = graph(alpha, 64)
    off = lowering.lower_graph(g, "input_1:0", {0: OUT}, fuse=False, channel_padding="none", pw_math="f32")
    on = lowering.lower_graph(g, "input_1:0", {0: OUT}, fuse=False, pw_math="f32")
    nodes = {n.name: n for n in tfo.parse_graphdef(data)}
    assert len(off.layers) == len(on.layers)
    widened = 0
    for A, B in zip(off.layers, on.layers):
        assert A.name == B.name and tuple(A.out_shape[:2]) == tuple(B.out_shape[:2])
        if A.w is None:
            continue
        # padding off: the graph's kernel, times the BatchNorm's scale where the layer folds it into the kernel
        kern = nodes[[i for i in nodes[A.name].inputs if i.endswith("kernel")][0]].attr["value"].tensor.astype(np.float64)
        bn = A.name.rsplit("/", 1)[0].replace("depthwise/depthwise", "depthwise")
        bn = {"Conv1": "bn_Conv1", "Conv_1": "Conv_1_bn"}.get(bn, bn + "_BN")
        c = [nodes["%s/%s" % (bn, k)].attr["value"].tensor.astype(np.float64) for k in ("gamma", "beta", "moving_mean", "moving_variance")]
        scale = (c[0].astype(np.float32) / np.sqrt(c[3].astype(np.float32) + np.float32(1e-3))).astype(np.float64)
        ka = _effective_kernel(A)
        assert ka.shape == kern.shape
        assert np.allclose(ka, kern * (scale.reshape(1, 1, -1, 1) if A.kind == lowering.OP_DWCONV3X3 else scale), rtol=1e-6, atol=1e-9), A.name
        # padding on: the same numbers in the real channels, exact zeros in the rest (kernel, scale and shift)
        kb = _effective_kernel(B)
        sl = tuple(slice(0, d) for d in ka.shape)
        assert np.allclose(kb[sl], ka, rtol=1e-6, atol=1e-12), A.name
        rest = kb.copy()
        rest[sl] = 0
        assert not rest.any(), A.name
        co = A.out_shape[2]
        for v in (B.scale, B.shift):
            assert v is None or not v[co:].any()
        widened += B.out_shape[2] > co
    assert widened >= 15
    assert on.outputs[0][1] == off.outputs[0][1] == info["features"]


def test_describe_names_a_product_kernel_for_every_layer():
    for alpha, size in ((1.0, 96), (1.4, 64)):
        data, info, g = graph(alpha, size)
        for opts in (MODES if alpha == 1.0 else MODES[:1]):
            plan = lowering.lower_graph(g, "input_1:0", {0: OUT}, None, **opts)
            rows = plan.describe(4)
            assert len(rows) == len(plan.layers)
            for r in rows:
                assert r["inside"] is not None or r["family"], r
                assert set(r["family"]) <= lowering.PRODUCT_KERNEL_FAMILIES, r
            fams = {f for r in rows for f in r["family"]}
            if not opts:      # the default plan: no 1x1 layer is left on the scalar general kernel
                assert "conv2d_f32_kernel" not in fams and {"conv_f32_mfma_kernel", "pwconv_f16s_kernel", "dwconv3x3_kernel"} <= fams


def test_channel_padding_rule_sends_a_wide_ratio_to_the_general_kernel():
    """pad_channels' one rule: padded / real width against CHANNEL_PAD_MAX_RATIO."""
    data, info, g = graph(1.0, 32, blocks=3)
    assert lowering.CHANNEL_PAD_MAX_RATIO >= 1.0
    for bad in ("some", 0.5, True):
        with pytest.raises(ValueError):
            lowering.lower_graph(g, "input_1:0", {0: OUT}, channel_padding=bad)
    # channel_padding=<number>: the bound in place of the constant (what tools/bench_configs.py mobilenetv2 sweeps)
    assert {L.out_shape[2] for L in lowering.lower_graph(g, "input_1:0", {0: OUT}, channel_padding=2.0).layers} == {32, 16, 128, 24, 192, 1280}
    assert ([L.out_shape for L in lowering.lower_graph(g, "input_1:0", {0: OUT}, channel_padding=lowering.CHANNEL_PAD_MAX_RATIO).layers] ==
            [L.out_shape for L in lowering.lower_graph(g, "input_1:0", {0: OUT}).layers])
    none = lowering.lower_graph(g, "input_1:0", {0: OUT}, channel_padding="none")
    assert all(L.out_shape[2] in (32, 16, 96, 24, 144, 1280) for L in none.layers)
    assert [L.kind for L in none.layers].count(lowering.OP_CONV_F32) == 6          # every 1x1 layer but none of the 3x3 ones
    # widths 16 -> 64 (x 4), 24 -> 64 (x 2.67), 96 -> 128 (x 1.33), 144 -> 192 (x 1.33): a bound of 2 leaves the first two alone
    layers = lowering.lower_graph(g, "input_1:0", {0: OUT}, channel_padding="none", fuse=False).layers
    real = lowering.pad_channels(layers, [len(layers) - 1], max_ratio=2.0)
    assert sorted(set(real.values())) == [96, 144] and {L.out_shape[2] for L in layers} == {32, 16, 128, 24, 192, 1280}
    layers = lowering.lower_graph(g, "input_1:0", {0: OUT}, channel_padding="none", fuse=False).layers
    real = lowering.pad_channels(layers, [len(layers) - 1], max_ratio=4.0)
    assert sorted(set(real.values())) == [16, 24, 96, 144] and {L.out_shape[2] for L in layers} == {32, 64, 128, 192, 1280}


def test_existing_plans_are_untouched():
    """tools/plan_digest.py's digests of the shipped MobileNet-v1 plan at 192 x 192 and of three ResNet-style plans -- the general mode's
    residual Add and its Pad + VALID stem and pool run through the branches this family's lowering shares with them -- computed on the
    commit before MobileNetV2 support."""
    spec = importlib.util.spec_from_file_location("plan_digest", os.path.join(ROOT, "tools", "plan_digest.py"))
    pd = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(pd)
    g = graphdef.read_graph(pd.MODEL_PB)
    plan = lowering.lower_graph(g, "input_1:0", pd.ALL_OUTS, (192, 192))
    assert pd.digest(plan) == "53cda981b4d8c0a518670ffda8f96df641f8e4876a39152c57413830b5ea9517"
    plan = lowering.lower_graph(g, "input_1:0", pd.ALL_OUTS, (192, 192), input_bound=256.0)
    assert pd.digest(plan) == "e698cad995c511e7a3a27daa3f3912afa96e8ffcc4f07cd5376c6672e4bfc291"
    for (pool, bn, head, hw), dtype, want in (
            (("SAME", "fused", "avgpool", 40), "bf16", "a2f21f888538191945cb5cac8fd429552cbd2df56379f72924c2da1f383513a0"),
            (("PADVALID", "muladd", "mean", 38), "f32g", "b343079cfbdf54557e1e917aae57949192ca7cf9eb590cdfaf2b92a916c5a79d")):
        mg = graphdef.read_graph(pd.mini_resnet_graph.build(3, hw, pool, bn, 64, head)[0])
        plan = lowering.lower_graph(mg, "input:0", {0: "pool5_7x7_s1:0"}, dtype=dtype, fuse=True, launch_fusion=True)
        assert pd.digest(plan) == want, (pool, dtype)
    plan = pd.resnet50.build_plan(pd.resnet50.synthetic_weights(7), (64, 64), "caffe", dtype="bf16", fuse=True, pair=True, subsample=True)
    assert pd.digest(plan) == "bac4f1250d042e7d3e15ff03e7e531826a4676e991fed42eb4972545fa6e7d9f"


def test_registry_rows_of_the_reference(tmp_path):
    """facerec_test.py:216-217: file names, tensor names and convert2BGR=False (missing files: FileNotFoundError, as for the other rows)."""
    from hse_facerec_tf_amd import get_tf_face_recognizer
    for name, fname in (("mobilenet2", "mobilenet2_alpha=1_192_augm_ft_sgd.pb"), ("vgg2_mobilenet2", "vgg2_mobilenet2_224-08-0.87.pb")):
        with pytest.raises(FileNotFoundError) as e:
            get_tf_face_recognizer(name, models_dir=str(tmp_path))
        assert fname in str(e.value)
