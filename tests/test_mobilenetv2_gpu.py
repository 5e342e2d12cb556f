"""MobileNetV2 graphs (tests/keras_mobilenetv2_graph.py) on the GPU against oracle/tf_graph.py's GraphOracle in fp64.

Bar, as for the other models (tests/test_e2e_gpu.py): every element above 1e-2 of the tensor's maximum within 1e-4 relative of the oracle's,
and the whole tensor within 1e-5 of its scale.  The max-norm figure (max|a - b| / max|b|) of every comparison is recorded and printed when
the module is done (-s shows it)."""
import os

import numpy as np
import pytest

import keras_mobilenetv2_graph as kg
from oracle import tf_graph as tfo

pytestmark = pytest.mark.gpu

BAR = 1e-4
BAR_MAXNORM = 1e-5
OUT = "global_average_pooling2d_1/Mean:0"
TEST_IMAGE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "test_image.jpg")
MAXNORM = {}
_CASES = {}


def grade(got, want, what):
    a, b = np.asarray(got, np.float64).reshape(-1), np.asarray(want, np.float64).reshape(-1)
    assert a.shape == b.shape, (what, a.shape, b.shape)
    scale = np.abs(b).max() + 1e-30
    err = np.abs(a - b)
    big = np.abs(b) > 1e-2 * scale
    worst = float((err[big] / np.abs(b)[big]).max())
    MAXNORM[what] = float(err.max() / scale)
    print("%s: worst relative error above 1e-2 of the maximum %.3g, max-norm %.3g" % (what, worst, MAXNORM[what]))
    assert worst < BAR, "%s: element-wise relative error %.3g (max-norm %.3g)" % (what, worst, MAXNORM[what])
    assert MAXNORM[what] < BAR_MAXNORM, "%s: max-norm error %.3g" % (what, MAXNORM[what])


def case(alpha, size, style, batch, blocks=None, fetch=(OUT,)):
    """(graph bytes, info, parsed graph, input, the oracle's tensors): built once, shared, never written to."""
    key = (alpha, size, style, batch, blocks, tuple(fetch))
    if key not in _CASES:
        from hse_facerec_tf_amd import graphdef
        data, info = kg.build(alpha, size, 11, style, blocks=blocks)
        x = np.random.RandomState(size + batch).uniform(-1, 1, (batch, size, size, 3)).astype(np.float32)
        if batch >= 3:
            x[2] = x[0]
        want = tfo.GraphOracle(tfo.parse_graphdef(data), np.float64).run(list(fetch), {"input_1:0": x})
        for a in (x, *want):
            a.setflags(write=False)
        _CASES[key] = (data, info, graphdef.read_graph(data), x, want)
    return _CASES[key]


@pytest.fixture(scope="module")
def torch_():
    import torch
    assert torch.cuda.is_available()
    yield torch
    for what, v in MAXNORM.items():      # the record: whatever subset of this module ran
        print("max-norm %-70s %.3g" % (what, v))


def run(torch_, plan, x, slots=(0,)):
    from hse_facerec_tf_amd.engine import Engine
    eng = Engine(plan, max_batch=x.shape[0])
    out = eng.forward(torch_.from_numpy(x.copy()).cuda(), slots)      # (the shared input is read-only)
    res = [out[k].cpu().numpy() for k in ("features", "age_probs", "gender")[:len(slots)]]
    eng.close()
    return res


@pytest.mark.parametrize("opts", [{}, {"channel_padding": "none"}, {"dtype": "f32g"}], ids=["default", "unpadded", "f32g"])
@pytest.mark.parametrize("size", [96, 80])
def test_full_graph_features_in_every_mode(torch_, size, opts):
    """Alpha 1.0, Keras style, batch 3.  96 x 96: even maps 48 ... 3; 80 x 80: correct_pad's odd branch (the last stride-2 depthwise sees
    5 x 5).  The default plan (channel padding, split-f16 and fp32 MFMA GEMMs, residuals on conv_f32_mfma), the plan without channel
    padding and the fp32-grade general mode meet the same bar on the same input; images 0 and 2 are one image and get the same bits."""
    from hse_facerec_tf_amd import lowering
    data, info, g, x, want = case(1.0, size, "keras", 3)
    plan = lowering.lower_graph(g, "input_1:0", {0: OUT}, None, **opts)
    got = run(torch_, plan, x)[0]
    assert got.shape == (3, 1280)
    grade(got, want[0], "alpha 1.0 %d %s" % (size, opts or "default"))
    assert np.array_equal(got[0], got[2])


@pytest.mark.parametrize("opts", [{}, {"channel_padding": "none"}, {"dtype": "f32g"}], ids=["default", "unpadded", "f32g"])
@pytest.mark.parametrize("alpha,size", [(1.0, 96), (1.4, 64)])
def test_an_image_gets_the_same_bits_whatever_its_batch(torch_, alpha, size, opts):
    """The bulk paths promise that an image's embedding does not depend on how the images were batched.  Pinned here for the routes the
    MobileNetV2 plans add: conv_f32_mfma with a residual, the pointwise GEMMs on zero-padded widths, conv2d_f32 at a layer's own width --
    one engine, the first image alone, the first two, and the whole batch."""
    from hse_facerec_tf_amd import lowering
    from hse_facerec_tf_amd.engine import Engine
    data, info, g, x, want = case(alpha, size, "keras", 3 if alpha == 1.0 else 2)
    eng = Engine(lowering.lower_graph(g, "input_1:0", {0: OUT}, None, **opts), max_batch=x.shape[0])
    xd = torch_.from_numpy(x.copy()).cuda()
    full = eng.forward(xd)["features"].clone()
    for n in range(1, x.shape[0]):
        assert torch_.equal(eng.forward(xd[:n].contiguous())["features"], full[:n]), "batch of %d" % n
    assert torch_.equal(eng.forward(xd[-1:].contiguous())["features"], full[-1:])
    eng.close()


def test_alpha_1_4_widths(torch_):
    """Widths 24 / 48 / 88 / 136 (expanded: 144, 288, 528, 816): the ones no MFMA multiple fits."""
    from hse_facerec_tf_amd import lowering
    data, info, g, x, want = case(1.4, 64, "keras", 2)
    assert {24, 48, 88, 136} <= set(info["widths"])
    for opts in ({}, {"channel_padding": "none"}):
        got = run(torch_, lowering.lower_graph(g, "input_1:0", {0: OUT}, None, **opts), x)[0]
        assert got.shape == (2, 1792)
        grade(got, want[0], "alpha 1.4 64 %s" % (opts or "default"))


def test_slim_style_graph(torch_):
    from hse_facerec_tf_amd import lowering
    data, info, g, x, want = case(1.0, 96, "slim", 3)
    got = run(torch_, lowering.lower_graph(g, "input_1:0", {0: OUT}), x)[0]
    grade(got, want[0], "alpha 1.0 96 slim")
    assert np.array_equal(got[0], got[2])


@pytest.mark.parametrize("style", ["keras", "slim"])
def test_every_block_output_as_an_intermediate(torch_, style):
    """blocks=4 at 32 x 32: expanded_conv (16 wide), the stride-2 block_1, the residual block_2, the stride-2 block_3 -- each block's
    output tensor requested next to the features, so a wrong pad or residual is located at its block."""
    from hse_facerec_tf_amd import lowering
    names = kg.build(1.0, 32, 11, style, blocks=4)[1]["block_outputs"]
    data, info, g, x, want = case(1.0, 32, style, 3, 4, tuple(n + ":0" for n in names) + (OUT,))
    for opts in ({}, {"channel_padding": "none"}):
        for pair in (names[:2], names[2:]):
            plan = lowering.lower_graph(g, "input_1:0", {0: OUT, 1: pair[0] + ":0", 2: pair[1] + ":0"}, None, **opts)
            feats, a, b = run(torch_, plan, x, (0, 1, 2))
            grade(a, want[names.index(pair[0])], "%s %s %s" % (style, pair[0], opts or "default"))
            grade(b, want[names.index(pair[1])], "%s %s %s" % (style, pair[1], opts or "default"))
            grade(feats, want[-1], "%s features next to %s %s" % (style, pair[0], opts or "default"))


@pytest.mark.parametrize("output", ["global_average_pooling2d_1/Mean", "reshape_1/Mean"])
def test_tensorflow_inference_entry_points(torch_, tmp_path, output):
    """facerec_test.py:216-217: TensorFlowInference(pb, 'input_1:0', '<output>:0', convert2BGR=False) -- x / 127.5 - 1 on RGB.  The
    file-path call equals the batched path on the same image, on the host-preprocess and the device-preprocess routes, and the batched
    path equals the oracle."""
    from hse_facerec_tf_amd import TensorFlowInference, preprocess
    data, info = kg.build(1.0, 96, 11, "keras", output=output)
    pb = tmp_path / "mobilenet2.pb"
    pb.write_bytes(data)
    tfi = TensorFlowInference(str(pb), 'input_1:0', output + ':0', convert2BGR=False, max_batch=4)
    assert (tfi.w, tfi.h) == (96, 96) and tfi.feature_dim == 1280 and tfi.dtype == "f32" and not tfi.engine.accepts_u8
    f1 = tfi.extract_features(TEST_IMAGE)
    x = tfi.preprocess_image(TEST_IMAGE, False).astype(np.float32)
    assert x.min() >= -1.0 and x.max() <= 1.0
    fb = tfi.extract_batch(np.stack([x, x]))
    # one image alone and in a batch of two: one plan, and an image's bits do not depend on its batch
    assert f1.shape == (1280,) and np.array_equal(fb[0], f1) and np.array_equal(fb[1], f1)
    want = tfo.GraphOracle(tfo.parse_graphdef(data), np.float64).run(output + ":0", {"input_1:0": x[None]})
    grade(f1, want, "extract_features %s" % output)
    grade(fb[0], want, "extract_batch %s" % output)
    img = preprocess.imread_rgb(TEST_IMAGE)
    fd = tfi.extract_images(img[None]).cpu().numpy()[0]        # resize and x / 127.5 - 1 on the device
    grade(fd, want, "extract_images %s" % output)
    tfi.close_session()
