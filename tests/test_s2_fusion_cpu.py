"""The stride-2 depthwise -> pointwise launch fusion without a GPU: what lowering.mark_dwpw_pairs flags, what Plan.describe reports,
that the flag changes nothing the plan computes (tests/plan_ref.py), and what hsefr_plan_validate refuses."""
import numpy as np
import pytest

from conftest import MODEL_PB
from hse_facerec_tf_amd import _lib, graphdef, lowering

FEAT = "global_pooling/Mean:0"
DW4 = "conv_dw_4/depthwise"
DW4_RELU = "conv_dw_4_relu/clip_by_value:0"


def lower(size=192, fetch=None, **kw):
    return lowering.lower_graph(graphdef.read_graph(MODEL_PB), "input_1:0", fetch or {0: FEAT}, (size, size), **kw)


def flagged(plan):
    return [L.name for L in plan.layers if L.flags & lowering.OPF_DWPW_NEXT]


@pytest.mark.parametrize("size", [192, 224])
def test_the_pass_flags_exactly_conv_dw_4(size):
    plan, plain = lower(size), lower(size, s2_fusion="none")
    assert flagged(plan) == [DW4] and flagged(plain) == []
    assert [(L.kind, L.name) for L in plan.layers] == [(L.kind, L.name) for L in plain.layers]
    assert plan.bytes_per_image() == plain.bytes_per_image() and plan.flops_per_image() == plain.flops_per_image()


def test_the_pass_flags_nothing_where_the_pair_must_stay_two_launches():
    asked = lower(fetch={0: FEAT, 1: DW4_RELU})          # conv_dw_4_relu is a requested output: its tensor must be written
    assert asked.layers[asked.outputs[1][0]].name == DW4 and flagged(asked) == []
    assert flagged(lower(pw_math="f32")) == []
    assert flagged(lower(s2_fusion="none")) == []
    with pytest.raises(ValueError):
        lower(s2_fusion="all")


def test_describe_names_the_kernel_and_shows_conv_pw_4_inside_it():
    plan = lower()
    rows = plan.describe(256)
    i = [r["layer"] for r in rows if r["name"] == DW4][0]
    assert rows[i]["family"] == ["dwpws2_f16s_kernel"] and rows[i]["inside"] is None
    assert rows[i + 1]["name"].startswith("conv_pw_4") and rows[i + 1]["inside"] == i and rows[i + 1]["kernels"] == []
    plain = lower(s2_fusion="none").describe(256)
    assert plain[i]["family"] == ["dwconv3x3_kernel"] and plain[i + 1]["family"] == ["pwconv_f16s_kernel"]


def test_the_flag_changes_nothing_the_plan_computes():
    import plan_ref
    x = np.random.RandomState(5).uniform(-128, 128, (1, 96, 96, 3)).astype(np.float32)
    outs = [plan_ref.run(lower(96, s2_fusion=s2).serialize(), x) for s2 in ("auto", "none")]
    assert flagged(lower(96)) == [DW4]
    assert np.array_equal(outs[0]["features"], outs[1]["features"]) and outs[0]["features"].shape == (1, 1024)


def pair_layers(dw_stride=2, extra_reader=False, lead=False):
    L = lowering.Layer
    rs = np.random.RandomState(3)
    h = w = 16
    oh = ow = h // dw_stride
    kd, sc, sh = rs.randn(3, 3, 128, 1).astype(np.float32), np.ones(128, np.float32), np.zeros(128, np.float32)
    kp, psh = rs.randn(1, 1, 128, 256).astype(np.float32), np.zeros(256, np.float32)
    layers = []
    if lead:
        layers.append(L(lowering.OP_DWCONV3X3, "lead", -1, (h, w, 128), (h, w, 128), w=kd, scale=sc, shift=sh, act=lowering.ACT_RELU6, kh=3, kw=3,
                        stride=1, pad_t=1, pad_l=1))
    layers.append(L(lowering.OP_DWCONV3X3, "dw", len(layers) - 1, (h, w, 128), (oh, ow, 128), w=kd, scale=sc, shift=sh, act=lowering.ACT_RELU6,
                    kh=3, kw=3, stride=dw_stride, pad_t=2 - dw_stride, pad_l=2 - dw_stride, flags=lowering.OPF_DWPW_NEXT))
    dw = len(layers) - 1
    layers.append(L(lowering.OP_PWCONV_F32, "pw", dw, (oh, ow, 128), (oh, ow, 256), w=kp, shift=psh, act=lowering.ACT_RELU6, a_log2=12))
    if extra_reader:
        layers.append(L(lowering.OP_PWCONV_F32, "pw_b", dw, (oh, ow, 128), (oh, ow, 256), w=kp, shift=psh, act=lowering.ACT_RELU6, a_log2=12))
    return layers


def validate(layers):
    out = len(layers) - 1
    plan = lowering.Plan(layers, (16, 16, 128), lowering.assign_buffers(layers, {out}), {0: (out, int(np.prod(layers[out].out_shape)))}, {})
    blob = plan.serialize()
    return _lib.lib().hsefr_plan_validate(blob, len(blob)), _lib.last_error()


def test_validate_accepts_the_pattern_and_refuses_everything_else():
    rc, msg = validate(pair_layers())
    assert rc == 0, msg
    cases = {"a stride-1 depthwise": pair_layers(dw_stride=1), "a third reader": pair_layers(extra_reader=True)}
    other = pair_layers(lead=True)
    other[2].src = 0                                   # the next op reads another buffer (the lead layer's, the same shape class)
    other[2].in_shape = (16, 16, 128)
    other[2].out_shape = (16, 16, 256)
    cases["a next op that reads another buffer"] = other
    busy = pair_layers()
    busy[1].flags = lowering.OPF_HEADS
    cases["a second op with flags"] = busy
    for what, layers in cases.items():
        rc, msg = validate(layers)
        assert rc == _lib.ERR_INVALID and "DWPW_NEXT" in msg, (what, rc, msg)
