"""The pointwise -> stride-1 block launch fusion (conv_pw_2 -> conv_dw_3 + conv_pw_3) without a GPU: what lowering.mark_pw_blocks flags, what
Plan.describe reports, that the flag changes nothing the plan computes (tests/plan_ref.py), and what hsefr_plan_validate refuses."""
import numpy as np
import pytest

from conftest import MODEL_PB
from hse_facerec_tf_amd import _lib, graphdef, lowering

FEAT = "global_pooling/Mean:0"
PW2 = "conv_pw_2"
PW2_RELU = "conv_pw_2_relu/clip_by_value:0"
KERNEL = "pwblk_stream_f16s_kernel"


def lower(size=192, fetch=None, **kw):
    return lowering.lower_graph(graphdef.read_graph(MODEL_PB), "input_1:0", fetch or {0: FEAT}, (size, size), **kw)


def flagged(plan):
    return [L.name for L in plan.layers if L.flags & lowering.OPF_PWBLK_NEXT]


def test_the_pass_flags_exactly_conv_pw_2_at_192():
    plan, plain = lower(192), lower(192, pw_block_fusion="none")
    names = flagged(plan)
    assert len(names) == 1 and names[0].startswith(PW2) and flagged(plain) == []
    i = [L.name for L in plan.layers].index(names[0])
    pw, blk = plan.layers[i], plan.layers[i + 1]
    assert tuple(pw.in_shape) == (48, 48, 64) and tuple(pw.out_shape) == (48, 48, 128) and blk.kind == lowering.OP_DWPW_F16S
    assert tuple(blk.out_shape) == (48, 48, 128) and blk.name.startswith("conv_pw_3")
    assert [(L.kind, L.name) for L in plan.layers] == [(L.kind, L.name) for L in plain.layers]
    assert plan.bytes_per_image() == plain.bytes_per_image() and plan.flops_per_image() == plain.flops_per_image()
    assert KERNEL in lowering.PRODUCT_KERNEL_FAMILIES


def test_the_224_plan_keeps_two_launches():
    """Its rows are 56 pixels: two ring rows of 58 cells do not fit beside the stages (DESIGN.md lesson 74)."""
    plan = lower(224)
    assert flagged(plan) == [] and lowering.PW_BLOCK_MAX_W == 48
    assert [tuple(L.out_shape) for L in plan.layers if L.name.startswith(PW2)] == [(56, 56, 128)]


def test_the_pass_flags_nothing_where_the_pair_must_stay_two_launches():
    asked = lower(fetch={0: FEAT, 1: PW2_RELU})          # conv_pw_2's tensor is a requested output: it must be written
    assert asked.layers[asked.outputs[1][0]].name.startswith(PW2) and flagged(asked) == []
    assert flagged(lower(pw_math="f32")) == []
    assert flagged(lower(launch_fusion=False)) == []
    assert flagged(lower(pw_block_fusion="none")) == []
    with pytest.raises(ValueError):
        lower(pw_block_fusion="all")


def test_describe_names_the_kernel_and_shows_the_block_inside_it():
    plan = lower()
    rows = plan.describe(256)
    i = [r["layer"] for r in rows if r["name"].startswith(PW2)][0]
    assert rows[i]["family"] == [KERNEL] and rows[i]["inside"] is None
    assert rows[i + 1]["name"].startswith("conv_pw_3") and rows[i + 1]["inside"] == i and rows[i + 1]["kernels"] == []
    plain = lower(pw_block_fusion="none").describe(256)
    assert plain[i]["family"] == ["pwconv_f16s_kernel"] and plain[i + 1]["family"] == ["dwpw3_f16s_kernel"]
    assert sum(1 for r in rows if r["kernels"]) == sum(1 for r in plain if r["kernels"]) - 1


def test_the_flag_changes_nothing_the_plan_computes():
    import plan_ref
    x = np.random.RandomState(5).uniform(-128, 128, (1, 96, 96, 3)).astype(np.float32)
    outs = [plan_ref.run(lower(96, pw_block_fusion=f).serialize(), x) for f in ("auto", "none")]
    assert len(flagged(lower(96))) == 1
    assert np.array_equal(outs[0]["features"], outs[1]["features"]) and outs[0]["features"].shape == (1, 1024)


def block_layers(blk_stride=1, extra_reader=False, lead=False, second_flag=False):
    L = lowering.Layer
    rs = np.random.RandomState(3)
    h = w = 16
    oh = ow = h // blk_stride
    k2, s2 = rs.randn(1, 1, 64, 128).astype(np.float32), np.zeros(128, np.float32)
    kd, sc, sh = rs.randn(3, 3, 128, 1).astype(np.float32), np.ones(128, np.float32), np.zeros(128, np.float32)
    k3, s3 = rs.randn(1, 1, 128, 128).astype(np.float32), np.zeros(128, np.float32)
    layers = []
    if lead:
        layers.append(L(lowering.OP_PWCONV_F32, "lead", -1, (h, w, 64), (h, w, 128), w=k2, shift=s2, act=lowering.ACT_RELU6, a_log2=12))
    layers.append(L(lowering.OP_PWCONV_F32, "pw", -1, (h, w, 64), (h, w, 128), w=k2, shift=s2, act=lowering.ACT_RELU6, a_log2=12,
                    flags=lowering.OPF_PWBLK_NEXT))
    pw = len(layers) - 1
    layers.append(L(lowering.OP_DWPW_F16S, "blk", pw, (h, w, 128), (oh, ow, 128), w=kd, scale=sc, shift=sh, act=lowering.ACT_RELU6, kh=3, kw=3,
                    stride=blk_stride, pad_t=2 - blk_stride, pad_l=2 - blk_stride, sealed=True, w2=k3, shift2=s3, a_log2=12,
                    flags=lowering.OPF_PWBLK_NEXT if second_flag else 0))
    if extra_reader:
        layers.append(L(lowering.OP_DWPW_F16S, "blk_b", pw, (h, w, 128), (h, w, 128), w=kd, scale=sc, shift=sh, act=lowering.ACT_RELU6, kh=3, kw=3,
                        stride=1, pad_t=1, pad_l=1, sealed=True, w2=k3, shift2=s3, a_log2=12))
    return layers


def validate(layers):
    out = len(layers) - 1
    plan = lowering.Plan(layers, (16, 16, 64), lowering.assign_buffers(layers, {out}), {0: (out, int(np.prod(layers[out].out_shape)))}, {})
    blob = plan.serialize()
    return _lib.lib().hsefr_plan_validate(blob, len(blob)), _lib.last_error()


def test_the_marking_pass_agrees_with_the_hand_made_pattern():
    layers = block_layers()
    layers[0].flags = 0
    assert lowering.mark_pw_blocks(layers, [1]) == 1 and layers[0].flags == lowering.OPF_PWBLK_NEXT
    layers = block_layers(blk_stride=2)
    layers[0].flags = 0
    assert lowering.mark_pw_blocks(layers, [1]) == 0


def test_validate_accepts_the_pattern_and_refuses_everything_else():
    rc, msg = validate(block_layers())
    assert rc == 0, msg
    cases = {"a stride-2 block": block_layers(blk_stride=2), "a third reader": block_layers(extra_reader=True),
             "a second flagged op": block_layers(second_flag=True)}
    other = block_layers(lead=True)
    other[2].src = 0                                   # the block reads another buffer (the lead layer's, the same shape)
    cases["a next op that reads another buffer"] = other
    for what, layers in cases.items():
        rc, msg = validate(layers)
        assert rc == _lib.ERR_INVALID and "PWBLK_NEXT" in msg, (what, rc, msg)
