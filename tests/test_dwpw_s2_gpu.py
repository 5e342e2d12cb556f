"""The stride-2 depthwise -> pointwise launch (csrc/dwpw_f16s.hip, dwpws2_f16s_kernel: 128 -> 256 channels, 8 x 8 output patches, one
persistent workgroup per CU) at op level: bit for bit the two launches it replaces (ops.dwconv3x3 + ops.pwconv1x1_f16split), and the
fp64 oracle at the project's fp32_grade bar.  Shapes are the smallest at which the kernel can go wrong: one exact patch, an odd map
(top / left padding, partial patches both ways), a map smaller than a patch, several patches with a partial last row and column, each
at three images (at most 27 work items: one per workgroup).  A workgroup walks SEVERAL items only beyond 256 of them: 320 one-patch
images (every item the same geometry), and 48 odd 19 x 35 images of six patches each -- 288 items, so the workgroups that take a
second one meet a patch of another position, another image and other padding factors under their load and compute cursors."""
import numpy as np
import pytest

from oracle import tf_graph as tfo
from test_e2e_gpu import fp32_grade  # noqa: E402  (the element-wise form of the bar)

pytestmark = pytest.mark.gpu

C, COUT = 128, 256
KERNEL = "dwpws2_f16s_kernel"
SHAPES = [(16, 16), (15, 13), (6, 6), (20, 36)]      # input maps -> 8x8, 8x7, 3x3, 10x18


@pytest.fixture(scope="module")
def env():
    import torch
    from hse_facerec_tf_amd import ops
    assert torch.cuda.is_available()
    return torch, ops


def dev(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).cuda()


def act_np(v, act):
    return np.minimum(np.maximum(v, 0), 6) if act == 2 else v


_CASES = {}


def case(torch, ops, n, h, w, c=C, cout=COUT):
    """Operands on the device, the fp64 depthwise result and the two-launch outputs per activation: computed once, shared, never changed."""
    key = (n, h, w, c, cout)
    if key not in _CASES:
        rs = np.random.RandomState(h * 131 + w * 7 + n + c)
        t = {"x": rs.uniform(0, 6, (n, h, w, c)).astype(np.float32), "kd": (rs.randn(3, 3, c, 1) / 3).astype(np.float32),
             "sc": rs.uniform(0.2, 2, c).astype(np.float32), "sh": rs.randn(c).astype(np.float32),
             "kp": (rs.randn(c, cout) / np.sqrt(c)).astype(np.float32), "psh": rs.randn(cout).astype(np.float32)}
        t["mid"] = act_np(tfo.depthwise_conv2d(t["x"].astype(np.float64), t["kd"], (2, 2), "SAME") * t["sc"] + t["sh"], 2)
        t["d"] = {k: dev(torch, t[k].reshape(3, 3, c) if k == "kd" else t[k]) for k in ("x", "kd", "sc", "sh", "psh")}
        t["prep"] = ops.split_weights_device(dev(torch, t["kp"].T), t["d"]["x"].device)
        t["two"], t["want"] = {}, {}
        _CASES[key] = t
    return _CASES[key]


def two_launches(ops, t, act):
    if act not in t["two"]:
        d = t["d"]
        t["two"][act] = ops.pwconv1x1_f16split(ops.dwconv3x3(d["x"], d["kd"], d["sc"], d["sh"], 2), None, d["psh"], act, prepared=t["prep"])
        mid = t["mid"]
        t["want"][act] = act_np(mid.reshape(-1, mid.shape[3]).dot(t["kp"].astype(np.float64)) + t["psh"], act).reshape(mid.shape[:3] + (-1,))
    return t["two"][act], t["want"][act]


def fused(ops, t, act):
    d = t["d"]
    return ops.dwpw_f16split(d["x"], d["kd"], d["sc"], d["sh"], None, d["psh"], 2, act, prepared=t["prep"])


@pytest.mark.parametrize("act", [2, 0], ids=["relu6", "none"])
@pytest.mark.parametrize("hw", SHAPES, ids=lambda s: "%dx%d" % s)
def test_one_launch_is_the_two_launches_bit_for_bit_and_fp32_grade(env, hw, act):
    torch, ops = env
    t = case(torch, ops, 3, hw[0], hw[1])
    y2, want = two_launches(ops, t, act)
    y = fused(ops, t, act)
    assert tuple(y.shape) == want.shape == (3, (hw[0] + 1) // 2, (hw[1] + 1) // 2, COUT)
    assert torch.equal(y, y2)
    fp32_grade(y.cpu().numpy(), want, "dwpw s2 %dx%d act %d" % (hw + (act,)))


def test_more_work_items_than_resident_workgroups(env):
    torch, ops = env
    t = case(torch, ops, 320, 16, 16)
    y2, want = two_launches(ops, t, 2)
    y = fused(ops, t, 2)
    assert torch.equal(y, y2)
    fp32_grade(y.cpu().numpy(), want, "dwpw s2 320 x 16x16")


def test_a_workgroup_walks_items_of_differing_odd_patches(env):
    """19 x 35 -> 10 x 18: top / left padding, 2 x 3 patches per image with a partial last row and column; 48 images = 288 items on 256
    workgroups, so 32 of them take two items that differ in position, image and padding."""
    torch, ops = env
    t = case(torch, ops, 48, 19, 35)
    y2, want = two_launches(ops, t, 2)
    y = fused(ops, t, 2)
    assert tuple(y.shape) == (48, 10, 18, COUT)
    assert torch.equal(y, y2)
    fp32_grade(y.cpu().numpy(), want, "dwpw s2 48 x 19x35")


def test_three_launches_agree_bit_for_bit(env):
    torch, ops = env
    t = case(torch, ops, 3, 20, 36)
    ys = [fused(ops, t, 2).clone() for _ in range(3)]
    assert torch.equal(ys[0], ys[1]) and torch.equal(ys[0], ys[2])


def pair_plan(t, h, w, lead, s2):
    """A plan of the pair alone (the engine's first launch sweeps forwards) or behind a stride-1 depthwise layer (its second launch
    sweeps backwards): lowering's own pass marks it."""
    from hse_facerec_tf_amd import lowering, ops
    L = lowering.Layer
    oh, ow, pt, pl = ops._same(h, w, 3, 2)
    layers = []
    if lead:
        layers.append(L(lowering.OP_DWCONV3X3, "lead", -1, (h, w, C), (h, w, C), w=t["kd"], scale=t["sc"], shift=t["sh"], act=lowering.ACT_RELU6,
                        kh=3, kw=3, stride=1, pad_t=1, pad_l=1))
    layers.append(L(lowering.OP_DWCONV3X3, "dw", len(layers) - 1, (h, w, C), (oh, ow, C), w=t["kd"], scale=t["sc"], shift=t["sh"],
                    act=lowering.ACT_RELU6, kh=3, kw=3, stride=2, pad_t=pt, pad_l=pl))
    layers.append(L(lowering.OP_PWCONV_F32, "pw", len(layers) - 1, (oh, ow, C), (oh, ow, COUT), w=t["kp"].reshape(1, 1, C, COUT), shift=t["psh"],
                    act=lowering.ACT_RELU6, a_log2=12))
    out = len(layers) - 1
    assert lowering.mark_dwpw_pairs(layers, [out]) == 1
    if not s2:
        layers[out - 1].flags = 0
    return lowering.Plan(layers, (h, w, C), lowering.assign_buffers(layers, {out}), {0: (out, oh * ow * COUT)}, {})


@pytest.mark.parametrize("lead", [False, True], ids=["forwards", "backwards"])
def test_both_sweep_directions_through_the_engine(env, lead):
    torch, ops = env
    from hse_facerec_tf_amd.engine import Engine
    h, w = 20, 36
    t = case(torch, ops, 3, h, w)
    d = t["d"]
    plan = pair_plan(t, h, w, lead, True)
    rows = plan.describe(3)
    assert rows[-2]["family"] == [KERNEL] and rows[-1]["inside"] == len(rows) - 2
    x = ops.dwconv3x3(d["x"], d["kd"], d["sc"], d["sh"], 1) if lead else d["x"]
    want = ops.pwconv1x1_f16split(ops.dwconv3x3(x, d["kd"], d["sc"], d["sh"], 2), None, d["psh"], 2, prepared=t["prep"])
    outs = []
    for s2 in (True, False):
        eng = Engine(pair_plan(t, h, w, lead, s2), max_batch=3)
        outs.append(eng.forward(d["x"], (0,))["features"].clone())
        eng.close()
    assert torch.equal(outs[0], outs[1])
    assert torch.equal(outs[0].reshape(want.shape), want)


def test_forced_old_route_gives_the_same_bits(env):
    torch, ops = env
    from hse_facerec_tf_amd import _lib
    if not hasattr(_lib.lib(), "hsefr_debug_set"):
        pytest.skip("the dwpw_s2_off knob exists in development builds of the library only")
    t = case(torch, ops, 3, 15, 13)
    y = fused(ops, t, 2)
    _lib.check(_lib.lib().hsefr_debug_set(b"dwpw_s2_off", 1))
    try:
        y_old = fused(ops, t, 2)
    finally:
        _lib.check(_lib.lib().hsefr_debug_set(b"dwpw_s2_off", 0))
    assert torch.equal(y, y_old)


def test_an_uncovered_shape_keeps_the_general_kernel(env):
    torch, ops = env
    t = case(torch, ops, 2, 15, 13, c=96)
    y2, want = two_launches(ops, t, 2)
    y = fused(ops, t, 2)
    assert torch.equal(y, y2)
    fp32_grade(y.cpu().numpy(), want, "dwpw s2 c=96")
