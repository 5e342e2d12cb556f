"""conv_pw_2 + the stride-1 depthwise-pointwise block as one row-streaming launch (csrc/pwblk_stream.hip, pwblk_stream_f16s_kernel:
64 -> 128 -> 128 channels, rows of at most 48 pixels, one persistent workgroup per CU) at op level: bit for bit the two launches it
replaces (ops.pwconv1x1_f16split + ops.dwpw_f16split, stride 1), and the fp64 oracle at the project's fp32_grade bar.  Shapes are the
smallest at which the kernel can go wrong: a one-row map (both row paddings meet in one depthwise step), an odd width below one 32-pixel
column block, one pixel past a block, the workload's 48-pixel row -- three images each, which the launcher splits into row segments.
A workgroup walks SEVERAL items only beyond 256 of them: 300 one-segment images, and 130 images in two segments of differing length."""
import numpy as np
import pytest

from oracle import tf_graph as tfo
from test_e2e_gpu import fp32_grade  # noqa: E402  (the element-wise form of the bar)

pytestmark = pytest.mark.gpu

CIN, C, COUT = 64, 128, 128
KERNEL = "pwblk_stream_f16s_kernel"
SHAPES = [(1, 16), (2, 13), (5, 33), (7, 48)]


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


def case(torch, ops, n, h, w, cin=CIN, c=C, cout=COUT):
    """Operands on the device, the fp64 depthwise result and the two-launch outputs per activation: computed once, shared, never changed."""
    key = (n, h, w, cin, c, cout)
    if key not in _CASES:
        rs = np.random.RandomState(h * 131 + w * 7 + n + c + cin)
        t = {"x": rs.uniform(0, 6, (n, h, w, cin)).astype(np.float32), "k2": (rs.randn(cin, c) / np.sqrt(cin)).astype(np.float32),
             "s2": rs.randn(c).astype(np.float32), "kd": (rs.randn(3, 3, c, 1) / 3).astype(np.float32),
             "sc": rs.uniform(0.2, 2, c).astype(np.float32), "sh": rs.randn(c).astype(np.float32),
             "k3": (rs.randn(c, cout) / np.sqrt(c)).astype(np.float32), "s3": rs.randn(cout).astype(np.float32)}
        pw2 = act_np(t["x"].astype(np.float64).reshape(-1, cin).dot(t["k2"].astype(np.float64)) + t["s2"], 2).reshape(n, h, w, c)
        t["mid"] = act_np(tfo.depthwise_conv2d(pw2, t["kd"], (1, 1), "SAME") * t["sc"] + t["sh"], 2)
        t["d"] = {k: dev(torch, t[k].reshape(3, 3, c) if k == "kd" else t[k]) for k in ("x", "s2", "kd", "sc", "sh", "s3")}
        t["prep2"] = ops.split_weights_device(dev(torch, t["k2"].T), t["d"]["x"].device)
        t["prep3"] = ops.split_weights_device(dev(torch, t["k3"].T), t["d"]["x"].device)
        t["two"], t["want"] = {}, {}
        _CASES[key] = t
    return _CASES[key]


def two_launches(ops, t, act):
    if act not in t["two"]:
        d = t["d"]
        pw2 = ops.pwconv1x1_f16split(d["x"], None, d["s2"], 2, prepared=t["prep2"])
        t["two"][act] = ops.dwpw_f16split(pw2, d["kd"], d["sc"], d["sh"], None, d["s3"], 1, act, prepared=t["prep3"])
        mid = t["mid"]
        t["want"][act] = act_np(mid.reshape(-1, mid.shape[3]).dot(t["k3"].astype(np.float64)) + t["s3"], act).reshape(mid.shape[:3] + (-1,))
    return t["two"][act], t["want"][act]


def fused(ops, t, act, segs=0):
    d = t["d"]
    return ops.pwblk_f16split(d["x"], None, d["s2"], d["kd"], d["sc"], d["sh"], None, d["s3"], act, segs=segs, prepared2=t["prep2"],
                              prepared3=t["prep3"])


@pytest.mark.parametrize("act", [2, 0], ids=["relu6", "none"])
@pytest.mark.parametrize("hw", SHAPES, ids=lambda s: "%dx%d" % s)
def test_one_launch_is_the_two_launches_bit_for_bit_and_fp32_grade(env, hw, act):
    torch, ops = env
    t = case(torch, ops, 3, hw[0], hw[1])
    y2, want = two_launches(ops, t, act)
    y = fused(ops, t, act)
    assert tuple(y.shape) == want.shape == (3, hw[0], hw[1], COUT)
    assert torch.equal(y, y2)
    fp32_grade(y.cpu().numpy(), want, "pwblk %dx%d act %d" % (hw + (act,)))


@pytest.mark.parametrize("n,hw", [(3, (7, 48)), (2, (48, 48))], ids=["7x48", "48x48"])
def test_the_bits_do_not_depend_on_the_row_segments(env, n, hw):
    torch, ops = env
    t = case(torch, ops, n, hw[0], hw[1])
    y2, want = two_launches(ops, t, 2)
    for segs in (1, 2, 3):
        assert torch.equal(fused(ops, t, 2, segs), y2), segs
    fp32_grade(y2.cpu().numpy(), want, "pwblk %dx%d" % hw)


def test_more_work_items_than_resident_workgroups(env):
    torch, ops = env
    t = case(torch, ops, 300, 3, 16)
    y2, want = two_launches(ops, t, 2)
    y = fused(ops, t, 2)
    assert torch.equal(y, y2)
    fp32_grade(y.cpu().numpy(), want, "pwblk 300 x 3x16")


def test_a_workgroup_walks_items_of_differing_segments(env):
    """5 x 20 in two segments of 2 and 3 rows; 130 images = 260 items on 256 workgroups, so four of them take two items that differ in
    image, first row and length."""
    torch, ops = env
    t = case(torch, ops, 130, 5, 20)
    y2, want = two_launches(ops, t, 2)
    y = fused(ops, t, 2, 2)
    assert torch.equal(y, y2)
    fp32_grade(y.cpu().numpy(), want, "pwblk 130 x 5x20")


def test_three_launches_agree_bit_for_bit(env):
    torch, ops = env
    t = case(torch, ops, 3, 7, 48)
    ys = [fused(ops, t, 2).clone() for _ in range(3)]
    assert torch.equal(ys[0], ys[1]) and torch.equal(ys[0], ys[2])


def block_plan(t, h, w, lead, fuse):
    """A plan of the pair alone (the engine's first launch sweeps forwards) or behind a stride-1 depthwise layer on the 64-channel input
    (its second launch sweeps backwards): lowering's own pass marks it."""
    from hse_facerec_tf_amd import lowering
    L = lowering.Layer
    rs = np.random.RandomState(11)
    layers = []
    if lead:
        layers.append(L(lowering.OP_DWCONV3X3, "lead", -1, (h, w, CIN), (h, w, CIN), w=(rs.randn(3, 3, CIN, 1) / 3).astype(np.float32),
                        scale=np.ones(CIN, np.float32), shift=np.zeros(CIN, np.float32), act=lowering.ACT_RELU6, kh=3, kw=3, stride=1, pad_t=1, pad_l=1))
    layers.append(L(lowering.OP_PWCONV_F32, "pw", len(layers) - 1, (h, w, CIN), (h, w, C), w=t["k2"].reshape(1, 1, CIN, C), shift=t["s2"],
                    act=lowering.ACT_RELU6, a_log2=12))
    layers.append(L(lowering.OP_DWPW_F16S, "blk", len(layers) - 1, (h, w, C), (h, w, COUT), w=t["kd"], scale=t["sc"], shift=t["sh"],
                    act=lowering.ACT_RELU6, kh=3, kw=3, stride=1, pad_t=1, pad_l=1, sealed=True, w2=t["k3"].reshape(1, 1, C, COUT), shift2=t["s3"],
                    a_log2=12))
    out = len(layers) - 1
    assert lowering.mark_pw_blocks(layers, [out]) == 1
    if not fuse:
        layers[out - 1].flags = 0
    return lowering.Plan(layers, (h, w, CIN), lowering.assign_buffers(layers, {out}), {0: (out, h * w * COUT)}, {})


@pytest.mark.parametrize("lead", [False, True], ids=["forwards", "backwards"])
def test_both_sweep_directions_through_the_engine(env, lead):
    torch, ops = env
    from hse_facerec_tf_amd.engine import Engine
    h, w = 7, 48
    t = case(torch, ops, 3, h, w)
    plan = block_plan(t, h, w, lead, True)
    rows = plan.describe(3)
    assert rows[-2]["family"] == [KERNEL] and rows[-1]["inside"] == len(rows) - 2
    outs = []
    for fuse in (True, False):
        eng = Engine(block_plan(t, h, w, lead, fuse), max_batch=3)
        outs.append(eng.forward(t["d"]["x"], (0,))["features"].clone())
        eng.close()
    assert torch.equal(outs[0], outs[1])
    if not lead:
        assert torch.equal(outs[0].reshape(3, h, w, COUT), two_launches(ops, t, 2)[0])


@pytest.mark.parametrize("shape", [(4, 64, CIN, C, COUT), (5, 20, 96, 128, 128)], ids=["64wide", "96channels"])
def test_an_uncovered_shape_runs_as_the_two_launches(env, shape):
    torch, ops = env
    h, w, cin, c, cout = shape
    t = case(torch, ops, 2, h, w, cin, c, cout)
    y2, want = two_launches(ops, t, 2)
    y = fused(ops, t, 2)
    assert torch.equal(y, y2)
    fp32_grade(y.cpu().numpy(), want, "pwblk uncovered %dx%d cin=%d" % (h, w, cin))
