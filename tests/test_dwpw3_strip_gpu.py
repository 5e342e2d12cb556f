"""Strip tiling of the wave-specialised stride-1 depthwise -> pointwise launch (csrc/dwpw_f16s.hip, dwpw3_f16s_kernel): where it takes fewer
patches, 16 x 8 patches are laid over the batch as ONE map of n * OH rows, so a patch may hold the last rows of image i and the first
rows of image i + 1 with one zero halo row between them.  The reference is the same op called once per image: a one-image strip has no
seam (and at n = 1 the strip never takes fewer patches, so the call takes the per-image tiling), and the batched result must be that bit
for bit.  Every case also goes against the fp64 oracle at the 2e-6 bar of tests/test_kernels_gpu.py.

Shapes (patch rows at which an image starts inside a 16-row patch, by n * OH):
  3 x 24x24   8 (patch 1), 0 (patch 3: the seam is a patch edge)      4 x 28x28   12, 8, 4
  3 x 20x24   4, 8                                                    2 x 16x12   seam on a patch edge, width not a multiple of 8
  1 x 24x24   no seam                                                 5 x 24x24   120 rows: the last patch row is partial
  2 x 12x12, 2 x 18x24   OH < 16 / OH % 4 != 0: per-image tiling      3 x 24x20   strip tiling with a partial last patch column
(2 x 16x12 and 1 x 24x24 take as many patches either way, so the launcher keeps the per-image tiling for them; 3 x 24x20 is this file's own
addition for a partial column under strip tiling.)  The last row of every image is about +5 and the first row about -5: a depthwise tap
that crossed a seam would move the result by whole units."""
import numpy as np
import pytest

from oracle import tf_graph as tfo

pytestmark = pytest.mark.gpu

TOL = 2e-6
KERNEL = "dwpw3_f16s_kernel"
CHANNELS = [(32, 128), (256, 256)]
SHAPES = [(3, 24, 24), (4, 28, 28), (3, 20, 24), (2, 16, 12), (1, 24, 24), (5, 24, 24), (2, 12, 12), (2, 18, 24), (3, 24, 20)]


@pytest.fixture(scope="module")
def env():
    import torch
    from hse_facerec_tf_amd import ops
    assert torch.cuda.is_available()
    return torch, ops


def dev(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).cuda()


def rel(a, b):
    return float(np.abs(np.asarray(a, np.float64) - np.asarray(b, np.float64)).max() / (np.abs(b).max() + 1e-30))


def act_np(v, act):
    return np.minimum(np.maximum(v, 0), 6) if act == 2 else (np.maximum(v, 0) if act == 1 else v)


_CASES = {}


def case(torch, ops, n, h, w, c, cout):
    """Operands on the device, the fp64 depthwise result, and per activation the per-image outputs and the oracle's: computed once, shared,
    never changed."""
    key = (n, h, w, c, cout)
    if key not in _CASES:
        rs = np.random.RandomState(h * 131 + w * 7 + n + c)
        x = rs.uniform(0, 6, (n, h, w, c)).astype(np.float32)
        x[:, -1] = 5 + rs.uniform(-0.5, 0.5, (n, w, c))
        x[:, 0] = -5 + rs.uniform(-0.5, 0.5, (n, w, c))
        t = {"x": x, "kd": (rs.randn(3, 3, c, 1) / 3).astype(np.float32), "sc": rs.uniform(0.2, 2, c).astype(np.float32),
             "sh": rs.randn(c).astype(np.float32), "kp": (rs.randn(c, cout) / np.sqrt(c)).astype(np.float32), "psh": rs.randn(cout).astype(np.float32)}
        t["mid"] = act_np(tfo.depthwise_conv2d(x.astype(np.float64), t["kd"], (1, 1), "SAME") * t["sc"] + t["sh"], 2)
        t["d"] = {k: dev(torch, t[k].reshape(3, 3, c) if k == "kd" else t[k]) for k in ("x", "kd", "sc", "sh", "psh")}
        t["prep"] = ops.split_weights_device(dev(torch, t["kp"].T), t["d"]["x"].device)
        t["per_image"], t["want"] = {}, {}
        _CASES[key] = t
    return _CASES[key]


def block(ops, t, x, act):
    d = t["d"]
    return ops.dwpw_f16split(x, d["kd"], d["sc"], d["sh"], None, d["psh"], 1, act, prepared=t["prep"])


def references(torch, ops, t, act):
    if act not in t["per_image"]:
        x = t["d"]["x"]
        t["per_image"][act] = torch.cat([block(ops, t, x[i:i + 1].contiguous(), act) for i in range(x.shape[0])])
        mid = t["mid"]
        t["want"][act] = act_np(mid.reshape(-1, mid.shape[3]).dot(t["kp"].astype(np.float64)) + t["psh"], act).reshape(mid.shape[:3] + (-1,))
    return t["per_image"][act], t["want"][act]


def check(torch, ops, shape, cc, act):
    t = case(torch, ops, *shape, *cc)
    one_by_one, want = references(torch, ops, t, act)
    y = block(ops, t, t["d"]["x"], act)
    assert tuple(y.shape) == want.shape == shape + (cc[1],)
    err = rel(y.cpu().numpy(), want)
    print("dwpw3 strip %s %s act %d: differing elements %d, max-rel-err vs fp64 %.3e" %
          (shape, cc, act, int((y != one_by_one).sum()), err))
    assert torch.equal(y, one_by_one)
    assert err < TOL


@pytest.mark.parametrize("cc", CHANNELS, ids=lambda c: "%dto%d" % c)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%dx%d" % s)
def test_the_batch_is_the_images_one_by_one_bit_for_bit_and_fp32_grade(env, shape, cc):
    torch, ops = env
    check(torch, ops, shape, cc, 2)


@pytest.mark.parametrize("act", [0, 1], ids=["none", "relu"])
def test_the_other_activations(env, act):
    torch, ops = env
    check(torch, ops, (3, 24, 24), (256, 256), act)


@pytest.mark.parametrize("cc", CHANNELS, ids=lambda c: "%dto%d" % c)
def test_a_workgroup_walks_patches_of_differing_seams(env, cc):
    """61 images of 24 x 24: 1464 rows = 92 patch rows (the last one partial) x 3 = 276 work items on 256 workgroups, so twenty of them take
    a second patch whose seam sits elsewhere than the first one's, under the halo prefetch and the depthwise cursors (at 32 channels a
    patch is ONE step, and the prefetch runs two patches ahead)."""
    torch, ops = env
    check(torch, ops, (61, 24, 24), cc, 2)


def test_three_launches_agree_bit_for_bit(env):
    torch, ops = env
    t = case(torch, ops, 4, 28, 28, 32, 128)
    ys = [block(ops, t, t["d"]["x"], 2).clone() for _ in range(3)]
    assert torch.equal(ys[0], ys[1]) and torch.equal(ys[0], ys[2])


def block_plan(t, h, w, c, cout, lead):
    """A plan of the block alone (the engine's first launch sweeps forwards) or behind a stride-1 depthwise layer (its second launch sweeps
    backwards)."""
    from hse_facerec_tf_amd import lowering
    L = lowering.Layer
    layers = []
    if lead:
        layers.append(L(lowering.OP_DWCONV3X3, "lead", -1, (h, w, c), (h, w, c), w=t["kd"], scale=t["sc"], shift=t["sh"], act=lowering.ACT_RELU6,
                        kh=3, kw=3, stride=1, pad_t=1, pad_l=1))
    layers.append(L(lowering.OP_DWPW_F16S, "blk", len(layers) - 1, (h, w, c), (h, w, cout), w=t["kd"], scale=t["sc"], shift=t["sh"],
                    act=lowering.ACT_RELU6, kh=3, kw=3, stride=1, pad_t=1, pad_l=1, sealed=True, w2=t["kp"].reshape(1, 1, c, cout), shift2=t["psh"],
                    a_log2=12))
    out = len(layers) - 1
    return lowering.Plan(layers, (h, w, c), lowering.assign_buffers(layers, {out}), {0: (out, h * w * cout)}, {})


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%dx%d" % s)
def test_which_shapes_take_the_strip_tiling(shape):
    """The launcher's own answer (Plan.describe): per-image tiling of every shape here is the 8 x 16 patch (both patches pad alike and the
    tie goes to TW = 16), so TW = 8 in the kernel's template arguments is the strip tiling."""
    n, h, w = shape
    rs = np.random.RandomState(0)
    t = {"kd": rs.randn(3, 3, 32, 1).astype(np.float32), "sc": np.ones(32, np.float32), "sh": np.zeros(32, np.float32),
         "kp": rs.randn(32, 128).astype(np.float32), "psh": np.zeros(128, np.float32)}
    strip = shape in [(3, 24, 24), (4, 28, 28), (3, 20, 24), (5, 24, 24), (3, 24, 20)]
    assert block_plan(t, h, w, 32, 128, False).describe(n)[-1]["kernels"] == ["%s<%d, 128, 3, 2>" % (KERNEL, 8 if strip else 16)]


@pytest.mark.parametrize("lead", [False, True], ids=["forwards", "backwards"])
def test_both_sweep_directions_through_the_engine(env, lead):
    torch, ops = env
    from hse_facerec_tf_amd.engine import Engine
    n, h, w, c, cout = 3, 24, 24, 256, 256
    t = case(torch, ops, n, h, w, c, cout)
    d = t["d"]
    plan = block_plan(t, h, w, c, cout, lead)
    assert plan.describe(n)[-1]["family"] == [KERNEL]
    x = ops.dwconv3x3(d["x"], d["kd"], d["sc"], d["sh"], 1) if lead else d["x"]
    want = torch.cat([block(ops, t, x[i:i + 1].contiguous(), 2) for i in range(n)])
    eng = Engine(plan, max_batch=n)
    got = eng.forward(d["x"], (0,))["features"].clone()
    eng.close()
    assert torch.equal(got.reshape(want.shape), want)
