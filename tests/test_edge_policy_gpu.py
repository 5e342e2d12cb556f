"""Cache policy per producer -> consumer edge of the MobileNet-192 plan (DESIGN.md lesson 76): streaming loads, non-temporal stores and
the dropped drain-step loads change WHERE bytes wait, never their value, so every test is `torch.equal` against the route that does not run
the changed code.

  pwblk_stream_f16s_kernel  (shipped: the drain steps' out-of-range loads; measured and not shipped: streaming input loads, a store flavour
                            chosen per row from the row's position in a workgroup's sweep) against pwconv1x1_f16split + dwpw_f16split,
                            the two launches it replaces: 5 x 8x8 and 2 x 48x48 in one and in two row segments -- every workgroup's rows
                            fall on both sides of any split point, every workgroup drains -- both sweep directions through the engine,
                            and 130 x 8x8 in two segments: 260 items on 256 workgroups, so four of them walk two items
  dwpws2_f16s_kernel        (shipped: non-temporal epilogue stores; not shipped: streaming input loads) against dwconv3x3 +
                            pwconv1x1_f16split: 3 x 16x16 and 1 x 18x14, which has partial patches both ways
  dwpw3_f16s_kernel         (shipped: streaming halo pieces of the 16 x 8 patch; not shipped: non-temporal epilogue stores) against the
                            same op image by image: 6 x 16x16x256, whose seams lie on patch edges (the launcher keeps the per-image tiling
                            there: as many patches either way), and 3 x 24x24x256, which takes the strip tiling with a seam at patch row 8
  end to end                the 192 plan on 3 images against the plan lowered without the two fused launches, five forwards, the same bits
                            every time
The operands and references are those of tests/test_pwblk_stream_gpu.py, test_dwpw_s2_gpu.py and test_dwpw3_strip_gpu.py (computed once per
shape and shared)."""
import numpy as np
import pytest

import test_dwpw3_strip_gpu as strip
import test_dwpw_s2_gpu as s2
import test_pwblk_stream_gpu as pb
from conftest import MODEL_PB
from test_e2e_gpu import FETCH  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def env():
    import torch
    from hse_facerec_tf_amd import ops
    assert torch.cuda.is_available()
    return torch, ops


@pytest.mark.parametrize("segs", [1, 2])
@pytest.mark.parametrize("shape", [(5, 8, 8), (2, 48, 48)], ids=lambda s: "%dx%dx%d" % s)
def test_pwblk_stream_is_the_two_launches_bit_for_bit(env, shape, segs):
    torch, ops = env
    t = pb.case(torch, ops, *shape)
    y2, _ = pb.two_launches(ops, t, 2)
    y = pb.fused(ops, t, 2, segs)
    assert tuple(y.shape) == shape + (pb.COUT,)
    assert torch.equal(y, y2)


@pytest.mark.parametrize("lead", [False, True], ids=["forwards", "backwards"])
@pytest.mark.parametrize("shape", [(5, 8, 8), (2, 48, 48)], ids=lambda s: "%dx%dx%d" % s)
def test_pwblk_stream_in_both_sweep_directions(env, shape, lead):
    torch, ops = env
    from hse_facerec_tf_amd.engine import Engine
    n, h, w = shape
    t = pb.case(torch, ops, n, h, w)
    assert pb.block_plan(t, h, w, lead, True).describe(n)[-2]["family"] == [pb.KERNEL]
    outs = []
    for fuse in (True, False):
        eng = Engine(pb.block_plan(t, h, w, lead, fuse), max_batch=n)
        outs.append(eng.forward(t["d"]["x"], (0,))["features"].clone())
        eng.close()
    assert torch.equal(outs[0], outs[1])
    if not lead:
        assert torch.equal(outs[0].reshape(n, h, w, pb.COUT), pb.two_launches(ops, t, 2)[0])


def test_pwblk_stream_with_more_items_than_workgroups(env):
    torch, ops = env
    t = pb.case(torch, ops, 130, 8, 8)
    y2, _ = pb.two_launches(ops, t, 2)
    assert torch.equal(pb.fused(ops, t, 2, 2), y2)


@pytest.mark.parametrize("shape", [(3, 16, 16), (1, 18, 14)], ids=lambda s: "%dx%dx%d" % s)
def test_dwpws2_is_the_depthwise_and_the_pointwise_op_bit_for_bit(env, shape):
    torch, ops = env
    t = s2.case(torch, ops, *shape)
    y2, _ = s2.two_launches(ops, t, 2)
    y = s2.fused(ops, t, 2)
    assert tuple(y.shape) == (shape[0], (shape[1] + 1) // 2, (shape[2] + 1) // 2, s2.COUT)
    assert torch.equal(y, y2)


@pytest.mark.parametrize("shape,tw", [((6, 16, 16), 16), ((3, 24, 24), 8)], ids=["6x16x16", "3x24x24"])
def test_dwpw3_on_the_batch_is_the_images_one_by_one_bit_for_bit(env, shape, tw):
    torch, ops = env
    t = strip.case(torch, ops, *shape, 256, 256)
    # (the launcher's own answer: TW = 8 in the kernel's template arguments is the strip tiling)
    assert strip.block_plan(t, shape[1], shape[2], 256, 256, False).describe(shape[0])[-1]["kernels"] == ["%s<%d, 256, 2, 2>" % (strip.KERNEL, tw)]
    one_by_one, _ = strip.references(torch, ops, t, 2)
    y = strip.block(ops, t, t["d"]["x"], 2)
    assert tuple(y.shape) == shape + (256,)
    assert torch.equal(y, one_by_one)


def test_the_192_plan_against_the_unfused_plan_five_times(env):
    torch, ops = env
    from hse_facerec_tf_amd import graphdef, lowering
    from hse_facerec_tf_amd.engine import Engine
    graph = graphdef.read_graph(MODEL_PB)
    fetch = {0: FETCH[0], 1: FETCH[1], 2: FETCH[2]}
    x = torch.from_numpy(np.random.RandomState(76).uniform(-128, 128, (3, 192, 192, 3)).astype(np.float32)).cuda()
    plan = lowering.lower_graph(graph, "input_1:0", fetch, (192, 192))
    kernels = [k for row in plan.describe(3) for k in row["kernels"]]
    for family in (pb.KERNEL, s2.KERNEL, strip.KERNEL):
        assert any(k.startswith(family) for k in kernels), family
    eng = Engine(lowering.lower_graph(graph, "input_1:0", fetch, (192, 192), pw_block_fusion="none", s2_fusion="none"), max_batch=3)
    want = {k: v.clone() for k, v in eng.forward(x, (0, 1, 2)).items()}
    eng.close()
    eng = Engine(plan, max_batch=3)
    for turn in range(5):
        got = eng.forward(x, (0, 1, 2))
        for k in want:
            assert torch.equal(got[k], want[k]), (k, turn)
    eng.close()
