"""lower_graph(pw_block_fusion=...): conv_pw_2 + the block conv_dw_3 / conv_pw_3 as one row-streaming launch (HSEFR_OPF_PWBLK_NEXT) against
the same plan with two launches -- the same bits in every output, both at the golden bar (192: the workload's 48-pixel rows; 100: an odd
25 x 25 map); the all-layers forward still produces conv_pw_2's tensor; and one forward of the workload's own shape (batch 256, 192 x 192)."""
import os

import numpy as np
import pytest

from conftest import GOLDEN, MODEL_PB
from test_e2e_gpu import FETCH, fp32_grade  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def torch_():
    import torch
    assert torch.cuda.is_available()
    return torch


def lower(size, fusion, fetch=None):
    from hse_facerec_tf_amd import graphdef, lowering
    return lowering.lower_graph(graphdef.read_graph(MODEL_PB), "input_1:0", fetch or {0: FETCH[0], 1: FETCH[1], 2: FETCH[2]}, (size, size),
                                pw_block_fusion=fusion)


@pytest.mark.parametrize("size", [192, 100])
def test_one_launch_and_two_launches_give_the_same_bits(torch_, size):
    from hse_facerec_tf_amd import engine, lowering
    z = np.load(os.path.join(GOLDEN, "e2e_synthetic.npz"))
    n = z["feat_%d" % size].shape[0]
    x = torch_.from_numpy(np.random.RandomState(123).uniform(-128, 128, (n, size, size, 3)).astype(np.float32)).cuda()
    outs = {}
    for fusion in ("auto", "none"):
        plan = lower(size, fusion)
        flagged = [L.name for L in plan.layers if L.flags & lowering.OPF_PWBLK_NEXT]
        assert len(flagged) == (1 if fusion == "auto" else 0) and all(f.startswith("conv_pw_2") for f in flagged)
        eng = engine.Engine(plan, max_batch=n)
        outs[fusion] = {k: v.clone() for k, v in eng.forward(x, (0, 1, 2)).items()}
        eng.close()
        for k, g in (("features", "feat"), ("age_probs", "age"), ("gender", "gender")):
            fp32_grade(outs[fusion][k].cpu().numpy(), z["%s_%d" % (g, size)], "%s %d pw_block_fusion=%s" % (k, size, fusion))
    for k in outs["none"]:
        assert torch_.equal(outs["auto"][k], outs["none"][k]), k


@pytest.mark.parametrize("size", [192, 100])
def test_the_all_layers_forward_still_writes_the_pointwise_tensor(torch_, size):
    """forward_all_layers + layer_output of conv_pw_2.  (In the whole plan a later layer recycles that buffer before the forward ends, so
    the plan is cut behind the block: the flagged engine runs first, its buffer cannot hold the unflagged engine's result by chance.
    In the cut plan the block's output is pinned; the whole plans above exchange the two buffers' roles.)"""
    from hse_facerec_tf_amd import engine, lowering
    z = np.load(os.path.join(GOLDEN, "e2e_synthetic.npz"))
    n = z["feat_%d" % size].shape[0]
    x = torch_.from_numpy(np.random.RandomState(123).uniform(-128, 128, (n, size, size, 3)).astype(np.float32)).cuda()
    mids, ends = {}, {}
    for fusion in ("auto", "none"):
        whole = lower(size, fusion, {0: FETCH[0]})
        i = [k for k, L in enumerate(whole.layers) if L.name.startswith("conv_pw_2")][0]
        assert bool(whole.layers[i].flags & lowering.OPF_PWBLK_NEXT) == (fusion == "auto")
        layers = whole.layers[:i + 2]
        plan = lowering.Plan(layers, whole.in_hwc, lowering.assign_buffers(layers, {i + 1}), {0: (i + 1, int(np.prod(layers[i + 1].out_shape)))}, {})
        eng = engine.Engine(plan, max_batch=n)
        ends[fusion] = eng.forward(x, (0,))["features"].clone()      # one launch for the pair (auto): conv_pw_2's buffer is not written
        eng.forward_all_layers(x)                                 # every op on its own
        mids[fusion] = eng.layer_output(i, n).clone()
        eng.close()
    assert torch_.equal(ends["auto"], ends["none"])
    assert torch_.equal(mids["auto"], mids["none"])
    assert 0.0 < float(mids["auto"].max()) <= 6.0 and float(mids["auto"].min()) >= 0.0


def test_the_workload_shape_batch_256(torch_):
    from hse_facerec_tf_amd import engine
    g = torch_.Generator(device="cuda").manual_seed(7)
    x = (torch_.rand((256, 192, 192, 3), device="cuda", generator=g) * 256.0 - 128.0).contiguous()
    feats = {}
    for fusion in ("auto", "none"):
        eng = engine.Engine(lower(192, fusion, {0: FETCH[0]}), max_batch=256)
        feats[fusion] = eng.forward(x, (0,))["features"].clone()
        eng.close()
    assert bool(torch_.isfinite(feats["auto"]).all()) and torch_.equal(feats["auto"], feats["none"])
