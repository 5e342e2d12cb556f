"""lower_graph(s2_fusion=...): conv_dw_4 + conv_pw_4 as one launch (HSEFR_OPF_DWPW_NEXT) against the same plan with two launches --
the same bits in every output, both at the golden bar; the all-layers forward still produces the depthwise tensor; and one forward of
the workload's own shape (batch 256, 192 x 192)."""
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


def lower(size, s2, fetch=None):
    from hse_facerec_tf_amd import graphdef, lowering
    return lowering.lower_graph(graphdef.read_graph(MODEL_PB), "input_1:0", fetch or {0: FETCH[0], 1: FETCH[1], 2: FETCH[2]}, (size, size),
                                s2_fusion=s2)


@pytest.mark.parametrize("size", [192, 100])
def test_one_launch_and_two_launches_give_the_same_bits(torch_, size):
    from hse_facerec_tf_amd import engine, lowering
    z = np.load(os.path.join(GOLDEN, "e2e_synthetic.npz"))
    n = z["feat_%d" % size].shape[0]
    x = torch_.from_numpy(np.random.RandomState(123).uniform(-128, 128, (n, size, size, 3)).astype(np.float32)).cuda()
    outs = {}
    for s2 in ("auto", "none"):
        plan = lower(size, s2)
        flagged = [L.name for L in plan.layers if L.flags & lowering.OPF_DWPW_NEXT]
        assert flagged == (["conv_dw_4/depthwise"] if s2 == "auto" else [])
        eng = engine.Engine(plan, max_batch=n)
        outs[s2] = {k: v.clone() for k, v in eng.forward(x, (0, 1, 2)).items()}
        eng.close()
        for k, g in (("features", "feat"), ("age_probs", "age"), ("gender", "gender")):
            fp32_grade(outs[s2][k].cpu().numpy(), z["%s_%d" % (g, size)], "%s %d s2_fusion=%s" % (k, size, s2))
    for k in outs["none"]:
        assert torch_.equal(outs["auto"][k], outs["none"][k]), k


@pytest.mark.parametrize("size", [192, 100])
def test_the_all_layers_forward_still_writes_the_depthwise_tensor(torch_, size):
    """forward_all_layers + layer_output of conv_dw_4.  (In the whole plan a later layer recycles that buffer before the forward ends, so
    the plan is cut behind conv_pw_4: the flagged engine runs first, its buffer cannot hold the unflagged engine's result by chance.)"""
    from hse_facerec_tf_amd import engine, lowering
    z = np.load(os.path.join(GOLDEN, "e2e_synthetic.npz"))
    n = z["feat_%d" % size].shape[0]
    x = torch_.from_numpy(np.random.RandomState(123).uniform(-128, 128, (n, size, size, 3)).astype(np.float32)).cuda()
    mids, ends = {}, {}
    for s2 in ("auto", "none"):
        whole = lower(size, s2, {0: FETCH[0]})
        i = [k for k, L in enumerate(whole.layers) if L.name == "conv_dw_4/depthwise"][0]
        assert bool(whole.layers[i].flags & lowering.OPF_DWPW_NEXT) == (s2 == "auto")
        layers = whole.layers[:i + 2]
        plan = lowering.Plan(layers, whole.in_hwc, lowering.assign_buffers(layers, {i + 1}), {0: (i + 1, int(np.prod(layers[i + 1].out_shape)))}, {})
        eng = engine.Engine(plan, max_batch=n)
        ends[s2] = eng.forward(x, (0,))["features"].clone()      # one launch for the pair (auto): the depthwise buffer is not written
        eng.forward_all_layers(x)                                 # every op on its own
        mids[s2] = eng.layer_output(i, n).clone()
        eng.close()
    assert torch_.equal(ends["auto"], ends["none"])
    assert torch_.equal(mids["auto"], mids["none"])
    assert 0.0 < float(mids["auto"].max()) <= 6.0 and float(mids["auto"].min()) >= 0.0


def test_the_workload_shape_batch_256(torch_):
    from hse_facerec_tf_amd import engine
    g = torch_.Generator(device="cuda").manual_seed(7)
    x = (torch_.rand((256, 192, 192, 3), device="cuda", generator=g) * 256.0 - 128.0).contiguous()
    feats = {}
    for s2 in ("auto", "none"):
        eng = engine.Engine(lower(192, s2, {0: FETCH[0]}), max_batch=256)
        feats[s2] = eng.forward(x, (0,))["features"].clone()
        eng.close()
    assert bool(torch_.isfinite(feats["auto"]).all()) and torch_.equal(feats["auto"], feats["none"])
