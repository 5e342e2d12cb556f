"""The bits of the four product stems, pinned (csrc/stem2_fused.hip, stem3_fused.hip, stem4_fused.hip, stem5_stream.hip): every
kernel, both input forms and every activation instance run twice -- the two runs equal bit for bit -- and the sha256 of the output
bytes equals the digest recorded in golden/stem_bits.json.  The patch kernels share their cursor and their stages C-E through
csrc/stem_patch.h: a change there that moves one sum or one FMA of any generation shows here.

Shapes: the smallest at which each shared piece can go wrong -- one all-border patch, odd edges, several tiles and two images,
5 x 5 tiles (patches with th, tw >= 1 lie inside the 36 x 68 map: the `interior` fast path and the masked path both run), and
528 patches against the 512-workgroup grid (the persistent loop, the prefetched window and `advance` with its carries run a
second iteration).  ReLU6 everywhere; the other two template instances at one shape.

Inputs and weights come from numpy.random.RandomState on the host.  `python tests/test_stem_bits_gpu.py [out.json]` records the
digests from the library that is loaded."""
import hashlib
import json
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "stem_bits.json")
MEAN_BGR = (103.939, 116.779, 123.68)
ACT_NONE, ACT_RELU, ACT_RELU6 = 0, 1, 2
ODD = [(1, 3, 3), (1, 7, 5), (2, 13, 21), (1, 72, 136), (33, 64, 128)]            # stem2_fused, stem3_fused: any edge
QUAD = [(1, 4, 4), (1, 8, 4), (2, 12, 20), (1, 72, 136), (33, 64, 128)]           # stem4_fused, stem5_stream: edges % 4 == 0


def _cases():
    out = []
    for kernel, forms, shapes, all_acts in (("stem2_fused", ("f32",), ODD, (2, 13, 21)), ("stem3_fused", ("f32",), ODD, (2, 13, 21)),
                                            ("stem4_fused", ("f32", "u8"), QUAD, (2, 12, 20)), ("stem5_stream", ("f32", "u8"), QUAD, (2, 12, 20))):
        for form in forms:
            out += [(kernel, form, shape, ACT_RELU6) for shape in shapes]
            out += [(kernel, form, all_acts, act) for act in (ACT_RELU, ACT_NONE)]
    return out


CASES = _cases()


def case_id(case):
    kernel, form, (n, h, w), act = case
    return "%s-%s-%dx%dx%d-act%d" % (kernel, form, n, h, w, act)


def host_data(shape):
    """Weights, a float image inside the declared bound (|x| < 256: bytes minus the BGR mean, plus a fraction) and a byte image."""
    n, h, w = shape
    rs = np.random.RandomState(1000 * n + 37 * h + w)
    cw = (rs.randn(3, 3, 3, 32) * 0.02).astype(np.float32)
    cw[..., 5] *= 40.0
    cw[..., 9] *= 0.01
    wt = dict(cw=cw, csh=rs.randn(32), k1=rs.randn(3, 3, 32) / 3, sc1=rs.rand(32) + 0.5, sh1=rs.randn(32) * 0.3,
              kp=rs.randn(64, 32) / 32 ** 0.5, psh=rs.randn(64), k2=rs.randn(3, 3, 64) / 3, sc2=rs.rand(64) + 0.5, sh2=rs.randn(64) * 0.3)
    wt = {k: np.ascontiguousarray(v, dtype=np.float32) for k, v in wt.items()}
    rgb = rs.randint(0, 256, (n, h, w, 3)).astype(np.uint8)
    x = (rs.randint(0, 256, (n, h, w, 3)) - np.array(MEAN_BGR) + rs.uniform(-0.5, 0.5, (n, h, w, 3))).astype(np.float32)
    assert float(np.abs(x).max()) < 256.0
    return wt, x, rgb


_DATA = {}


def run_case(torch, ops, case):
    kernel, form, shape, act = case
    if shape not in _DATA:
        wt, x, rgb = host_data(shape)
        d = {k: torch.from_numpy(v).cuda() for k, v in wt.items() if k != "kp"}
        _DATA[shape] = (d, ops.split_weights_device(wt["kp"], "cuda"), torch.from_numpy(x).cuda(), torch.from_numpy(rgb).cuda())
    d, prep, x, rgb = _DATA[shape]
    kw = dict(act=act, prepared=prep)
    if form == "u8":
        kw["u8_mean_bgr"] = MEAN_BGR
    y = getattr(ops, kernel)(rgb if form == "u8" else x, d["cw"], d["csh"], d["k1"], d["sc1"], d["sh1"], None, d["psh"], d["k2"], d["sc2"],
                             d["sh2"], **kw)
    n, h, w = shape
    assert tuple(y.shape) == (n, (h + 3) // 4, (w + 3) // 4, 64)
    return y


def digest(y):
    return hashlib.sha256(y.cpu().numpy().tobytes()).hexdigest()


@pytest.fixture(scope="module")
def env():
    import torch
    assert torch.cuda.is_available()
    from hse_facerec_tf_amd import ops
    assert (ops.ACT_NONE, ops.ACT_RELU, ops.ACT_RELU6) == (ACT_NONE, ACT_RELU, ACT_RELU6)
    return torch, ops


@pytest.fixture(scope="module")
def recorded():
    with open(FIXTURE) as f:
        return json.load(f)


def test_the_fixture_lists_exactly_these_cases(recorded):
    assert sorted(recorded) == sorted(case_id(c) for c in CASES)


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_stem_bits(env, recorded, case):
    torch, ops = env
    a = run_case(torch, ops, case)
    b = run_case(torch, ops, case)
    assert torch.equal(a, b), "two launches differ"
    assert bool(torch.isfinite(a).all())
    assert digest(a) == recorded[case_id(case)]


if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import torch
    from hse_facerec_tf_amd import ops
    table = {}
    for c in CASES:
        a, b = run_case(torch, ops, c), run_case(torch, ops, c)
        assert torch.equal(a, b), case_id(c)
        table[case_id(c)] = digest(a)
        print(case_id(c), table[case_id(c)])
    path = sys.argv[1] if len(sys.argv) > 1 else FIXTURE
    with open(path, "w") as f:
        json.dump(table, f, indent=1, sort_keys=True)
        f.write("\n")
    print("recorded %d digests in %s" % (len(table), path))
