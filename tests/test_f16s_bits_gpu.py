"""The bits of the split-f16 pointwise family, pinned (csrc/pwconv_f16s.hip, dwpw_f16s.hip, pwblk_stream.hip, dwconv.hip SPLIT,
pwconv_ps.hip): every case runs twice -- the two runs equal bit for bit -- and the sha256 of the output bytes equals the digest
recorded in golden/f16s_bits.json.  These kernels take their row layout, their split and their three-MFMA product from
csrc/f16s.h: a change there that moves one rounding or one product of any kernel shows here.  (The stems, which share the header
through stem_patch.h, are pinned by test_stem_bits_gpu.py.)

Shapes: the smallest at which each shared piece can go wrong, and the kernel instance each reaches (ReLU6 unless stated) --
  pw    pwconv1x1_f16split (m, k, cout), pwconv_f16s_kernel<BM, BN>:  (1, 32, 64) one partial 64x64 tile; (200, 96, 128) 64x64 with
        three K tiles, so both register sets, at all three activations; (19589, 32, 320) 64x64, 1535 tiles on 768 workgroups;
        (98381, 32, 64) 128x64, 769 tiles on 768 workgroups; (65613, 64, 128) 128x128, 513 tiles on 512 workgroups (each persistent
        loop runs a second tile in one workgroup)
  dwpw  dwpw_f16split (n, h, w, c, cout, stride):  (1, 8, 16, 32, 128) dwpw_fast<16,128,3>; (2, 16, 8, 64, 128) <8,128,3>;
        (3, 24, 24, 128, 128) the same kernel in strip mode; (1, 8, 16, 256, 256) <16,256,2>; (1, 9, 17, 96, 256) <8,256,2> with
        partial patches; (18, 40, 48, 32, 128) 270 patches on 256 workgroups; (2, 15, 13, 128, 256, stride 2) the stride-2 streaming
        kernel; (1, 8, 16, 288, 128), (1, 5, 7, 32, 192), (1, 9, 11, 32, 64, stride 2) and (1, 33, 31, 64, 128, stride 2) the general
        kernel; the other two activations at the first case and at the 288-channel one
  blk   pwblk_f16split (n, h, w) at 64 -> 128 -> 128 channels, pwblk_stream_kernel:  (2, 5, 33) also without activation, (3, 7, 48)
  dws   dwconv3x3_split (n, h, w, c, stride), dwconv's SPLIT instances:  (3, 7, 5, 32, 1) and (2, 9, 11, 64, 2)
  ps    pwconv1x1_presplit (m, k, cout), input from split_rows_encode:  (300, 256, 128); (65537, 32, 128) tile height 9, 257 tiles on
        256 workgroups; (300, 64, 128) with ReLU and with none
  psdw  pwconv1x1_presplit_dw (n, h, w, stride) at k = 64, cout = 128, three maps:  12x12 and 14x14 at both strides, 7x7, and 6x12,
        4x16, 5x20 (the masked epilogue at tile heights 9, 8 and 7); 12x12 without activation
  psgap pwconv1x1_presplit_gap (n, h, w) at k = 64, cout = 128, three maps:  6x6, 7x7, 10x10, and 12x12 with ReLU

Inputs and weights come from numpy.random.RandomState on the host.  `python tests/test_f16s_bits_gpu.py [out.json]` records the
digests from the library that is loaded; the committed ones were recorded from the library as it was BEFORE its kernels took
their vocabulary from f16s.h."""
import hashlib
import json
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "f16s_bits.json")
ACT_NONE, ACT_RELU, ACT_RELU6 = 0, 1, 2
PSDW = [(12, 12, 1), (12, 12, 2), (14, 14, 1), (14, 14, 2), (7, 7, 1), (6, 12, 1), (4, 16, 1), (5, 20, 1)]


def _cases():
    out = [("pw", s, ACT_RELU6) for s in ((1, 32, 64), (200, 96, 128), (19589, 32, 320), (98381, 32, 64), (65613, 64, 128))]
    out += [("pw", (200, 96, 128), a) for a in (ACT_RELU, ACT_NONE)]
    dwpw = [(1, 8, 16, 32, 128, 1), (2, 16, 8, 64, 128, 1), (3, 24, 24, 128, 128, 1), (1, 8, 16, 256, 256, 1), (1, 9, 17, 96, 256, 1),
            (18, 40, 48, 32, 128, 1), (2, 15, 13, 128, 256, 2), (1, 8, 16, 288, 128, 1), (1, 5, 7, 32, 192, 1), (1, 9, 11, 32, 64, 2),
            (1, 33, 31, 64, 128, 2)]
    out += [("dwpw", s, ACT_RELU6) for s in dwpw]
    out += [("dwpw", s, a) for s in ((1, 8, 16, 32, 128, 1), (1, 8, 16, 288, 128, 1)) for a in (ACT_RELU, ACT_NONE)]
    out += [("blk", (2, 5, 33), ACT_RELU6), ("blk", (3, 7, 48), ACT_RELU6), ("blk", (2, 5, 33), ACT_NONE)]
    out += [("dws", (3, 7, 5, 32, 1), ACT_RELU6), ("dws", (2, 9, 11, 64, 2), ACT_RELU6)]
    out += [("ps", (300, 256, 128), ACT_RELU6), ("ps", (65537, 32, 128), ACT_RELU6), ("ps", (300, 64, 128), ACT_RELU), ("ps", (300, 64, 128), ACT_NONE)]
    out += [("psdw", (3, h, w, s), ACT_RELU6) for h, w, s in PSDW] + [("psdw", (3, 12, 12, 1), ACT_NONE)]
    out += [("psgap", (3, h, h), ACT_RELU6) for h in (6, 7, 10)] + [("psgap", (3, 12, 12), ACT_RELU)]
    return out


CASES = _cases()


def case_id(case):
    op, shape, act = case
    return "%s-%s-act%d" % (op, "x".join(str(v) for v in shape), act)


def activations(rs, shape):
    """ReLU6-range values with exact zeros, the bound itself and tiny values (the split's precondition: |x| * 2^12 < 32768)."""
    x = rs.uniform(0, 6, shape).astype(np.float32)
    x[rs.rand(*shape) < 0.3] = 0.0
    x[rs.rand(*shape) < 0.05] = 6.0
    x[rs.rand(*shape) < 0.05] *= 1e-5
    return x


def pointwise(rs, cout, k):
    """A pointwise kernel [cout, k] with output channels decades apart and one all-zero channel, and its shift."""
    w = (rs.randn(cout, k) / np.sqrt(k)).astype(np.float32) * (10.0 ** rs.uniform(-2, 2, cout)).astype(np.float32)[:, None]
    w[cout // 2] = 0.0
    return w, rs.randn(cout).astype(np.float32)


def depthwise(rs, c):
    return (rs.randn(3, 3, c) / 3).astype(np.float32), (rs.rand(c) + 0.5).astype(np.float32), (rs.randn(c) * 0.3).astype(np.float32)


def host_data(op, shape):
    rs = np.random.RandomState(sum((31 ** i) * v for i, v in enumerate(shape)) % (2 ** 31) + len(op))
    if op in ("pw", "ps"):
        m, k, cout = shape
        return (activations(rs, (m, k)),) + pointwise(rs, cout, k)
    if op == "dwpw":
        n, h, w, c, cout, _ = shape
        return (activations(rs, (n, h, w, c)),) + depthwise(rs, c) + pointwise(rs, cout, c)
    if op == "blk":
        return (activations(rs, shape + (64,)),) + pointwise(rs, 128, 64) + depthwise(rs, 128) + pointwise(rs, 128, 128)
    if op == "dws":
        n, h, w, c, _ = shape
        return (activations(rs, (n, h, w, c)),) + depthwise(rs, c)
    if op == "psdw":
        return (activations(rs, shape[:3] + (64,)),) + pointwise(rs, 128, 64) + depthwise(rs, 128)
    assert op == "psgap"
    return (activations(rs, shape + (64,)),) + pointwise(rs, 128, 64)


_DATA = {}


def run_case(torch, ops, case):
    op, shape, act = case
    if (op, shape) not in _DATA:
        _DATA.clear()                  # cases of one (op, shape) follow each other: one shape's device data at a time
        _DATA[(op, shape)] = [torch.from_numpy(a).cuda() for a in host_data(op, shape)]
    d = _DATA[(op, shape)]
    if op == "pw":
        return ops.pwconv1x1_f16split(d[0], d[1], d[2], act)
    if op == "dwpw":
        return ops.dwpw_f16split(d[0], d[1], d[2], d[3], d[4], d[5], shape[5], act)
    if op == "blk":
        return ops.pwblk_f16split(d[0], d[1], d[2], d[3], d[4], d[5], d[6], d[7], act)
    if op == "dws":
        return ops.dwconv3x3_split(d[0], d[1], d[2], d[3], shape[4], act)
    xs = ops.split_rows_encode(d[0])
    if op == "ps":
        return ops.pwconv1x1_presplit(xs, d[1], d[2], act)
    if op == "psdw":
        return ops.pwconv1x1_presplit_dw(xs, d[1], d[2], d[3], d[4], d[5], act, dw_stride=shape[3])
    return ops.pwconv1x1_presplit_gap(xs, d[1], d[2], act)


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
def test_f16s_bits(env, recorded, case):
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
        assert torch.equal(a, b) and bool(torch.isfinite(a).all()), case_id(c)
        table[case_id(c)] = digest(a)
        print(case_id(c), table[case_id(c)])
    path = sys.argv[1] if len(sys.argv) > 1 else FIXTURE
    with open(path, "w") as f:
        json.dump(table, f, indent=1, sort_keys=True)
        f.write("\n")
    print("recorded %d digests in %s" % (len(table), path))
