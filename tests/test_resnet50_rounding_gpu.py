"""Every epilogue of the bf16 ResNet path, BIT FOR BIT against the documented formula

    y = bf16( act( bf16( fma(acc, scale[c], shift[c]) ) + R ) ),      R = residual | bf16(projection) | nothing

on the exact operands of tests/bf16_exact_cases.py: every product and every partial sum is exact in fp32 in any order, so each
output bit is fixed, and the reference (NumPy float64 + oracle.resnet50.bf16_round) shares no code with the kernels.  What the
tolerance of the vs-oracle tests and the cross-family bit-for-bit tests cannot see -- truncation, round half away, a missing
intermediate rounding, ReLU on the wrong side of the add, on every element or in one tile shape's tail path only -- fails here;
tests/test_resnet50_rounding_cpu.py shows that each of these would change a stated share of every case.

Which kernel serves which row is decided by launch_conv_bf16 and the *_supported / *_preferred predicates; the intended family of
each row is named in tests/bf16_exact_cases.py next to the row."""
import numpy as np
import pytest

import bf16_exact_cases as gen

pytestmark = pytest.mark.gpu

_ids = lambda r: "x".join(str(int(v)) for v in r)      # noqa: E731


@pytest.fixture(scope="module")
def env():
    import torch
    from hse_facerec_tf_amd import ops
    assert torch.cuda.is_available()
    return torch, ops


def dev(env, a):
    """Values that are bf16 numbers -> a CUDA bfloat16 tensor of exactly these bits."""
    return env[1].bf16_from_bits(gen.bits(a))


def f32(env, a):
    return env[0].from_numpy(np.ascontiguousarray(a, dtype=np.float32)).cuda()


def wt(env, kern):
    return env[1].bf16_from_bits(gen.pack_conv_weight(kern.astype(np.float32)))


def got_bits(env, t):
    torch = env[0]
    assert t.dtype == torch.bfloat16
    return t.contiguous().view(torch.int16).cpu().numpy().view(np.uint16)


def assert_bits(env, got, expected, what):
    """expected = (stored values, the values the final conversion saw) from the reference; got: the device's bfloat16 tensor."""
    want, pre = expected
    g, w = got_bits(env, got), gen.bits(want)
    assert g.shape == w.shape, "%s: shape %s, expected %s" % (what, g.shape, w.shape)
    if np.array_equal(g, w):
        return
    bad = np.argwhere(g != w)
    i = tuple(int(v) for v in bad[0])
    pytest.fail("%s: %d of %d elements differ; first at %s: fp32 value before the final conversion %r (bits 0x%08x), expected bf16 bits 0x%04x, "
                "device returned 0x%04x" % (what, len(bad), g.size, i, float(pre[i]), int(np.float32(pre[i]).view(np.uint32)), int(w[i]), int(g[i])))


CONV_FORMS = [(row, res, act) for row in gen.EXACT_CONV_ROWS for res in (False, True) for act in (0, 1)]


@pytest.mark.parametrize("row,res,act", CONV_FORMS, ids=["%s-res%d-act%d" % (_ids(r), res, act) for r, res, act in CONV_FORMS])
def test_conv_bf16_bit_for_bit(env, row, res, act):
    """ops.conv_bf16 on every row of test_conv_bf16_vs_oracle (but the two tile-count rows) and on two rows that reach the general kernel's
    128 x 128 and 128 x 64 tiles, each with and without a residual, linear and ReLU."""
    torch, ops = env
    case = gen.conv_case(row)
    k, s = row[5], row[6]
    L = case.layer
    got = ops.conv_bf16(dev(env, case.x), wt(env, case.kern), f32(env, L.scale), f32(env, L.shift), k, k, s, case.pad,
                        dev(env, case.res) if res else None, act)
    assert_bits(env, got, case.expect(res, act), "%s res=%d act=%d" % (case.name, res, act))


@pytest.mark.parametrize("act", [0, 1])
@pytest.mark.parametrize("row", gen.PROJ_ROWS, ids=_ids)
def test_conv1x1_proj_bf16_bit_for_bit(env, row, act):
    """act(bf16(a) + bf16(p)): the persistent PROJ kernel, an odd stride-2 view, and the four-wave PROJ kernel (the last row)."""
    torch, ops = env
    case = gen.proj_case(row)
    A, P = case.main, case.proj
    got = ops.conv1x1_proj_bf16(dev(env, case.x), wt(env, case.k1), f32(env, A.scale), f32(env, A.shift), dev(env, case.x2), wt(env, case.k2),
                                f32(env, P.scale), f32(env, P.shift), row[6], act)
    assert_bits(env, got, case.expect(act), "%s act=%d" % (case.name, act))


@pytest.mark.parametrize("act", [0, 1])
@pytest.mark.parametrize("row", gen.SRES_ROWS, ids=_ids)
def test_conv1x1_sres_bf16_bit_for_bit(env, row, act):
    """act(bf16(a) + res[:, ::st, ::st]): the residual gathered from a larger (here also an odd) map."""
    torch, ops = env
    case = gen.sres_case(row)
    L = case.layer
    got = ops.conv1x1_sres_bf16(dev(env, case.x), wt(env, case.kern), f32(env, L.scale), f32(env, L.shift), dev(env, case.res_map), row[5], act)
    assert_bits(env, got, case.expect(act), "%s act=%d" % (case.name, act))


@pytest.mark.parametrize("act2", [0, 1])
@pytest.mark.parametrize("act1", [0, 1])
@pytest.mark.parametrize("row", gen.PAIR_ROWS, ids=_ids)
def test_conv1x1_pair_bf16_bit_for_bit(env, row, act1, act2):
    """Both outputs of the increase -> reduce pair; y2 against the reference computed from the EXPECTED y1.  Residual and projected
    shortcut, y1 stored everywhere and at even pixels only, all four activation combinations."""
    torch, ops = env
    case = gen.pair_case(row)
    A = case.main
    kw = dict(act1=act1, act2=act2, y1_sub2=case.sub2)
    if case.projected:
        kw.update(x2=dev(env, case.x2), wp_packed=wt(env, case.kp), scale_p=f32(env, case.proj.scale), shift_p=f32(env, case.proj.shift))
    else:
        kw.update(res=dev(env, case.res))
    y1, y2 = ops.conv1x1_pair_bf16(dev(env, case.x), wt(env, case.k1), f32(env, A.scale), f32(env, A.shift), wt(env, case.k2), f32(env, case.sc2),
                                   f32(env, case.sh2), **kw)
    want1, want2 = case.expect(act1, act2)
    if case.sub2:
        want1 = tuple(a[:, ::2, ::2, :] for a in want1)
    what = "%s act1=%d act2=%d" % (case.name, act1, act2)
    assert_bits(env, y1, want1, what + " y1")
    assert_bits(env, y2, want2, what + " y2")


def _stem_args(env, case):
    L = case.layer
    return f32(env, case.x), env[1].bf16_from_bits(gen.pack_stem_weight(case.kern.astype(np.float32))), f32(env, L.scale), f32(env, L.shift)


@pytest.mark.parametrize("row", gen.STEM_ROWS, ids=_ids)
def test_stem7x7_bf16_bit_for_bit(env, row):
    """bf16(relu(s x.w + b)) on integer pixels (the patch stem, csrc/conv_bf16.hip)."""
    torch, ops = env
    case = gen.stem_case(row)
    assert_bits(env, ops.stem7x7_bf16(*_stem_args(env, case)), case.expect(), case.name)


@pytest.mark.parametrize("row", gen.STEM_POOL_ROWS, ids=_ids)
def test_stem7x7_pool_bf16_bit_for_bit(env, row):
    """conv1 + ReLU + clipped max-pool in one kernel (the streaming stem; the 7 x 9 image runs the patch kernel): the pooled map bit for
    bit, and bit for bit the two-kernel path where that pools without padding -- on exact inputs no accumulation order differs."""
    torch, ops = env
    case = gen.stem_case(row)
    ceil, ppad = case.pool
    args = _stem_args(env, case)
    got = ops.stem7x7_pool_bf16(*args, ceil_mode=ceil, pool_pad=ppad)
    want, conv1_pre = case.expect()
    g, w = got_bits(env, got), gen.bits(want)
    assert g.shape == w.shape
    if not np.array_equal(g, w):
        bad = np.argwhere(g != w)
        i = n, py, px, c = tuple(int(v) for v in bad[0])
        win = conv1_pre[n, max(2 * py - ppad, 0):2 * py - ppad + 3, max(2 * px - ppad, 0):2 * px - ppad + 3, c]
        pytest.fail("%s: %d of %d elements differ; first at %s: fp32 values of its window before the conversion %s, expected bf16 bits 0x%04x, device "
                    "returned 0x%04x" % (case.name, len(bad), g.size, i, win.tolist(), int(w[i]), int(g[i])))
    if ppad == 0:
        two = ops.maxpool3x3s2_bf16(ops.stem7x7_bf16(*args), ceil)
        assert torch.equal(got.view(torch.int16), two.view(torch.int16)), "%d elements differ from the two-kernel path" % int((got != two).sum())


SENTINEL = -12345.5


@pytest.mark.parametrize("row", gen.GAP_ROWS, ids=_ids)
def test_gap_bf16_exact_sums_ragged_channel_groups_and_untouched_neighbours(env, row):
    """ops.gap_bf16 on multiples of 1/4 (the fp32 sum is exact in any order): bit-exact where hw is a power of two, else equal to
    float32(sum) / float32(hw) or one fp32 ulp from it (how the division rounds is the compiler's choice).  c = 72 has a ragged last group
    of 8-channel lanes.  Then the same call into the middle of a buffer of sentinels: nothing outside [n, c] is written."""
    torch, ops = env
    from hse_facerec_tf_amd import _lib
    n, hw, c = row
    case = gen.GapCase(row)
    x = dev(env, case.x)
    got = ops.gap_bf16(x)
    assert tuple(got.shape) == (n, c) and got.dtype == torch.float32
    g = got.cpu().numpy()
    if case.exact_division:
        bad = np.argwhere(g.view(np.uint32) != case.want.view(np.uint32))
    else:
        lo, hi = np.nextafter(case.want, np.float32(-np.inf)), np.nextafter(case.want, np.float32(np.inf))
        bad = np.argwhere((g != case.want) & (g != lo) & (g != hi))
    if len(bad):
        i = tuple(int(v) for v in bad[0])
        pytest.fail("%s: %d of %d elements differ%s; first at %s: sum %r / %d, expected %r, device returned %r" % (
            case.name, len(bad), g.size, "" if case.exact_division else " by more than one fp32 ulp", i, float(case.sum[i]), hw, float(case.want[i]), float(g[i])))
    guard = 256
    buf = torch.full((guard + n * c + guard,), SENTINEL, dtype=torch.float32, device="cuda")
    _lib.check(_lib.lib().hsefr_gap_bf16(x.data_ptr(), buf.data_ptr() + 4 * guard, n, hw, c, _lib.current_stream_ptr()), "hsefr_gap_bf16")
    b = buf.cpu().numpy()
    assert np.array_equal(b[guard:guard + n * c].view(np.uint32), g.reshape(-1).view(np.uint32))
    assert (b[:guard] == np.float32(SENTINEL)).all() and (b[guard + n * c:] == np.float32(SENTINEL)).all()
