"""Exact operands and references for the bf16 ResNet kernels: what tests/test_resnet50_rounding_gpu.py feeds every epilogue of
csrc/conv*_bf16.hip and the stems, and what tests/test_resnet50_rounding_cpu.py checks before that test may claim anything.

The documented formula (hse_facerec_tf_amd/ops.py, the headers of csrc/conv*_bf16.hip):

    y = bf16( act( bf16( fma(acc, scale[c], shift[c]) ) + R ) ),      R = residual | bf16(projection) | nothing

With dyadic operands -- activations in {0..3}, weights in {-2..2}, scales in {1, 1/2, 1/4}, shifts and residuals multiples of 1/4
-- every product and every partial sum is exact in fp32 IN ANY ORDER, so the formula fixes every output bit, whatever the tile
shape, the K blocking or the matrix instruction.  The references here are NumPy float64 with oracle.resnet50.bf16_round (the
integer-bit round-to-nearest-even formula) at exactly the documented rounding points; they share no code with the kernels.  From
the package under test only the bit-packing helpers are imported (float32 -> bf16 bits, the weight layouts).

Every generator asserts, for every case (``_check_sums`` / ``_check_f32``):
  * max sum |x| |w| / granularity < 2^24: no summation order can round;
  * every pre-rounding value v satisfies v == float32(v).

``Model`` states WHERE an implementation may deviate: the reference is ``Model()``; the alternatives (truncation, round half away
from zero, one rounding instead of two, ReLU before the residual add, a neighbouring channel's constants) are used by the CPU
test alone, which demands that the reference differs from each in a stated share of the elements of every case.

Everything is a pure function of the case's name, which seeds its RandomState.
"""
import functools
import zlib
from collections import namedtuple

import numpy as np

from oracle import resnet50 as ores
from oracle import tf_graph as tfo

from hse_facerec_tf_amd.resnet50 import pack_conv_weight, pack_stem_weight, to_bf16_bits  # noqa: F401  (bit packing only)

# ---------------------------------------------------------------------------------------------------------------------------------
# the shapes
# ---------------------------------------------------------------------------------------------------------------------------------
# n, h, w, c, cout, k, s, res, act: the rows of tests/test_resnet50_gpu.py::test_conv_bf16_vs_oracle, stated once.  The kernel family
# named in front of a group is the one launch_conv_bf16 (csrc/conv_bf16.hip) routes its rows to.
CONV_SHAPES = [
    # the general implicit GEMM (conv_bf16_kernel), the persistent 1x1 (conv1x1_bf16_kernel: 1x1 stride 1) and, for the deep ones (3x3 up
    # to 150 000 pixels, stride-2 1x1 from 256 channels, 1x1 from 1024 channels), the LDS-DMA GEMM
    (2, 14, 14, 64, 64, 1, 1, False, 1), (2, 14, 14, 64, 256, 1, 1, True, 1), (1, 28, 28, 256, 128, 1, 2, False, 1),
    (2, 13, 11, 128, 128, 3, 1, False, 1), (1, 56, 56, 64, 64, 3, 1, False, 1), (3, 7, 7, 512, 512, 3, 1, False, 1),
    (2, 7, 7, 512, 2048, 1, 1, True, 1), (1, 15, 15, 256, 512, 1, 2, False, 0), (1, 9, 9, 1024, 256, 1, 1, False, 1),
    (5, 5, 5, 64, 192, 3, 1, True, 0),
    # the LDS-DMA implicit GEMM (csrc/conv_dma_bf16.hip): stride-2 projection from 512 channels, many tiles per workgroup with a
    # ragged last tile, residual + ReLU on a 3x3, a 5x5 kernel, stride 2 with padding
    (2, 9, 9, 512, 128, 1, 2, False, 0), (37, 14, 14, 64, 256, 3, 1, True, 1), (3, 11, 13, 128, 64, 5, 1, False, 1),
    (2, 12, 12, 64, 128, 3, 2, False, 1),
    # the window 3x3 kernel (csrc/conv3x3_win_bf16.hip; maps at least 40 wide): its four tile shapes, ragged image groups, residual
    (2, 6, 40, 64, 128, 3, 1, True, 1), (1, 4, 48, 128, 256, 3, 1, False, 1), (3, 2, 44, 64, 64, 3, 1, False, 0),
    (1, 28, 56, 64, 64, 3, 1, True, 1), (2, 5, 41, 192, 192, 3, 1, False, 1),
    # the four-wave window 3x3 kernel (csrc/conv3x3_w2_bf16.hip, round 5): its three geometries (rows of <= 16 / 32 / 64 pixels),
    # several channel slabs, residual, heights that are not a multiple of the tile's rows, columns dropped at the right edge,
    # more tiles than workgroups (a persistent workgroup walks two tiles)
    (2, 14, 14, 256, 256, 3, 1, False, 1), (3, 13, 12, 64, 128, 3, 1, True, 1), (1, 15, 16, 128, 128, 3, 1, False, 0),
    (2, 28, 28, 128, 128, 3, 1, False, 1), (1, 9, 25, 64, 128, 3, 1, True, 1), (1, 30, 32, 64, 256, 3, 1, False, 1),
    (2, 6, 50, 128, 64, 3, 1, True, 1), (1, 7, 64, 64, 192, 3, 1, False, 1), (260, 14, 14, 64, 128, 3, 1, False, 1),
    # the four-wave 1x1 GEMM (csrc/conv1x1_w4_bf16.hip, round 5: K-deep reductions with >= 20 000 output pixels): stride 1 and 2 (gathered
    # rows), a ragged last tile, several tiles per workgroup
    (103, 14, 14, 256, 128, 1, 1, False, 1), (30, 53, 54, 256, 128, 1, 2, False, 1), (27, 28, 28, 512, 256, 1, 1, False, 0),
    # ... and the four-wave window 3x3 kernel's FLAT geometry for maps of at most 7 x 7: whole images per tile, ragged image groups,
    # 6-pixel edges, residual
    (6, 7, 7, 128, 128, 3, 1, False, 1), (5, 6, 7, 64, 64, 3, 1, True, 1), (2, 7, 6, 128, 192, 3, 1, False, 0), (131, 7, 7, 64, 128, 3, 1, True, 1)]

# (n, h, w, c, cout, k, s) of the exact test: every row above but the two whose only purpose is a tile count (n = 260, n = 131); each
# runs with and without a residual and with both activations
EXACT_CONV_ROWS = [r[:7] for r in CONV_SHAPES if r[0] not in (260, 131)]
# ... and the general kernel's two larger tiles, which no row above reaches (choose_tile_b takes 64 x 64 while one round of workgroups
# holds every tile): 24 948 pixels make 390 tiles of 128 x 128 for 256 channels (one round, where 64 x 64 needs three) and 585 tiles of
# 128 x 64 for 192 channels (one round, 64 x 64 two); stride 2 from 64 channels stays off the LDS-DMA GEMM.  The last tile is ragged.
EXACT_CONV_ROWS += [(33, 55, 53, 64, 256, 3, 2), (33, 55, 53, 64, 192, 1, 2)]

# n, oh, ow, c, cout, c2, stride2, h2, w2: the persistent PROJ kernel (conv1x1_bf16.hip), an odd stride-2 view, and the four-wave PROJ
# kernel (conv1x1_w4_bf16.hip: >= 192 tiles of 224 x 128 and K + K2 >= 256)
PROJ_ROWS = [(2, 14, 14, 64, 256, 64, 1, 14, 14), (5, 9, 11, 64, 192, 128, 2, 17, 22), (14, 28, 28, 128, 512, 256, 2, 56, 56)]

# n, oh, ow, c, cout, res_stride, h2, w2: the strided-residual form (conv1x1_bf16.hip), an odd larger map
SRES_ROWS = [(2, 28, 28, 64, 256, 2, 56, 56), (2, 13, 9, 64, 128, 2, 25, 17)]

# n, h, w, projected shortcut, y1 stored at even pixels only: the increase -> reduce pair (conv1x1_pair_bf16.hip), 64 -> 256 -> 64
PAIR_ROWS = [(2, 14, 14, False, False), (1, 9, 7, True, False), (1, 13, 9, False, True), (1, 13, 9, True, True)]

# n, h, w: the patch stem (stem7x7_bf16_kernel)
STEM_ROWS = [(2, 64, 64), (3, 37, 37)]

# n, h, w, ceil_mode, pool_pad: the streaming stem (stem7s_stream_kernel); the 7 x 9 image is below its minimum and runs the patch
# kernel (stem7x7_pool_bf16_kernel)
STEM_POOL_ROWS = [(2, 64, 64, True, 0), (3, 37, 51, True, 0), (2, 38, 38, False, 1), (2, 7, 9, True, 0)]

# n, hw, c: c = 72 is nine 8-channel lanes, the ragged last channel group of gap_bf16_kernel
GAP_ROWS = [(n, hw, c) for n in (1, 3) for hw in (1, 49, 50, 64) for c in (8, 64, 72, 2048)]


# ---------------------------------------------------------------------------------------------------------------------------------
# rounding models
# ---------------------------------------------------------------------------------------------------------------------------------
def _bits32(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def rne(a):
    """The documented conversion: round to nearest, ties to even."""
    return ores.bf16_round(a)


def trunc(a):
    """Drop the low 16 bits (round toward zero)."""
    return (_bits32(a) & np.uint32(0xFFFF0000)).view(np.float32).astype(np.float64)


def half_away(a):
    """Round to nearest, ties away from zero (add half an ulp to the magnitude, then drop)."""
    u = _bits32(a).astype(np.uint64)
    return (((u + 0x8000) >> 16) << 16).astype(np.uint32).view(np.float32).astype(np.float64)


def bits(a):
    """bf16 bit patterns (uint16) of values that ARE bf16 values."""
    a32 = np.ascontiguousarray(a, dtype=np.float32)
    u = a32.view(np.uint32)
    assert not (u & np.uint32(0xFFFF)).any()
    return (u >> np.uint32(16)).astype(np.uint16)


class Model(namedtuple("Model", "first final proj single relu_first neighbour")):
    """Where an implementation rounds and in which order it works.  first: the conversion of fma(acc, scale, shift); proj: the same for
    the projected shortcut; final: the conversion of the stored value.  single: R is added to the UNROUNDED value(s).  relu_first: the
    activation is applied before R is added (and again after).  neighbour: channel c uses the constants of channel c - 1."""
    __slots__ = ()

    def __new__(cls, first=rne, final=rne, proj=rne, single=False, relu_first=False, neighbour=False):
        return super().__new__(cls, first, final, proj, single, relu_first, neighbour)


REFERENCE = Model()


def alternatives(has_r, projected, act):
    """name -> (model, the least share of elements in which the reference must differ from it).  The shares are conditions that keep
    the bit-for-bit test from being vacuous, not measurements."""
    alt = {"trunc-first": (Model(first=trunc), 0.05), "half-away-first": (Model(first=half_away), 0.01),
           "neighbour": (Model(neighbour=True), 0.50)}
    if has_r:       # (without an R the stored value is bf16(act(bf16(v))): the final conversion has nothing to round)
        alt.update({"trunc-final": (Model(final=trunc), 0.05), "half-away-final": (Model(final=half_away), 0.01),
                    "single": (Model(single=True), 0.05)})
        if act == 1:
            alt["relu-first"] = (Model(relu_first=True), 0.20)
    if projected:
        alt.update({"trunc-proj": (Model(proj=trunc), 0.05), "half-away-proj": (Model(proj=half_away), 0.01)})
    return alt


# ---------------------------------------------------------------------------------------------------------------------------------
# exactness
# ---------------------------------------------------------------------------------------------------------------------------------
def _granularity(a):
    """The largest power of two that divides every element."""
    a = np.asarray(a, np.float64)
    for k in range(0, 64):
        s = a * 2.0 ** k
        if np.array_equal(s, np.rint(s)):
            return 2.0 ** -k
    raise AssertionError("not dyadic")


def _check_sums(x, kern, stride, pad):
    """No summation order can round: every partial sum is a multiple of g = gran(x) gran(w) and below 2^24 g in magnitude."""
    g = _granularity(x) * _granularity(kern)
    bound = tfo.conv2d(np.abs(x), np.abs(kern), (stride, stride), "", explicit_pads=(pad,) * 4).max() / g
    assert bound < 2.0 ** 24, bound


def _check_f32(*values):
    for v in values:
        assert np.array_equal(v, v.astype(np.float32).astype(np.float64)), "a pre-rounding value is not an fp32 number"


def _rs(name):
    return np.random.RandomState(zlib.crc32(name.encode()))


def _name(kind, row):
    return kind + "-" + "x".join(str(int(v)) for v in row)


# ---------------------------------------------------------------------------------------------------------------------------------
# operands
# ---------------------------------------------------------------------------------------------------------------------------------
def _acts(rs, shape):
    return rs.randint(0, 4, shape).astype(np.float64)


def _weights(rs, shape):
    return rs.randint(-2, 3, shape).astype(np.float64)


def _scale(rs, cout):
    """Powers of two; every channel's differs from both neighbours' (cyclically)."""
    sc = np.array([1.0, 0.5, 0.25])[(np.arange(cout) + rs.randint(3)) % 3]
    sc[-1] = [v for v in (1.0, 0.5, 0.25) if v not in (sc[0], sc[-2])][0]
    assert (sc != np.roll(sc, 1)).all()
    return sc.astype(np.float32)


def _shift(rs, cout, span=2400):
    return (rs.randint(-span, span + 1, cout) / 4.0).astype(np.float32)


def _residual(rs, shape, span=1200):
    return ores.bf16_round(rs.randint(-span, span + 1, shape) / 4.0)


class Layer:
    """One convolution's exact accumulator with its constants: pre(model) is fma(acc, scale[c], shift[c]) in float64."""

    def __init__(self, x, kern, scale, shift, stride=1, pad=0):
        _check_sums(x, kern, stride, pad)
        self.kern, self.scale, self.shift = kern, scale, shift
        self.acc = tfo.conv2d(x, kern, (stride, stride), "", explicit_pads=(pad,) * 4)
        self._pre = self.acc * self.scale.astype(np.float64) + self.shift.astype(np.float64)
        self._pre.setflags(write=False)
        _check_f32(self._pre)

    def pre(self, m):
        if not m.neighbour:
            return self._pre
        return self.acc * np.roll(self.scale.astype(np.float64), 1) + np.roll(self.shift.astype(np.float64), 1)


def epilogue(pre, r, r_pre, act, m, check=False):
    """The documented formula from the pre-rounding value(s): r is a stored bf16 residual, r_pre the projection's pre-rounding value (at
    most one of them).  -> (stored value, the value the final conversion saw)."""
    relu = (lambda a: np.maximum(a, 0)) if act == 1 else (lambda a: a)
    assert r is None or r_pre is None
    if m.single:
        t = pre + (r if r is not None else r_pre if r_pre is not None else 0.0)
    else:
        t = m.first(pre)
        if m.relu_first:
            t = relu(t)
        if r is not None:
            t = t + r
        elif r_pre is not None:
            t = t + m.proj(r_pre)
    t = relu(t)
    if check:
        _check_f32(t)
    return m.final(t), t


# ---------------------------------------------------------------------------------------------------------------------------------
# cases
# ---------------------------------------------------------------------------------------------------------------------------------
class ConvCase:
    """ops.conv_bf16 at one row of EXACT_CONV_ROWS: expect(res, act) for the four forms it runs in."""

    def __init__(self, row):
        n, h, w, c, cout, k, s = row
        self.row, self.name = row, _name("conv", row)
        rs = _rs(self.name)
        self.x, self.kern = _acts(rs, (n, h, w, c)), _weights(rs, (k, k, c, cout))
        self.pad = (k - 1) // 2
        self.layer = Layer(self.x, self.kern, _scale(rs, cout), _shift(rs, cout), s, self.pad)
        self.res = _residual(rs, self.layer.acc.shape)
        for res in (False, True):
            for act in (0, 1):
                self.expect(res, act, check=True)

    def expect(self, res, act, m=REFERENCE, check=False):
        return epilogue(self.layer.pre(m), self.res if res else None, None, act, m, check)


class ProjCase:
    """ops.conv1x1_proj_bf16: act(bf16(a) + bf16(p)), p the stride-2 (or stride-1) projection of the block input."""

    def __init__(self, row):
        n, oh, ow, c, cout, c2, s2, h2, w2 = row
        self.row, self.name = row, _name("proj", row)
        rs = _rs(self.name)
        self.x, self.k1 = _acts(rs, (n, oh, ow, c)), _weights(rs, (1, 1, c, cout))
        self.x2, self.k2 = _acts(rs, (n, h2, w2, c2)), _weights(rs, (1, 1, c2, cout))
        self.main = Layer(self.x, self.k1, _scale(rs, cout), _shift(rs, cout))
        self.proj = Layer(self.x2, self.k2, _scale(rs, cout), _shift(rs, cout, 1200), s2)
        assert self.proj.acc.shape == self.main.acc.shape
        for act in (0, 1):
            self.expect(act, check=True)

    def expect(self, act, m=REFERENCE, check=False):
        return epilogue(self.main.pre(m), None, self.proj.pre(m._replace(neighbour=False)), act, m, check)


class SresCase:
    """ops.conv1x1_sres_bf16: the residual is every res_stride-th pixel of a larger map."""

    def __init__(self, row):
        n, oh, ow, c, cout, st, h2, w2 = row
        self.row, self.name = row, _name("sres", row)
        rs = _rs(self.name)
        self.x, self.kern = _acts(rs, (n, oh, ow, c)), _weights(rs, (1, 1, c, cout))
        self.layer = Layer(self.x, self.kern, _scale(rs, cout), _shift(rs, cout))
        self.res_map = _residual(rs, (n, h2, w2, cout))
        self.res = self.res_map[:, ::st, ::st, :][:, :oh, :ow, :]
        assert self.res.shape == self.layer.acc.shape
        for act in (0, 1):
            self.expect(act, check=True)

    def expect(self, act, m=REFERENCE, check=False):
        return epilogue(self.layer.pre(m), self.res, None, act, m, check)


class PairCase:
    """ops.conv1x1_pair_bf16: y1 = act1(bf16(s1 x.w1 + b1) + R), y2 = act2(bf16(s2 y1.w2 + b2)) from the EXPECTED y1 (the reference's own,
    whatever model it is asked for: a deviation in y1 propagates)."""
    C, C1, C2 = 64, 256, 64

    def __init__(self, row):
        n, h, w, proj, sub2 = row
        self.row, self.name, self.projected, self.sub2 = row, _name("pair", row), proj, sub2
        rs = _rs(self.name)
        self.x, self.k1 = _acts(rs, (n, h, w, self.C)), _weights(rs, (1, 1, self.C, self.C1))
        self.k2 = rs.choice([-1.0, 0.0, 1.0], size=(1, 1, self.C1, self.C2), p=[0.0625, 0.875, 0.0625])
        self.sc2, self.sh2 = _scale(rs, self.C2), np.abs(_shift(rs, self.C2, 600))
        # (value ranges of their own: a conversion can meet a tie only where it drops bits, |v| >= 64 on the 1/4 lattice these values live
        # on, and meets one less often the more bits it drops.  y1 wants magnitudes of 64 .. 256 -- shifts within +-150, residuals within
        # +-50 -- and y2 = s2 y1.w2 + b2, a sum over 256 such values, wants to stay in the hundreds: w2 in {-1, 0, 1}, seven eighths zero.  b2 >= 0: with only
        # 64 channels, ReLU must not zero whole channels, or a neighbouring channel's constants give the same zeros)
        self.main = Layer(self.x, self.k1, _scale(rs, self.C1), _shift(rs, self.C1, 1000))
        self.res = self.x2 = self.kp = self.proj = None
        if proj:
            self.x2, self.kp = _acts(rs, (n, h, w, 64)), _weights(rs, (1, 1, 64, self.C1))
            self.proj = Layer(self.x2, self.kp, _scale(rs, self.C1), _shift(rs, self.C1, 1000))
        else:
            self.res = _residual(rs, (n, h, w, self.C1), 200)
        self._second = {}
        for act1 in (0, 1):
            for act2 in (0, 1):
                self.expect(act1, act2, check=True)

    def expect_y1(self, act1, m=REFERENCE, check=False):
        return epilogue(self.main.pre(m), self.res, None if self.proj is None else self.proj.pre(m._replace(neighbour=False)), act1, m, check)

    def second(self, y1):
        return Layer(y1, self.k2, self.sc2, self.sh2)

    def expect(self, act1, act2, m1=REFERENCE, m2=REFERENCE, check=False):
        """-> ((y1, pre-final y1), (y2, pre-final y2)); y1 is the full map, the caller takes [:, ::2, ::2] where it is stored compact."""
        y1 = self.expect_y1(act1, m1, check)
        if m1 is not REFERENCE:
            second = self.second(y1[0])
        elif act1 in self._second:
            second = self._second[act1]
        else:
            second = self._second[act1] = self.second(y1[0])
        return y1, epilogue(second.pre(m2), None, None, act2, m2, check)


def _clipped_maxpool(c1, ceil, ppad):
    """3x3 / stride 2 max-pool with ppad rows / columns of padding in front, the last window clipped (ceil mode) or dropped."""
    n, oh, ow, c = c1.shape
    ph = (-(-(oh + 2 * ppad - 3) // 2) if ceil else (oh + 2 * ppad - 3) // 2) + 1
    pw = (-(-(ow + 2 * ppad - 3) // 2) if ceil else (ow + 2 * ppad - 3) // 2) + 1
    pb, pr = max((ph - 1) * 2 + 3 - oh - ppad, 0), max((pw - 1) * 2 + 3 - ow - ppad, 0)
    xp = np.pad(c1, ((0, 0), (ppad, pb), (ppad, pr), (0, 0)), constant_values=-np.inf)
    out = np.full((n, ph, pw, c), -np.inf)
    for dy in range(3):
        for dx in range(3):
            out = np.maximum(out, xp[:, dy:dy + 2 * (ph - 1) + 1:2, dx:dx + 2 * (pw - 1) + 1:2, :])
    return out


class StemCase:
    """ops.stem7x7_bf16 (pool = None) and ops.stem7x7_pool_bf16 (pool = (ceil_mode, pool_pad)): bf16(relu(s x.w + b)) on fp32 pixels that
    are integers in [-128, 127], then the clipped max-pool of the stored values."""

    def __init__(self, row):
        n, h, w = row[:3]
        self.row, self.pool = row, (row[3:] or None)
        self.name = _name("stem", [int(v) for v in row])
        rs = _rs(self.name)
        self.x = rs.randint(-128, 128, (n, h, w, 3)).astype(np.float64)
        self.kern = _weights(rs, (7, 7, 3, 64))
        assert np.array_equal(ores.bf16_round(self.x), self.x)            # the kernel converts the pixels to bf16: exact here
        self.layer = Layer(self.x, self.kern, _scale(rs, 64), _shift(rs, 64), 2, 3)
        self.expect(check=True)

    def expect(self, m=REFERENCE, check=False):
        """-> (stored value, the conv1 map's value before its conversion -- unpooled)."""
        y, t = epilogue(self.layer.pre(m), None, None, 1, m, check)
        return (y if self.pool is None else _clipped_maxpool(y, *self.pool)), t


class GapCase:
    """ops.gap_bf16: bf16 inputs that are multiples of 1/4 (|k| <= 255: eight significant bits), so the fp32 sum is exact in any order."""

    def __init__(self, row):
        n, hw, c = row
        self.row, self.name = row, _name("gap", row)
        self.x = _rs(self.name).randint(-255, 256, (n, hw, 1, c)) / 4.0
        assert np.array_equal(ores.bf16_round(self.x), self.x) and hw * 255 < 2 ** 24
        self.sum = self.x.sum(axis=(1, 2))
        _check_f32(self.sum)
        self.exact_division = hw & (hw - 1) == 0
        self.want = (self.sum.astype(np.float32) / np.float32(hw)).astype(np.float32)


# One case at a time is kept: the tests walk the rows in order, every form of a row behind the other.
@functools.lru_cache(maxsize=1)
def conv_case(row):
    return ConvCase(row)


@functools.lru_cache(maxsize=1)
def proj_case(row):
    return ProjCase(row)


@functools.lru_cache(maxsize=1)
def sres_case(row):
    return SresCase(row)


@functools.lru_cache(maxsize=1)
def pair_case(row):
    return PairCase(row)


@functools.lru_cache(maxsize=1)
def stem_case(row):
    return StemCase(row)


def share(a, b):
    """The share of elements in which two results differ."""
    return float(np.mean(a != b))
