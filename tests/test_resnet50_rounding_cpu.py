"""The bit-for-bit test of the bf16 ResNet kernels (tests/test_resnet50_rounding_gpu.py) can see what it claims to see: on every
case it runs, the reference of tests/bf16_exact_cases.py differs from each plausible wrong implementation -- truncation and round
half away at each rounding point, one rounding of y + R instead of two, ReLU before the residual add, a neighbouring channel's scale
and shift -- in at least the share of elements that ``alternatives`` states.  The shares are floors that keep the GPU test from being
vacuous; a case that misses one gets other value ranges, never a lower floor.

The generators assert exactness themselves (no summation order can round; every pre-rounding value is an fp32 number), so building
a case here is that check."""
import numpy as np
import pytest

from oracle import resnet50 as ores

import bf16_exact_cases as gen


def check_floors(what, want, expect, alts):
    """expect(model) -> stored values; every alternative differs from ``want`` in at least its floor."""
    report = []
    for name, (model, floor) in sorted(alts.items()):
        s = gen.share(want, expect(model))
        report.append("%s %.3f (>= %.2f)" % (name, s, floor))
        assert s >= floor, "%s: the reference differs from '%s' in %.4f of the elements, floor %.2f" % (what, name, s, floor)
    print(what, "; ".join(report))


def test_rounding_models_on_known_values():
    """The three conversions on values whose result is known by hand: 1 + 2^-8 is a tie between 1 and 1 + 2^-7 (even: 1),
    1 + 3 * 2^-8 a tie between 1 + 2^-7 and 1 + 2^-6 (even: the upper)."""
    v = np.array([1 + 2.0 ** -8, 1 + 3 * 2.0 ** -8, 1 + 2.0 ** -8 + 2.0 ** -12, 1 + 2.0 ** -7 - 2.0 ** -12, -(1 + 2.0 ** -8), -(1 + 2.0 ** -7 - 2.0 ** -12)])
    u = 2.0 ** -7
    assert np.array_equal(gen.rne(v), [1, 1 + 2 * u, 1 + u, 1 + u, -1, -(1 + u)])
    assert np.array_equal(gen.trunc(v), [1, 1 + u, 1, 1, -1, -1])
    assert np.array_equal(gen.half_away(v), [1 + u, 1 + 2 * u, 1 + u, 1 + u, -(1 + u), -(1 + u)])
    assert np.array_equal(gen.bits(np.array([1.0, -2.0, 0.0])), [0x3F80, 0xC000, 0])
    with pytest.raises(AssertionError):
        gen.bits(v[:1])


def test_generators_refuse_inexact_operands():
    """The exactness conditions are live: operands whose sums could round, and pre-rounding values outside fp32, are refused."""
    x = np.full((1, 1, 1, 64), 2.0 ** 12)
    with pytest.raises(AssertionError):
        gen.Layer(x, np.full((1, 1, 64, 64), 2.0 ** 7), np.ones(64, np.float32), np.zeros(64, np.float32))
    with pytest.raises(AssertionError):
        gen.Layer(np.full((1, 1, 1, 64), 3.0), np.ones((1, 1, 64, 64)), np.ones(64, np.float32), np.full(64, 2.0 ** -24, np.float32))
    assert gen._granularity(np.array([0.75, 2.0, -0.5])) == 0.25


def test_shape_lists_keep_every_family():
    """The rows each kernel family needs are in the lists the GPU test walks, and only the two tile-count rows left."""
    need = [(2, 14, 14, 64, 64, 1, 1), (5, 5, 5, 64, 192, 3, 1), (2, 12, 12, 64, 128, 3, 2), (2, 14, 14, 64, 256, 1, 1), (2, 7, 7, 512, 2048, 1, 1),
            (2, 9, 9, 512, 128, 1, 2), (37, 14, 14, 64, 256, 3, 1), (3, 11, 13, 128, 64, 5, 1), (2, 14, 14, 256, 256, 3, 1), (3, 13, 12, 64, 128, 3, 1),
            (1, 30, 32, 64, 256, 3, 1), (1, 7, 64, 64, 192, 3, 1), (6, 7, 7, 128, 128, 3, 1), (5, 6, 7, 64, 64, 3, 1), (103, 14, 14, 256, 128, 1, 1),
            (30, 53, 54, 256, 128, 1, 2), (27, 28, 28, 512, 256, 1, 1)]
    assert set(need) <= set(gen.EXACT_CONV_ROWS) and len(set(gen.EXACT_CONV_ROWS)) == len(gen.EXACT_CONV_ROWS)
    assert sorted(r[0] for r in gen.CONV_SHAPES if r[:7] not in gen.EXACT_CONV_ROWS) == [131, 260]
    assert {(n, hw, c) for n in (1, 3) for hw in (1, 49, 50, 64) for c in (8, 64, 72, 2048)} == set(gen.GAP_ROWS)


@pytest.mark.parametrize("row", gen.EXACT_CONV_ROWS, ids=lambda r: "x".join(map(str, r)))
def test_conv_cases_tell_the_alternatives_apart(row):
    case = gen.conv_case(row)
    for res in (False, True):
        for act in (0, 1):
            want = case.expect(res, act)[0]
            assert np.array_equal(ores.bf16_round(want), want)
            check_floors("%s res=%d act=%d" % (case.name, res, act), want, lambda m: case.expect(res, act, m)[0], gen.alternatives(res, False, act))


@pytest.mark.parametrize("row", gen.PROJ_ROWS, ids=lambda r: "x".join(map(str, r)))
def test_proj_cases_tell_the_alternatives_apart(row):
    case = gen.proj_case(row)
    for act in (0, 1):
        want = case.expect(act)[0]
        check_floors("%s act=%d" % (case.name, act), want, lambda m: case.expect(act, m)[0], gen.alternatives(True, True, act))


@pytest.mark.parametrize("row", gen.SRES_ROWS, ids=lambda r: "x".join(map(str, r)))
def test_sres_cases_tell_the_alternatives_apart(row):
    case = gen.sres_case(row)
    for act in (0, 1):
        want = case.expect(act)[0]
        check_floors("%s act=%d" % (case.name, act), want, lambda m: case.expect(act, m)[0], gen.alternatives(True, False, act))
    # ... and the gathered residual is not the map's leading block: a kernel that ignored the stride would be seen
    assert gen.share(case.res, case.res_map[:, :case.res.shape[1], :case.res.shape[2], :]) > 0.9


@pytest.mark.parametrize("row", gen.PAIR_ROWS, ids=lambda r: "x".join(str(int(v)) for v in r))
def test_pair_cases_tell_the_alternatives_apart(row):
    case = gen.pair_case(row)
    for act1 in (0, 1):
        want1 = case.expect_y1(act1)[0]
        check_floors("%s y1 act1=%d" % (case.name, act1), want1, lambda m: case.expect_y1(act1, m)[0], gen.alternatives(True, case.projected, act1))
        for act2 in (0, 1):
            want2 = case.expect(act1, act2)[1][0]
            check_floors("%s y2 act1=%d act2=%d" % (case.name, act1, act2), want2, lambda m: case.expect(act1, act2, m2=m)[1][0],
                         gen.alternatives(False, False, act2))
            # y2 is computed from y1 as stored: a y1 that kept its unrounded value in registers would be seen in y2
            alt = case.expect(act1, act2, m1=gen.Model(final=gen.trunc))[1][0]
            assert gen.share(want2, alt) >= 0.05, gen.share(want2, alt)
    if case.sub2:      # the even pixels are not the map's leading block
        full = case.expect_y1(0)[0]
        sub = full[:, ::2, ::2, :]
        assert gen.share(sub, full[:, :sub.shape[1], :sub.shape[2], :]) > 0.9


@pytest.mark.parametrize("row", gen.STEM_ROWS + gen.STEM_POOL_ROWS, ids=lambda r: "x".join(str(int(v)) for v in r))
def test_stem_cases_tell_the_alternatives_apart(row):
    case = gen.stem_case(row)
    want = case.expect()[0]
    check_floors(case.name, want, lambda m: case.expect(m)[0], gen.alternatives(False, False, 1))


@pytest.mark.parametrize("row", gen.GAP_ROWS, ids=lambda r: "x".join(map(str, r)))
def test_gap_cases_are_exact(row):
    case = gen.GapCase(row)
    n, hw, c = row
    assert case.want.shape == (n, c) and case.want.dtype == np.float32
    assert np.abs(case.want.astype(np.float64) * hw - case.sum).max() <= np.abs(case.sum).max() * 2.0 ** -23
    if case.exact_division:
        assert hw in (1, 64) and np.array_equal(case.want.astype(np.float64) * hw, case.sum)
    assert len(np.unique(case.want)) > min(n * c, 100) // 2          # a channel mix-up gives another value
