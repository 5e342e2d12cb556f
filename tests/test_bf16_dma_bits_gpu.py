"""The bits of the LDS-DMA bf16 convolution kernels, pinned (csrc/conv_dma_bf16.hip, conv3x3_w2_bf16.hip, conv1x1_w4_bf16.hip,
conv3x3_win_bf16.hip) and of the increase -> reduce pair (conv1x1_pair_bf16.hip): every case runs twice -- the two runs equal bit
for bit -- and the sha256 of the output bytes equals the digest recorded in golden/bf16_dma_bits.json.  The kernels share their
address helpers, the LDS-DMA piece, the staging of a tile's scale / shift, the epilogue of eight channels and the persistent tile
walk through csrc/bf16_dma.h: a change there that moves one sum, one FMA, one rounding or one tile of any kernel shows here.

Inputs are NOT dyadic (uniform fractions from numpy.random.RandomState, seeded from the row's name, rounded to bf16), so the order
of the accumulation matters: tests/test_resnet50_rounding_gpu.py pins the rounding points on operands that are exact in any order
and by construction cannot see that order.

The rows are tuples of tests/bf16_exact_cases.py.  Which kernel family a conv row reaches is ASSERTED: the row as a one- or two-op
plan (the convolution, and in front of it a 1x1 layer that produces its residual) is described by the library's own launchers
(Plan.describe / hsefr_plan_describe: launch_conv_bf16 with the launch suppressed, under the same knobs), and the family must be the
one in ROUTES below.  The predicates of launch_conv_bf16 (csrc/conv_bf16.hip) behind each route; each conv row runs as (residual,
ReLU) and as (no residual, linear).  ops.conv1x1_proj_bf16 and ops.conv1x1_pair_bf16 are not plan ops of their own: the PROJ row's
route is stated from conv1x1_w4_proj_preferred, the pair has one kernel.

  conv_dma    2x9x9x512x128 k1 s2          `deep`: 1x1, stride 2, c >= 256 (both forms)
              30x53x54x256x128 k1 s2       WITH its residual: conv1x1_w4_bf16_preferred wants c >= 512 then, `deep` holds: 21 870 pixels
                                           as 342 tiles of 128 x 64 on 256 workgroups -- the tile walk, the ragged last tile and the
                                           constants' parity buffer run a second tile
              3x11x13x128x64 k5 s1         `deep`: 5x5 (both forms)
  w2          3x13x12x64x128               w2_config 1 (rows of <= 16 pixels), conv3x3_w2_bf16_preferred
              37x14x14x64x256              w2_config 1 too: the row was the LDS-DMA GEMM's until the four-wave kernel took the 14-pixel maps
              1x9x25x64x128                w2_config 2 (<= 32 pixels)
              2x6x50x128x64                w2_config 3 (<= 64 pixels, 64 channels), two channel slabs
              5x6x7x64x64                  w2_config 4 (FLAT)
              260x14x14x64x128             w2_config 1, 260 tiles on 256 workgroups: the walk and the parity buffer run a second tile
  w4          103x14x14x256x128 k1 s1      WITHOUT a residual: conv1x1_w4_bf16_preferred (c >= 256, >= 20 000 pixels); with it the row
                                           runs conv1x1_bf16.hip, which is not one of these kernels and is pinned all the same
              30x53x54x256x128 k1 s2       without a residual (gathered rows)
              proj 14x28x28x128x512 <- 256 conv1x1_w4_proj_preferred: 196 tiles of 224 x 128, K + K2 >= 256; both activations
  (general)   2x12x12x64x128 k3 s2         conv_bf16.hip since the stride-2 3x3 from 64 channels left the LDS-DMA GEMM (`deep` excludes it);
                                           a development build runs it on conv_dma below
  pair        the four PAIR_ROWS, ReLU / ReLU and linear / linear: both outputs in one digest

A development build (HSEFR_LIB=libhsefr_dev.so) also runs, through its knobs, conv3x3_win_bf16.hip -- which the product does not
contain -- on its four tile shapes (w3_off = 2, w2_off = 1) and conv_dma_bf16.hip on the rows the product routes elsewhere (cd_off = 2,
w2_off = 1; the 260-image row with cd_rb = 4: 399 tiles of 128 x 128).  With the product library those cases are skipped.

`python tests/test_bf16_dma_bits_gpu.py [out.json]` records the digests of the cases the loaded library can run and keeps the others."""
import hashlib
import json
import os
import sys
import zlib

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bf16_exact_cases as gen  # noqa: E402

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "bf16_dma_bits.json")
DEV_ONLY = "needs a development build of the library (HSEFR_LIB=libhsefr_dev.so): "


def _rows(source, wanted):
    """The tuples of bf16_exact_cases.py themselves: (n, h, w, c, cout, k, s) prefixes looked up in its lists, not restated."""
    found = [r for r in source if tuple(r[:len(wanted[0])]) in wanted]
    assert len(found) == len(wanted), (found, wanted)
    return found


DMA_ROWS = _rows(gen.EXACT_CONV_ROWS, [(2, 9, 9, 512, 128, 1, 2), (37, 14, 14, 64, 256, 3, 1), (2, 12, 12, 64, 128, 3, 2), (3, 11, 13, 128, 64, 5, 1)])
W2_ROWS = _rows([r[:7] for r in gen.CONV_SHAPES], [(3, 13, 12, 64, 128, 3, 1), (1, 9, 25, 64, 128, 3, 1), (2, 6, 50, 128, 64, 3, 1), (5, 6, 7, 64, 64, 3, 1),
                                                   (260, 14, 14, 64, 128, 3, 1)])
W4_ROWS = _rows(gen.EXACT_CONV_ROWS, [(103, 14, 14, 256, 128, 1, 1), (30, 53, 54, 256, 128, 1, 2)])
PROJ_ROWS = _rows(gen.PROJ_ROWS, [(14, 28, 28, 128, 512, 256, 2, 56, 56)])
WIN_ROWS = _rows(gen.EXACT_CONV_ROWS, [(2, 6, 40, 64, 128, 3, 1), (1, 4, 48, 128, 256, 3, 1), (3, 2, 44, 64, 64, 3, 1), (1, 28, 56, 64, 64, 3, 1)])
FORCED_DMA_ROWS = _rows([r[:7] for r in gen.CONV_SHAPES], [(37, 14, 14, 64, 256, 3, 1), (2, 12, 12, 64, 128, 3, 2), (260, 14, 14, 64, 128, 3, 1)])
FORMS = [(True, 1), (False, 0)]       # (residual, act): residual + ReLU, no residual + linear

# (kind, row, form, knobs): knobs are development-build settings; a case with knobs needs a development build
CASES = [("conv", r, f, ()) for r in DMA_ROWS + W2_ROWS + W4_ROWS for f in FORMS]
CASES += [("proj", r, (None, act), ()) for r in PROJ_ROWS for act in (1, 0)]
CASES += [("pair", r, (None, act), ()) for r in gen.PAIR_ROWS for act in (1, 0)]
CASES += [("win", r, f, (("w3_off", 2), ("w2_off", 1))) for r in WIN_ROWS for f in FORMS]
CASES += [("dma", r, f, (("cd_off", 2), ("w2_off", 1)) + ((("cd_rb", 4),) if r[0] == 260 else ())) for r in FORCED_DMA_ROWS for f in FORMS]


DMA, W2, W4, WIN, C11, GEN = ("conv_dma_bf16_kernel", "conv3x3_w2_bf16_kernel", "conv1x1_w4_bf16_kernel", "conv3x3_win_bf16_kernel", "conv1x1_bf16_kernel",
                             "conv_bf16_kernel")
# (kind, row[:7]) -> family without a residual, family with one
ROUTES = {("conv", (2, 9, 9, 512, 128, 1, 2)): (DMA, DMA), ("conv", (37, 14, 14, 64, 256, 3, 1)): (W2, W2), ("conv", (2, 12, 12, 64, 128, 3, 2)): (GEN, GEN),
          ("conv", (3, 11, 13, 128, 64, 5, 1)): (DMA, DMA), ("conv", (103, 14, 14, 256, 128, 1, 1)): (W4, C11), ("conv", (30, 53, 54, 256, 128, 1, 2)): (W4, DMA)}
ROUTES.update({("conv", tuple(r)): (W2, W2) for r in W2_ROWS})
ROUTES.update({("win", tuple(r)): (WIN, WIN) for r in WIN_ROWS})
ROUTES.update({("dma", tuple(r)): (DMA, DMA) for r in FORCED_DMA_ROWS})


def set_knobs(knobs, off=False):
    from hse_facerec_tf_amd import _lib
    for key, v in knobs:
        _lib.check(_lib.lib().hsefr_debug_set(key.encode(), 0 if off else v), "hsefr_debug_set")


def route_family(row, res, knobs):
    """The kernel family launch_conv_bf16 picks for the row at its batch, asked of the library itself (no launch)."""
    from hse_facerec_tf_amd import lowering as lw
    n, h, w, c, cout, k, s = row
    pad = (k - 1) // 2
    oh, ow = (h + 2 * pad - k) // s + 1, (w + 2 * pad - k) // s + 1
    const = lambda kk: dict(w=np.zeros((cout, kk * kk * c), np.uint16), scale=np.ones(cout, np.float32), shift=np.zeros(cout, np.float32))      # noqa: E731
    layers = []
    if res:      # a 1x1 layer at the row's stride has the row's output shape
        layers.append(lw.Layer(lw.OP_CONV_BF16, "res", -1, (h, w, c), (oh, ow, cout), kh=1, kw=1, stride=s, **const(1)))
    layers.append(lw.Layer(lw.OP_CONV_BF16, "conv", -1, (h, w, c), (oh, ow, cout), act=1, kh=k, kw=k, stride=s, pad_t=pad, pad_l=pad,
                           res=0 if res else -1, **const(k)))
    for i, L in enumerate(layers):
        L.out_buf = i
    plan = lw.Plan(layers, (h, w, c), [L.out_bytes for L in layers], {}, {})
    set_knobs(knobs)
    try:
        return plan.describe(n)[-1]["family"]
    finally:
        set_knobs(knobs, off=True)


def case_id(case):
    kind, row, (res, act), _ = case
    return "%s-%s-%sact%d" % (kind, "x".join(str(int(v)) for v in row), "" if res is None else "res%d-" % res, act)


def _rs(name):
    return np.random.RandomState(zlib.crc32(name.encode()))


_DATA = {}


def _data(torch, kind, row):
    """The row's operands on the device, drawn once: activations in [0, 2), weights within +-sqrt(3 / K), scales in [0.5, 1.5),
    shifts and residuals in [-1, 1), each rounded to bf16 (float32 for the constants)."""
    key = ("conv" if kind in ("win", "dma") else kind,) + tuple(row)
    if key in _DATA:
        return _DATA[key]
    rs = _rs("-".join(str(v) for v in key))
    bf = lambda a: torch.from_numpy(a.astype(np.float32)).cuda().to(torch.bfloat16)      # noqa: E731
    f32 = lambda a: torch.from_numpy(a.astype(np.float32)).cuda()                        # noqa: E731
    act = lambda *shape: bf(rs.random_sample(shape) * 2.0)                               # noqa: E731
    wgt = lambda cout, k: bf((rs.random_sample((cout, k)) * 2.0 - 1.0) * (3.0 / k) ** 0.5)      # noqa: E731
    sc = lambda c: f32(rs.random_sample(c) + 0.5)                                        # noqa: E731
    sh = lambda c: f32(rs.random_sample(c) * 2.0 - 1.0)                                  # noqa: E731
    res = lambda *shape: bf(rs.random_sample(shape) * 2.0 - 1.0)                         # noqa: E731
    if key[0] == "conv":
        n, h, w, c, cout, k, s = row
        pad = (k - 1) // 2
        oh, ow = (h + 2 * pad - k) // s + 1, (w + 2 * pad - k) // s + 1
        d = dict(x=act(n, h, w, c), w=wgt(cout, k * k * c), sc=sc(cout), sh=sh(cout), res=res(n, oh, ow, cout))
    elif key[0] == "proj":
        n, oh, ow, c, cout, c2, s2, h2, w2 = row
        d = dict(x=act(n, oh, ow, c), w=wgt(cout, c), sc=sc(cout), sh=sh(cout), x2=act(n, h2, w2, c2), w2=wgt(cout, c2), sc2=sc(cout), sh2=sh(cout))
    else:
        n, h, w, proj, sub2 = row
        d = dict(x=act(n, h, w, 64), w1=wgt(256, 64), sc1=sc(256), sh1=sh(256), w2=wgt(64, 256), sc2=sc(64), sh2=sh(64))
        if proj:
            d.update(x2=act(n, h, w, 64), wp_packed=wgt(256, 64), scale_p=sc(256), shift_p=sh(256))
        else:
            d.update(res=res(n, h, w, 256))
    _DATA[key] = d
    return d


def is_dev_build():
    from hse_facerec_tf_amd import _lib
    return hasattr(_lib.lib(), "hsefr_debug_set")


def run_case(torch, ops, case):
    """-> the case's output tensors (one; the pair: y1 and y2)."""
    kind, row, (res, act), knobs = case
    d = _data(torch, kind, row)
    set_knobs(knobs)
    try:
        if kind == "proj":
            return (ops.conv1x1_proj_bf16(d["x"], d["w"], d["sc"], d["sh"], d["x2"], d["w2"], d["sc2"], d["sh2"], row[6], act),)
        if kind == "pair":
            extra = {k: d[k] for k in ("res", "x2", "wp_packed", "scale_p", "shift_p") if k in d}
            return ops.conv1x1_pair_bf16(d["x"], d["w1"], d["sc1"], d["sh1"], d["w2"], d["sc2"], d["sh2"], act1=act, act2=act, y1_sub2=row[4], **extra)
        k, s = row[5], row[6]
        return (ops.conv_bf16(d["x"], d["w"], d["sc"], d["sh"], k, k, s, (k - 1) // 2, d["res"] if res else None, act),)
    finally:
        set_knobs(knobs, off=True)


def digest(torch, ys):
    h = hashlib.sha256()
    for y in ys:
        assert y.dtype == torch.bfloat16
        h.update(y.contiguous().view(torch.int16).cpu().numpy().tobytes())
    return h.hexdigest()


@pytest.fixture(scope="module")
def env():
    import torch
    assert torch.cuda.is_available()
    from hse_facerec_tf_amd import ops
    return torch, ops


@pytest.fixture(scope="module")
def recorded():
    with open(FIXTURE) as f:
        return json.load(f)


def test_the_fixture_lists_exactly_these_cases(recorded):
    assert sorted(recorded) == sorted(case_id(c) for c in CASES)


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_bf16_dma_bits(env, recorded, case):
    torch, ops = env
    if case[3] and not is_dev_build():
        pytest.skip(DEV_ONLY + ("conv3x3_win_bf16.hip is not part of the product" if case[0] == "win" else "the product has no knob that forces conv_dma_bf16.hip"))
    if case[0] in ("conv", "win", "dma"):
        assert route_family(case[1], case[2][0], case[3]) == [ROUTES[case[0], tuple(case[1])][int(case[2][0])]]
    a = run_case(torch, ops, case)
    b = run_case(torch, ops, case)
    for ya, yb in zip(a, b):
        assert torch.equal(ya, yb), "two launches differ"
        assert bool(torch.isfinite(ya.float()).all())
    assert digest(torch, a) == recorded[case_id(case)]


if __name__ == "__main__":
    import torch
    from hse_facerec_tf_amd import ops
    path = sys.argv[1] if len(sys.argv) > 1 else FIXTURE
    table = {}
    if os.path.exists(path):
        with open(path) as f:
            table = json.load(f)
    wanted = {case_id(c) for c in CASES}
    table = {k: v for k, v in table.items() if k in wanted}
    for c in CASES:
        if c[3] and not is_dev_build():
            continue
        a, b = run_case(torch, ops, c), run_case(torch, ops, c)
        assert all(torch.equal(ya, yb) for ya, yb in zip(a, b)), case_id(c)
        d = digest(torch, a)
        if case_id(c) in table and table[case_id(c)] != d:
            print("CHANGED", case_id(c))
        table[case_id(c)] = d
        print(case_id(c), d)
    with open(path, "w") as f:
        json.dump(table, f, indent=1, sort_keys=True)
        f.write("\n")
    print("recorded %d digests in %s" % (len(table), path))
