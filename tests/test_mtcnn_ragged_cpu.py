"""CPU suite: the mixed-size detector pass without a GPU -- the names libhsefr_ragged.so exports, its tables' layout and the bodies it
shares with libhsefr.so (what holds for every library is in tests/test_libraries_cpu.py), every entry point's argument checks before any device work, and the two pure planning functions: mtcnn.ragged_plan (the tables the kernels read) and
mtcnn.plan_mixed_passes (which frames share which pass)."""
import ctypes
import os
import re

import numpy as np
import pytest

import build_table

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "hsefr_ragged.h")
NAMES = ["hsefr_ragged_capacity", "hsefr_ragged_conv2d", "hsefr_ragged_crops", "hsefr_ragged_last_error_string", "hsefr_ragged_maxpool",
         "hsefr_ragged_pyramid", "hsefr_ragged_stage1", "hsefr_ragged_stage_finish", "hsefr_ragged_version"]
SHAPES = [(588, 784), (784, 588), (480, 600), (294, 392), (90, 200), (20, 500), (12, 12)]
MINSIZE, FACTOR = 32, 0.709


# ---- the library -----------------------------------------------------------------------------------------------------------------
def test_header_library_and_binding_agree():
    from hse_facerec_tf_amd import _lib
    assert sorted(_lib.RAGGED_SIGNATURES) == NAMES
    assert "HSEFR_KNOB" not in open(os.path.join(ROOT, "hse_facerec_tf_amd", "csrc", "mtcnn_ragged.hip")).read()
    L = _lib.ragged_lib()
    # the list capacity is the shared header's constant in both libraries
    assert L.hsefr_ragged_capacity() == _lib.lib().hsefr_mtcnn_post_capacity()


def test_the_tables_have_the_headers_layout():
    """The NumPy dtypes of mtcnn_ragged.py against the structs of the header: sizes as the header's comments state them, fields in order."""
    from hse_facerec_tf_amd import mtcnn_ragged as mr
    src = open(HEADER).read()
    for name, dt in (("frame", mr.FRAME_DT), ("level", mr.LEVEL_DT), ("map", mr.MAP_DT), ("cells", mr.CELLS_DT)):
        body, size = re.search(r"typedef struct \{([^}]*)\} hsefr_ragged_%s;\s*/\* (\d+) bytes \*/" % name, src, flags=re.S).groups()
        fields = [f.strip() for decl in re.findall(r"(?:int64_t|int32_t|double)\s+([^;]+);", body) for f in decl.split(",")]
        assert fields == list(dt.names), name
        assert dt.itemsize == int(size), name
        widths = {"int64_t": 8, "double": 8, "int32_t": 4}
        at = 0
        for ctype, decl in re.findall(r"(int64_t|int32_t|double)\s+([^;]+);", body):
            for f in decl.split(","):
                assert dt.fields[f.strip()][1] == at and dt.fields[f.strip()][0].itemsize == widths[ctype], (name, f)
                at += widths[ctype]


def test_both_libraries_compile_the_shared_one_frame_bodies():
    """The bit identity rests on it: the bodies live in the two headers, and both sources include them instead of holding a copy."""
    csrc = os.path.join(ROOT, "hse_facerec_tf_amd", "csrc")
    post, px = open(os.path.join(csrc, "mtcnn_post_frame.h")).read(), open(os.path.join(csrc, "area_resize_px.h")).read()
    for body in ("stage1_level_frame", "stage1_finish_frame", "stage23_finish_frame", "nms_sorted", "sort_keys"):
        assert re.search(r"__device__[^;{]*\b%s\(" % body, post), body
    for body in ("area_level_pixel", "area_level_row", "area_crop_pixel"):
        assert re.search(r"__device__[^;{]*\b%s\(" % body, px), body
    for source, headers in (("mtcnn_post.hip", ["mtcnn_post_frame.h"]), ("area_resize.hip", ["area_resize_px.h"]),
                            ("mtcnn_ragged.hip", ["mtcnn_post_frame.h", "area_resize_px.h"])):
        src = open(os.path.join(csrc, source)).read()
        for h in headers:
            assert '#include "%s"' % h in src, (source, h)
        for body in ("stage1_level_frame", "stage1_finish_frame", "stage23_finish_frame", "area_level_pixel", "area_level_row", "area_crop_pixel"):
            assert not re.search(r"__device__[^;{]*\b%s\(" % body, src), (source, body)      # called, not defined again
    # and with the same flags, rebuilt when either header changes
    table = build_table.rows()
    assert table["ragged"]["flags"] == table["hsefr"]["flags"] and table["ragged"]["srcs"] == ["mtcnn_ragged.hip"]
    assert build_table.stale_against("ragged", "mtcnn_post_frame.h", "area_resize_px.h", "include/hsefr_ragged.h")


# ---- argument checks before any device work ------------------------------------------------------------------------------------------
@pytest.fixture()
def host():
    """A host buffer whose address stands in for every pointer: no call below reaches a launch."""
    from hse_facerec_tf_amd import _lib
    buf = ctypes.create_string_buffer(4096)
    return _lib, _lib.ragged_lib(), ctypes.cast(buf, ctypes.c_void_p).value, buf


def refused(_lib, rc, status, word):
    msg = _lib.ragged_last_error()
    assert rc == status and word in msg, (rc, msg, word)


def test_pyramid_checks_its_arguments_without_a_gpu(host):
    _lib, L, p, _ = host

    def call(frames=p, fb=100, ftab=p, nf=1, items=p, ni=1, bi=p, nb=1, levels=p, le=100, lds=0):
        return L.hsefr_ragged_pyramid(frames, fb, ftab, nf, items, ni, bi, nb, levels, le, lds, None)
    for kw in (dict(ni=0), dict(nb=0), dict(nf=0), dict(ni=0, frames=None, ftab=None, items=None, bi=None, levels=None), dict(ni=0, nb=0, nf=0)):
        assert call(**kw) == 0, kw                                                      # nothing to do: OK, no launch, whatever the pointers
    for kw in (dict(nf=-1), dict(ni=-1), dict(nb=-2), dict(fb=-1), dict(le=-5)):
        refused(_lib, call(**kw), _lib.ERR_INVALID, "negative size")
    for lds in (-1, 65537, 1 << 30):
        refused(_lib, call(lds=lds), _lib.ERR_INVALID, "LDS")
    for kw in (dict(ftab=None), dict(items=None), dict(bi=None)):
        refused(_lib, call(**kw), _lib.ERR_INVALID, "null table")
    refused(_lib, call(frames=None), _lib.ERR_INVALID, "null frame")
    refused(_lib, call(levels=None), _lib.ERR_INVALID, "null level")
    assert call(ni=0, lds=-1) != 0                                                      # a bad scalar is refused for an empty list too
    with pytest.raises(ValueError, match="null table"):
        _lib.ragged_check(call(items=None), "hsefr_ragged_pyramid")


def test_conv2d_and_maxpool_check_their_arguments_without_a_gpu(host):
    _lib, L, p, _ = host

    def conv(x=p, xp=10, w=p, bias=p, alpha=p, y=p, yp=10, maps=p, ni=1, bi=p, nb=1, c=3, cout=10, kh=3, kw=3, stride=1, pad_t=0, pad_l=0, co=2):
        return L.hsefr_ragged_conv2d(x, xp, w, bias, alpha, y, yp, maps, ni, bi, nb, c, cout, kh, kw, stride, pad_t, pad_l, co, None)
    for kw in (dict(ni=0), dict(nb=0), dict(ni=0, x=None, w=None, y=None, maps=None, bi=None)):
        assert conv(**kw) == 0, kw
    for kw in (dict(stride=2), dict(pad_t=1), dict(pad_l=1), dict(stride=3, pad_t=1, pad_l=1)):
        refused(_lib, conv(**kw), _lib.ERR_UNSUPPORTED, "not supported")
        refused(_lib, conv(ni=0, **kw), _lib.ERR_UNSUPPORTED, "not supported")        # also for an empty list
    for kw in (dict(ni=-1), dict(nb=-1), dict(xp=-1), dict(yp=-1)):
        refused(_lib, conv(**kw), _lib.ERR_INVALID, "negative size")
    for kw in (dict(c=0), dict(cout=-2), dict(kh=0), dict(kw=-1), dict(stride=0)):
        refused(_lib, conv(**kw), _lib.ERR_INVALID, "bad shape")
    for kw in (dict(co=3), dict(co=0), dict(co=4, cout=10), dict(co=2, cout=5), dict(co=8, cout=16)):
        refused(_lib, conv(**kw), _lib.ERR_INVALID, "co = ")
    for kw in (dict(maps=None), dict(bi=None)):
        refused(_lib, conv(**kw), _lib.ERR_INVALID, "null table")
    refused(_lib, conv(x=None), _lib.ERR_INVALID, "null input")
    refused(_lib, conv(w=None), _lib.ERR_INVALID, "null weight")
    refused(_lib, conv(y=None), _lib.ERR_INVALID, "null output")
    refused(_lib, conv(w=p + 4, co=4, cout=16), _lib.ERR_INVALID, "not aligned")      # a float4 weight load from a 4-byte boundary
    refused(_lib, conv(w=p + 4, co=2), _lib.ERR_INVALID, "not aligned")
    with pytest.raises(NotImplementedError, match="stride 2"):
        _lib.ragged_check(conv(stride=2), "hsefr_ragged_conv2d")

    def pool(x=p, xp=10, y=p, yp=10, maps=p, ni=1, bi=p, nb=1, c=10, k=2, stride=2):
        return L.hsefr_ragged_maxpool(x, xp, y, yp, maps, ni, bi, nb, c, k, stride, None)
    for kw in (dict(ni=0), dict(nb=0), dict(ni=0, x=None, y=None, maps=None, bi=None)):
        assert pool(**kw) == 0, kw
    for kw in (dict(ni=-1), dict(nb=-1), dict(xp=-1), dict(yp=-1)):
        refused(_lib, pool(**kw), _lib.ERR_INVALID, "negative size")
    for kw in (dict(c=0), dict(k=0), dict(stride=0), dict(k=-2), dict(stride=1 << 20)):
        refused(_lib, pool(**kw), _lib.ERR_INVALID, "bad shape")
    for kw in (dict(maps=None), dict(bi=None)):
        refused(_lib, pool(**kw), _lib.ERR_INVALID, "null table")
    refused(_lib, pool(x=None), _lib.ERR_INVALID, "null input")
    refused(_lib, pool(y=None), _lib.ERR_INVALID, "null output")


def test_the_box_logic_entries_check_their_arguments_without_a_gpu(host):
    _lib, L, p, _ = host

    def stage1(prob=p, reg=p, cells=10, ftab=p, nf=1, ctab=p, ni=1, found=p, counters=p, boxes=p, tab=p):
        return L.hsefr_ragged_stage1(prob, reg, cells, ftab, nf, ctab, ni, 0.6, found, counters, boxes, tab, None)
    assert stage1(nf=0) == 0 and stage1(nf=0, prob=None, reg=None, ftab=None, ctab=None, found=None, counters=None, boxes=None, tab=None) == 0
    for kw in (dict(nf=-1), dict(ni=-1), dict(cells=-1)):
        refused(_lib, stage1(**kw), _lib.ERR_INVALID, "negative size")
    for kw in (dict(ftab=None), dict(ctab=None)):
        refused(_lib, stage1(**kw), _lib.ERR_INVALID, "null table")
    for kw in (dict(prob=None), dict(reg=None)):
        refused(_lib, stage1(**kw), _lib.ERR_INVALID, "null map")
    for kw in (dict(found=None), dict(counters=None), dict(boxes=None), dict(tab=None)):
        refused(_lib, stage1(**kw), _lib.ERR_INVALID, "null list")

    def crops(frames=p, fb=100, ftab=p, nf=1, tables=p, offsets=p, dst=p, rows=8, n=1, size=24):
        return L.hsefr_ragged_crops(frames, fb, ftab, nf, tables, offsets, dst, rows, n, size, None)
    assert crops(n=0) == 0 and crops(nf=0) == 0 and crops(n=0, frames=None, ftab=None, tables=None, offsets=None, dst=None) == 0
    for kw in (dict(nf=-1), dict(rows=-1), dict(n=-1), dict(size=0), dict(fb=-1)):
        refused(_lib, crops(**kw), _lib.ERR_INVALID, "bad shape")
    refused(_lib, crops(nf=1 << 20, rows=1 << 12), _lib.ERR_UNSUPPORTED, "31 bits")
    refused(_lib, crops(size=1 << 16), _lib.ERR_UNSUPPORTED, "31 bits")
    for kw in (dict(ftab=None), dict(tables=None), dict(offsets=None)):
        refused(_lib, crops(**kw), _lib.ERR_INVALID, "null table")
    refused(_lib, crops(frames=None), _lib.ERR_INVALID, "null frame")
    refused(_lib, crops(dst=None), _lib.ERR_INVALID, "null crop")

    def finish(stage=2, b_in=p, offsets=p, total=1, prob=p, reg=p, pts=p, b_out=p, tab=p, points=p, counters=p, ftab=p, nf=1):
        return L.hsefr_ragged_stage_finish(stage, b_in, offsets, total, prob, reg, pts, 0.7, b_out, tab, points, counters, ftab, nf, None)
    assert finish(nf=0) == 0 and finish(stage=3, nf=0, b_in=None, offsets=None, ftab=None) == 0
    for kw in (dict(stage=1), dict(stage=4), dict(nf=-1), dict(total=-1)):
        refused(_lib, finish(**kw), _lib.ERR_INVALID, "stage_finish: stage")
    for kw in (dict(ftab=None), dict(offsets=None)):
        refused(_lib, finish(**kw), _lib.ERR_INVALID, "null table")
    for kw in (dict(b_in=None), dict(b_out=None), dict(counters=None), dict(tab=None), dict(prob=None), dict(reg=None), dict(stage=3, pts=None),
               dict(stage=3, points=None)):
        refused(_lib, finish(**kw), _lib.ERR_INVALID, "null pointer")


# ---- ragged_plan ----------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def plan():
    from hse_facerec_tf_amd import mtcnn
    return mtcnn.ragged_plan(SHAPES, MINSIZE, FACTOR)


def reference_scales(h, w):
    """MTCNNDetector.pyramid_scales, restated (facial_analysis.py:489-497)."""
    m = 12.0 / MINSIZE
    side, scales, k = min(h, w) * m, [], 0
    while side >= 12:
        scales.append(m * np.power(FACTOR, k))
        side *= FACTOR
        k += 1
    return scales


def test_plan_items_are_every_frames_levels_in_order(plan):
    from hse_facerec_tf_amd import mtcnn
    assert plan.n_frames == len(SHAPES) and plan.frames.dtype.itemsize == 24
    item, at = 0, 0
    for f, (h, w) in enumerate(SHAPES):
        scales = reference_scales(h, w)
        assert scales == mtcnn.MTCNNDetector.pyramid_scales.__get__(type("D", (), dict(minsize=MINSIZE, FACTOR=FACTOR))())(h, w)
        row = plan.frames[f]
        assert (int(row["offset"]), int(row["h"]), int(row["w"]), int(row["first_item"]), int(row["n_items"])) == (at, h, w, item, len(scales))
        at += h * w * 3                                                                  # back to back: (90, 200) starts on an odd... any byte
        for k, s in enumerate(scales):
            lv = plan.levels[item + k]
            assert (int(lv["frame"]), int(lv["dh"]), int(lv["dw"])) == (f, int(np.ceil(h * s)), int(np.ceil(w * s)))
            assert plan.scales[item + k] == s and plan.cells["scale"][item + k] == s     # the detector's floats, not recomputed ones
        item += len(scales)
    assert plan.n_items == item and plan.frames_bytes == at
    assert plan.frames["offset"].dtype == np.int64 and plan.levels["level_off"].dtype == np.int64
    # (20, 500) and (12, 12) are too small for a level: no items
    assert int(plan.frames["n_items"][5]) == 0 and int(plan.frames["n_items"][6]) == 0
    assert [int(n) for n in plan.frames["n_items"][:5]] == [9, 9, 8, 7, 4]
    # an odd frame size puts the next frame on an odd address
    odd = mtcnn.ragged_plan([(37, 53), (64, 48)], 20, FACTOR)
    assert int(odd.frames["offset"][1]) == 37 * 53 * 3 and int(odd.frames["offset"][1]) % 2 == 1


def test_plan_layers_follow_from_one_another(plan):
    from hse_facerec_tf_amd import mtcnn_ragged as mr
    d0, d1 = plan.dims[0]
    assert np.array_equal(d0, plan.levels["dw"]) and np.array_equal(d1, plan.levels["dh"])          # the nets see (W', H')
    want = [(d0, d1)]
    want.append((want[-1][0] - 2, want[-1][1] - 2))                                      # 3 x 3 VALID
    want.append((-(-want[-1][0] // 2), -(-want[-1][1] // 2)))                            # 2 x 2 / 2 SAME
    want.append((want[-1][0] - 2, want[-1][1] - 2))                                      # 3 x 3 VALID
    want.append((want[-1][0] - 2, want[-1][1] - 2))                                      # 3 x 3 VALID
    want.append(want[-1])                                                                # 1 x 1
    assert len(plan.dims) == 6 and len(plan.layers) == 5
    for g, (a, b) in enumerate(want):
        assert np.array_equal(plan.dims[g][0], a) and np.array_equal(plan.dims[g][1], b), g
        assert plan.pixels[g] == int((a * b).sum())
    assert [(l["kind"], l["k"], l["stride"], l["tpp"]) for l in plan.layers] == [("conv", 3, 1, 5), ("pool", 2, 2, 10), ("conv", 3, 1, 4),
                                                                                 ("conv", 3, 1, 8), ("conv", 1, 1, 1)]
    # a level of ceil(12 / scale) pixels (the smallest a face of minsize pixels fills) ends at 1 x 1
    ends = mr.layer_dims(np.array([12, 12, 13]), np.array([12, 40, 13]))
    assert [(int(a[0]), int(b[0])) for a, b in ends] == [(12, 12), (10, 10), (5, 5), (3, 3), (1, 1), (1, 1)]
    assert (int(ends[-1][0][1]), int(ends[-1][1][1])) == (1, 15) and (int(ends[-1][0][2]), int(ends[-1][1][2])) == (2, 2)
    assert min(int(plan.dims[-1][0].min()), int(plan.dims[-1][1].min())) >= 1
    # the stage-1 table: the last layer's maps
    assert np.array_equal(plan.cells["w"], plan.dims[-1][0]) and np.array_equal(plan.cells["h"], plan.dims[-1][1])
    assert np.array_equal(plan.cells["cell_off"], np.concatenate([[0], np.cumsum(plan.dims[-1][0] * plan.dims[-1][1])[:-1]]))


def test_plan_offsets_are_running_sums_in_int64(plan):
    lv = plan.levels
    assert np.array_equal(lv["level_off"], np.concatenate([[0], np.cumsum(lv["dh"].astype(np.int64) * lv["dw"] * 3)[:-1]]))
    for g, layer in enumerate(plan.layers):
        m = layer["maps"]
        assert m.dtype.itemsize == 40 and m["in_off"].dtype == np.int64 and m["out_off"].dtype == np.int64
        assert np.array_equal(m["ih"], plan.dims[g][0]) and np.array_equal(m["iw"], plan.dims[g][1])
        assert np.array_equal(m["oh"], plan.dims[g + 1][0]) and np.array_equal(m["ow"], plan.dims[g + 1][1])
        assert np.array_equal(m["in_off"], np.concatenate([[0], np.cumsum(plan.dims[g][0] * plan.dims[g][1])[:-1]]))
        assert np.array_equal(m["out_off"], np.concatenate([[0], np.cumsum(plan.dims[g + 1][0] * plan.dims[g + 1][1])[:-1]]))
    # a layer's output offsets are the next layer's input offsets: the buffers chain without a copy
    for a, b in zip(plan.layers, plan.layers[1:]):
        assert np.array_equal(a["maps"]["out_off"], b["maps"]["in_off"])
    # a pass whose offsets leave 32 bits: 700 frames of 2000 x 2000 pass 2^31 bytes, and their levels 2^31 floats
    from hse_facerec_tf_amd import mtcnn
    big = mtcnn.ragged_plan([(2000, 2000 + i) for i in range(700)], 20, FACTOR)
    assert int(big.frames["offset"][-1]) > 1 << 32 and int(big.levels["level_off"][-1]) > 1 << 31
    assert int(big.layers[0]["maps"]["out_off"][-1]) == int((big.dims[1][0] * big.dims[1][1])[:-1].sum())
    from hse_facerec_tf_amd.mtcnn_ragged import PNET_CHANNELS, frame_workspace_bytes
    assert big.workspace_bytes == big.frames_bytes + 4 * sum(p * c for p, c in zip(big.pixels, PNET_CHANNELS))
    assert big.workspace_bytes == sum(frame_workspace_bytes(h, w, 20, FACTOR) for h, w in big.shapes)


def check_block_map(first_block, block_item, threads):
    """Every workgroup lies inside its item's padded range, and the ranges cover every output once."""
    covered = np.zeros(len(threads), np.int64)
    assert np.all(np.diff(block_item) >= 0) and (len(block_item) == 0 or (block_item[0] == 0 and block_item[-1] == len(threads) - 1))
    for b, it in enumerate(block_item):
        local = b - int(first_block[it])
        assert 0 <= local * 256 < int(threads[it]), (b, it)                             # the workgroup holds at least one live thread
        covered[it] += min(256, int(threads[it]) - local * 256)
    assert np.array_equal(covered, threads)                                             # each output exactly once
    blocks = -(-np.asarray(threads) // 256)
    assert np.array_equal(first_block, np.concatenate([[0], np.cumsum(blocks)[:-1]])) and len(block_item) == int(blocks.sum())


def test_plan_block_maps_cover_every_output_once(plan):
    for g, layer in enumerate(plan.layers):
        m = layer["maps"]
        threads = m["oh"].astype(np.int64) * m["ow"] * layer["tpp"]
        check_block_map(m["first_block"], layer["block_item"], threads)
    lv = plan.levels
    threads = np.where(lv["rows"] != 0, lv["dh"].astype(np.int64) * 256, lv["dh"].astype(np.int64) * lv["dw"])
    check_block_map(lv["first_block"], plan.level_block_item, threads)
    # the row form is chosen as hsefr_mtcnn_pyramid_level chooses it: a decimated level whose LDS fits
    for it in range(plan.n_items):
        h, w = SHAPES[int(lv["frame"][it])]
        dh, dw = int(lv["dh"][it]), int(lv["dw"][it])
        hoff = (dw * 24 + 15) & ~15
        need = hoff + (int(h / dh) + 3) * dw * 12
        assert int(lv["rows"][it]) == int(need <= 65536) and (not lv["rows"][it] or int(lv["hoff"][it]) == hoff)
        assert not lv["rows"][it] or need <= plan.level_lds <= 65536
    # boundary cases of the map itself
    from hse_facerec_tf_amd.mtcnn_ragged import block_map
    first, item = block_map(np.array([256, 257, 1, 512]))
    assert first.tolist() == [0, 1, 3, 4] and item.tolist() == [0, 1, 1, 2, 3, 3]
    first, item = block_map(np.zeros(0, np.int64))
    assert len(first) == 0 and len(item) == 0


def test_a_plan_without_frames_or_levels_is_empty():
    from hse_facerec_tf_amd import mtcnn
    for shapes in ([], [(20, 500)], [(12, 12), (5, 7)]):
        p = mtcnn.ragged_plan(shapes, MINSIZE, FACTOR)
        assert p.n_items == 0 and p.pixels == [0] * 6 and len(p.level_block_item) == 0 and p.level_lds == 0
        assert all(len(l["block_item"]) == 0 and len(l["maps"]) == 0 for l in p.layers)
        assert p.workspace_bytes == p.frames_bytes == sum(h * w * 3 for h, w in shapes)
    with pytest.raises(ValueError, match="bad size"):
        mtcnn.ragged_plan([(0, 10)], MINSIZE, FACTOR)


# ---- plan_mixed_passes ------------------------------------------------------------------------------------------------------------------
def test_plan_mixed_passes():
    from hse_facerec_tf_amd import mtcnn
    from hse_facerec_tf_amd.mtcnn_ragged import frame_workspace_bytes
    a, b, c, d, e, small = (588, 784), (784, 588), (480, 600), (294, 392), (300, 400), (20, 500)
    shapes = [a, b, a, c, small, d, a, e]
    passes = mtcnn.plan_mixed_passes(shapes, 32)
    # the same-size group is untouched (what plan_passes gives), the lone frames are gathered in list order, the frame without a
    # level stands alone
    assert passes == [(a, [0, 2, 6]), (None, [1, 3, 5, 7]), (small, [4])]
    assert [p for p in mtcnn.plan_passes(shapes, 32) if len(p[1]) > 1] == [passes[0]]
    # max_frames bounds both kinds; the frame a same-size group leaves over is alone in its pass and joins the ragged ones
    passes = mtcnn.plan_mixed_passes(shapes, 2)
    assert passes == [(a, [0, 2]), (None, [1, 3]), (None, [5, 6]), (small, [4]), (e, [7])]
    passes = mtcnn.plan_mixed_passes(shapes, 3)
    assert passes == [(a, [0, 2, 6]), (None, [1, 3, 5]), (small, [4]), (e, [7])]          # a leftover single frame: the single-frame call
    # max_bytes: a pass closes before the frame that would exceed it
    need = {s: frame_workspace_bytes(s[0], s[1], 32, 0.709) for s in shapes}
    assert need[small] == 20 * 500 * 3 and need[b] > need[c] > need[d]
    lone = [b, c, d, e]
    passes = mtcnn.plan_mixed_passes(lone, 32, max_bytes=need[b] + need[c])
    assert passes == [(None, [0, 1]), (None, [2, 3])]
    passes = mtcnn.plan_mixed_passes(lone, 32, max_bytes=need[b] + need[c] - 1)
    assert passes == [(None, [1, 2, 3]), (b, [0])]
    passes = mtcnn.plan_mixed_passes(lone, 32, max_bytes=1)                              # a tiny limit: passes of one, single-frame calls
    assert passes == [(s, [i]) for i, s in enumerate(lone)]
    # the detector's constants decide what a frame needs
    assert frame_workspace_bytes(90, 200, 32, 0.709) < frame_workspace_bytes(90, 200, 20, 0.709)
    assert mtcnn.plan_mixed_passes([(30, 30), (40, 40)], 32, minsize=20) == [(None, [0, 1])]
    assert mtcnn.plan_mixed_passes([(30, 30), (40, 40)], 32, minsize=32) == [((40, 40), [1]), ((30, 30), [0])] or \
        mtcnn.plan_mixed_passes([(30, 30), (40, 40)], 32, minsize=32) == [((30, 30), [0]), ((40, 40), [1])]
    # every index exactly once, whatever the limits
    rng = np.random.RandomState(3)
    for trial in range(20):
        shapes = [(int(rng.choice([100, 200, 300, 17])), int(rng.choice([150, 250, 9]))) for _ in range(int(rng.randint(0, 40)))]
        mf = int(rng.randint(1, 9))
        passes = mtcnn.plan_mixed_passes(shapes, mf, max_bytes=int(rng.choice([1, 10 ** 6, 4 << 30])))
        assert sorted(i for _, idx in passes for i in idx) == list(range(len(shapes)))
        for hw, idx in passes:
            assert 1 <= len(idx) <= mf and idx == sorted(idx)
            if hw is None:
                assert len(idx) >= 2 and len({shapes[i] for i in idx}) >= 1
            else:
                assert all(shapes[i] == hw for i in idx)
    with pytest.raises(ValueError, match="max_frames"):
        mtcnn.plan_mixed_passes(shapes, 0)
    assert mtcnn.plan_mixed_passes([], 4) == []


def test_the_flag_reaches_the_detector_only_when_it_is_in_use():
    """process_images, process_album and process_video pass mixed_sizes on only when it is set: a detector or an img_processing object
    written against the signatures without it keeps working."""
    from hse_facerec_tf_amd import album
    from hse_facerec_tf_amd.facial_analysis import FacialImageProcessing
    assert FacialImageProcessing._mixed_kw(False) == {} and FacialImageProcessing._mixed_kw(True) == {"mixed_sizes": True}
    assert album.MIXED_SIZES_DEFAULT in (True, False)

    class OldDetector:
        def detect_batch(self, imgs, max_frames=32):
            return [(np.empty((0, 5)), np.empty((10, 0), np.float32)) for _ in imgs]

    class Proc:
        detector = OldDetector()
        _mixed_kw = staticmethod(FacialImageProcessing._mixed_kw)
    assert len(FacialImageProcessing.detect_faces_batch(Proc(), [np.zeros((4, 4, 3), np.uint8)] * 2)) == 2
    with pytest.raises(TypeError, match="mixed_sizes"):
        FacialImageProcessing.detect_faces_batch(Proc(), [np.zeros((4, 4, 3), np.uint8)], mixed_sizes=True)
    # unasked, the album follows the default and the detector's abilities; asked, the caller's word
    assert album._use_mixed_sizes(Proc(), None) is False
    assert album._use_mixed_sizes(Proc(), True) is True and album._use_mixed_sizes(Proc(), False) is False

    class Ragged:
        device_boxes = True

        def detect_ragged(self, frames):
            return []

    class Proc2:
        detector = Ragged()
    assert album._use_mixed_sizes(Proc2(), None) is album.MIXED_SIZES_DEFAULT
