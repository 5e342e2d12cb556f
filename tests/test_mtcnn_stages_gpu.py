"""GPU suite: the four kernels of csrc/mtcnn_post.hip the detector runs (stage1_level, stage1_finish, stage23_finish<2>,
stage23_finish<3>), called through _lib's single-frame entries (the detector's pass launches the same kernels per frame), one stage at a time, against the
oracle's stage functions (oracle.mtcnn) on every case of tests/mtcnn_stage_cases.py at the library's own capacity.

Exact: counts, float64 boxes, int32 crop rows, float32 landmark bits.  Every call runs twice on fresh buffers (candidates are
appended with an LDS atomic: the result must not depend on arrival order).  The outputs are pre-filled (NaN, a negative int32
pattern): rows at and past the returned count, and everything when a call flags overflow, must still hold the fill.  Then the
crops hsefr_mtcnn_crops cuts from the device's own table, and the overflow fallback of the detector end to end.

Single-workgroup kernels on lists of a few thousand boxes: the file runs in seconds."""
import numpy as np
import pytest

from oracle import mtcnn as om

import mtcnn_stage_cases as gen
from conftest import TEST_IMAGE

pytestmark = pytest.mark.gpu

TAB_FILL = -7777
COUNT_FILL = 99                       # in counters[1..3]: shows that a stage wrote its count (0 included)


@pytest.fixture(scope="module")
def cap():
    from hse_facerec_tf_amd import _lib
    c = int(_lib.lib().hsefr_mtcnn_post_capacity())
    assert c >= 1025                  # the lists above the 1024-thread workgroup are part of what is tested
    return c


@pytest.fixture(scope="module")
def cases(cap):
    return dict(level=gen.by_name(gen.level_cases(cap)), sequence=gen.by_name(gen.sequence_cases(cap)), finish=gen.by_name(gen.finish_cases(cap)),
                net2=gen.by_name(gen.net_cases(2, cap)), net3=gen.by_name(gen.net_cases(3, cap)))


@pytest.fixture(scope="module")
def det():
    from hse_facerec_tf_amd.mtcnn import MTCNNDetector
    return MTCNNDetector(minsize=32)


# ---- the device side of one call -----------------------------------------------------------------------------------------------------
class Buffers:
    """found / counters / outputs of one frame, pre-filled."""

    def __init__(self, cap):
        import torch
        self.cap = cap
        self.found = torch.full((cap, 9), float("nan"), dtype=torch.float64, device="cuda")
        self.boxes = torch.full((cap, 5), float("nan"), dtype=torch.float64, device="cuda")
        self.tab = torch.full((cap, 8), TAB_FILL, dtype=torch.int32, device="cuda")
        self.points = torch.full((cap, 10), float("nan"), dtype=torch.float32, device="cuda")
        self.counters = torch.tensor([0, COUNT_FILL, COUNT_FILL, COUNT_FILL, 0, 0, 0, 0], dtype=torch.int32, device="cuda")

    def read(self):
        return dict(found=self.found.cpu().numpy(), boxes=self.boxes.cpu().numpy(), tab=self.tab.cpu().numpy(),
                    points=self.points.cpu().numpy(), counters=self.counters.cpu().numpy())


def dev(a, dtype):
    import torch
    a = np.ascontiguousarray(a, dtype=dtype)
    if a.size == 0:                   # an empty list still gets a real pointer
        return torch.zeros((1,) + a.shape[1:], dtype=torch.from_numpy(a).dtype, device="cuda")
    return torch.from_numpy(a).cuda()


def run_level(buf, c):
    from hse_facerec_tf_amd import _lib
    prob = dev(np.stack([np.float32(1) - c["prob"], c["prob"]], axis=-1), np.float32)       # [W', H', 2] as P-Net's prob1
    reg = dev(c["reg"], np.float32)
    w, h = c["prob"].shape
    _lib.check(_lib.lib().hsefr_mtcnn_stage1_level(prob.data_ptr(), reg.data_ptr(), int(w), int(h), float(c["scale"]), float(np.float32(c["thr"])),
                                                   buf.found.data_ptr(), buf.counters.data_ptr(), _lib.current_stream_ptr()), "hsefr_mtcnn_stage1_level")


def run_finish(buf, img_w, img_h):
    from hse_facerec_tf_amd import _lib
    _lib.check(_lib.lib().hsefr_mtcnn_stage1_finish(buf.found.data_ptr(), buf.counters.data_ptr(), buf.boxes.data_ptr(), buf.tab.data_ptr(),
                                                    int(img_w), int(img_h), _lib.current_stream_ptr()), "hsefr_mtcnn_stage1_finish")


def run_net(buf, c):
    from hse_facerec_tf_amd import _lib
    stage, n = c["stage"], c["boxes_in"].shape[0]
    boxes_in, prob, reg = dev(c["boxes_in"], np.float64), dev(c["prob"], np.float32), dev(c["reg"], np.float32)
    pts = dev(c["pts"], np.float32)
    _lib.check(_lib.lib().hsefr_mtcnn_stage_finish(stage, boxes_in.data_ptr(), n, prob.data_ptr(), reg.data_ptr(), pts.data_ptr() if stage == 3 else None,
                                                   float(np.float32(c["thr"])), buf.boxes.data_ptr(), buf.tab.data_ptr() if stage == 2 else None,
                                                   buf.points.data_ptr() if stage == 3 else None, buf.counters.data_ptr(), int(c["img_w"]), int(c["img_h"]),
                                                   _lib.current_stream_ptr()), "hsefr_mtcnn_stage_finish")


# ---- comparisons --------------------------------------------------------------------------------------------------------------------
def untouched(a, start=0):
    a = a[start:]
    return bool(np.all(a == TAB_FILL)) if a.dtype == np.int32 else bool(np.all(np.isnan(a)))


def same_bits(got, want):
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    return got.dtype == want.dtype == np.float32 and got.shape == want.shape and np.array_equal(got.view(np.uint32), want.view(np.uint32))


def show(name, what, got, want):
    """The arrays behind a failure, where they first differ."""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    if got.shape != want.shape:
        return "%s %s: shape %s, oracle %s" % (name, what, got.shape, want.shape)
    bad = np.argwhere(~((got == want) | (np.isnan(got) & np.isnan(want))))
    if bad.size == 0:
        return "%s %s: equal" % (name, what)
    r = int(bad[0][0])
    return "%s %s: %d of %d rows differ, first row %d\n  device %r\n  oracle %r" % (name, what, np.unique(bad[:, 0]).size, got.shape[0], r, got[r], want[r])


def check_counters(name, got, want):
    assert list(got) == list(want), "%s: counters %s, expected %s" % (name, list(got), list(want))


def twice(cap, fn):
    """fn(Buffers) on two fresh sets of buffers: both read back, equal bit for bit; returns the first."""
    outs = []
    for _ in range(2):
        buf = Buffers(cap)
        fn(buf)
        outs.append(buf.read())
    for k in outs[0]:
        assert np.array_equal(outs[0][k].view(np.uint8), outs[1][k].view(np.uint8)), "two runs of the same call differ in %s" % k
    return outs[0]


# ---- stage 1, one level --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", gen.names(gen.level_cases()))
def test_stage1_level_is_the_oracles(name, cap, cases):
    c = cases["level"][name]
    want = om.stage1_level(c["prob"], c["reg"], c["scale"], c["thr"])
    got = twice(cap, lambda buf: run_level(buf, c))
    print(name, "map", c["prob"].shape, "scale", c["scale"], "firing", c["n_fire"], "oracle rows", want.shape[0], "counters", list(got["counters"]))
    if c["n_fire"] > cap:             # overflow: the flag, and nothing else
        check_counters(name, got["counters"], [0, COUNT_FILL, COUNT_FILL, COUNT_FILL, 1, 0, 0, 0])
        assert untouched(got["found"]), name
    else:
        k = want.shape[0]
        check_counters(name, got["counters"], [k, COUNT_FILL, COUNT_FILL, COUNT_FILL, 0, 0, 0, 0])
        assert np.array_equal(got["found"][:k], want), show(name, "found", got["found"][:k], want)
        assert untouched(got["found"], k), "%s: rows past %d written" % (name, k)
    assert untouched(got["boxes"]) and untouched(got["tab"]) and untouched(got["points"]), name


# ---- stage 1, levels sharing one found / counters, then the finish ---------------------------------------------------------------
@pytest.mark.parametrize("name", gen.names(gen.sequence_cases()))
def test_level_sequence_and_finish_are_the_oracles(name, cap, cases):
    c = cases["sequence"][name]
    rows = [om.stage1_level(l["prob"], l["reg"], l["scale"], l["thr"]) for l in c["levels"]]
    at = c["overflow_at"]
    fits = rows if at is None else rows[:at]
    want_found = np.concatenate(fits, axis=0)
    n = want_found.shape[0]
    assert n <= cap and (at is None or n + rows[at].shape[0] > cap)

    def levels(buf):
        for l in c["levels"]:
            run_level(buf, l)
    got = twice(cap, levels)
    print(name, "oracle rows per level", [r.shape[0] for r in rows], "counters", list(got["counters"]))
    check_counters(name, got["counters"], [n, COUNT_FILL, COUNT_FILL, COUNT_FILL, 0 if at is None else 1, 0, 0, 0])
    assert np.array_equal(got["found"][:n], want_found), show(name, "found", got["found"][:n], want_found)     # the concatenation, in level order
    assert untouched(got["found"], n), name

    def all_of_it(buf):
        levels(buf)
        run_finish(buf, c["img_w"], c["img_h"])
    got2 = twice(cap, all_of_it)
    assert np.array_equal(got2["found"].view(np.uint8), got["found"].view(np.uint8)), "%s: the finish wrote to found" % name
    if at is not None:                # an overflowed frame: count 0, nothing written
        check_counters(name, got2["counters"], [n, 0, COUNT_FILL, COUNT_FILL, 1, 0, 0, 0])
        assert untouched(got2["boxes"]) and untouched(got2["tab"]) and untouched(got2["points"]), name
        return
    wb, wt = om.stage1_finish(want_found, c["img_w"], c["img_h"])
    m = wb.shape[0]
    check_counters(name, got2["counters"], [n, m, COUNT_FILL, COUNT_FILL, 0, 0, 0, 0])
    assert np.array_equal(got2["boxes"][:m], wb), show(name, "boxes", got2["boxes"][:m], wb)
    assert np.array_equal(got2["tab"][:m], wt), show(name, "crop rows", got2["tab"][:m], wt)
    assert untouched(got2["boxes"], m) and untouched(got2["tab"], m) and untouched(got2["points"]), name


# ---- stage-1 finish on synthetic lists ------------------------------------------------------------------------------------------------
def finish_on_device(cap, c):
    import torch
    n = c["found"].shape[0]

    def fn(buf):
        buf.found[:n] = torch.from_numpy(c["found"]).cuda()
        buf.counters[0] = n
        run_finish(buf, c["img_w"], c["img_h"])
    return twice(cap, fn)


@pytest.mark.parametrize("name", gen.names(gen.finish_cases()))
def test_stage1_finish_is_the_oracles(name, cap, cases):
    c = cases["finish"][name]
    n = c["found"].shape[0]
    wb, wt = om.stage1_finish(c["found"], c["img_w"], c["img_h"])
    m = wb.shape[0]
    got = finish_on_device(cap, c)
    print(name, "rows", n, "oracle boxes", m, "counters", list(got["counters"]))
    check_counters(name, got["counters"], [n, m, COUNT_FILL, COUNT_FILL, 0, 0, 0, 0])
    assert np.array_equal(got["boxes"][:m], wb), show(name, "boxes", got["boxes"][:m], wb)
    assert np.array_equal(got["tab"][:m], wt), show(name, "crop rows", got["tab"][:m], wt)
    assert untouched(got["boxes"], m) and untouched(got["tab"], m) and untouched(got["points"]), name
    assert np.array_equal(got["found"][:n], c["found"]) and untouched(got["found"], n), name


def test_stage1_finish_of_an_empty_or_overflowed_frame_writes_count_zero_only(cap, cases):
    import torch
    c = cases["finish"]["finish/clustered/300"]
    for n, flag in ((0, 0), (300, 1), (0, 1)):
        def fn(buf):
            buf.found[:300] = torch.from_numpy(c["found"]).cuda()
            buf.counters[0] = n
            buf.counters[4] = flag
            run_finish(buf, c["img_w"], c["img_h"])
        got = twice(cap, fn)
        check_counters("finish n=%d flag=%d" % (n, flag), got["counters"], [n, 0, COUNT_FILL, COUNT_FILL, flag, 0, 0, 0])
        assert untouched(got["boxes"]) and untouched(got["tab"]) and untouched(got["points"])
        assert np.array_equal(got["found"][:300], c["found"]) and untouched(got["found"], 300)


# ---- stages 2 and 3 --------------------------------------------------------------------------------------------------------------------
def check_net(name, cap, c):
    stage, n = c["stage"], c["boxes_in"].shape[0]
    got = twice(cap, lambda buf: run_net(buf, c))
    want_counters = [0, COUNT_FILL, COUNT_FILL, COUNT_FILL, 0, 0, 0, 0]
    if n > cap:                       # overflow: the flag and count 0, nothing else
        want_counters[4], want_counters[stage] = 1, 0
        print(name, "n", n, "counters", list(got["counters"]))
        check_counters(name, got["counters"], want_counters)
        assert untouched(got["boxes"]) and untouched(got["tab"]) and untouched(got["points"]) and untouched(got["found"]), name
        return got, None
    if stage == 2:
        wb, wt = om.stage2_finish(c["boxes_in"], c["prob"], c["reg"], c["thr"], c["img_w"], c["img_h"])
    else:
        wb, wp = om.stage3_finish(c["boxes_in"], c["prob"], c["reg"], c["pts"], c["thr"])
    m = wb.shape[0]
    want_counters[stage] = m
    print(name, "n", n, "oracle boxes", m, "counters", list(got["counters"]))
    check_counters(name, got["counters"], want_counters)
    assert np.array_equal(got["boxes"][:m], wb), show(name, "boxes", got["boxes"][:m], wb)
    assert untouched(got["boxes"], m) and untouched(got["found"]), name
    if stage == 2:
        assert np.array_equal(got["tab"][:m], wt), show(name, "crop rows", got["tab"][:m], wt)
        assert untouched(got["tab"], m) and untouched(got["points"]), name
    else:
        assert same_bits(got["points"][:m], wp), show(name, "landmarks", got["points"][:m], wp)
        assert untouched(got["points"], m) and untouched(got["tab"]), name
    return got, wb


@pytest.mark.parametrize("name", gen.names(gen.net_cases(2)))
def test_stage2_finish_is_the_oracles(name, cap, cases):
    check_net(name, cap, cases["net2"][name])


@pytest.mark.parametrize("name", gen.names(gen.net_cases(3)))
def test_stage3_finish_is_the_oracles(name, cap, cases):
    check_net(name, cap, cases["net3"][name])


# ---- crops from the table the device wrote ---------------------------------------------------------------------------------------------
def crops_from_table(img, tab, m, size):
    import torch
    from hse_facerec_tf_amd import _lib
    h, w = img.shape[:2]
    frame = torch.from_numpy(img).cuda()
    d_tab = torch.from_numpy(np.ascontiguousarray(tab[:m])).cuda()
    out = torch.empty((m, size, size, 3), dtype=torch.float32, device="cuda")
    _lib.check(_lib.lib().hsefr_mtcnn_crops(frame.data_ptr(), d_tab.data_ptr(), out.data_ptr(), h, w, m, size, _lib.current_stream_ptr()), "hsefr_mtcnn_crops")
    return out.cpu().numpy()


def host_crops(det, img, boxes, size):
    det.device_resize = False         # MTCNNDetector._crops' NumPy path: pad() + INTER_AREA per box
    try:
        return det._crops(img, np.asarray(boxes, np.float64), size).cpu().numpy()
    finally:
        det.device_resize = True


def test_crops_cut_from_the_device_table_match_the_host_crops_of_the_oracle_boxes(det, cap, cases):
    """The bound is test_device_crops_match_the_host_restatement's: float64 box sums in another order, round-off of the final float32."""
    clips = {1: set(), 2: set()}
    todo = [(1, c, 24) for c in cases["finish"].values() if c["crops"]] + [(2, c, 48) for c in cases["net2"].values() if c["crops"]]
    assert len(todo) >= 8
    for stage, c, size in todo:
        img = np.random.RandomState(c["img_w"] * 1000 + c["img_h"]).randint(0, 256, (c["img_h"], c["img_w"], 3)).astype(np.uint8)
        if stage == 1:
            got = finish_on_device(cap, c)
            wb, wt = om.stage1_finish(c["found"], c["img_w"], c["img_h"])
        else:
            got = twice(cap, lambda buf: run_net(buf, c))
            wb, wt = om.stage2_finish(c["boxes_in"], c["prob"], c["reg"], c["thr"], c["img_w"], c["img_h"])
        m = wb.shape[0]
        assert m > 0 and int(got["counters"][stage]) == m, c["name"]
        assert np.array_equal(got["tab"][:m], wt), show(c["name"], "crop rows", got["tab"][:m], wt)      # only a right table is handed on
        clips[stage] |= set(gen.clip_sides(wb, c["img_w"], c["img_h"]))
        a = crops_from_table(img, got["tab"], m, size)
        b = host_crops(det, img, wb, size)
        err = float(np.abs(a - b).max())
        print(c["name"], "boxes", m, "size", size, "max crop difference %.3e" % err)
        assert a.shape == b.shape == (m, size, size, 3) and err < 2e-6, (c["name"], err)
    for stage in (1, 2):
        assert set(gen.REQUIRED_CLIPS) <= clips[stage], (stage, set(gen.REQUIRED_CLIPS) - clips[stage])


# ---- the overflow fallback, end to end ----------------------------------------------------------------------------------------------
def flood_pnet(det, shape, cap):
    """Wrap det.pnet (as an instance attribute) so that a compact block of more than cap cells of the face map of the given
    shape fires: that level overflows its device list.  Deterministic in the map's shape, so every pass over the frame sees it."""
    inner = det.pnet
    bx = 48
    by = cap // bx + 1
    assert bx * by > cap and shape[1] >= bx + 10 and shape[2] >= by + 10

    def pnet(x):
        reg_t, prob_t = inner(x)
        if tuple(prob_t.shape) == tuple(shape):
            prob_t = prob_t.clone()
            prob_t[0, 5:5 + bx, 5:5 + by, 1] = 0.99
            prob_t[0, 5:5 + bx, 5:5 + by, 0] = 0.01
        return [reg_t, prob_t]
    det.pnet = pnet


def test_an_overflowed_frame_is_redone_on_the_host_and_leaves_the_detector_sound(cap):
    from hse_facerec_tf_amd import preprocess
    from hse_facerec_tf_amd.mtcnn import MTCNNDetector
    img = preprocess.imread_rgb(TEST_IMAGE)
    h, w = img.shape[:2]
    device, host = MTCNNDetector(minsize=32), MTCNNDetector(minsize=32, device_boxes=False)
    assert device.device_boxes and not host.device_boxes
    want_boxes, want_points = MTCNNDetector(minsize=32)(img)              # a fresh detector, nothing wrapped
    assert want_boxes.shape[0] >= 4
    scale = device.pyramid_scales(h, w)[0]
    import torch
    frame = torch.from_numpy(np.ascontiguousarray(img)).cuda()
    shape0 = tuple(device.pnet(device._level_device(frame, h, w, int(np.ceil(h * scale)), int(np.ceil(w * scale))))[1].shape)
    for d in (device, host):
        flood_pnet(d, shape0, cap)
    bd, pd = device(img)
    bh, ph = host(img)
    print("flooded level", shape0, "boxes", bd.shape, "fallbacks", device.host_fallbacks, host.host_fallbacks)
    assert device.host_fallbacks == 1 and host.host_fallbacks == 0
    assert bd.shape == bh.shape and bd.shape[0] > 0 and np.array_equal(bd, bh)
    assert pd.shape == ph.shape == (10, bd.shape[0]) and np.array_equal(pd, ph)
    del device.pnet                                                        # the class's own method again
    b2, p2 = device(img)
    assert device.host_fallbacks == 1
    assert np.array_equal(b2, want_boxes) and np.array_equal(p2, want_points)
