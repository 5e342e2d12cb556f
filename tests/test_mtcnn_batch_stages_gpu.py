"""GPU suite: the batched entry points of the MTCNN cascade (hsefr_mtcnn_*_batch), one launch over several frames, against the
single-frame entry points on each frame alone -- which tests/test_mtcnn_stages_gpu.py holds to the oracle.  The frames are the
seeded cases of tests/mtcnn_stage_cases.py; a launch mixes an empty frame, a frame with exactly one candidate (the flipped-regression
branch), a frame with exactly the capacity and one above it (which overflows: its own flag, nobody else's).

Exact: every byte of every frame's found / boxes / crop table / points / counters equals what the single-frame call leaves in
buffers pre-filled the same way (NaN, a negative int32 pattern), so rows beyond a frame's count are untouched here as they are there.

One workgroup per frame on lists of a few thousand boxes: the file runs in seconds."""
import numpy as np
import pytest

from oracle import mtcnn as om

import mtcnn_stage_cases as gen
import test_mtcnn_stages_gpu as one          # the single-frame calls and their pre-filled buffers

pytestmark = pytest.mark.gpu

cap = one.cap                                # the fixture: the library's own capacity
COUNT_FILL, TAB_FILL = one.COUNT_FILL, one.TAB_FILL


class BatchBuffers:
    """found / boxes / tab / points / counters of B frames, pre-filled as test_mtcnn_stages_gpu.Buffers fills one frame's."""

    def __init__(self, cap, n_frames):
        import torch
        self.cap, self.n = cap, n_frames
        self.found = torch.full((n_frames, cap, 9), float("nan"), dtype=torch.float64, device="cuda")
        self.boxes = torch.full((n_frames, cap, 5), float("nan"), dtype=torch.float64, device="cuda")
        self.tab = torch.full((n_frames, cap, 8), TAB_FILL, dtype=torch.int32, device="cuda")
        self.points = torch.full((n_frames, cap, 10), float("nan"), dtype=torch.float32, device="cuda")
        self.counters = torch.tensor([[0, COUNT_FILL, COUNT_FILL, COUNT_FILL, 0, 0, 0, 0]] * n_frames, dtype=torch.int32, device="cuda")

    def read(self):
        return dict(found=self.found.cpu().numpy(), boxes=self.boxes.cpu().numpy(), tab=self.tab.cpu().numpy(),
                    points=self.points.cpu().numpy(), counters=self.counters.cpu().numpy())


def same_bytes(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a.view(np.uint8), b.view(np.uint8))


def compare_frames(got, singles, what):
    """got: BatchBuffers.read(); singles: one Buffers.read() per frame."""
    for b, want in enumerate(singles):
        assert list(got["counters"][b]) == list(want["counters"]), "%s frame %d: counters %s, alone %s" % (what, b, list(got["counters"][b]),
                                                                                                         list(want["counters"]))
        for k in ("found", "boxes", "tab", "points"):
            assert same_bytes(got[k][b], want[k]), one.show("%s frame %d" % (what, b), k, got[k][b], want[k])


def stack_dev(arrays, dtype):
    import torch
    return torch.from_numpy(np.ascontiguousarray(np.stack(arrays), dtype=dtype)).cuda()


def run_level_batch(buf, cs):
    from hse_facerec_tf_amd import _lib
    prob = stack_dev([np.stack([np.float32(1) - c["prob"], c["prob"]], axis=-1) for c in cs], np.float32)
    reg = stack_dev([c["reg"] for c in cs], np.float32)
    w, h = cs[0]["prob"].shape
    _lib.check(_lib.lib().hsefr_mtcnn_stage1_level_batch(prob.data_ptr(), reg.data_ptr(), len(cs), int(w), int(h), float(cs[0]["scale"]),
                                                         float(np.float32(cs[0]["thr"])), buf.found.data_ptr(), buf.counters.data_ptr(),
                                                         _lib.current_stream_ptr()), "hsefr_mtcnn_stage1_level_batch")


def run_finish_batch(buf, img_w, img_h):
    from hse_facerec_tf_amd import _lib
    _lib.check(_lib.lib().hsefr_mtcnn_stage1_finish_batch(buf.found.data_ptr(), buf.counters.data_ptr(), buf.boxes.data_ptr(), buf.tab.data_ptr(),
                                                          buf.n, int(img_w), int(img_h), _lib.current_stream_ptr()), "hsefr_mtcnn_stage1_finish_batch")


def at_scale(c, scale):
    """The case at the launch's scale: one launch has one scale, the single-frame call it is compared with takes the same."""
    c = dict(c)
    c["scale"] = float(scale)
    return c


# ---- stage 1: two levels sharing each frame's found / counters, then the finish -------------------------------------------------------
LEVEL_LABELS = ["17", "0", "1", "cap", "cap+1", "1025", "1"]            # frame order: empty and overflowing frames between full ones
SECOND_LABELS = ["1025", "17", "0", "1", "2", "17", "1023"]             # the next level of each frame, appended behind the first's rows


def expected_found(levels, cap):
    """The oracle's rows of one frame's levels under the device's capacity rule: a level with more than cap firing cells, or whose
    survivors would take the list past cap, raises the flag and appends nothing."""
    rows, flag = [np.empty((0, 9))], 0
    for c in levels:
        r = om.stage1_level(c["prob"], c["reg"], c["scale"], c["thr"]) if c["n_fire"] <= cap else None
        if r is None or sum(x.shape[0] for x in rows) + r.shape[0] > cap:
            flag = 1
        else:
            rows.append(r)
    return np.concatenate(rows, axis=0), flag


def test_stage1_levels_and_finish_of_many_frames_equal_each_frame_alone(cap):
    level = gen.by_name(gen.level_cases(cap))
    first = [at_scale(level["level/clustered/" + l], gen.PYRAMID[1]) for l in LEVEL_LABELS]
    second = [at_scale(level["level/scattered/" + l], gen.PYRAMID[3]) for l in SECOND_LABELS]
    assert [c["n_fire"] for c in first] == [17, 0, 1, cap, cap + 1, 1025, 1]
    img_w, img_h = 784, 588
    n = len(first)

    def batch(finish):
        buf = BatchBuffers(cap, n)
        run_level_batch(buf, first)
        run_level_batch(buf, second)
        if finish:
            run_finish_batch(buf, img_w, img_h)
        return buf.read()

    def alone(b, finish):
        buf = one.Buffers(cap)
        one.run_level(buf, first[b])
        one.run_level(buf, second[b])
        if finish:
            one.run_finish(buf, img_w, img_h)
        return buf.read()
    for finish in (False, True):
        got = batch(finish)
        again = batch(finish)
        for k in got:
            assert same_bytes(got[k], again[k]), "two runs of the same launches differ in %s" % k
        singles = [alone(b, finish) for b in range(n)]
        print("finish" if finish else "levels", "counters", got["counters"][:, :5].tolist())
        compare_frames(got, singles, "levels + finish" if finish else "levels")
    # what the comparison rests on, stated on the batch itself: the overflow flag is the cap + 1 frame's alone, every other frame has
    # rows from both levels in level order, the single-cell frames took the flipped regression
    flags = got["counters"][:, 4].tolist()
    assert flags == [0, 0, 0, 0, 1, 0, 0], flags
    assert got["counters"][4, 1] == 0 and one.untouched(got["boxes"][4]) and one.untouched(got["tab"][4])
    for b in range(n):
        want, flag = expected_found((first[b], second[b]), cap)
        assert flag == flags[b]
        k = want.shape[0]
        assert got["counters"][b, 0] == k and np.array_equal(got["found"][b, :k], want), one.show("frame %d" % b, "found", got["found"][b, :k], want)
        assert one.untouched(got["found"][b], k) and one.untouched(got["points"][b])
        m = int(got["counters"][b, 1])
        assert one.untouched(got["boxes"][b], m) and one.untouched(got["tab"][b], m)
    c1 = first[2]
    xi, yi = [int(v) for v in c1["cells"][0]]
    w = c1["prob"].shape[0]
    assert w - 1 - xi != xi and np.array_equal(got["found"][2, 0, 5:9], c1["reg"][w - 1 - xi, yi].astype(np.float64))


def test_stage1_finish_of_synthetic_lists_of_many_frames(cap):
    import torch
    finish = gen.by_name(gen.finish_cases(cap))
    c300 = finish["finish/clustered/300"]
    # (case, rows of it that count, overflow flag set beforehand)
    frames = [(finish["finish/clustered/cap"], cap, 0), (c300, 0, 0), (finish["finish/clustered/1"], 1, 0), (c300, 300, 1),
              (finish["finish/clustered/2"], 2, 0), (c300, 300, 0)]
    img_w, img_h = c300["img_w"], c300["img_h"]
    assert all(c["img_w"] == img_w and c["img_h"] == img_h for c, _, _ in frames)
    buf = BatchBuffers(cap, len(frames))
    singles = []
    for b, (c, n, flag) in enumerate(frames):
        rows = torch.from_numpy(c["found"]).cuda()
        buf.found[b, :rows.shape[0]] = rows
        buf.counters[b, 0] = n
        buf.counters[b, 4] = flag
        alone = one.Buffers(cap)
        alone.found[:rows.shape[0]] = rows
        alone.counters[0] = n
        alone.counters[4] = flag
        one.run_finish(alone, img_w, img_h)
        singles.append(alone.read())
    run_finish_batch(buf, img_w, img_h)
    got = buf.read()
    print("counters", got["counters"][:, :5].tolist())
    compare_frames(got, singles, "finish")
    wb, wt = om.stage1_finish(frames[0][0]["found"], img_w, img_h)
    m = wb.shape[0]
    assert got["counters"][0, 1] == m and np.array_equal(got["boxes"][0, :m], wb) and np.array_equal(got["tab"][0, :m], wt)
    assert got["counters"][:, 1].tolist()[1] == 0 and got["counters"][:, 1].tolist()[3] == 0
    for b in range(len(frames)):
        k = int(got["counters"][b, 1])
        assert one.untouched(got["boxes"][b], k) and one.untouched(got["tab"][b], k) and one.untouched(got["points"][b])


# ---- stages 2 and 3: the nets' outputs of all frames as one list, ranges by offsets ---------------------------------------------------
NET_LABELS = ["700", "0", "5", "cap+1", "1", "cap", "17"]                  # an empty range between two others; unequal lengths


@pytest.mark.parametrize("stage", [2, 3])
def test_stage_finish_of_many_frames_equals_each_frame_alone(stage, cap):
    import torch
    from hse_facerec_tf_amd import _lib
    net = gen.by_name(gen.net_cases(stage, cap))
    cs = [net["stage%d/random/%s" % (stage, l)] for l in NET_LABELS]
    counts = [c["boxes_in"].shape[0] for c in cs]
    assert counts == [700, 0, 5, cap + 1, 1, cap, 17]
    img_w, img_h = cs[0]["img_w"], cs[0]["img_h"]
    offsets = np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)
    total = int(offsets[-1])
    boxes_in = torch.full((len(cs), cap, 5), float("nan"), dtype=torch.float64, device="cuda")
    for b, c in enumerate(cs):
        rows = torch.from_numpy(c["boxes_in"][:cap]).cuda()               # (the cap + 1 frame: refused before a row is read)
        boxes_in[b, :rows.shape[0]] = rows
    prob = one.dev(np.concatenate([c["prob"] for c in cs]), np.float32)
    reg = one.dev(np.concatenate([c["reg"] for c in cs]), np.float32)
    pts = one.dev(np.concatenate([c["pts"] for c in cs]), np.float32)
    d_off = torch.from_numpy(offsets).cuda()

    def batch():
        buf = BatchBuffers(cap, len(cs))
        _lib.check(_lib.lib().hsefr_mtcnn_stage_finish_batch(stage, boxes_in.data_ptr(), d_off.data_ptr(), total, prob.data_ptr(), reg.data_ptr(),
                                                             pts.data_ptr() if stage == 3 else None, float(np.float32(cs[0]["thr"])),
                                                             buf.boxes.data_ptr(), buf.tab.data_ptr() if stage == 2 else None,
                                                             buf.points.data_ptr() if stage == 3 else None, buf.counters.data_ptr(), len(cs),
                                                             int(img_w), int(img_h), _lib.current_stream_ptr()), "hsefr_mtcnn_stage_finish_batch")
        return buf.read()
    got, again = batch(), batch()
    for k in got:
        assert same_bytes(got[k], again[k]), "two runs of the same launch differ in %s" % k
    singles = []
    for c in cs:
        alone = one.Buffers(cap)
        one.run_net(alone, c)
        singles.append(alone.read())
    print("stage", stage, "counts", counts, "kept", got["counters"][:, stage].tolist(), "flags", got["counters"][:, 4].tolist())
    compare_frames(got, singles, "stage %d" % stage)
    assert got["counters"][:, 4].tolist() == [0, 0, 0, 1, 0, 0, 0]
    kept = got["counters"][:, stage].tolist()
    assert kept[1] == 0 and kept[3] == 0 and kept[0] > 0 and kept[2] > 0 and kept[5] > 0
    for b in range(len(cs)):
        assert one.untouched(got["boxes"][b], kept[b]) and one.untouched(got["found"][b])
        assert one.untouched(got["tab"][b], kept[b] if stage == 2 else 0) and one.untouched(got["points"][b], kept[b] if stage == 3 else 0)
    # a range that is not inside the list: that frame is flagged and writes count 0, the others are what they were
    bad = offsets.copy()
    bad[3], bad[4] = total + 5, total + 9                                  # frame 2 ends, frame 3 lies, frame 4 starts beyond the list
    d_off.copy_(torch.from_numpy(bad).cuda())
    got2 = batch()
    assert got2["counters"][:, 4].tolist() == [0, 0, 1, 1, 1, 0, 0] and got2["counters"][[2, 3, 4], stage].tolist() == [0, 0, 0]
    for b in (0, 1, 5, 6):
        for k in got:
            assert same_bytes(got2[k][b], got[k][b]), (b, k)
    for b in (2, 3, 4):
        assert one.untouched(got2["boxes"][b]) and one.untouched(got2["tab"][b]) and one.untouched(got2["points"][b])


# ---- pyramid levels and crops of a stack of frames ------------------------------------------------------------------------------------
@pytest.mark.parametrize("h, w, hs, ws", [(147, 201, 56, 76),             # general decimation: the row kernel
                                          (147, 201, 147, 201),            # same size
                                          (96, 128, 48, 64), (96, 129, 32, 43),   # integer factors 2 and 3
                                          (40, 56, 90, 70)])               # enlarging
def test_pyramid_level_of_a_stack_equals_each_frame_alone(h, w, hs, ws):
    import torch
    from hse_facerec_tf_amd import _lib
    L = _lib.lib()
    frames = np.random.RandomState(h * 1000 + ws).randint(0, 256, (3, h, w, 3)).astype(np.uint8)
    stack = torch.from_numpy(frames).cuda()
    got = torch.full((3, ws, hs, 3), float("nan"), dtype=torch.float32, device="cuda")
    _lib.check(L.hsefr_mtcnn_pyramid_level_batch(stack.data_ptr(), got.data_ptr(), 3, h, w, hs, ws, _lib.current_stream_ptr()),
               "hsefr_mtcnn_pyramid_level_batch")
    for b in range(3):
        alone = torch.full((ws, hs, 3), float("nan"), dtype=torch.float32, device="cuda")
        _lib.check(L.hsefr_mtcnn_pyramid_level(stack[b].data_ptr(), alone.data_ptr(), h, w, hs, ws, _lib.current_stream_ptr()),
                   "hsefr_mtcnn_pyramid_level")
        assert not np.isnan(alone.cpu().numpy()).any()
        assert same_bytes(got[b].cpu().numpy(), alone.cpu().numpy()), (b, h, w, hs, ws)


@pytest.mark.parametrize("size", [24, 48])
def test_crops_of_a_stack_equal_each_frames_crops(size, cap):
    import torch
    from hse_facerec_tf_amd import _lib
    L = _lib.lib()
    _, img_w, img_h, corners = gen.edge_boxes()[0]                         # boxes over every edge and corner of a 200 x 150 frame
    rs = np.random.RandomState(size)
    picks = [list(range(len(corners))), [], [6, 0, 3], [7], [], [1, 2, 4, 5, 5]]          # rows per frame: unequal, two empty
    frames = rs.randint(0, 256, (len(picks), img_h, img_w, 3)).astype(np.uint8)
    tabs = [om.crop_table(corners[p], img_w, img_h) if p else np.empty((0, 8), np.int32) for p in picks]
    counts = [len(p) for p in picks]
    offsets = np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)
    total = int(offsets[-1])
    stack = torch.from_numpy(frames).cuda()
    d_tab = torch.full((len(picks), cap, 8), TAB_FILL, dtype=torch.int32, device="cuda")
    for b, t in enumerate(tabs):
        if len(t):
            d_tab[b, :len(t)] = torch.from_numpy(t).cuda()
    d_off = torch.from_numpy(offsets).cuda()
    got = torch.full((total + 2, size, size, 3), float("nan"), dtype=torch.float32, device="cuda")
    _lib.check(L.hsefr_mtcnn_crops_batch(stack.data_ptr(), d_tab.data_ptr(), d_off.data_ptr(), got.data_ptr(), len(picks), img_h, img_w, total, size,
                                         _lib.current_stream_ptr()), "hsefr_mtcnn_crops_batch")
    got = got.cpu().numpy()
    assert np.isnan(got[total:]).all() and not np.isnan(got[:total]).any()                 # the list, and nothing behind it
    for b, t in enumerate(tabs):
        if not len(t):
            continue
        alone = torch.full((len(t), size, size, 3), float("nan"), dtype=torch.float32, device="cuda")
        _lib.check(L.hsefr_mtcnn_crops(stack[b].data_ptr(), d_tab[b].data_ptr(), alone.data_ptr(), img_h, img_w, len(t), size, _lib.current_stream_ptr()),
                   "hsefr_mtcnn_crops")
        assert same_bytes(got[offsets[b]:offsets[b + 1]], alone.cpu().numpy()), (b, size)


def test_the_batched_entry_points_check_their_arguments(cap):
    import torch
    from hse_facerec_tf_amd import _lib
    L = _lib.lib()
    buf = BatchBuffers(cap, 2)
    x = torch.zeros(64, dtype=torch.float32, device="cuda")
    st = _lib.current_stream_ptr()
    p = x.data_ptr()
    assert L.hsefr_mtcnn_pyramid_level_batch(p, p, 0, 4, 4, 2, 2, st) == _lib.ERR_INVALID                       # B >= 1
    assert L.hsefr_mtcnn_pyramid_level_batch(None, p, 1, 4, 4, 2, 2, st) == _lib.ERR_INVALID
    assert L.hsefr_mtcnn_pyramid_level_batch(p, p, 1, 40000, 40000, 2, 2, st) == _lib.ERR_UNSUPPORTED            # 3 h w leaves 31 bits
    assert L.hsefr_mtcnn_stage1_level_batch(p, p, 0, 2, 2, 0.5, 0.6, buf.found.data_ptr(), buf.counters.data_ptr(), st) == _lib.ERR_INVALID
    assert L.hsefr_mtcnn_stage1_level_batch(p, p, 2, 2, 2, 0.5, 0.6, None, buf.counters.data_ptr(), st) == _lib.ERR_INVALID
    assert L.hsefr_mtcnn_stage1_level_batch(p, p, 2, 65536, 65536, 0.5, 0.6, buf.found.data_ptr(), buf.counters.data_ptr(), st) == _lib.ERR_INVALID
    assert L.hsefr_mtcnn_stage1_finish_batch(buf.found.data_ptr(), buf.counters.data_ptr(), buf.boxes.data_ptr(), buf.tab.data_ptr(), 0, 10, 10, st) \
        == _lib.ERR_INVALID
    assert L.hsefr_mtcnn_stage1_finish_batch(buf.found.data_ptr(), buf.counters.data_ptr(), buf.boxes.data_ptr(), buf.tab.data_ptr(), 2, 0, 10, st) \
        == _lib.ERR_INVALID
    assert L.hsefr_mtcnn_crops_batch(p, buf.tab.data_ptr(), buf.counters.data_ptr(), p, 0, 4, 4, 1, 24, st) == _lib.ERR_INVALID
    assert L.hsefr_mtcnn_crops_batch(p, buf.tab.data_ptr(), None, p, 2, 4, 4, 1, 24, st) == _lib.ERR_INVALID
    assert L.hsefr_mtcnn_crops_batch(p, buf.tab.data_ptr(), buf.counters.data_ptr(), p, 2, 40000, 40000, 1, 24, st) == _lib.ERR_UNSUPPORTED
    args = (buf.boxes.data_ptr(), buf.counters.data_ptr(), 0, p, p)
    assert L.hsefr_mtcnn_stage_finish_batch(2, *args, None, 0.7, buf.boxes.data_ptr(), buf.tab.data_ptr(), None, buf.counters.data_ptr(), 0, 10, 10, st) \
        == _lib.ERR_INVALID                                                                                     # B >= 1
    assert L.hsefr_mtcnn_stage_finish_batch(2, *args, None, 0.7, buf.boxes.data_ptr(), None, None, buf.counters.data_ptr(), 2, 10, 10, st) \
        == _lib.ERR_INVALID                                                                                     # stage 2 needs crop tables
    assert L.hsefr_mtcnn_stage_finish_batch(3, *args, p, 0.7, buf.boxes.data_ptr(), None, None, buf.counters.data_ptr(), 2, 10, 10, st) \
        == _lib.ERR_INVALID                                                                                     # stage 3 needs points out
    assert L.hsefr_mtcnn_stage_finish_batch(4, *args, p, 0.7, buf.boxes.data_ptr(), buf.tab.data_ptr(), buf.points.data_ptr(), buf.counters.data_ptr(), 2,
                                            10, 10, st) == _lib.ERR_INVALID
    torch.cuda.synchronize()
    got = buf.read()                                                                                            # nothing was launched
    assert one.untouched(got["found"]) and one.untouched(got["boxes"]) and one.untouched(got["tab"]) and one.untouched(got["points"])
