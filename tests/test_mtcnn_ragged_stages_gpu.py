"""GPU suite: what tests/test_mtcnn_ragged_gpu.py leaves open in libhsefr_ragged.so (csrc/mtcnn_ragged.hip), step by step and EXACT (every
comparison is on bytes; no tolerance anywhere):

  * hsefr_ragged_stage_finish, stages 2 and 3, on seven frames of seven sizes (mtcnn_stage_cases.ragged_net_cases) against the
    single-frame entry on each frame alone with its own size -- which the same run holds to the oracle -- and, on frames of one size,
    against hsefr_mtcnn_stage_finish_batch; ranges that leave the list;
  * hsefr_ragged_crops on frames of three sizes packed back to back (odd addresses, empty frames first, in the middle and last,
    a grid that ends inside a workgroup) against hsefr_mtcnn_crops on each frame alone, its four guards, and a frame beyond 2^31 bytes;
  * the table guards of the pyramid, the convolution, the pooling and stage 1;
  * the convolution's three input-load widths on inputs 0, 4 and 8 bytes past 16-byte alignment.

The rule of every guard case: the entry point is told sizes SMALLER than what the test allocated (pixels in front of and behind the
packed buffers, a table row in front of and behind the tables, a whole frame with its items behind the declared lists), and ONE item
in the middle of the list is corrupted so that whatever the corrupted entry points at is still allocated and holds finite data.  A
guard that is missing or off by one then shows as a value that was written or changed -- never as a fault.  Expected: status OK, the
corrupted item's outputs still hold their NaN fill, every other byte equals the uncorrupted run's.

Lists of at most cap + 1 rows, frames of at most 784 x 588, one 2.2 GB allocation that is not filled: the file runs in seconds."""
import numpy as np
import pytest

from oracle import mtcnn as om

import mtcnn_stage_cases as gen
import test_mtcnn_batch_stages_gpu as bt     # BatchBuffers, compare_frames, same_bytes
import test_mtcnn_ragged_gpu as rg           # ragged_conv, ragged_pool, ragged_levels, the stage-1 runs, upload, bits
import test_mtcnn_stages_gpu as one          # the single-frame calls, their pre-filled buffers and the oracle comparison

pytestmark = pytest.mark.gpu

cap = one.cap                                # the fixture: the library's own capacity
TAB_FILL = one.TAB_FILL


def frame_table(sizes, offsets=None):
    """hsefr_ragged_frame rows for frames of (w, h): offset, h, w, and no items (the box logic and the crops do not read them)."""
    from hse_facerec_tf_amd.mtcnn_ragged import FRAME_DT
    t = np.zeros(len(sizes), FRAME_DT)
    for b, (w, h) in enumerate(sizes):
        t[b] = (0 if offsets is None else int(offsets[b]), h, w, 0, 0)
    return t


# ---- hsefr_ragged_stage_finish ---------------------------------------------------------------------------------------------------------
class FinishInputs:
    """The nets' outputs of all frames as one list, with more than cap rows of slack behind it: a range that leaves the list still
    points at allocated rows (copies of the list's first rows, so a kernel that followed it would find boxes that pass)."""

    def __init__(self, cs, cap):
        import torch
        self.cs, self.cap = cs, cap
        self.counts = [c["boxes_in"].shape[0] for c in cs]
        self.offsets = np.concatenate([[0], np.cumsum(self.counts)]).astype(np.int32)
        self.total = int(self.offsets[-1])
        slack = cap + 16
        assert self.total >= slack
        self.boxes_in = torch.full((len(cs), cap, 5), float("nan"), dtype=torch.float64, device="cuda")
        for b, c in enumerate(cs):
            rows = torch.from_numpy(c["boxes_in"][:cap]).cuda()            # (the cap + 1 frame: refused before a row is read)
            self.boxes_in[b, :rows.shape[0]] = rows

        def packed(key):
            a = np.concatenate([c[key] for c in cs])
            return one.dev(np.concatenate([a, a[:slack]]), np.float32)
        self.prob, self.reg, self.pts = packed("prob"), packed("reg"), packed("pts")
        assert self.prob.shape[0] == self.total + slack

    def ragged(self, stage, offsets, table):
        from hse_facerec_tf_amd import _lib
        n = len(self.cs)
        d_off, d_tab = rg.upload(np.asarray(offsets, np.int32)), rg.upload(table)
        buf = bt.BatchBuffers(self.cap, n)
        _lib.ragged_check(_lib.ragged_lib().hsefr_ragged_stage_finish(
            stage, self.boxes_in.data_ptr(), d_off.data_ptr(), self.total, self.prob.data_ptr(), self.reg.data_ptr(),
            self.pts.data_ptr() if stage == 3 else None, float(np.float32(self.cs[0]["thr"])), buf.boxes.data_ptr(),
            buf.tab.data_ptr() if stage == 2 else None, buf.points.data_ptr() if stage == 3 else None, buf.counters.data_ptr(), d_tab.data_ptr(), n,
            _lib.current_stream_ptr()), "hsefr_ragged_stage_finish")
        return buf.read()

    def same_size(self, stage, offsets, img_w, img_h):
        from hse_facerec_tf_amd import _lib
        n = len(self.cs)
        d_off = rg.upload(np.asarray(offsets, np.int32))
        buf = bt.BatchBuffers(self.cap, n)
        _lib.check(_lib.lib().hsefr_mtcnn_stage_finish_batch(
            stage, self.boxes_in.data_ptr(), d_off.data_ptr(), self.total, self.prob.data_ptr(), self.reg.data_ptr(),
            self.pts.data_ptr() if stage == 3 else None, float(np.float32(self.cs[0]["thr"])), buf.boxes.data_ptr(),
            buf.tab.data_ptr() if stage == 2 else None, buf.points.data_ptr() if stage == 3 else None, buf.counters.data_ptr(), n, int(img_w),
            int(img_h), _lib.current_stream_ptr()), "hsefr_mtcnn_stage_finish_batch")
        return buf.read()


def assert_same_read(a, b, what):
    for k in a:
        assert bt.same_bytes(a[k], b[k]), "%s: %s differs" % (what, k)


def assert_refused(got, b, stage):
    """A frame whose range is not inside the list: flagged, count 0, nothing else."""
    want = [0, one.COUNT_FILL, one.COUNT_FILL, one.COUNT_FILL, 1, 0, 0, 0]
    want[stage] = 0
    assert list(got["counters"][b]) == want, (b, list(got["counters"][b]))
    assert one.untouched(got["boxes"][b]) and one.untouched(got["tab"][b]) and one.untouched(got["points"][b]) and one.untouched(got["found"][b]), b


@pytest.mark.parametrize("stage", [2, 3])
def test_ragged_stage_finish_equals_each_frame_alone_with_its_own_size(stage, cap):
    """ragged_stage23_kernel takes img_w, img_h from its frame's row of the frame table.  Stage 2 clips its crop table against them, and
    tests/test_mtcnn_ragged_stages_cpu.py shows from the oracle that on these lists another frame's size gives another table."""
    cs = gen.ragged_net_cases(stage, cap)
    sizes = [(c["img_w"], c["img_h"]) for c in cs]
    assert sizes == gen.RAGGED_SIZES and len(set(sizes)) == 7
    inp = FinishInputs(cs, cap)
    assert inp.counts == [700, 0, 5, cap + 1, 1, cap, 17]
    table = frame_table(sizes)
    got, again = inp.ragged(stage, inp.offsets, table), inp.ragged(stage, inp.offsets, table)
    assert_same_read(got, again, "two runs of the same launch")
    # every frame alone with its own size -- and that call against the oracle, which closes the chain at the new sizes
    singles = [one.check_net(c["name"], cap, c)[0] for c in cs]
    print("stage", stage, "counts", inp.counts, "kept", got["counters"][:, stage].tolist(), "flags", got["counters"][:, 4].tolist())
    bt.compare_frames(got, singles, "ragged stage %d" % stage)
    assert got["counters"][:, 4].tolist() == [0, 0, 0, 1, 0, 0, 0]
    kept = got["counters"][:, stage].tolist()
    assert kept[1] == 0 and kept[3] == 0 and kept[0] > 0 and kept[2] > 0 and kept[5] > 0 and kept[6] > 0
    for b in range(len(cs)):
        assert one.untouched(got["boxes"][b], kept[b]) and one.untouched(got["found"][b])
        assert one.untouched(got["tab"][b], kept[b] if stage == 2 else 0) and one.untouched(got["points"][b], kept[b] if stage == 3 else 0)
    # ranges that are not inside the list: those frames are flagged and write count 0, the others are what they were.  The slack
    # behind the list keeps every row such a range names inside allocated memory
    bad = inp.offsets.copy()
    bad[3], bad[4] = inp.total + 5, inp.total + 9                          # frame 2 ends, frame 3 lies, frame 4 starts beyond the list
    got2 = inp.ragged(stage, bad, table)
    for b in (2, 3, 4):
        assert_refused(got2, b, stage)
    for b in (0, 1, 5, 6):
        for k in got:
            assert bt.same_bytes(got2[k][b], got[k][b]), (b, k)
    bad = inp.offsets.copy()
    bad[7] = bad[6] - 3                                                    # lo > hi: the last frame ends before it starts
    got3 = inp.ragged(stage, bad, table)
    assert_refused(got3, 6, stage)
    for b in range(6):
        for k in got:
            assert bt.same_bytes(got3[k][b], got[k][b]), (b, k)


@pytest.mark.parametrize("stage", [2, 3])
def test_ragged_stage_finish_on_frames_of_one_size_equals_the_same_size_entry(stage, cap):
    net = gen.by_name(gen.net_cases(stage, cap))
    cs = [net["stage%d/random/%s" % (stage, l)] for l in bt.NET_LABELS]
    inp = FinishInputs(cs, cap)
    assert inp.counts == [700, 0, 5, cap + 1, 1, cap, 17] and all((c["img_w"], c["img_h"]) == (320, 240) for c in cs)
    table = frame_table([(320, 240)] * len(cs))
    got, want = inp.ragged(stage, inp.offsets, table), inp.same_size(stage, inp.offsets, 320, 240)
    assert want["counters"][:, 4].tolist() == [0, 0, 0, 1, 0, 0, 0] and want["counters"][0, stage] > 0
    assert_same_read(got, want, "ragged against same-size, stage %d" % stage)
    bad = inp.offsets.copy()
    bad[3], bad[4] = inp.total + 5, inp.total + 9
    assert_same_read(inp.ragged(stage, bad, table), inp.same_size(stage, bad, 320, 240), "bad ranges, stage %d" % stage)


# ---- hsefr_ragged_crops ------------------------------------------------------------------------------------------------------------------
CROP_SIZES = [0, 1, 2, 1, 0, 2]                                            # which of gen.ragged_edge_frames() each of the six frames is
CROP_PICKS = [[], list(range(8)), [6, 0, 3], [], [1, 2, 4, 5, 5, 7], []]   # rows per frame: unequal; empty first, in the middle, last


class CropFrames:
    """Six frames of three sizes back to back in one uint8 buffer, their crop tables from the oracle, and every frame's crops from
    hsefr_mtcnn_crops on that frame alone (computed once per size)."""

    def __init__(self, cap):
        import torch
        self.cap = cap
        kinds = gen.ragged_edge_frames()
        rs = np.random.RandomState(48)
        self.sizes = [(kinds[i][1], kinds[i][2]) for i in CROP_SIZES]
        self.frames = [rs.randint(0, 256, (h, w, 3)).astype(np.uint8) for w, h in self.sizes]
        self.tabs = [om.crop_table(kinds[i][3][p], kinds[i][1], kinds[i][2]) if p else np.empty((0, 8), np.int32) for i, p in zip(CROP_SIZES, CROP_PICKS)]
        self.counts = [len(p) for p in CROP_PICKS]
        self.offsets = np.concatenate([[0], np.cumsum(self.counts)]).astype(np.int32)
        self.total = int(self.offsets[-1])
        nbytes = [f.size for f in self.frames]
        self.at = np.concatenate([[0], np.cumsum(nbytes)]).astype(np.int64)            # byte offset of every frame, and the end
        self.packed = torch.from_numpy(np.concatenate([f.reshape(-1) for f in self.frames])).cuda()
        self.table = frame_table(self.sizes, self.at)

    def tables(self, rows=None):
        """[B, cap, 8] filled with TAB_FILL, the frames' rows at stride ``rows`` (default cap; a frame's rows beyond it are left out)."""
        buf = np.full((len(self.tabs), self.cap, 8), TAB_FILL, np.int32)
        rows = self.cap if rows is None else rows
        view = buf.reshape(-1)[:len(self.tabs) * rows * 8].reshape(len(self.tabs), rows, 8)
        for b, t in enumerate(self.tabs):
            view[b, :min(len(t), rows)] = t[:rows]
        return buf

    def alone(self, size):
        """-> [total, size, size, 3]: hsefr_mtcnn_crops on each frame alone with its own table, in list order."""
        out = np.concatenate([one.crops_from_table(f, t, len(t), size) for f, t in zip(self.frames, self.tabs) if len(t)])
        assert out.shape[0] == self.total and not np.isnan(out).any()
        return out

    def ragged(self, size, table=None, tables=None, offsets=None, rows=None, frames_bytes=None, n=None):
        """hsefr_ragged_crops with one thing changed -> [total + 2, size, size, 3], NaN where nothing was written."""
        import torch
        from hse_facerec_tf_amd import _lib
        d_ftab = rg.upload(self.table if table is None else table)
        d_tab = rg.upload(self.tables() if tables is None else tables)
        d_off = rg.upload(self.offsets if offsets is None else np.asarray(offsets, np.int32))
        out = torch.full((self.total + 2, size, size, 3), float("nan"), dtype=torch.float32, device="cuda")
        n = self.total if n is None else n
        assert n <= self.total + 2
        rc = _lib.ragged_lib().hsefr_ragged_crops(self.packed.data_ptr(), int(self.at[-1]) if frames_bytes is None else int(frames_bytes), d_ftab.data_ptr(),
                                                  len(self.frames), d_tab.data_ptr(), d_off.data_ptr(), out.data_ptr(), self.cap if rows is None else rows, n,
                                                  size, _lib.current_stream_ptr())
        assert rc == 0, _lib.ragged_last_error()
        return out.cpu().numpy()


def assert_crops(got, want, skipped, what):
    """got [total + 2, ...] against the single-frame crops: the crops in ``skipped`` and the two behind the list still NaN, every other
    crop's bytes equal."""
    total = want.shape[0]
    for k in range(total):
        if k in skipped:
            assert np.isnan(got[k]).all(), "%s: crop %d was written" % (what, k)
        else:
            assert bt.same_bytes(got[k], want[k]), "%s: crop %d differs" % (what, k)
    assert np.isnan(got[total:]).all(), "%s: written behind the list" % what


@pytest.mark.parametrize("size", [24, 48])
def test_ragged_crops_equal_each_frames_crops_and_the_guards_skip_only_their_frame(size, cap):
    cf = CropFrames(cap)
    assert len(set(cf.sizes)) >= 3 and any(int(a) % 2 == 1 for a in cf.at[:-1])        # three sizes; a frame on an odd address
    assert cf.counts[0] == 0 and cf.counts[3] == 0 and cf.counts[-1] == 0 and cf.counts[1] != cf.counts[2] != cf.counts[4]
    assert cf.total % 2 == 1
    if size == 24:                   # 576 threads a crop: the grid ends inside a workgroup (48 * 48 is a multiple of 256: no total does it there)
        assert cf.total * size * size % 256 != 0
    want = cf.alone(size)
    got = cf.ragged(size)
    assert_crops(got, want, (), "crops")
    assert bt.same_bytes(got, cf.ragged(size))                                          # two runs
    lo, hi = cf.offsets[:-1], cf.offsets[1:]
    # frames_bytes one byte short of the last non-empty frame's end (the buffer itself is as long as before)
    assert_crops(cf.ragged(size, frames_bytes=cf.at[5] - 1), want, set(range(lo[4], hi[4])), "frames_bytes one short")
    assert_crops(cf.ragged(size, frames_bytes=cf.at[5]), want, (), "frames_bytes at the frame's end")      # (frame 5 has no crop to lose)
    # a frame without rows
    table = cf.table.copy()
    table["h"][2] = 0
    assert_crops(cf.ragged(size, table=table), want, set(range(lo[2], hi[2])), "h = 0")
    # a table stride below one frame's count: that frame's crops from index `rows` on are not in the table
    rows = 7
    assert [c > rows for c in cf.counts] == [False, True, False, False, False, False]
    assert_crops(cf.ragged(size, tables=cf.tables(rows), rows=rows), want, {lo[1] + 7}, "rows = 7")
    # offsets[b + 1] < offsets[b].  The search gives every k between offsets[0] and offsets[B] a frame whose range holds it, so a gap
    # -- crops no frame owns -- exists at the list's ends only: here the last frame ends at 14 and the launch covers 19 crops, of which
    # 17 and 18 lie at or past the last frame's start and past its end
    bad = cf.offsets.copy()
    bad[6] = 14
    assert bad[6] < bad[5] == cf.total
    assert_crops(cf.ragged(size, offsets=bad, n=cf.total + 2), want, (), "offsets[6] < offsets[5]")
    bad = cf.offsets.copy()
    bad[0] = 3                                                                          # and at the front: frame 0 = [3, 0)
    assert_crops(cf.ragged(size, offsets=bad), want, (), "offsets[1] < offsets[0]")


def test_ragged_crops_of_a_frame_past_two_to_the_31(cap):
    """The frame offset is 64-bit: a 2.2 GB frame buffer that is allocated but not filled, the second frame's bytes 2.16e9 bytes in (on
    an odd address).  Only the two small frames hold data."""
    import torch
    from hse_facerec_tf_amd import _lib
    kinds = gen.ragged_edge_frames()
    rs = np.random.RandomState(31)
    total_bytes, far = 2_200_000_000, 2_160_000_001
    metas = [kinds[0], kinds[1]]
    frames = [rs.randint(0, 256, (h, w, 3)).astype(np.uint8) for _, w, h, _ in metas]
    assert far > 2 ** 31 and far % 2 == 1 and far + frames[1].size <= total_bytes
    buffer = torch.empty(total_bytes, dtype=torch.uint8, device="cuda")
    buffer[:frames[0].size].copy_(torch.from_numpy(frames[0].reshape(-1)))
    buffer[far:far + frames[1].size].copy_(torch.from_numpy(frames[1].reshape(-1)))
    table = frame_table([(w, h) for _, w, h, _ in metas], [0, far])
    tabs = [om.crop_table(c[[0, 3, 5]], w, h) for _, w, h, c in metas[:1]] + [om.crop_table(metas[1][3], metas[1][1], metas[1][2])]
    offsets = np.asarray([0, 3, 11], np.int32)
    d_tabs = np.full((2, cap, 8), TAB_FILL, np.int32)
    for b, t in enumerate(tabs):
        d_tabs[b, :len(t)] = t
    d_ftab, d_tab, d_off = rg.upload(table), rg.upload(d_tabs), rg.upload(offsets)
    for size in (24, 48):
        out = torch.full((13, size, size, 3), float("nan"), dtype=torch.float32, device="cuda")
        _lib.ragged_check(_lib.ragged_lib().hsefr_ragged_crops(buffer.data_ptr(), total_bytes, d_ftab.data_ptr(), 2, d_tab.data_ptr(), d_off.data_ptr(),
                                                               out.data_ptr(), cap, 11, size, _lib.current_stream_ptr()), "hsefr_ragged_crops")
        got = out.cpu().numpy()
        assert np.isnan(got[11:]).all()
        for b, (f, t) in enumerate(zip(frames, tabs)):
            alone = one.crops_from_table(f, t, len(t), size)
            assert not np.isnan(alone).any() and bt.same_bytes(got[offsets[b]:offsets[b + 1]], alone), (size, b)


# ---- the table guards of the convolution and the pooling ---------------------------------------------------------------------------------
def blocks_of(block_item, m):
    return int(np.count_nonzero(block_item == m))


def map_corruptions(kind, k, m):
    """name -> tweak(maps, block_item, x_pixels, y_pixels) on item m: one case per clause of the kernels' guards.  Each leaves what it
    points at inside the allocated slack."""
    def px(maps):
        return int(maps["ih"][m]) * int(maps["iw"][m]), int(maps["oh"][m]) * int(maps["ow"][m])

    def in_off_negative(maps, bi, xp, yp):
        maps["in_off"][m] = -1

    def in_end_one_past(maps, bi, xp, yp):
        maps["in_off"][m] = xp + 1 - px(maps)[0]

    def out_end_one_past(maps, bi, xp, yp):
        maps["out_off"][m] = yp + 1 - px(maps)[1]

    def no_rows(maps, bi, xp, yp):
        maps["ih"][m] = 0

    def oh_one_more(maps, bi, xp, yp):
        maps["oh"][m] = int(maps["ih"][m]) - k + 2 if kind == "conv" else -(-int(maps["ih"][m]) // 2) + 1

    def oh_one_less(maps, bi, xp, yp):
        maps["oh"][m] = -(-int(maps["ih"][m]) // 2) - 1

    def first_block_past_the_item(maps, bi, xp, yp):
        maps["first_block"][m] += blocks_of(bi, m)

    def block_item_minus_one(maps, bi, xp, yp):
        bi[bi == m] = -1

    def block_item_n_items(maps, bi, xp, yp):
        bi[bi == m] = len(maps)
    out = [in_off_negative, in_end_one_past, out_end_one_past, no_rows, oh_one_more, first_block_past_the_item, block_item_minus_one,
           block_item_n_items]
    if kind == "pool":
        out.append(oh_one_less)
    return out


def check_map_guards(kind, run, ch, k, m):
    """run(tweak) -> (items, y).  The uncorrupted run, then every corruption of item m against it."""
    import torch
    seen = {}

    def look(maps, bi, xp, yp):
        seen.update(maps=maps.copy(), bi=bi.copy(), xp=xp, yp=yp)
    _, good = run(look)
    maps, xp, yp = seen["maps"], seen["xp"], seen["yp"]
    assert 0 < m < len(maps) - 1 and blocks_of(seen["bi"], m) >= 2                       # in the middle, more than one workgroup
    # the boundary itself is computed: the last item ends exactly at the declared sizes, and everything declared is written
    assert int(maps["in_off"][-1]) + int(maps["ih"][-1]) * int(maps["iw"][-1]) == xp
    assert int(maps["out_off"][-1]) + int(maps["oh"][-1]) * int(maps["ow"][-1]) == yp
    assert good.numel() > yp * ch and not torch.isnan(good[:yp * ch]).any() and torch.isnan(good[yp * ch:]).all()
    lo = int(maps["out_off"][m]) * ch
    hi = lo + int(maps["oh"][m]) * int(maps["ow"][m]) * ch
    good_bits = rg.bits(good)
    for tweak in map_corruptions(kind, k, m):
        _, y = run(tweak)
        got = rg.bits(y)
        assert torch.isnan(y[lo:hi]).all(), "%s %s: the corrupted item was written" % (kind, tweak.__name__)
        assert np.array_equal(got[:lo], good_bits[:lo]) and np.array_equal(got[hi:], good_bits[hi:]), "%s %s: another item changed" % (kind, tweak.__name__)

    # a first workgroup ONE too large moves the item's later workgroups one down: each computes the pixels of the one before it, at
    # their place, so what is written is right and the item's last workgroup's pixels are not written
    def first_block_one_more(maps, bi, xp, yp):
        maps["first_block"][m] += 1
    _, y = run(first_block_one_more)
    got = rg.bits(y)
    assert np.array_equal(got[:lo], good_bits[:lo]) and np.array_equal(got[hi:], good_bits[hi:])
    unwritten = torch.isnan(y[lo:hi]).cpu().numpy()
    assert unwritten.any() and not unwritten.all() and np.array_equal(got[lo:hi][~unwritten], good_bits[lo:hi][~unwritten])


def test_conv_guards_skip_the_corrupted_item_and_nothing_else():
    import torch
    c, cout, k, co = 16, 32, 3, 4
    rs = np.random.RandomState(41)
    w = torch.from_numpy(rs.normal(0, 0.3, (k, k, c, cout)).astype(np.float32)).cuda()
    bias = torch.from_numpy(rs.normal(0, 0.5, cout).astype(np.float32)).cuda()
    alpha = torch.from_numpy(rs.uniform(0.05, 0.9, cout).astype(np.float32)).cuda()
    items = [torch.from_numpy(rs.normal(0, 1, (a, b, c)).astype(np.float32)).cuda() for a, b in rg.item_sizes(k, cout // co)]
    # two pixels in front of the packed input (in_off = -1 stays inside), four behind both buffers
    check_map_guards("conv", lambda tweak: rg.ragged_conv(items, w, bias, alpha, co, base=2 * c, tweak=tweak, slack=4), cout, k, 3)


def test_maxpool_guards_skip_the_corrupted_item_and_nothing_else():
    import torch
    c = 10
    rs = np.random.RandomState(42)
    sizes = [(1, 1), (3, 3), (10, 10), (7, 10), (32, 32), (1, 2 * rg.past_a_boundary(c) - 1), (9, 4)]
    items = [torch.from_numpy(rs.normal(0, 1, (a, b, c)).astype(np.float32)).cuda() for a, b in sizes]
    check_map_guards("pool", lambda tweak: rg.ragged_pool(items, c, tweak=tweak, slack=4, base=2 * c), c, 2, 4)


# ---- the table guards of the pyramid ----------------------------------------------------------------------------------------------------
PYRAMID_SHAPES = [(37, 53), (64, 48), (120, 100), (53, 37), (64, 48)]       # the last frame and its items lie BEHIND the declared lists


def test_pyramid_guards_skip_the_corrupted_item_and_nothing_else():
    import torch
    from hse_facerec_tf_amd import mtcnn
    rs = np.random.RandomState(43)
    frames = [rs.randint(0, 256, (h, w, 3)).astype(np.uint8) for h, w in PYRAMID_SHAPES]

    def make():
        return mtcnn.ragged_plan(PYRAMID_SHAPES, 12, rg.FACTOR)
    plan = make()
    n_frames = len(PYRAMID_SHAPES) - 1
    n_items = int(plan.frames["first_item"][n_frames])
    declared = dict(n_frames=n_frames, n_items=n_items, n_blocks=int(plan.levels["first_block"][n_items]),
                    levels_elems=int(plan.levels["level_off"][n_items]))
    assert n_items < plan.n_items and declared["levels_elems"] < plan.pixels[0] * 3 and declared["n_blocks"] < len(plan.level_block_item)
    elems = declared["levels_elems"]
    good = rg.ragged_levels(frames, plan, **declared)
    assert not torch.isnan(good[:elems]).any() and torch.isnan(good[elems:]).all()      # the declared lists, and nothing behind them
    # the same bits as the plan of the first four frames alone gives
    assert np.array_equal(rg.bits(good[:elems]), rg.bits(rg.ragged_levels(frames[:n_frames], mtcnn.ragged_plan(PYRAMID_SHAPES[:n_frames], 12, rg.FACTOR))))
    good_bits = rg.bits(good)
    m = int(plan.frames["first_item"][1]) + 1                                           # the second level of frame 1: the row form
    assert 0 < m < n_items - 1 and int(plan.levels["rows"][m]) == 1 and int(plan.levels["frame"][m]) == 1
    size = int(plan.levels["dh"][m]) * int(plan.levels["dw"][m]) * 3
    lo = int(plan.levels["level_off"][m])

    def skipped_only(levels, ranges, what):
        got = rg.bits(levels)
        keep = np.ones(got.shape[0], bool)
        for a, b in ranges:
            assert torch.isnan(levels[a:b]).all(), "%s: the item at %d was written" % (what, a)
            keep[a:b] = False
        assert np.array_equal(got[keep], good_bits[keep]), "%s: another item changed" % what

    def corrupt(field, value):
        p = make()
        p.levels[field][m] = value
        return p
    # frame = n_frames: the row behind the declared frame table is frame 4, a valid frame of frame 1's size
    assert PYRAMID_SHAPES[n_frames] == PYRAMID_SHAPES[1]
    skipped_only(rg.ragged_levels(frames, corrupt("frame", n_frames), **declared), [(lo, lo + size)], "frame = n_frames")
    skipped_only(rg.ragged_levels(frames, corrupt("level_off", elems + 1 - size), **declared), [(lo, lo + size)], "level end one past")
    assert int(plan.levels["hoff"][m]) % 16 == 0
    skipped_only(rg.ragged_levels(frames, corrupt("hoff", int(plan.levels["hoff"][m]) + 8), **declared), [(lo, lo + size)], "hoff + 8")
    # 16 bytes of LDS fewer than the plan asks for: every row-form item that needs more stays unwritten, the others are written
    lds = plan.level_lds - 16
    needs = {}
    for it in range(n_items):
        if int(plan.levels["rows"][it]):
            h = PYRAMID_SHAPES[int(plan.levels["frame"][it])][0]
            dh, dw = int(plan.levels["dh"][it]), int(plan.levels["dw"][it])
            needs[it] = int(plan.levels["hoff"][it]) + (int(h / dh) + 3) * dw * 12
    assert max(needs.values()) == plan.level_lds
    short = [it for it, need in needs.items() if need > lds]
    assert 1 <= len(short) < len(needs)
    ranges = [(int(plan.levels["level_off"][it]), int(plan.levels["level_off"][it]) + int(plan.levels["dh"][it]) * int(plan.levels["dw"][it]) * 3)
              for it in short]
    skipped_only(rg.ragged_levels(frames, make(), lds_bytes=lds, **declared), ranges, "16 bytes of LDS fewer")


# ---- the table guards of stage 1 ----------------------------------------------------------------------------------------------------------
STAGE1_SHAPES = [(300, 400), (64, 48), (15, 500), (37, 53), (120, 100), (64, 48)]     # the last frame's items and cells lie BEHIND the lists


def test_stage1_guards_drop_the_level_or_the_frames_levels_and_nothing_else(cap):
    from hse_facerec_tf_amd import mtcnn

    def make():
        return mtcnn.ragged_plan(STAGE1_SHAPES, 20, rg.FACTOR)
    plan = make()
    n_frames = len(STAGE1_SHAPES) - 1
    n_items = int(plan.frames["first_item"][n_frames])
    n_cells = int(plan.cells["cell_off"][n_items])
    assert n_items < plan.n_items and n_cells < plan.pixels[-1]
    declared = dict(n_frames=n_frames, n_items=n_items, n_cells=n_cells)
    prob, reg = rg.stage1_maps(plan, np.random.RandomState(44), lambda it, cells: 3 + it % 5)
    want = rg.run_single_frame_stage1(plan, prob, reg, cap, n_frames=n_frames)
    good = rg.run_ragged_stage1(plan, prob, reg, cap, **declared)
    assert (want[0][[0, 1, 3, 4], 1] > 0).all() and want[0][:, 4].sum() == 0, want[0]
    for f in range(n_frames):
        rg.assert_frame_rows_equal(good, want, f, "declared lists")

    def others_unchanged(got, f_bad, what):
        for f in range(n_frames):
            if f != f_bad:
                rg.assert_frame_rows_equal(got, want, f, what)
    # a frame whose item range ends one past the declared list: the finish on no levels
    f_bad = 3
    p = make()
    p.frames["first_item"][f_bad] = n_items + 1 - int(p.frames["n_items"][f_bad])
    assert int(p.frames["n_items"][f_bad]) >= 2
    mine = set(range(int(plan.frames["first_item"][f_bad]), int(plan.frames["first_item"][f_bad]) + int(plan.frames["n_items"][f_bad])))
    no_levels = rg.run_single_frame_stage1(plan, prob, reg, cap, n_frames=n_frames, skip=mine)
    assert no_levels[0][f_bad].sum() == 0
    got = rg.run_ragged_stage1(p, prob, reg, cap, **declared)
    rg.assert_frame_rows_equal(got, no_levels, f_bad, "item range one past the list")
    others_unchanged(got, f_bad, "item range one past the list")
    # one level in the middle of the list, its cells ending one past the declared maps / its scale 0: the frame without that level
    it = n_items // 2
    f_bad = int(plan.levels["frame"][it])
    assert 0 < it < n_items - 1
    without = rg.run_single_frame_stage1(plan, prob, reg, cap, n_frames=n_frames, skip={it})
    assert int(without[0][f_bad, 0]) < int(want[0][f_bad, 0])                            # the level had rows to lose
    p = make()
    p.cells["cell_off"][it] = n_cells + 1 - int(p.cells["w"][it]) * int(p.cells["h"][it])
    got = rg.run_ragged_stage1(p, prob, reg, cap, **declared)
    rg.assert_frame_rows_equal(got, without, f_bad, "cells end one past the maps")
    others_unchanged(got, f_bad, "cells end one past the maps")
    p = make()
    p.cells["scale"][it] = 0.0
    got = rg.run_ragged_stage1(p, prob, reg, cap, **declared)
    rg.assert_frame_rows_equal(got, without, f_bad, "scale 0")
    others_unchanged(got, f_bad, "scale 0")


# ---- the convolution's input-load widths -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c,cout,k", [(10, 16, 3), (16, 32, 3), (32, 4, 1)])
def test_ragged_conv_on_inputs_4_and_8_bytes_past_16_byte_alignment(c, cout, k):
    """ragged_conv2d_kernel picks its input load from the alignment of the item's first pixel, x + in_off * C floats: xvec = 4 on 16
    bytes, 2 on 8, 1 otherwise.  The packed input starts 0, 1 and 2 floats into a 16-byte-aligned tensor:

      C = 16, 32 (a pixel is 64 / 128 bytes, so every item is aligned as the base is):
        base + 0   xvec 4   the float4 loop (`xvec >= 4 && C % 4 == 0`)
        base + 2   xvec 2   the float2 loop (`xvec >= 2 && C % 2 == 0`)
        base + 1   xvec 1   the scalar tail does all of C
      C = 10 (a pixel is 40 bytes: items at an even pixel offset are aligned as the base is, items at an odd one 8 bytes further):
        base + 0   xvec 4 (even) / 2 (odd): C % 4 != 0 sends both to the float2 loop
        base + 2   xvec 2 (even) / 4 (odd): the float2 loop
        base + 1   xvec 1   the scalar tail
    Every output's FMA chain is the same whatever the width: the bits are ops.conv2d_direct's in all three placements."""
    import torch
    from hse_facerec_tf_amd import ops
    from hse_facerec_tf_amd.mtcnn_ragged import conv_co
    rs = np.random.RandomState(c * 100 + cout + 7)
    w = torch.from_numpy(rs.normal(0, 0.3, (k, k, c, cout)).astype(np.float32)).cuda()
    bias = torch.from_numpy(rs.normal(0, 0.5, cout).astype(np.float32)).cuda()
    alpha = torch.from_numpy(rs.uniform(0.05, 0.9, cout).astype(np.float32)).cuda()
    co = conv_co(cout)
    sizes = rg.item_sizes(k, cout // co)
    items = [torch.from_numpy(rs.normal(0, 1, (a, b, c)).astype(np.float32)).cuda() for a, b in sizes]
    want = [ops.conv2d_direct(t[None].contiguous(), w, bias, alpha, 1, "VALID")[0] for t in items]
    seen = {}

    def look(maps, bi, xp, yp):
        seen["in_off"] = maps["in_off"].copy()
    for base in (0, 1, 2):
        got, y = rg.ragged_conv(items, w, bias, alpha, co, base=base, tweak=look)
        assert not torch.isnan(y).any(), base                                           # every output written
        for i, g in enumerate(got):
            assert np.array_equal(rg.bits(g), rg.bits(want[i])), (base, sizes[i])
    assert {int(o) % 2 for o in seen["in_off"]} == {0, 1}                               # items at even and at odd pixel offsets
