"""GPU suite: the mixed-size detector pass (libhsefr_ragged.so, MTCNNDetector.detect_ragged, detect_batch / process_images with
mixed_sizes=True) against the single-frame entries, BIT FOR BIT: every comparison is np.array_equal on the uint32 views of the floats
(or on the integers / float64 values themselves).  Step by step -- the ragged convolution and pooling against ops.conv2d_direct /
ops.maxpool item by item, the ragged pyramid against hsefr_mtcnn_pyramid_level per (frame, level), ragged stage 1 against
hsefr_mtcnn_stage1_level per level plus hsefr_mtcnn_stage1_finish per frame -- and end to end against ``det(frame)``.  The
single-frame results are computed once per module and never changed."""
import numpy as np
import pytest

from oracle import pipeline as opl

from conftest import TEST_IMAGE

pytestmark = pytest.mark.gpu

FACTOR = 0.709


def bits(t):
    a = t.detach().cpu().numpy() if hasattr(t, "detach") else np.asarray(t)
    assert a.dtype == np.float32
    return np.ascontiguousarray(a).view(np.uint32)


def upload(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).cuda()


# ---- ragged conv / pool against ops.conv2d_direct / ops.maxpool item by item ---------------------------------------------------------
def past_a_boundary(tpp):
    """The smallest pixel count n > 1 whose n * tpp threads end as little past a workgroup boundary as tpp allows: one thread where tpp
    is odd, gcd(tpp, 256) threads (one thread GROUP of a pixel at the least) otherwise."""
    g = int(np.gcd(tpp, 256))
    return next(n for n in range(2, 4096) if (n * tpp) % 256 == g and n * tpp > 256)


def item_sizes(k, tpp):
    """Output sizes -> input sizes of the cases the kernels can go wrong on: a 1 x 1 output, 12 x 12, odd x even, an item whose thread
    range ends exactly on a workgroup boundary (16 x 16 outputs: 256 * tpp threads) and one that ends just past one."""
    outs = [(1, 1), (12 - k + 1, 12 - k + 1), (7 - k + 1, 10 - k + 1), (16, 16), (1, past_a_boundary(tpp)), (5, 3)]
    assert (16 * 16 * tpp) % 256 == 0 and (past_a_boundary(tpp) * tpp) % 256 == np.gcd(tpp, 256)
    return [(a + k - 1, b + k - 1) for a, b in outs]


SLACK_FILL = 1.5                   # what the allocated pixels outside the declared buffers hold: finite, so a read of them shows in a result


def packed_input(items, c, base, slack):
    """The items back to back, ``base`` floats into a larger tensor (the pointer is 4 * base bytes past the allocation's alignment)
    with ``slack`` pixels behind: what lies in front of and behind the packed input is allocated and holds SLACK_FILL."""
    import torch
    flat = torch.cat([t.reshape(-1) for t in items]) if items else torch.empty(0, device="cuda")
    whole = torch.full((base + flat.numel() + slack * c,), SLACK_FILL, dtype=torch.float32, device="cuda")
    assert whole.data_ptr() % 16 == 0
    whole[base:base + flat.numel()] = flat
    return whole, whole[base:]


def upload_maps(maps):
    """The map table with one more row in front and one behind: maps[-1] and maps[n_items] are allocated, and hold a copy of the item of
    the most workgroups as map_tables laid it out (a workgroup that followed a table entry there would write).
    -> (the tensor, the pointer to row 0)."""
    big = int(np.argmax(maps["oh"].astype(np.int64) * maps["ow"]))
    spare = maps[big:big + 1]
    t = upload(np.concatenate([spare, maps, spare]))
    return t, t.data_ptr() + maps.dtype.itemsize


def ragged_conv(items, w, bias, alpha, co, base=0, tweak=None, slack=0):
    """hsefr_ragged_conv2d over the items -> (every item's output, the whole output buffer).  ``base``, ``slack``: see packed_input; the
    output has ``slack`` pixels behind too, and the entry point is told the sizes WITHOUT the slack.  ``tweak(maps, block_item, x_pixels,
    y_pixels)`` edits the tables in place before they go up."""
    import torch
    from hse_facerec_tf_amd import _lib
    from hse_facerec_tf_amd import mtcnn_ragged as mr
    k, c, cout = int(w.shape[0]), int(w.shape[2]), int(w.shape[3])
    d0, d1 = np.array([t.shape[0] for t in items]), np.array([t.shape[1] for t in items])
    maps, block_item, in_px, out_px = mr.map_tables((d0, d1), (d0 - k + 1, d1 - k + 1), cout // co)
    if tweak is not None:
        tweak(maps, block_item, in_px, out_px)
    whole, x = packed_input(items, c, base, slack)
    y = torch.full((max((out_px + slack) * cout, 1),), float("nan"), dtype=torch.float32, device="cuda")
    (t_maps, p_maps), d_blocks = (upload_maps(maps), upload(block_item)) if len(items) else ((None, None), None)
    _lib.ragged_check(_lib.ragged_lib().hsefr_ragged_conv2d(
        x.data_ptr(), in_px, w.data_ptr(), bias.data_ptr(), None if alpha is None else alpha.data_ptr(), y.data_ptr(), out_px,
        p_maps, len(items), None if d_blocks is None else d_blocks.data_ptr(), len(block_item), c, cout,
        k, k, 1, 0, 0, co, _lib.current_stream_ptr()), "hsefr_ragged_conv2d")
    torch.cuda.synchronize()
    out, at = [], 0
    for a, b in zip(d0 - k + 1, d1 - k + 1):
        out.append(y[at * cout:(at + int(a * b)) * cout].reshape(int(a), int(b), cout))
        at += int(a * b)
    return out, y


def ragged_pool(items, c, tweak=None, slack=0, base=0):
    """hsefr_ragged_maxpool 2 x 2 / 2 over the items -> (every item's output, the whole output buffer); the arguments of ragged_conv."""
    import torch
    from hse_facerec_tf_amd import _lib
    from hse_facerec_tf_amd import mtcnn_ragged as mr
    d0, d1 = np.array([t.shape[0] for t in items], np.int64), np.array([t.shape[1] for t in items], np.int64)
    maps, block_item, in_px, out_px = mr.map_tables((d0, d1), (-(-d0 // 2), -(-d1 // 2)), c)
    if tweak is not None:
        tweak(maps, block_item, in_px, out_px)
    whole, x = packed_input(items, c, base, slack)
    y = torch.full((max((out_px + slack) * c, 1),), float("nan"), dtype=torch.float32, device="cuda")
    (t_maps, p_maps), d_blocks = (upload_maps(maps), upload(block_item)) if len(items) else ((None, None), None)
    _lib.ragged_check(_lib.ragged_lib().hsefr_ragged_maxpool(
        x.data_ptr(), in_px, y.data_ptr(), out_px, p_maps, len(items), None if d_blocks is None else d_blocks.data_ptr(), len(block_item), c, 2, 2,
        _lib.current_stream_ptr()), "hsefr_ragged_maxpool")
    torch.cuda.synchronize()
    out, at = [], 0
    for a, b in zip(-(-d0 // 2), -(-d1 // 2)):
        out.append(y[at * c:(at + int(a * b)) * c].reshape(int(a), int(b), c))
        at += int(a * b)
    return out, y


@pytest.mark.parametrize("c,cout,k", [(3, 10, 3), (10, 16, 3), (16, 32, 3), (32, 2, 1), (32, 4, 1)])
def test_ragged_conv_equals_conv2d_direct_item_by_item(c, cout, k):
    """P-Net's five layer shapes: every CO (4 / 2 / 1) and every input-vector path (C = 3 scalar, 10 two at a time, 16 / 32 four)."""
    import torch
    from hse_facerec_tf_amd import ops
    from hse_facerec_tf_amd.mtcnn_ragged import conv_co
    rs = np.random.RandomState(c * 100 + cout)
    w = torch.from_numpy(rs.normal(0, 0.3, (k, k, c, cout)).astype(np.float32)).cuda()
    bias = torch.from_numpy(rs.normal(0, 0.5, cout).astype(np.float32)).cuda()
    alpha = torch.from_numpy(rs.uniform(0.05, 0.9, cout).astype(np.float32)).cuda()
    co = conv_co(cout)
    sizes = item_sizes(k, cout // co)
    items = [torch.from_numpy(rs.normal(0, 1, (a, b, c)).astype(np.float32)).cuda() for a, b in sizes]
    want = [ops.conv2d_direct(t[None].contiguous(), w, bias, alpha, 1, "VALID")[0] for t in items]
    assert tuple(want[0].shape) == (1, 1, cout)
    for order in (list(range(len(items))), list(range(len(items)))[::-1], [1]):                      # the list, reversed, a list of one
        for use_co in sorted({co, 1, 2 if cout % 2 == 0 else 1}):
            got, y = ragged_conv([items[i] for i in order], w, bias, alpha, use_co)
            assert not torch.isnan(y).any()                                                            # every output written
            for i, g in zip(order, got):
                assert np.array_equal(bits(g), bits(want[i])), (order, use_co, sizes[i])
    got, y = ragged_conv([items[0]], w, bias, None, co)                                               # no PReLU: the 1 x 1 head layers
    assert np.array_equal(bits(got[0]), bits(ops.conv2d_direct(items[0][None].contiguous(), w, bias, None, 1, "VALID")[0]))
    got, y = ragged_conv([], w, bias, alpha, co)                                                      # an empty list: no launch, no error
    assert got == [] and torch.isnan(y).all()


def test_ragged_maxpool_equals_maxpool_item_by_item():
    import torch
    from hse_facerec_tf_amd import ops
    rs = np.random.RandomState(11)
    c = 10
    # 7 x 10: the first axis' last window is clipped, the second axis' is not; 1 x 1 and 3 x 3 inputs; 32 x 32 -> 16 x 16 x 10 threads = 10
    # workgroups exactly; 1 x 153 -> 77 pixels = 770 threads, two past a boundary (ten threads a pixel: the least an even count allows)
    sizes = [(1, 1), (3, 3), (10, 10), (7, 10), (32, 32), (1, 2 * past_a_boundary(c) - 1), (9, 4)]
    assert (16 * 16 * c) % 256 == 0 and (past_a_boundary(c) * c) % 256 == 2
    items = [torch.from_numpy(rs.normal(0, 1, (a, b, c)).astype(np.float32)).cuda() for a, b in sizes]
    want = [ops.maxpool(t[None].contiguous(), 2, 2, "SAME")[0] for t in items]
    assert tuple(want[3].shape) == (4, 5, c)
    for order in (list(range(len(items))), list(range(len(items)))[::-1], [3], []):
        sel = [items[i] for i in order]
        _, y = ragged_pool(sel, c)
        assert torch.isnan(y).all() if not sel else not torch.isnan(y).any()
        at = 0
        for i in order:
            n = int(np.prod(want[i].shape))
            assert np.array_equal(bits(y[at:at + n]), bits(want[i].reshape(-1))), (order, sizes[i])
            at += n


# ---- the ragged pyramid against hsefr_mtcnn_pyramid_level per (frame, level) ---------------------------------------------------------
def ragged_levels(frames, plan, buffer=None, **declared):
    """hsefr_ragged_pyramid over the plan -> the packed level buffer.  ``buffer``: the packed frames on the device already.
    ``declared``: n_frames, n_items, n_blocks, levels_elems, lds_bytes to tell the entry point instead of the plan's (the tables and
    buffers are the whole plan's either way)."""
    import torch
    from hse_facerec_tf_amd import _lib
    from hse_facerec_tf_amd.mtcnn_ragged import DevicePlan
    assert set(declared) <= {"n_frames", "n_items", "n_blocks", "levels_elems", "lds_bytes"}
    dplan = DevicePlan(plan, torch.device("cuda", torch.cuda.current_device()))
    packed = buffer if buffer is not None else torch.from_numpy(np.concatenate([f.reshape(-1) for f in frames])).cuda()
    levels = torch.full((plan.pixels[0] * 3,), float("nan"), dtype=torch.float32, device="cuda")
    _lib.ragged_check(_lib.ragged_lib().hsefr_ragged_pyramid(
        packed.data_ptr(), plan.frames_bytes, dplan.frames, declared.get("n_frames", plan.n_frames), dplan.levels,
        declared.get("n_items", plan.n_items), dplan.level_block_item, declared.get("n_blocks", len(plan.level_block_item)), levels.data_ptr(),
        declared.get("levels_elems", plan.pixels[0] * 3), declared.get("lds_bytes", plan.level_lds), _lib.current_stream_ptr()),
        "hsefr_ragged_pyramid")
    torch.cuda.synchronize()
    return levels


def assert_levels_equal_the_single_frame_levels(frames, plan, levels):
    import torch
    from hse_facerec_tf_amd import _lib
    assert not torch.isnan(levels).any()
    for it in range(plan.n_items):
        lv = plan.levels[it]
        f, dh, dw, off = int(lv["frame"]), int(lv["dh"]), int(lv["dw"]), int(lv["level_off"])
        h, w = frames[f].shape[:2]
        one = torch.from_numpy(frames[f]).cuda()
        want = torch.empty((dw, dh, 3), dtype=torch.float32, device="cuda")
        _lib.check(_lib.lib().hsefr_mtcnn_pyramid_level(one.data_ptr(), want.data_ptr(), h, w, dh, dw, _lib.current_stream_ptr()),
                   "hsefr_mtcnn_pyramid_level")
        assert np.array_equal(bits(levels[off:off + dh * dw * 3]), bits(want.reshape(-1))), (it, f, dh, dw, int(lv["rows"]))


def test_ragged_pyramid_equals_the_single_frame_levels():
    from hse_facerec_tf_amd import mtcnn
    rs = np.random.RandomState(21)
    frames = [rs.randint(0, 256, (h, w, 3)).astype(np.uint8) for h, w in ((37, 53), (64, 48), (120, 100), (53, 37))]
    for minsize in (20, 12):                             # minsize 12: the first level is the frame itself, which takes the per-pixel form
        plan = mtcnn.ragged_plan([f.shape[:2] for f in frames], minsize, FACTOR)
        counts = [int(n) for n in plan.frames["n_items"]]
        assert len(set(counts)) >= 3 and min(counts) >= 2, counts                       # the level counts differ
        assert int(plan.frames["offset"][1]) % 2 == 1                                   # a frame on an odd byte offset
        forms = set(int(r) for r in plan.levels["rows"])
        assert forms == ({1} if minsize == 20 else {0, 1}), forms
        assert_levels_equal_the_single_frame_levels(frames, plan, ragged_levels(frames, plan))
    # a plan without items: no launch, no error
    empty = mtcnn.ragged_plan([(5, 7)], 20, FACTOR)
    assert empty.n_items == 0 and ragged_levels([np.zeros((5, 7, 3), np.uint8)], empty).numel() == 0


def test_ragged_pyramid_frame_offsets_past_two_to_the_31():
    """The frame offset is 64-bit: a 2.2 GB frame buffer that is allocated but not filled, the second frame's bytes 2.16e9 bytes in (on
    an odd address).  Only the two small frames hold data."""
    import torch
    from hse_facerec_tf_amd import mtcnn
    rs = np.random.RandomState(22)
    frames = [rs.randint(0, 256, (h, w, 3)).astype(np.uint8) for h, w in ((37, 53), (64, 48))]
    plan = mtcnn.ragged_plan([f.shape[:2] for f in frames], 20, FACTOR)
    total, far = 2_200_000_000, 2_160_000_001
    assert far > 2 ** 31 and far + frames[1].size <= total
    plan.frames["offset"][1] = far
    plan.frames_bytes = total
    buffer = torch.empty(total, dtype=torch.uint8, device="cuda")
    buffer[:frames[0].size].copy_(torch.from_numpy(frames[0].reshape(-1)))
    buffer[far:far + frames[1].size].copy_(torch.from_numpy(frames[1].reshape(-1)))
    assert_levels_equal_the_single_frame_levels(frames, plan, ragged_levels(frames, plan, buffer))
    # a frame that does not lie inside the buffer is skipped, not followed: its levels stay unwritten
    plan.frames_bytes = far + frames[1].size - 1
    levels = ragged_levels(frames, plan, buffer)
    first = int(plan.levels["level_off"][int(plan.frames["first_item"][1])])
    assert not torch.isnan(levels[:first]).any() and torch.isnan(levels[first:]).all()


# ---- ragged stage 1 against the per-level and per-frame entries ----------------------------------------------------------------------
def stage1_maps(plan, rs, per_item):
    """Synthetic P-Net outputs over the plan's last layer: background below the threshold, ``per_item(it, cells)`` firing cells per item
    with distinct scores."""
    n_cells = plan.pixels[-1]
    prob = rs.uniform(0.0, 0.3, (n_cells, 2)).astype(np.float32)
    reg = rs.normal(0, 0.1, (n_cells, 4)).astype(np.float32)
    for it in range(plan.n_items):
        off, cells = int(plan.cells["cell_off"][it]), int(plan.cells["w"][it]) * int(plan.cells["h"][it])
        k = min(per_item(it, cells), cells)
        where = off + rs.choice(cells, k, replace=False)
        prob[where, 1] = rs.permutation(np.linspace(0.62, 0.99, k)).astype(np.float32)
    return prob, reg


def run_ragged_stage1(plan, prob, reg, cap, n_frames=None, n_items=None, n_cells=None):
    """``n_frames``, ``n_items``, ``n_cells``: what to tell the entry point instead of the plan's counts (the tables and maps are the whole
    plan's either way)."""
    import torch
    from hse_facerec_tf_amd import _lib
    from hse_facerec_tf_amd.mtcnn_ragged import DevicePlan
    dplan = DevicePlan(plan, torch.device("cuda", torch.cuda.current_device()))
    n = plan.n_frames if n_frames is None else n_frames
    d_prob, d_reg = torch.from_numpy(prob).cuda(), torch.from_numpy(reg).cuda()
    found = torch.zeros((n, cap, 9), dtype=torch.float64, device="cuda")
    boxes = torch.zeros((n, cap, 5), dtype=torch.float64, device="cuda")
    tab = torch.zeros((n, cap, 8), dtype=torch.int32, device="cuda")
    counters = torch.zeros((n, 8), dtype=torch.int32, device="cuda")
    _lib.ragged_check(_lib.ragged_lib().hsefr_ragged_stage1(
        d_prob.data_ptr(), d_reg.data_ptr(), plan.pixels[-1] if n_cells is None else n_cells, dplan.frames, n, dplan.cells,
        plan.n_items if n_items is None else n_items, float(np.float32(0.6)), found.data_ptr(),
        counters.data_ptr(), boxes.data_ptr(), tab.data_ptr(), _lib.current_stream_ptr()), "hsefr_ragged_stage1")
    return [t.cpu().numpy() for t in (counters, found, boxes, tab)]


def run_single_frame_stage1(plan, prob, reg, cap, n_frames=None, skip=()):
    """Per frame: hsefr_mtcnn_stage1_level on each of its levels, then hsefr_mtcnn_stage1_finish.  ``skip``: items to leave out;
    ``n_frames``: the first frames of the plan only."""
    import torch
    from hse_facerec_tf_amd import _lib
    L = _lib.lib()
    n = plan.n_frames if n_frames is None else n_frames
    d_prob, d_reg = torch.from_numpy(prob).cuda(), torch.from_numpy(reg).cuda()
    found = torch.zeros((n, cap, 9), dtype=torch.float64, device="cuda")
    boxes = torch.zeros((n, cap, 5), dtype=torch.float64, device="cuda")
    tab = torch.zeros((n, cap, 8), dtype=torch.int32, device="cuda")
    counters = torch.zeros((n, 8), dtype=torch.int32, device="cuda")
    st = _lib.current_stream_ptr()
    for f in range(n):
        first, count = int(plan.frames["first_item"][f]), int(plan.frames["n_items"][f])
        for it in range(first, first + count):
            if it in skip:
                continue
            off, w, h = int(plan.cells["cell_off"][it]), int(plan.cells["w"][it]), int(plan.cells["h"][it])
            _lib.check(L.hsefr_mtcnn_stage1_level(d_prob[off:].data_ptr(), d_reg[off:].data_ptr(), w, h, float(plan.scales[it]), float(np.float32(0.6)),
                                                  found[f].data_ptr(), counters[f].data_ptr(), st), "hsefr_mtcnn_stage1_level")
        _lib.check(L.hsefr_mtcnn_stage1_finish(found[f].data_ptr(), counters[f].data_ptr(), boxes[f].data_ptr(), tab[f].data_ptr(),
                                               int(plan.frames["w"][f]), int(plan.frames["h"][f]), st), "hsefr_mtcnn_stage1_finish")
    return [t.cpu().numpy() for t in (counters, found, boxes, tab)]


def assert_frame_rows_equal(got, want, f, what):
    (gc, gf, gb, gt), (wc, wf, wb, wt) = got, want
    assert np.array_equal(gc[f], wc[f]), (what, f, gc[f], wc[f])
    n0, n1 = int(wc[f, 0]), int(wc[f, 1])
    assert np.array_equal(gf[f, :n0].view(np.uint64), wf[f, :n0].view(np.uint64)), (what, f, "found")      # the levels' order, the same bits
    assert np.array_equal(gb[f, :n1].view(np.uint64), wb[f, :n1].view(np.uint64)), (what, f, "boxes")
    assert np.array_equal(gt[f, :n1], wt[f, :n1]), (what, f, "crop tables")


def test_ragged_stage1_equals_the_levels_and_the_finish_of_every_frame():
    from hse_facerec_tf_amd import _lib, mtcnn
    cap = int(_lib.lib().hsefr_mtcnn_post_capacity())
    assert int(_lib.ragged_lib().hsefr_ragged_capacity()) == cap
    shapes = [(300, 400), (64, 48), (15, 500), (37, 53), (120, 100)]                   # (15, 500): a frame without a level, in the middle
    plan = mtcnn.ragged_plan(shapes, 20, FACTOR)
    assert int(plan.frames["n_items"][2]) == 0 and plan.n_items >= 15
    rs = np.random.RandomState(31)
    # a handful of firing cells per item; item 1 has exactly ONE (the reference reads the regression maps flipped then), item 2 none
    prob, reg = stage1_maps(plan, rs, lambda it, cells: {1: 1, 2: 0}.get(it, 3 + it % 5))
    want = run_single_frame_stage1(plan, prob, reg, cap)
    got = run_ragged_stage1(plan, prob, reg, cap)
    assert want[0][:, 4].sum() == 0 and want[0][2].sum() == 0 and (want[0][[0, 1, 3, 4], 1] > 0).all(), want[0]
    assert int(want[0][0, 0]) > int(plan.frames["n_items"][0])                          # several rows per level: the order is tested
    for f in range(len(shapes)):
        assert_frame_rows_equal(got, want, f, "stage 1")
    # the handled overflow: more firing cells than a list holds in ONE item of ONE frame -- that frame's flag is set, the other
    # frames' rows are what they are without the flood
    it = 1                                                                              # the second level of frame 0
    off, cells = int(plan.cells["cell_off"][it]), int(plan.cells["w"][it]) * int(plan.cells["h"][it])
    assert cells > cap + 52
    flooded = prob.copy()
    flooded[off:off + cap + 52, 1] = np.float32(0.95)
    got_f = run_ragged_stage1(plan, flooded, reg, cap)
    want_f = run_single_frame_stage1(plan, flooded, reg, cap)
    assert got_f[0][0, 4] == 1 and got_f[0][0, 1] == 0 and np.array_equal(got_f[0], want_f[0]), got_f[0]
    assert got_f[0][1:, 4].sum() == 0
    for f in range(1, len(shapes)):
        assert_frame_rows_equal(got_f, want, f, "next to the flooded frame")


# ---- end to end -------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def det():
    from hse_facerec_tf_amd.mtcnn import MTCNNDetector
    return MTCNNDetector(minsize=32)


@pytest.fixture(scope="module")
def mixed():
    """The six frames of test_mixed_sizes_come_back_in_list_order, the reference photo transposed and an all-black 300 x 400 frame."""
    img = opl.imread_rgb(TEST_IMAGE)
    small = np.zeros((20, 500, 3), np.uint8)
    small[5:15, 100:400] = 200
    out = [img, img[40:520, 100:700], img[::2, ::2], img[:90, :200], small, img, np.transpose(img, (1, 0, 2)), np.zeros((300, 400, 3), np.uint8)]
    return [np.ascontiguousarray(f) for f in out]


@pytest.fixture(scope="module")
def serial(det, mixed):
    """The single-frame call on every frame, before anything ragged runs -- and the coverage the tests below need, from it alone."""
    out = [det(f) for f in mixed]
    counts = [b.shape[0] for b, _ in out]
    levels = [len(det.pyramid_scales(*f.shape[:2])) for f in mixed]
    print("faces per frame, one frame at a time:", counts, "levels:", levels)
    assert sum(c > 0 for c in counts) >= 3 and len({c for c in counts if c}) >= 2, counts          # faces, in lists of different lengths
    assert any(c == 0 and n > 0 for c, n in zip(counts, levels)), (counts, levels)                   # levels and no face
    assert any(n == 0 for n in levels), levels                                                       # no level
    assert det.host_fallbacks == 0
    return out


def assert_same(got, want, what=""):
    """One frame's batched result against its single-frame result (tests/test_mtcnn_batch_gpu.py)."""
    gb, gp = got
    wb, wp = want
    n = wb.shape[0]
    assert gb.dtype == np.float64 and gp.dtype == np.float32, what
    if n == 0:
        assert gb.shape == (0, 5) and gp.shape == (10, 0), (what, gb.shape, gp.shape)
        return
    assert gb.shape == (n, 5) and gp.shape == (10, n), (what, gb.shape, gp.shape)
    assert np.array_equal(gb.view(np.uint64), wb.view(np.uint64)) and np.array_equal(gp.view(np.uint32), wp.view(np.uint32)), what


def test_mixed_sizes_equal_the_single_frame_calls(det, mixed, serial):
    passes, in_passes = det.ragged_passes, det.ragged_frames
    got = det.detect_batch(mixed, mixed_sizes=True)
    assert len(got) == len(mixed)
    for i, (g, w) in enumerate(zip(got, serial)):
        assert_same(g, w, "frame %d" % i)
    # the two same-size photos form their own pass, the frame without a level none, the other five ONE ragged pass
    assert det.host_fallbacks == 0 and det.ragged_passes - passes == 1 and det.ragged_frames - in_passes == 5
    got, sources = det.detect_batch(mixed, mixed_sizes=True, return_stacks=True)
    assert [s is not None for s in sources] == [True, False, False, False, False, True, False, False]      # None for the frames of a ragged pass
    for i, (g, w) in enumerate(zip(got, serial)):
        assert_same(g, w, "with stacks, frame %d" % i)
    # a permutation
    perm = [6, 3, 0, 7, 4, 1, 5, 2]
    passes = det.ragged_passes
    for i, g in zip(perm, det.detect_batch([mixed[i] for i in perm], mixed_sizes=True)):
        assert_same(g, serial[i], "permuted, frame %d" % i)
    assert det.ragged_passes - passes == 1
    # max_frames 3: the five lone frames make a ragged pass of three and one of two
    passes, in_passes = det.ragged_passes, det.ragged_frames
    for i, (g, w) in enumerate(zip(det.detect_batch(mixed, max_frames=3, mixed_sizes=True), serial)):
        assert_same(g, w, "max_frames 3, frame %d" % i)
    assert det.ragged_passes - passes == 2 and det.ragged_frames - in_passes == 5
    # every size once: no same-size pass at all
    once = [0, 1, 2, 3, 4, 6, 7]
    passes, in_passes = det.ragged_passes, det.ragged_frames
    for i, g in zip(once, det.detect_batch([mixed[i] for i in once], mixed_sizes=True)):
        assert_same(g, serial[i], "every size once, frame %d" % i)
    assert det.ragged_passes - passes == 1 and det.ragged_frames - in_passes == 6
    # without the flag nothing changed
    passes = det.ragged_passes
    for i, (g, w) in enumerate(zip(det.detect_batch(mixed), serial)):
        assert_same(g, w, "without the flag, frame %d" % i)
    assert det.ragged_passes == passes and det.host_fallbacks == 0
    assert det.detect_batch([], mixed_sizes=True) == []


def test_detect_ragged(det, mixed, serial):
    # all eight frames in ONE pass, the same-size pair and the frame without a level included
    for i, (g, w) in enumerate(zip(det.detect_ragged(mixed), serial)):
        assert_same(g, w, "one pass, frame %d" % i)
    # on same-size frames it equals detect_batch on them
    img = mixed[0]
    same = [img, np.ascontiguousarray(img[:, ::-1]), np.zeros_like(img), np.ascontiguousarray(img[::-1])]
    want = det.detect_batch(same)
    assert sum(b.shape[0] > 0 for b, _ in want) >= 2
    for i, (g, w) in enumerate(zip(det.detect_ragged(same), want)):
        assert_same(g, w, "same size, frame %d" % i)
    # the plan and its tables are kept per list of shapes
    assert det._ragged_plans[(tuple(f.shape[:2] for f in same), det.minsize)] is det._ragged_device_plan(tuple(f.shape[:2] for f in same))
    # frames without a level only, and no frames
    assert [(b.shape, p.shape) for b, p in det.detect_ragged([mixed[4], mixed[4][:, :300]])] == [((0, 5), (10, 0))] * 2
    assert det.detect_ragged([]) == []
    assert det.host_fallbacks == 0


def test_an_overflow_in_a_ragged_pass_sends_only_its_own_frame_to_the_single_frame_call(det, mixed, serial):
    """The handled overflow end to end: P-Net's face map of ONE item of a ragged pass is flooded with more firing cells than a list
    holds (written into the packed map between the net and stage 1).  detect_ragged hands that frame back as None and the others
    unchanged; detect_batch redoes it alone -- the single-frame call sees the unflooded map, so every result is the serial one."""
    from hse_facerec_tf_amd import _lib
    from hse_facerec_tf_amd.mtcnn_ragged import RaggedMaps
    cap = int(_lib.lib().hsefr_mtcnn_post_capacity())
    lone = [1, 2, 3, 6, 7]                                                               # the frames of the ragged pass, frame 6 flooded
    inner = det.pnet
    flooded = []

    def pnet(x):
        reg, prob = inner(x)
        if isinstance(x, RaggedMaps):
            plan = x.dplan.plan
            it = int(plan.frames["first_item"][3])                                       # the first level of the pass's fourth frame
            off, cells = int(plan.cells["cell_off"][it]), int(plan.cells["w"][it]) * int(plan.cells["h"][it])
            assert cells > cap + 10
            prob.data.reshape(-1, 2)[off:off + cap + 10, 1] = 0.95
            flooded.append(it)
        return reg, prob
    det.pnet = pnet
    try:
        got = det.detect_ragged([mixed[i] for i in lone])
        assert got[3] is None and len(flooded) == 1
        for k, i in enumerate(lone):
            if k != 3:
                assert_same(got[k], serial[i], "next to the overflowed frame, frame %d" % i)
        passes = det.ragged_passes
        for i, (g, w) in enumerate(zip(det.detect_batch(mixed, mixed_sizes=True), serial)):
            assert_same(g, w, "redone alone, frame %d" % i)
        assert det.ragged_passes - passes == 1 and len(flooded) == 2
    finally:
        del det.pnet                                                                     # the class's own method again
    assert det.host_fallbacks == 0                                                       # (the single-frame call itself did not overflow)


def test_argument_errors(det, mixed):
    from hse_facerec_tf_amd.mtcnn import MTCNNDetector
    with pytest.raises(ValueError, match="device_boxes"):
        MTCNNDetector(minsize=32, device_boxes=False).detect_ragged(mixed[:2])
    with pytest.raises(ValueError, match="uint8"):
        det.detect_ragged([mixed[1], mixed[2].astype(np.float32)])
    with pytest.raises(ValueError):
        det.detect_ragged([mixed[1][:, :, 0]])
    with pytest.raises(ValueError):
        det.detect_batch([mixed[1], mixed[2].astype(np.float32)], mixed_sizes=True)


# ---- process_images ---------------------------------------------------------------------------------------------------------------------
def assert_same_tuple(got, want, what):
    """Every field of process_image's tuple (tests/test_mtcnn_batch_gpu.py)."""
    gb, gp, ga, gg, gf = got
    wb, wp, wa, wg, wf = want
    assert gb == wb, what
    if len(wb) == 0 and np.asarray(wp).size == 0:                          # no detection: the single-frame path's empty shapes vary
        assert np.asarray(gp).size == 0 and ga == [] and gg == [] and gf == [], what
        return
    assert np.array_equal(gp, wp), what
    assert len(ga) == len(wa) == len(gg) == len(wg) == len(gf) == len(wf) == len(wb), what
    for k in range(len(wb)):
        assert ga[k] == wa[k] and np.array_equal(gg[k], wg[k]) and np.array_equal(gf[k], wf[k]), (what, k)


def test_process_images_with_mixed_sizes_equals_a_process_image_loop(mixed):
    from hse_facerec_tf_amd import FacialImageProcessing, preprocess_device
    fip = FacialImageProcessing(mtcnn_detector=True, minsize=32, latency_plan=False)
    try:
        bgr = [np.ascontiguousarray(f[..., ::-1]) for f in mixed]
        assert fip.device_frames_supported()
        for rotation in (0, 90):
            want = [fip.process_image(preprocess_device.turn_frame(f, rotation)) for f in bgr]
            if rotation == 0:
                assert sum(len(t[0]) > 0 for t in want) >= 3 and any(len(t[0]) == 0 for t in want)
            for kw in (dict(), dict(device_crops=True), dict(device_frames=True)):
                passes = fip.detector.ragged_passes
                got = fip.process_images(bgr, rotation=rotation, mixed_sizes=True, **kw)
                assert len(got) == len(want) and fip.detector.ragged_passes - passes == 1, (rotation, kw)
                for i, (g, w) in enumerate(zip(got, want)):
                    assert_same_tuple(g, w, "rotation %d, %r, frame %d" % (rotation, kw, i))
        passes = fip.detector.ragged_passes
        got, crops = fip.process_images(bgr, mixed_sizes=True, device_frames=True, return_crops=True, max_frames=2)
        plain, plain_crops = fip.process_images(bgr, return_crops=True)
        assert fip.detector.ragged_passes - passes == 2                                 # five lone frames, two per pass: 2 + 2, and one alone
        for i, (g, w, c, pc) in enumerate(zip(got, plain, crops, plain_crops)):
            assert_same_tuple(g, w, "max_frames 2, frame %d" % i)
            assert np.array_equal(c, pc), i
        assert fip.detector.host_fallbacks == 0
    finally:
        fip.close()
