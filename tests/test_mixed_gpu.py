"""GPU suite: the device stages of a mixed-size pass (libhsefr_mixed.so: preprocess_device.prepare_packed and face_crops_packed,
MTCNNDetector.detect_packed, detect_batch(packed_sources=True), process_images / process_album with mixed_device=True) -- byte for
byte NumPy, the host resize and the same-size libraries, and bit for bit the calls without the flag."""
import numpy as np
import pytest

from oracle import pipeline as opl

from conftest import TEST_IMAGE

pytestmark = pytest.mark.gpu

# offsets mod 4 when packed back to back: 0 0 0 0 0 3 3 0 3 2 0 (tests/test_mixed_cpu.py states which path each frame takes)
SHAPES = [(72, 132), (64, 48), (66, 40), (40, 70), (37, 53), (68, 36), (5, 7), (1, 9), (9, 1), (66, 129), (12, 12)]
TAIL = [(37, 53), (64, 48)]                    # 5033 pixels, not a multiple of 4: the rotation-0 tail
SENTINEL = 0xA5


def expected(x, rotation, swap):
    y = x if rotation == 0 else np.rot90(x, -1 if rotation == 90 else 1)
    return np.ascontiguousarray(y[..., ::-1] if swap else y)


def random_frames(shapes, seed=0):
    rs = np.random.RandomState(seed)
    return [rs.randint(0, 256, (h, w, 3)).astype(np.uint8) for h, w in shapes]


def pack(frames, offsets=None, total=None):
    """The frames in one host buffer at ``offsets`` (default: back to back), SENTINEL everywhere else."""
    from hse_facerec_tf_amd.mtcnn_ragged import packed_offsets
    offsets = packed_offsets([f.shape[:2] for f in frames]) if offsets is None else offsets
    total = int(offsets[-1]) + frames[-1].size if total is None else total
    buf = np.full(total, SENTINEL, np.uint8)
    for f, o in zip(frames, offsets):
        buf[int(o):int(o) + f.size] = f.reshape(-1)
    return buf, [int(o) for o in offsets]


def on_device(host, base=0):
    """The buffer on the device as a view that starts ``base`` bytes into its allocation."""
    import torch
    t = torch.empty(len(host) + base, dtype=torch.uint8, device="cuda")
    t[base:].copy_(torch.from_numpy(host))
    return t[base:]


# ---- prepare ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("swap", [True, False])
@pytest.mark.parametrize("rotation", [0, 90, 270])
def test_prepare_packed_equals_numpy_frame_by_frame(rotation, swap):
    import torch
    from hse_facerec_tf_amd import preprocess_device as pd
    for shapes in (SHAPES, TAIL):
        frames = random_frames(shapes, seed=len(shapes))
        host, offsets = pack(frames)
        for base, in_place in ((0, False), (1, False)) + (((0, True), (1, True)) if rotation == 0 else ()):
            src = on_device(host, base)
            assert src.data_ptr() % 4 == base
            out = pd.prepare_packed(src, shapes, rotation, swap, out=src if in_place else None)
            assert (out.data_ptr() == src.data_ptr()) == in_place and out.shape == src.shape
            got = out.cpu().numpy()
            if not in_place:
                assert np.array_equal(src.cpu().numpy(), host)                          # the source is only read
            for i, (f, o) in enumerate(zip(frames, offsets)):
                want = expected(f, rotation, swap)
                assert np.array_equal(got[o:o + f.size].reshape(want.shape), want), (shapes[i], rotation, swap, base, in_place)
                if base == 0 and not in_place:                                           # and what the same-size library writes for it
                    alone = pd.prepare_frames(torch.from_numpy(f[None]).cuda(), rotation, swap)[0].cpu().numpy()
                    assert np.array_equal(alone, want), shapes[i]


@pytest.mark.parametrize("rotation", [0, 90, 270])
def test_prepare_packed_writes_no_byte_outside_the_frames(rotation):
    """Bytes in front of the first frame, a gap between two frames, back-to-back frames and slack behind the last: SENTINEL before the
    call in the destination, unchanged after it; rows in an order that is not the offsets'."""
    from hse_facerec_tf_amd import preprocess_device as pd
    shapes = [(66, 129), (37, 53), (64, 48), (72, 132), (5, 7)]
    frames = random_frames(shapes, seed=7)
    sizes = [f.size for f in frames]
    o1 = 7                                                                               # seven bytes in front
    o2 = o1 + sizes[1]                                                                   # back to back with frame 1
    o0 = o2 + sizes[2] + 13                                                              # a gap of 13 bytes
    o3 = o0 + sizes[0]                                                                   # back to back
    o4 = o3 + sizes[3] + 1                                                               # a gap of one byte
    offsets = np.array([o0, o1, o2, o3, o4], np.int64)
    host, offsets = pack(frames, offsets, total=o4 + sizes[4] + 29)                      # 29 bytes of slack
    inside = np.zeros(len(host), bool)
    for f, o in zip(frames, offsets):
        inside[o:o + f.size] = True
    for swap in (True, False):
        for in_place in ((False, True) if rotation == 0 else (False,)):
            src = on_device(host)
            out = src if in_place else on_device(np.full(len(host), SENTINEL, np.uint8))
            assert pd.prepare_packed(src, shapes, rotation, swap, out=out, offsets=offsets) is out
            got = out.cpu().numpy()
            assert (got[~inside] == SENTINEL).all(), (rotation, swap, in_place)
            for f, o in zip(frames, offsets):
                want = expected(f, rotation, swap)
                assert np.array_equal(got[o:o + f.size].reshape(want.shape), want), (f.shape, rotation, swap, in_place)
    with pytest.raises(ValueError, match="overlap"):
        pd.prepare_packed(src, shapes, rotation, True, out=out if rotation else None, offsets=[o0, o1, o2 - 1, o3, o4])
    with pytest.raises(ValueError, match="do not fit"):
        pd.prepare_packed(src, shapes, rotation, True, offsets=[o0, o1, o2, o3, o4 + 30])
    if rotation:
        with pytest.raises(ValueError, match="in place"):
            pd.prepare_packed(src, shapes, rotation, True, out=src, offsets=offsets)


def test_offsets_past_two_to_the_31():
    """As the pyramid's test does: 2.2 GB allocated and not filled, the second frame at byte 2 160 000 001 -- a quarter turn of it and one
    crop from the turned frame."""
    import torch
    from hse_facerec_tf_amd import preprocess, preprocess_device as pd
    total, far = 2_200_000_000, 2_160_000_001
    shapes = [(40, 70), (300, 260)]
    frames = random_frames(shapes, seed=3)
    src = torch.empty(total, dtype=torch.uint8, device="cuda")
    out = torch.empty(total, dtype=torch.uint8, device="cuda")
    try:
        for f, o in zip(frames, (0, far)):
            src[o:o + f.size].copy_(torch.from_numpy(f.reshape(-1)))
        out[far - 16:far + frames[1].size + 16] = SENTINEL
        pd.prepare_packed(src, shapes, 90, True, out=out, offsets=[0, far])
        for f, o in zip(frames, (0, far)):
            want = expected(f, 90, True)
            assert np.array_equal(out[o:o + f.size].cpu().numpy().reshape(want.shape), want), o
        assert (out[far - 16:far].cpu().numpy() == SENTINEL).all() and (out[far + frames[1].size:far + frames[1].size + 16].cpu().numpy() == SENTINEL).all()
        turned = expected(frames[1], 90, True)                                           # [260, 300, 3]
        got = pd.face_crops_packed(out, [(70, 40), (260, 300)], [[1, 30, 20, 290, 255]], (224, 224), offsets=[0, far]).cpu().numpy()
        assert np.array_equal(got[0], preprocess.resize_linear_u8(turned[20:255, 30:290], 224, 224))
    finally:
        del src, out
        torch.cuda.empty_cache()


# ---- crops ----------------------------------------------------------------------------------------------------------------------------
CROP_SHAPES = SHAPES + [(300, 260)]
# (frame, x1, y1, x2, y2): rows in no frame order, several per frame, none for frames 2, 3 and 10
BOXES = [(11, 0, 0, 260, 300),          # a whole frame, larger than 224 both ways
         (0, 0, 0, 132, 72),            # a whole frame
         (5, 3, 4, 30, 60),             # a frame on an odd offset
         (4, 10, 10, 11, 11),           # 1 x 1
         (0, 100, 50, 132, 72),         # x2 = w and y2 = h
         (9, 0, 10, 129, 66),           # x1 = 0, x2 = w, y2 = h, odd offset mod 4 = 2
         (11, 20, 30, 250, 290),
         (6, 0, 0, 7, 5),
         (7, 2, 0, 9, 1),               # one row
         (8, 0, 3, 1, 9),               # one column
         (1, 5, 6, 40, 50),
         (0, 1, 1, 50, 40),
         (5, 0, 0, 36, 68)]


@pytest.fixture(scope="module")
def crop_frames():
    frames = random_frames(CROP_SHAPES, seed=11)
    host, offsets = pack(frames)
    assert [o % 4 for o in offsets[:11]] == [0, 0, 0, 0, 0, 3, 3, 0, 3, 2, 0]
    return frames, on_device(host)


@pytest.fixture(scope="module")
def host_crops_224(crop_frames):
    """The reference of the (224, 224) cases, computed once."""
    from hse_facerec_tf_amd import preprocess
    frames, _ = crop_frames
    return np.stack([preprocess.resize_linear_u8(frames[f][y1:y2, x1:x2], 224, 224) for f, x1, y1, x2, y2 in BOXES])


def test_face_crops_packed_equal_the_host_resize_and_the_same_size_library(crop_frames, host_crops_224):
    import torch
    from hse_facerec_tf_amd import preprocess_device as pd
    frames, packed = crop_frames
    got = pd.face_crops_packed(packed, CROP_SHAPES, BOXES, (224, 224))                    # the 16-byte store form
    assert got.data_ptr() % 16 == 0 and tuple(got.shape) == (len(BOXES), 224, 224, 3)
    got = got.cpu().numpy()
    for i, (f, x1, y1, x2, y2) in enumerate(BOXES):
        assert np.array_equal(got[i], host_crops_224[i]), BOXES[i]
        alone = pd.face_crops(torch.from_numpy(frames[f][None]).cuda(), [[0, x1, y1, x2, y2]], (224, 224))[0].cpu().numpy()
        assert np.array_equal(got[i], alone), BOXES[i]
    assert tuple(pd.face_crops_packed(packed, CROP_SHAPES, np.zeros((0, 5), np.int32), (224, 224)).shape) == (0, 224, 224, 3)
    with pytest.raises(ValueError, match="outside the 48 x 64 frame 1"):                  # inside frame 0, outside its own
        pd.face_crops_packed(packed, CROP_SHAPES, [[1, 0, 0, 100, 60]], (8, 8))


def test_face_crops_packed_byte_form_and_slices_of_a_batch(crop_frames):
    import torch
    from hse_facerec_tf_amd import preprocess, preprocess_device as pd
    frames, packed = crop_frames
    m = len(BOXES)
    # (7, 5): 105 bytes per face, the byte form; written into rows 1 .. m of a larger batch
    want = np.stack([preprocess.resize_linear_u8(frames[f][y1:y2, x1:x2], 5, 7) for f, x1, y1, x2, y2 in BOXES])
    batch = torch.full((m + 3, 7, 5, 3), SENTINEL, dtype=torch.uint8, device="cuda")
    assert pd.face_crops_packed(packed, CROP_SHAPES, BOXES, (7, 5), out=batch[1:m + 1]).data_ptr() == batch[1:].data_ptr()
    got = batch.cpu().numpy()
    assert np.array_equal(got[1:m + 1], want) and (got[0] == SENTINEL).all() and (got[m + 1:] == SENTINEL).all()
    # (8, 8): 192 bytes per face, a multiple of 16 -- the vector form on an aligned batch, the byte form on one that starts 8 bytes in
    want = np.stack([preprocess.resize_linear_u8(frames[f][y1:y2, x1:x2], 8, 8) for f, x1, y1, x2, y2 in BOXES])
    assert np.array_equal(pd.face_crops_packed(packed, CROP_SHAPES, BOXES, (8, 8)).cpu().numpy(), want)
    flat = torch.full((m * 192 + 32,), SENTINEL, dtype=torch.uint8, device="cuda")
    out = flat[8:8 + m * 192].view(m, 8, 8, 3)
    assert out.data_ptr() % 16 == 8
    pd.face_crops_packed(packed, CROP_SHAPES, BOXES, (8, 8), out=out)
    got = flat.cpu().numpy()
    assert np.array_equal(got[8:8 + m * 192].reshape(m, 8, 8, 3), want) and (got[:8] == SENTINEL).all() and (got[8 + m * 192:] == SENTINEL).all()
    with pytest.raises(ValueError, match="out must be"):
        pd.face_crops_packed(packed, CROP_SHAPES, BOXES, (8, 8), out=batch)


# ---- the detector ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def det():
    from hse_facerec_tf_amd.mtcnn import MTCNNDetector
    return MTCNNDetector(minsize=32)


@pytest.fixture(scope="module")
def mixed():
    """The frames of tests/test_mtcnn_ragged_gpu.py: six cut-outs of the reference photo (one size twice, one without a pyramid level),
    the photo transposed and an all-black 300 x 400 frame."""
    img = opl.imread_rgb(TEST_IMAGE)
    small = np.zeros((20, 500, 3), np.uint8)
    small[5:15, 100:400] = 200
    out = [img, img[40:520, 100:700], img[::2, ::2], img[:90, :200], small, img, np.transpose(img, (1, 0, 2)), np.zeros((300, 400, 3), np.uint8)]
    return [np.ascontiguousarray(f) for f in out]


@pytest.fixture(scope="module")
def serial(det, mixed):
    out = [det(f) for f in mixed]
    counts = [b.shape[0] for b, _ in out]
    assert sum(c > 0 for c in counts) >= 3 and det.host_fallbacks == 0, counts
    return out


def assert_same(got, want, what=""):
    gb, gp = got
    wb, wp = want
    n = wb.shape[0]
    assert gb.dtype == np.float64 and gp.dtype == np.float32, what
    if n == 0:
        assert gb.shape == (0, 5) and gp.shape == (10, 0), (what, gb.shape, gp.shape)
        return
    assert gb.shape == (n, 5) and gp.shape == (10, n), (what, gb.shape, gp.shape)
    assert np.array_equal(gb.view(np.uint64), wb.view(np.uint64)) and np.array_equal(gp.view(np.uint32), wp.view(np.uint32)), what


def test_detect_packed_equals_detect_ragged_and_the_single_frame_calls(det, mixed, serial):
    import torch
    from hse_facerec_tf_amd.mtcnn_ragged import PackedFrames
    shapes = [f.shape[:2] for f in mixed]
    packed = PackedFrames(torch.from_numpy(np.concatenate([f.reshape(-1) for f in mixed])).cuda(), shapes)
    got, ragged = det.detect_packed(packed), det.detect_ragged(mixed)
    assert len(got) == len(mixed)
    for i, (g, r, w) in enumerate(zip(got, ragged, serial)):
        assert_same(g, r, "against detect_ragged, frame %d" % i)
        assert_same(g, w, "against the single-frame call, frame %d" % i)
    for i, f in enumerate(mixed):
        assert np.array_equal(packed.frame(i).cpu().numpy(), f), i
    assert det.detect_packed(PackedFrames(packed.data, [])) == []
    no_level = det.detect_packed(PackedFrames(packed.data, [(20, 500), (12, 12)]))
    assert [(b.shape, p.shape) for b, p in no_level] == [((0, 5), (10, 0))] * 2
    with pytest.raises(ValueError, match="PackedFrames"):
        det.detect_packed(packed.data)
    with pytest.raises(ValueError, match="on the device"):
        det.detect_packed(PackedFrames(packed.data.cpu(), shapes))
    from hse_facerec_tf_amd.mtcnn import MTCNNDetector
    with pytest.raises(ValueError, match="device_boxes"):
        MTCNNDetector(minsize=32, device_boxes=False).detect_packed(packed)
    assert det.host_fallbacks == 0


def test_detect_batch_hands_back_the_packed_buffer_of_a_ragged_pass(det, mixed, serial):
    from hse_facerec_tf_amd.mtcnn_ragged import PackedFrames
    passes, in_passes = det.ragged_passes, det.ragged_frames
    got, sources = det.detect_batch(mixed, mixed_sizes=True, return_stacks=True, packed_sources=True)
    assert det.ragged_passes - passes == 1 and det.ragged_frames - in_passes == 5
    for i, (g, w) in enumerate(zip(got, serial)):
        assert_same(g, w, "frame %d" % i)
    # the same-size pair keeps its stack, the frame without a level has no source, the five of the ragged pass share ONE PackedFrames
    kinds = ["stack", "packed", "packed", "packed", None, "stack", "packed", "packed"]
    for i, (s, kind) in enumerate(zip(sources, kinds)):
        if kind is None:
            assert s is None
        elif kind == "stack":
            assert not isinstance(s[0], PackedFrames) and np.array_equal(s[0][s[1]].cpu().numpy(), mixed[i])
        else:
            assert isinstance(s[0], PackedFrames) and s[0].data.is_cuda and np.array_equal(s[0].frame(s[1]).cpu().numpy(), mixed[i]), i
    ragged = [s for s, kind in zip(sources, kinds) if kind == "packed"]
    assert all(s[0] is ragged[0][0] for s in ragged) and [s[1] for s in ragged] == [0, 1, 2, 3, 4]
    assert ragged[0][0].shapes == tuple(mixed[i].shape[:2] for i in (1, 2, 3, 6, 7))
    # without the keyword the sources of a ragged pass stay None
    _, sources = det.detect_batch(mixed, mixed_sizes=True, return_stacks=True)
    assert [s is not None for s in sources] == [True, False, False, False, False, True, False, False]


# ---- process_images ---------------------------------------------------------------------------------------------------------------------
def assert_same_tuple(got, want, what):
    """Every field of process_image's tuple (tests/test_mtcnn_ragged_gpu.py)."""
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


@pytest.fixture(scope="module")
def fip():
    from hse_facerec_tf_amd import FacialImageProcessing
    f = FacialImageProcessing(mtcnn_detector=True, minsize=32, latency_plan=False)
    yield f
    f.close()


@pytest.fixture(scope="module")
def bgr(mixed):
    return [np.ascontiguousarray(f[..., ::-1]) for f in mixed]


@pytest.fixture(scope="module")
def loop(fip, bgr):
    """The process_image loop per rotation, computed once and before any pass that is tampered with."""
    from hse_facerec_tf_amd import preprocess_device
    out = {rotation: [fip.process_image(preprocess_device.turn_frame(f, rotation)) for f in bgr] for rotation in (0, 90, 270)}
    assert sum(len(t[0]) > 0 for t in out[0]) >= 3 and any(len(t[0]) == 0 for t in out[0])
    return out


@pytest.mark.parametrize("rotation", [0, 90, 270])
def test_process_images_with_mixed_device_equals_a_process_image_loop(fip, bgr, loop, rotation, monkeypatch):
    from hse_facerec_tf_amd import preprocess_device
    want = loop[rotation]
    host_turns = []
    turn = preprocess_device.turn_frame
    monkeypatch.setattr(preprocess_device, "turn_frame", lambda f, r: (host_turns.append(f.shape), turn(f, r))[1])
    uploads = []
    resize_groups = preprocess_device.preprocess_faces_cv
    monkeypatch.setattr(preprocess_device, "preprocess_faces_cv", lambda crops, *a, **kw: (uploads.append(len(crops)), resize_groups(crops, *a, **kw))[1])
    for kw in (dict(device_crops=True), dict(device_frames=True)):
        del host_turns[:], uploads[:]
        passes, in_passes = fip.detector.ragged_passes, fip.detector.ragged_frames
        got = fip.process_images(bgr, rotation=rotation, mixed_sizes=True, mixed_device=True, **kw)
        counted = (fip.detector.ragged_passes - passes, fip.detector.ragged_frames - in_passes)
        assert len(got) == len(want) and counted == (1, 5), (rotation, kw)
        for i, (g, w) in enumerate(zip(got, want)):
            assert_same_tuple(g, w, "rotation %d, %r, frame %d" % (rotation, kw, i))
        assert uploads == [], (rotation, kw)                                             # no crop cut on the host and uploaded
        if "device_frames" in kw:
            assert host_turns == [], (rotation, kw)                                      # no frame turned (or converted) on the host
        # the same call without the flag counts its passes the same way
        passes, in_passes = fip.detector.ragged_passes, fip.detector.ragged_frames
        plain = fip.process_images(bgr, rotation=rotation, mixed_sizes=True, **kw)
        assert (fip.detector.ragged_passes - passes, fip.detector.ragged_frames - in_passes) == counted
        for i, (g, w) in enumerate(zip(got, plain)):
            assert_same_tuple(g, w, "against the call without the flag, rotation %d, %r, frame %d" % (rotation, kw, i))
    assert fip.detector.host_fallbacks == 0


def test_process_images_with_mixed_device_crops_and_several_passes(fip, bgr, loop):
    plain, plain_crops = fip.process_images(bgr, return_crops=True)
    for kw in (dict(device_crops=True), dict(device_frames=True)):
        passes = fip.detector.ragged_passes
        got, crops = fip.process_images(bgr, mixed_sizes=True, mixed_device=True, return_crops=True, max_frames=2, **kw)
        assert fip.detector.ragged_passes - passes == 2, kw                              # five lone frames, two per pass: 2 + 2, and one alone
        for i, (g, w, p, c, pc) in enumerate(zip(got, loop[0], plain, crops, plain_crops)):
            assert_same_tuple(g, w, "max_frames 2, %r, frame %d" % (kw, i))
            assert_same_tuple(g, p, "max_frames 2 against the plain call, %r, frame %d" % (kw, i))
            assert c.dtype == np.uint8 and np.array_equal(c, pc), (kw, i)
    with pytest.raises(ValueError, match="mixed_sizes"):
        fip.process_images(bgr, device_frames=True, mixed_device=True)
    with pytest.raises(ValueError, match="device_crops=True or device_frames=True"):
        fip.process_images(bgr, mixed_sizes=True, mixed_device=True)
    assert fip.detector.host_fallbacks == 0


def test_an_overflowed_frame_is_read_back_from_the_prepared_buffer_and_redone_alone(fip, bgr, loop, monkeypatch):
    """P-Net's face map of ONE item of the ragged pass is flooded, as tests/test_mtcnn_ragged_gpu.py floods it: by replacing det.pnet,
    between the net and stage 1.  detect_packed hands that frame back as None; process_images reads its bytes back from the buffer
    prepare_packed wrote -- the host never converted that frame -- and the single-frame call, which sees the unflooded map, gives the
    serial result."""
    from hse_facerec_tf_amd import _lib
    from hse_facerec_tf_amd.mtcnn_ragged import PackedFrames, RaggedMaps
    det = fip.detector
    cap = int(_lib.lib().hsefr_mtcnn_post_capacity())
    inner, flooded, read_back = det.pnet, [], []

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
    frame_of = PackedFrames.frame
    monkeypatch.setattr(PackedFrames, "frame", lambda self, i: (read_back.append((self.shapes[i], i)), frame_of(self, i))[1])
    det.pnet = pnet
    try:
        for rotation in (0, 90):
            del flooded[:], read_back[:]
            got = fip.process_images(bgr, rotation=rotation, mixed_sizes=True, device_frames=True, mixed_device=True)
            turned = (bgr[6].shape[1], bgr[6].shape[0]) if rotation else bgr[6].shape[:2]
            assert len(flooded) == 1 and read_back == [(turned, 3)], (rotation, flooded, read_back)
            for i, (g, w) in enumerate(zip(got, loop[rotation])):
                assert_same_tuple(g, w, "rotation %d, frame %d" % (rotation, i))
    finally:
        del det.pnet                                                                     # the class's own method again
    assert det.host_fallbacks == 0


# ---- the album --------------------------------------------------------------------------------------------------------------------------
def test_process_album_with_mixed_device_equals_it_without():
    """Eight photos of eight sizes: one is found only after a quarter turn, one is blank."""
    import time
    from hse_facerec_tf_amd import FacialImageProcessing, album
    photo = opl.imread_rgb(TEST_IMAGE)
    rgb = [photo, photo[40:520, 100:700], photo[::2, ::2], photo[:500, :700], photo[20:, 30:], photo[:, 50:750],
           np.rot90(photo, 1), np.zeros((300, 400, 3), np.uint8)]
    photos = [np.ascontiguousarray(f[..., ::-1]) for f in rgb]
    assert len({f.shape for f in photos}) == 8
    mdates = [time.gmtime(1.6e9 + i * 17 * 3600) for i in range(len(photos))]
    fip = FacialImageProcessing(mtcnn_detector=True, minsize=32, latency_plan=False)
    try:
        results, counted = [], []
        for mixed_device in (False, True):
            passes, in_passes = fip.detector.ragged_passes, fip.detector.ragged_frames
            results.append(album.process_album(fip, photos, mdates, mixed_sizes=True, mixed_device=mixed_device))
            counted.append((fip.detector.ragged_passes - passes, fip.detector.ragged_frames - in_passes))
        want, got = results
        assert counted[0] == counted[1] and counted[0][0] >= 2, counted                  # the first pass and at least one retry pass
        assert 6 in want.all_indices and 7 not in want.all_indices                       # found after its turn; the blank photo never
        assert want.all_indices.count(0) >= 1 and len(want.clusters) >= 1
        assert type(got) is type(want)
        for name, g, w in zip(want._fields, got, want):
            if name == "facial_images":
                assert len(g) == len(w) and all(np.array_equal(a, b) for a, b in zip(g, w))
            else:
                assert g == w, name
        assert fip.detector.host_fallbacks == 0
    finally:
        fip.close()
