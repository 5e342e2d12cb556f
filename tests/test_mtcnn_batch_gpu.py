"""GPU suite: MTCNNDetector.detect_batch and FacialImageProcessing.process_images -- many frames per pass -- against the single-frame
path on each frame alone, bit for bit: same-size frames in one pass, passes of several sizes, permutations and repeats, mixed sizes,
the batch invariance of the nets the batch path relies on, a candidate list that overflows in ONE frame of a pass, and the
argument errors.  The single-frame results are computed once per module and never changed."""
import numpy as np
import pytest

from oracle import pipeline as opl

from conftest import TEST_IMAGE

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def det():
    from hse_facerec_tf_amd.mtcnn import MTCNNDetector
    return MTCNNDetector(minsize=32)


@pytest.fixture(scope="module")
def img():
    return opl.imread_rgb(TEST_IMAGE)


def variants(img):
    """Eight frames of the reference photo's size."""
    h, w = img.shape[:2]
    half = img.copy()
    half[:, w // 2:] = 0                                                   # the faces of the left half only
    tile = np.tile(img[:90, :200], (h // 90 + 1, w // 200 + 1, 1))[:h, :w]  # the face-free corner, tiled
    out = [img, img[:, ::-1], img[::-1], (img * 0.6).astype(np.uint8), np.zeros_like(img), tile, half, np.roll(img, 150, axis=1)]
    return [np.ascontiguousarray(f) for f in out]


@pytest.fixture(scope="module")
def frames(img):
    return variants(img)


@pytest.fixture(scope="module")
def serial(det, frames):
    """The single-frame path on every frame, before anything batched runs."""
    out = [det(f) for f in frames]
    counts = [b.shape[0] for b, _ in out]
    print("faces per frame, one frame at a time:", counts)
    # the frames must exercise the batch path: an empty frame, a full one, and frames whose lists differ in length
    assert min(counts) == 0 and max(counts) >= 4 and len({c for c in counts if c}) >= 2, counts
    assert det.host_fallbacks == 0
    return out


def assert_same(got, want, what=""):
    """One frame's detect_batch result against its single-frame result."""
    gb, gp = got
    wb, wp = want
    n = wb.shape[0]
    assert gb.dtype == np.float64 and gp.dtype == np.float32, what
    if n == 0:
        assert gb.shape == (0, 5) and gp.shape == (10, 0), (what, gb.shape, gp.shape)
        return
    assert gb.shape == (n, 5) and gp.shape == (10, n), (what, gb.shape, gp.shape)
    assert np.array_equal(gb, wb) and np.array_equal(gp, wp), what


def test_batch_equals_frame_by_frame(det, frames, serial):
    got = det.detect_batch(frames)
    assert len(got) == len(frames)
    for i, (g, w) in enumerate(zip(got, serial)):
        assert_same(g, w, "frame %d" % i)
    assert det.host_fallbacks == 0


def test_position_and_batch_size_do_not_matter(det, frames, serial):
    for max_frames in (1, 3, 8):
        for i, (g, w) in enumerate(zip(det.detect_batch(frames, max_frames=max_frames), serial)):
            assert_same(g, w, "max_frames %d, frame %d" % (max_frames, i))
    perm = [5, 2, 7, 0, 6, 3, 1, 4]
    for i, g in zip(perm, det.detect_batch([frames[i] for i in perm])):
        assert_same(g, serial[i], "permuted, frame %d" % i)
    twice = [0, 2, 0, 6, 6, 4, 0]
    for i, g in zip(twice, det.detect_batch([frames[i] for i in twice], max_frames=4)):
        assert_same(g, serial[i], "repeated, frame %d" % i)
    assert det.host_fallbacks == 0


def test_mixed_sizes_come_back_in_list_order(det, img):
    small = np.zeros((20, 500, 3), np.uint8)
    small[5:15, 100:400] = 200
    mixed = [img, img[40:520, 100:700], img[::2, ::2], img[:90, :200], small, img]
    mixed = [np.ascontiguousarray(f) for f in mixed]
    assert det.pyramid_scales(20, 500) == []                              # no level: no launch for that frame
    want = [det(f) for f in mixed]
    assert [b.shape[0] > 0 for b, _ in want] == [True, True, True, False, False, True]
    for max_frames in (32, 1):
        got = det.detect_batch(mixed, max_frames=max_frames)
        for i, (g, w) in enumerate(zip(got, want)):
            assert_same(g, w, "mixed sizes, frame %d" % i)
    assert det.host_fallbacks == 0


def same_bits(a, b):
    a, b = a.cpu().numpy(), b.cpu().numpy()
    return a.dtype == b.dtype == np.float32 and a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def test_the_nets_are_batch_invariant(det, frames):
    """What _detect_pass relies on: a row of a net's output does not depend on the batch it stands in."""
    import torch
    from hse_facerec_tf_amd import _lib
    three = [frames[0], frames[2], frames[6]]
    h, w = three[0].shape[:2]
    stack = torch.from_numpy(np.stack(three)).cuda()
    for scale in (det.pyramid_scales(h, w)[1], det.pyramid_scales(h, w)[5]):
        hs, ws = int(np.ceil(h * scale)), int(np.ceil(w * scale))
        level = torch.empty((3, ws, hs, 3), dtype=torch.float32, device="cuda")
        _lib.check(_lib.lib().hsefr_mtcnn_pyramid_level_batch(stack.data_ptr(), level.data_ptr(), 3, h, w, hs, ws, _lib.current_stream_ptr()),
                   "hsefr_mtcnn_pyramid_level_batch")
        reg_t, prob_t = det.pnet(level)
        assert prob_t.shape[0] == 3 and reg_t.shape[0] == 3
        for b in range(3):
            assert same_bits(level[b], det._level_device(stack[b], h, w, hs, ws)[0]), (scale, b)
            reg_1, prob_1 = det.pnet(level[b:b + 1].contiguous())
            assert same_bits(reg_t[b], reg_1[0]) and same_bits(prob_t[b], prob_1[0]), (scale, b)
    rs = np.random.RandomState(7)
    for net, size in ((det.rnet, 24), (det.onet, 48)):
        crops = torch.from_numpy(rs.uniform(-1, 1, (11, size, size, 3)).astype(np.float32)).cuda()
        outs = net(crops)
        for b in (0, 5, 10):
            for o, o1 in zip(outs, net(crops[b:b + 1].contiguous())):
                assert same_bits(o[b], o1[0]), (size, b)
        for o, o4 in zip(outs, net(crops[3:7].contiguous())):             # ... nor on where the row stands in it
            assert same_bits(o[3:7], o4), size


# ---- overflow in one frame of a pass --------------------------------------------------------------------------------------------------
def flood_pnet_row(det, map_shape, cap, row):
    """Wrap det.pnet (as an instance attribute, as flood_pnet of test_mtcnn_stages_gpu.py does) so that a compact block of more than
    cap cells fires in ONE batch row of the face map of the given [W', H'] shape: ``row`` of a stacked level, the only row of a
    single frame's level.  That frame's level overflows its device list; the rows next to it are what P-Net gave."""
    inner = det.pnet
    bx = 48
    by = cap // bx + 1
    assert bx * by > cap and map_shape[0] >= bx + 10 and map_shape[1] >= by + 10

    def pnet(x):
        reg_t, prob_t = inner(x)
        if tuple(prob_t.shape[1:3]) == tuple(map_shape):
            r = row if prob_t.shape[0] > 1 else 0
            prob_t = prob_t.clone()
            prob_t[r, 5:5 + bx, 5:5 + by, 1] = 0.99
            prob_t[r, 5:5 + bx, 5:5 + by, 0] = 0.01
        return [reg_t, prob_t]
    det.pnet = pnet


def test_overflow_is_per_frame(frames, serial):
    import torch
    from hse_facerec_tf_amd import _lib
    from hse_facerec_tf_amd.mtcnn import MTCNNDetector
    cap = int(_lib.lib().hsefr_mtcnn_post_capacity())
    four = [frames[0], frames[6], frames[2], frames[1]]
    want = [serial[0], serial[6], serial[2], serial[1]]
    h, w = four[0].shape[:2]
    device, host = MTCNNDetector(minsize=32), MTCNNDetector(minsize=32, device_boxes=False)
    scale = device.pyramid_scales(h, w)[0]
    frame = torch.from_numpy(four[1]).cuda()
    map_shape = tuple(device.pnet(device._level_device(frame, h, w, int(np.ceil(h * scale)), int(np.ceil(w * scale))))[1].shape[1:3])
    flood_pnet_row(device, map_shape, cap, 1)
    flood_pnet_row(host, map_shape, cap, 0)
    got = device.detect_batch(four)
    flooded = host(four[1])                                                # the host path with the same flood on its one row
    print("flooded map", map_shape, "fallbacks", device.host_fallbacks, "boxes of the flooded frame", flooded[0].shape)
    assert device.host_fallbacks == 1 and host.host_fallbacks == 0
    for i in (0, 2, 3):
        assert_same(got[i], want[i], "frame %d next to the overflowed one" % i)
    assert flooded[0].shape[0] > 0
    assert_same(got[1], flooded, "the overflowed frame")
    del device.pnet                                                        # the class's own method again
    for i, g in enumerate(device.detect_batch(four)):
        assert_same(g, want[i], "after the flood, frame %d" % i)
    assert device.host_fallbacks == 1


# ---- process_images -------------------------------------------------------------------------------------------------------------------
def assert_same_tuple(got, want, what):
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


def test_process_images_equals_a_process_image_loop(frames):
    from hse_facerec_tf_amd import FacialImageProcessing
    fip = FacialImageProcessing(mtcnn_detector=True, minsize=32, latency_plan=False)
    bgr = [np.ascontiguousarray(frames[i][..., ::-1]) for i in (0, 4, 6, 2, 0)]
    want = [fip.process_image(f) for f in bgr]
    assert [len(t[0]) for t in want][1] == 0 and sum(len(t[0]) for t in want) >= 6
    got = fip.process_images(bgr)
    assert len(got) == len(want)
    for i, (g, w) in enumerate(zip(got, want)):
        assert_same_tuple(g, w, "frame %d" % i)
    for i, (g, w) in enumerate(zip(fip.process_images(bgr, max_frames=2), want)):
        assert_same_tuple(g, w, "max_frames 2, frame %d" % i)
    assert fip.process_images([]) == []
    # a detector that is a plain callable, without detect_batch
    calls = []
    inner = fip.detector

    def plain(rgb):
        calls.append(rgb.shape)
        return inner(rgb)
    fip.detector = plain
    try:
        got = fip.process_images(bgr[:3])
    finally:
        fip.detector = inner
        fip.close()
    assert len(calls) == 3
    for i, (g, w) in enumerate(zip(got, want[:3])):
        assert_same_tuple(g, w, "plain detector, frame %d" % i)


def test_argument_errors(det, frames):
    good = frames[0]
    with pytest.raises(ValueError):
        det.detect_batch([good, good.astype(np.float32)])
    with pytest.raises(ValueError):
        det.detect_batch([good[:, :, 0]])
    with pytest.raises(ValueError):
        det.detect_batch([good], max_frames=0)
    assert det.detect_batch([]) == []
