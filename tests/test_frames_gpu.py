"""GPU suite: the frame front end on the device -- hsefr_frames_prepare byte for byte against NumPy (np.rot90 and a channel reversal)
with sentinels around the output, MTCNNDetector.detect_stack against detect_batch, process_images(device_frames=True) against the host
path at every rotation, and process_album / process_video with device_frames=True against device_frames=False.  The host results are
computed once per module and never changed."""
import calendar
import time

import numpy as np
import pytest

from oracle import pipeline as opl

from conftest import TEST_IMAGE

pytestmark = pytest.mark.gpu

DAY = 86400
T0 = calendar.timegm((2019, 3, 4, 10, 0, 0))
TURNS = {0: 0, 90: -1, 270: 1}                      # rotation (degrees clockwise) -> np.rot90's k
SENTINEL = 0xA5


# ---- the kernel ----------------------------------------------------------------------------------------------------------------------
def expected(x, rotation, swap_rb):
    want = np.rot90(x, TURNS[rotation], axes=(1, 2))
    return np.ascontiguousarray(want[..., ::-1] if swap_rb else want)


def carve(flat, offset, shape):
    """A contiguous uint8 tensor of ``shape`` that starts ``offset`` bytes into the 1-D buffer ``flat``."""
    size = int(np.prod(shape))
    return flat[offset:offset + size].view(shape)


# whole and partial tiles in both directions; rows of 15 (3, 5), 189 (65, 63) and 201 (67 x 130 turned, 130 x 67) bytes; frames of 45
# bytes, so that frame 1 starts at an odd address; (2, 300): more tiles than rows; (1, 1): one pixel
SHAPES = [(1, 1), (3, 5), (64, 64), (65, 63), (67, 130), (130, 67), (2, 300)]


@pytest.mark.parametrize("hw", SHAPES, ids=lambda hw: "%dx%d" % hw)
def test_prepare_equals_numpy_byte_for_byte_and_writes_only_its_output(hw):
    import torch
    from hse_facerec_tf_amd import preprocess_device
    h, w = hw
    rng = np.random.RandomState(100 * h + w)
    for n in (1, 3):
        x = rng.randint(0, 256, (n, h, w, 3)).astype(np.uint8)
        size = x.size
        # the source once on an allocation boundary and once at an odd address
        holder = torch.full((size + 8,), SENTINEL, dtype=torch.uint8, device="cuda")
        sources = [torch.from_numpy(x).cuda(), carve(holder, 1, x.shape)]
        sources[1].copy_(sources[0])
        for rotation in (0, 90, 270):
            shape = (n, h, w, 3) if rotation == 0 else (n, w, h, 3)
            for swap_rb in (0, 1):
                want = expected(x, rotation, swap_rb)
                assert want.shape == shape
                for s, src in enumerate(sources):
                    # the output in the middle of sentinel bytes: at a 4-byte boundary, at an odd address, at an even one that is no
                    # multiple of 4
                    for offset in (64, 61, 62):
                        flat = torch.full((size + 128,), SENTINEL, dtype=torch.uint8, device="cuda")
                        out = carve(flat, offset, shape)
                        assert out.data_ptr() % 4 == offset % 4 and src.data_ptr() % 4 == s
                        got = preprocess_device.prepare_frames(src, rotation=rotation, swap_rb=bool(swap_rb), out=out)
                        assert got is out
                        f = flat.cpu().numpy()
                        case = (n, rotation, swap_rb, s, offset)
                        assert (f[:offset] == SENTINEL).all() and (f[offset + size:] == SENTINEL).all(), case
                        assert np.array_equal(f[offset:offset + size].reshape(shape), want), case
                    fresh = preprocess_device.prepare_frames(src, rotation=rotation, swap_rb=bool(swap_rb))
                    again = preprocess_device.prepare_frames(src, rotation=rotation, swap_rb=bool(swap_rb))
                    assert tuple(fresh.shape) == shape and fresh.dtype == torch.uint8
                    assert torch.equal(fresh, again) and np.array_equal(fresh.cpu().numpy(), want)      # two runs: equal bytes
                    assert np.array_equal(src.cpu().numpy(), x)                                        # the source is read only
                # in place at rotation 0
                for s, src in enumerate(sources if rotation == 0 else []):
                    flat = torch.full((size + 128,), SENTINEL, dtype=torch.uint8, device="cuda")
                    stack = carve(flat, 64 + s, x.shape)
                    stack.copy_(src)
                    assert preprocess_device.prepare_frames(stack, swap_rb=bool(swap_rb), out=stack) is stack
                    f = flat.cpu().numpy()
                    assert (f[:64 + s] == SENTINEL).all() and (f[64 + s + size:] == SENTINEL).all()
                    assert np.array_equal(f[64 + s:64 + s + size].reshape(x.shape), expected(x, 0, swap_rb)), (n, swap_rb, s)
        assert (holder.cpu().numpy()[[0] + list(range(size + 1, size + 8))] == SENTINEL).all()


def test_prepare_frames_defaults_slices_and_refusals():
    import torch
    from hse_facerec_tf_amd import preprocess_device
    x = np.random.RandomState(3).randint(0, 256, (4, 12, 20, 3)).astype(np.uint8)
    stack = torch.from_numpy(x).cuda()
    assert np.array_equal(preprocess_device.prepare_frames(stack).cpu().numpy(), x[..., ::-1])        # the defaults: BGR -> RGB, upright
    # into a slice of a larger tensor
    batch = torch.full((6, 20, 12, 3), 7, dtype=torch.uint8, device="cuda")
    preprocess_device.prepare_frames(stack, rotation=270, swap_rb=False, out=batch[1:5])
    b = batch.cpu().numpy()
    assert (b[0] == 7).all() and (b[5] == 7).all() and np.array_equal(b[1:5], expected(x, 270, 0))
    empty = preprocess_device.prepare_frames(stack[:0], rotation=90)
    assert tuple(empty.shape) == (0, 20, 12, 3)
    for kw in (dict(rotation=90, out=torch.empty((4, 12, 20, 3), dtype=torch.uint8, device="cuda")),     # not the turned shape
               dict(out=torch.empty((3, 12, 20, 3), dtype=torch.uint8, device="cuda")),
               dict(out=torch.empty((4, 12, 20, 3), dtype=torch.uint8)),                                 # on the host
               dict(out=torch.empty((4, 12, 20, 3), dtype=torch.int8, device="cuda")),
               dict(out=torch.empty((4, 12, 40, 3), dtype=torch.uint8, device="cuda")[:, :, ::2]),       # not contiguous
               dict(rotation=180), dict(rotation=45)):
        with pytest.raises(ValueError):
            preprocess_device.prepare_frames(stack, **kw)
    square = torch.from_numpy(np.ascontiguousarray(x[:, :, :12])).cuda()
    with pytest.raises(ValueError, match="in place"):
        preprocess_device.prepare_frames(square, rotation=90, out=square)                             # a quarter turn of a stack onto itself
    for bad in (stack.cpu(), stack.float(), stack[0], stack[:, ::2]):
        with pytest.raises(ValueError):
            preprocess_device.prepare_frames(bad)
    assert np.array_equal(stack.cpu().numpy(), x)


def test_frame_offsets_past_two_to_the_31():
    """The frame offset is 64-bit: 61 frames of 36 MB, so that the last one starts 2.16e9 bytes into each stack.  Only the first and the
    last frame hold data (two 36 MB uploads; the rest of the source is cleared, the destination is not even filled) and only they are
    read back and compared with NumPy: a quarter turn out of place, then rotation 0 in place."""
    import torch
    from hse_facerec_tf_amd import preprocess_device
    n, h, w = 61, 3000, 4000
    assert (n - 1) * h * w * 3 > 2 ** 31 > h * w * 3
    ends = np.random.RandomState(5).randint(0, 256, (2, h, w, 3)).astype(np.uint8)
    stack = torch.zeros((n, h, w, 3), dtype=torch.uint8, device="cuda")
    stack[0].copy_(torch.from_numpy(ends[0]))
    stack[n - 1].copy_(torch.from_numpy(ends[1]))
    got = preprocess_device.prepare_frames(stack, rotation=90)
    assert np.array_equal(torch.stack([got[0], got[n - 1]]).cpu().numpy(), expected(ends, 90, 1))
    del got
    assert preprocess_device.prepare_frames(stack, out=stack) is stack
    assert np.array_equal(torch.stack([stack[0], stack[n - 1]]).cpu().numpy(), expected(ends, 0, 1))
    assert not bool(stack[1:n - 1].any())                                              # and nothing spilled into the frames between


# ---- the frames of the pipeline tests ------------------------------------------------------------------------------------------------
def same_size_variants(img):
    """Eight frames of the reference photo's size: the photo, mirrored, upside down, dimmed, black, its face-free corner tiled, its left
    half alone, shifted."""
    h, w = img.shape[:2]
    half = img.copy()
    half[:, w // 2:] = 0
    tile = np.tile(img[:90, :200], (h // 90 + 1, w // 200 + 1, 1))[:h, :w]
    out = [img, img[:, ::-1], img[::-1], (img * 0.6).astype(np.uint8), np.zeros_like(img), tile, half, np.roll(img, 150, axis=1)]
    return [np.ascontiguousarray(f) for f in out]


@pytest.fixture(scope="module")
def fip():
    from hse_facerec_tf_amd import FacialImageProcessing
    return FacialImageProcessing(mtcnn_detector=True, minsize=32, latency_plan=False)


@pytest.fixture(scope="module")
def photo():
    return opl.imread_rgb(TEST_IMAGE)


@pytest.fixture(scope="module")
def rgb_frames(photo):
    return same_size_variants(photo)


@pytest.fixture(scope="module")
def frames(photo, rgb_frames):
    """BGR, as cv2.imread gives them: the eight same-size variants, then one frame of another size (alone in its group)."""
    return [np.ascontiguousarray(f[..., ::-1]) for f in rgb_frames + [np.ascontiguousarray(photo[40:520, 100:700])]]


@pytest.fixture(scope="module")
def host_path(fip, frames):
    out, crops = fip.process_images(frames, return_crops=True)
    counts = [len(r[0]) for r in out]
    print("faces per frame:", counts)
    # otherwise the comparisons are empty: a frame with four or more faces, one with none, and a face in the lone frame
    assert max(counts[:8]) >= 4 and min(counts[:8]) == 0 and counts[8] > 0, counts
    return out, crops


def stored_turned(frames, rotation):
    """The frames as a camera held sideways stores them: turning them by ``rotation`` gives ``frames`` back."""
    return [np.ascontiguousarray(np.rot90(f, -TURNS[rotation])) for f in frames]


def assert_same_results(got, want):
    """Boxes, points and ages equal; genders and features the same bits."""
    assert len(got) == len(want)
    for i, (g, w) in enumerate(zip(got, want)):
        assert g[0] == w[0], i                                                         # boxes: lists of ints
        assert np.array_equal(np.asarray(g[1]), np.asarray(w[1])), i                   # points
        assert len(g[2]) == len(w[2]) == len(g[3]) == len(g[4]) == len(w[0])
        for a, b in zip(g[2], w[2]):
            assert a == b, i                                                           # ages
        for k in (3, 4):                                                               # genders, features
            for a, b in zip(g[k], w[k]):
                assert a.dtype == b.dtype == np.float32 and np.array_equal(a.view(np.uint32), b.view(np.uint32)), (i, k)


def assert_same_crops(got, want):
    assert len(got) == len(want)
    for a, b in zip(got, want):
        assert a.dtype == b.dtype == np.uint8 and a.shape == b.shape and np.array_equal(a, b)


# ---- detect_stack --------------------------------------------------------------------------------------------------------------------
def test_detect_stack_equals_detect_batch(fip, rgb_frames):
    import torch
    det = fip.detector
    want = det.detect_batch(rgb_frames)
    assert max(b.shape[0] for b, _ in want) >= 4 and min(b.shape[0] for b, _ in want) == 0
    stack = torch.from_numpy(np.stack(rgb_frames)).cuda()
    got = det.detect_stack(stack)
    assert len(got) == len(want) == 8 and all(r is not None for r in got)
    for (gb, gp), (wb, wp) in zip(got, want):
        assert gb.dtype == wb.dtype and gp.dtype == wp.dtype and gb.shape == wb.shape and gp.shape == wp.shape
        assert np.array_equal(gb.view(np.uint64), wb.view(np.uint64)) and np.array_equal(gp.view(np.uint32), wp.view(np.uint32))
    assert np.array_equal(stack.cpu().numpy(), np.stack(rgb_frames))                   # the stack is read only
    tiny = det.detect_stack(torch.zeros((2, 8, 8, 3), dtype=torch.uint8, device="cuda"))            # no pyramid level: no launch
    assert [(b.shape, p.shape) for b, p in tiny] == [((0, 5), (10, 0))] * 2
    assert det.detect_stack(stack[:0]) == []
    for bad in (stack.cpu(), stack.float(), stack[0], stack[:, ::2]):
        with pytest.raises(ValueError):
            det.detect_stack(bad)


# ---- process_images ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rotation", [0, 90, 270])
def test_process_images_with_device_frames_equals_the_host_path(fip, frames, host_path, rotation, monkeypatch):
    from hse_facerec_tf_amd import preprocess_device
    want, want_crops = host_path
    given = stored_turned(frames, rotation)
    if rotation:
        # the host side: every frame turned on the host, then the host path
        host, host_crops = fip.process_images([np.ascontiguousarray(np.rot90(f, TURNS[rotation])) for f in given], return_crops=True)
        assert_same_results(host, want)                                                # (the same frames again)
        assert_same_results(fip.process_images(given, rotation=rotation), want)        # the host turn inside process_images
    else:
        host, host_crops = want, want_crops
    converted, prepared = [], []
    real_convert, real_prepare = type(fip)._bgr_to_rgb, preprocess_device.prepare_frames
    monkeypatch.setattr(fip, "_bgr_to_rgb", lambda d: (converted.append(np.asarray(d).shape), real_convert(d))[1])
    monkeypatch.setattr(preprocess_device, "prepare_frames",
                        lambda s, *a, **k: (prepared.append((tuple(s.shape), a, k.get("out") is s)), real_prepare(s, *a, **k))[1])
    got, crops = fip.process_images(given, device_frames=True, return_crops=True, rotation=rotation)
    # one launch for the pass of eight; the host converted exactly one frame, the lone one, already turned
    raw_shape = given[0].shape
    assert converted == [frames[8].shape], converted
    assert prepared == [((8,) + raw_shape, (rotation, True), rotation == 0)], prepared                # in place where nothing turns
    assert_same_results(got, host)
    assert_same_crops(crops, host_crops)
    assert_same_results(fip.process_images(given, device_frames=True, rotation=rotation), host)
    del converted[:], prepared[:]
    assert_same_results(fip.process_images(given, max_frames=3, device_frames=True, rotation=rotation), host)
    assert [p[0][0] for p in prepared] == [3, 3, 2] and len(converted) == 1            # passes of 3, 3 and 2; the lone frame
    # sizes that alternate: the faces of the same-size pass do not stand together in the batch
    mixed = [given[0], given[8], given[3], given[4]]
    assert_same_results(fip.process_images(mixed, device_frames=True, rotation=rotation), [host[0], host[8], host[3], host[4]])
    assert fip.process_images([], device_frames=True, return_crops=True, rotation=rotation) == ([], [])
    assert fip.process_images([], device_frames=True, rotation=rotation) == []


def test_passes_are_planned_on_the_turned_size(fip, frames, host_path, monkeypatch):
    """Portrait and landscape frames in one call: the passes and their stacks have the TURNED size.  (One rotation holds for every frame
    of a call, so two frames have the same size after the turn exactly when they have it before: a portrait and a landscape frame
    never share a pass, at any rotation -- each pair here runs as a pass of its own.)"""
    import torch
    want, _ = host_path
    upright = [frames[0], frames[6]]                                                   # 588 x 784
    sideways = stored_turned([frames[3], frames[7]], 270)                              # 784 x 588, upright after a quarter turn counter-clockwise
    given = [upright[0], sideways[0], upright[1], sideways[1]]
    stacks = []
    real = fip.detector.detect_stack
    monkeypatch.setattr(fip.detector, "detect_stack", lambda s: (stacks.append(tuple(s.shape)), real(s))[1])
    got = fip.process_images(given, device_frames=True, rotation=270)
    h, w = frames[0].shape[:2]
    assert stacks == [(2, w, h, 3), (2, h, w, 3)], stacks
    assert_same_results([got[1], got[3]], [want[3], want[7]])
    assert_same_results(got, fip.process_images(given, rotation=270))


def test_a_frame_whose_list_overflows_is_read_back_from_the_prepared_stack(fip, frames, host_path, monkeypatch):
    from hse_facerec_tf_amd import preprocess_device
    want, want_crops = host_path
    given = stored_turned(frames, 90)
    real = fip.detector.detect_stack

    def overflowing(stack):
        res = real(stack)
        res[0], res[6] = None, None                                                    # as a pass reports an overflow
        return res
    monkeypatch.setattr(fip.detector, "detect_stack", overflowing)
    host_crop_calls = []
    real_host = preprocess_device.preprocess_faces_cv
    monkeypatch.setattr(preprocess_device, "preprocess_faces_cv", lambda crops, *a, **k: (host_crop_calls.append(len(crops)),
                                                                                         real_host(crops, *a, **k))[1])
    got, crops = fip.process_images(given, device_frames=True, return_crops=True, rotation=90)
    assert_same_results(got, want)
    assert_same_crops(crops, want_crops)
    assert host_crop_calls == [len(want[0][0]) + len(want[6][0]) + len(want[8][0])]       # their faces were cut on the host


def test_device_frames_need_the_byte_path(fip, frames, monkeypatch):
    with monkeypatch.context() as m:
        m.setattr(fip, "device_preprocess", False)
        with pytest.raises(ValueError, match="device_frames"):
            fip.process_images(frames[:2], device_frames=True)
    with monkeypatch.context() as m:
        m.setattr(fip, "detector", lambda img: None)                                   # a detector without detect_stack
        with pytest.raises(ValueError, match="device_frames"):
            fip.process_images(frames[:2], device_frames=True)
    with pytest.raises(ValueError, match="rotation"):
        fip.process_images(frames[:2], device_frames=True, rotation=180)


def test_a_detector_without_device_boxes_keeps_the_host_frames(fip, frames, monkeypatch):
    """An MTCNNDetector without device_boxes has detect_stack but no batched path: device_frames=True is refused before anything is
    uploaded, and the album's default resolves to the host frames, as before the device frames existed."""
    from hse_facerec_tf_amd import album, preprocess_device
    from hse_facerec_tf_amd.mtcnn import MTCNNDetector
    monkeypatch.setattr(fip, "detector", MTCNNDetector(minsize=32, device_boxes=False))
    assert hasattr(fip.detector, "detect_stack") and not fip.device_frames_supported()
    monkeypatch.setattr(preprocess_device, "prepare_frames", lambda *a, **k: pytest.fail("prepare_frames was reached"))
    monkeypatch.setattr(fip.detector, "detect_stack", lambda *a, **k: pytest.fail("detect_stack was reached"))
    with pytest.raises(ValueError, match="device_frames"):
        fip.process_images(frames[:2], device_frames=True)
    with pytest.raises(ValueError, match="device_frames"):
        album.process_album(fip, frames[:2], [time.gmtime(T0)] * 2, device_frames=True)
    photos = [frames[0], frames[3], frames[4], frames[6]] + stored_turned([frames[0]], 90)
    mdates = [time.gmtime(T0 + i * 30 * 3600) for i in range(len(photos))]
    seen = []
    real = fip.process_images
    monkeypatch.setattr(fip, "process_images", lambda draws, **kw: (seen.append(kw["device_frames"]), real(draws, **kw))[1])
    unasked = album.process_album(fip, photos, mdates)                                 # None: resolves to the host frames
    want = album.process_album(fip, photos, mdates, device_frames=False)
    assert seen and not any(seen)
    assert len(want.all_indices) >= 8 and unasked.all_indices == want.all_indices and unasked.clusters == want.clusters
    assert (unasked.private_photos, unasked.public_photos) == (want.private_photos, want.public_photos)
    assert_same_crops(unasked.facial_images, want.facial_images)
    video = album.process_video(fip, [frames[0]] * 6, mdates[0], config=album.AlbumConfig()._replace(min_frames=1))
    assert video.processed_indices == [4, 5] and video.video_has_faces and not any(seen)


# ---- the album and the video ---------------------------------------------------------------------------------------------------------
def test_process_album_with_device_frames_equals_the_host_frames(fip, frames, photo, monkeypatch):
    from hse_facerec_tf_amd import album
    config = album.AlbumConfig()
    # twelve photos: the eight upright variants (two of them blank: black, and the face-free corner tiled), two stored a quarter turn
    # counter-clockwise (upright after pass 2's turn clockwise) and two stored a quarter turn clockwise (pass 3).  The detector finds a
    # face or two in most variants lying on their side or standing on their head, which ends the retries early; the photo's right
    # half and its lower half alone give none that way (measured), so these two reach pass 3
    h, w = photo.shape[:2]
    right, lower = photo.copy(), photo.copy()
    right[:, :w // 2] = 0
    lower[:h // 2] = 0
    late = [np.ascontiguousarray(f[..., ::-1]) for f in (right, lower)]
    photos = frames[:8] + stored_turned([frames[0], frames[3]], 90) + stored_turned(late, 270)
    mdates = [time.gmtime(T0 + i * 17 * 3600) for i in range(len(photos))]
    found_in = {}
    real = fip.process_images

    def recording(draws, **kw):
        out = real(draws, **kw)
        found_in.setdefault((kw["device_frames"], kw["rotation"]), []).append(sum(1 for r in out[0] if len(r[0])))
        return out
    monkeypatch.setattr(fip, "process_images", recording)
    want = album.process_album(fip, photos, mdates, config=config, device_frames=False)
    got = album.process_album(fip, photos, mdates, config=config, device_frames=True)
    print("photos with faces per (device_frames, rotation):", found_in)
    for device_frames in (False, True):
        assert sum(found_in[(device_frames, 0)]) >= 4
        assert sum(found_in[(device_frames, 90)]) >= 1 and sum(found_in[(device_frames, 270)]) >= 1      # passes 2 and 3 each found a photo
    assert len(want.clusters) >= 1 and len(want.all_indices) >= 20
    assert got.clusters == want.clusters and got.all_indices == want.all_indices
    assert got.cluster_genders == want.cluster_genders and got.cluster_ages == want.cluster_ages
    assert got.private_photos == want.private_photos and got.public_photos == want.public_photos
    assert_same_crops(got.facial_images, want.facial_images)
    assert 4 in want.public_photos                                                     # the black photo: no face in any pass
    # has_center_face took the turned width: a photo stored sideways is private by the same faces as its upright original
    assert (8 in want.private_photos) == (0 in want.private_photos)
    monkeypatch.undo()
    unasked = album.process_album(fip, photos, mdates, config=config)                  # None: the module's default
    assert unasked.clusters == want.clusters and unasked.all_indices == want.all_indices


def test_process_video_with_device_frames_equals_the_host_frames(fip, frames):
    from hse_facerec_tf_amd import album
    config = album.AlbumConfig()._replace(min_frames=3)
    blank, faces = frames[4], [frames[0], frames[3], frames[7], frames[6]]
    upright = [blank] * 9 + [faces[k % 4] for k in range(12)] + [blank] * 6 + [frames[0]] * 3
    assert len(upright) == 30
    video = stored_turned(upright, 90)
    mdate = time.gmtime(T0)
    want = album.process_video(fip, iter(video), mdate, rotation=90, config=config, device_frames=False)
    assert want.video_has_faces and len(want.clusters) >= 1 and len(want.processed_indices) >= 6
    assert want.processed_indices == album.process_video(fip, iter(upright), mdate, config=config, device_frames=False).processed_indices
    for kw in (dict(), dict(max_frames=4)):
        got = album.process_video(fip, iter(video), mdate, rotation=90, config=config, device_frames=True, **kw)
        assert got.processed_indices == want.processed_indices
        assert got.clusters == want.clusters and got.video_has_faces
        assert got.cluster_ages == want.cluster_ages and got.cluster_genders == want.cluster_genders
        assert_same_crops(got.cluster_images, want.cluster_images)
        assert len(got.cluster_features) == len(want.cluster_features)
        assert all(np.array_equal(a.view(np.uint32), b.view(np.uint32)) for a, b in zip(got.cluster_features, want.cluster_features))
