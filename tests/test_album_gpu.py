"""GPU suite: the album organiser on the device -- hsefr_album_face_crops byte for byte against the host restatement of cv2.resize on
the host crop, process_images(device_crops=True) against process_images(), process_album and process_video against the sequential
loops of process_photos.py written out here over process_image, and perform_clustering + summarize_clusters on planted clusters.
The host results are computed once per module and never changed."""
import calendar
import time

import numpy as np
import pytest

from oracle import pipeline as opl

from conftest import TEST_IMAGE
from test_mtcnn_batch_gpu import variants

pytestmark = pytest.mark.gpu

DAY = 86400
T0 = calendar.timegm((2019, 3, 4, 10, 0, 0))


# ---- the kernel ----------------------------------------------------------------------------------------------------------------------
def small_boxes(n_frames, h=40, w=56):
    """(frame, x1, y1, x2, y2) over [n_frames, 40, 56, 3]: inside the frame, flush with each border, the whole frame, one pixel, one
    column, one row, and the last pixel of the last frame; frames in turn, so several boxes share a frame and neighbours do not."""
    xyxy = [(10, 8, 30, 33), (0, 5, 20, 25), (7, 0, 37, 18), (30, 4, w, 30), (12, 20, 40, h), (0, 0, w, h), (17, 9, 18, 10),
            (20, 10, 21, 17), (3, 30, 8, 31), (40, 2, 47, 3), (50, 11, 51, 16), (9, 8, 31, 33), (0, 0, 1, 1), (0, h - 1, 3, h)]
    boxes = [(i % n_frames,) + b for i, b in enumerate(xyxy)]
    return boxes + [(n_frames - 1, w - 1, h - 1, w, h)]


def host_crops(frames, boxes):
    return [frames[f][y1:y2, x1:x2] for f, x1, y1, x2, y2 in boxes]


@pytest.mark.parametrize("n_frames", [1, 3])
@pytest.mark.parametrize("out_hw", [(224, 224), (8, 8), (5, 9)])
def test_face_crops_equal_the_host_resize_of_the_host_crop(n_frames, out_hw):
    import torch
    from hse_facerec_tf_amd import preprocess, preprocess_device
    frames = np.random.RandomState(7 + n_frames).randint(0, 256, (n_frames, 40, 56, 3)).astype(np.uint8)
    boxes = small_boxes(n_frames)
    oh, ow = out_hw
    stack = torch.from_numpy(frames).cuda()
    got = preprocess_device.face_crops(stack, boxes, out_hw)
    assert got.dtype == torch.uint8 and tuple(got.shape) == (len(boxes), oh, ow, 3)
    got = got.cpu().numpy()
    crops = host_crops(frames, boxes)
    for i, (box, crop) in enumerate(zip(boxes, crops)):
        want = preprocess.resize_linear_u8(crop, ow, oh)
        assert np.array_equal(got[i], want), (box, int(np.abs(got[i].astype(int) - want).max()))
    other = preprocess_device.preprocess_faces_cv(crops, out_hw, raw_u8=True).cpu().numpy()
    assert np.array_equal(got, other)
    assert np.array_equal(stack.cpu().numpy(), frames)                                 # the stack is read only


def test_face_crops_identity_shrink_slices_and_no_boxes():
    import torch
    from hse_facerec_tf_amd import preprocess, preprocess_device
    frame = np.random.RandomState(11).randint(0, 256, (1, 300, 260, 3)).astype(np.uint8)
    stack = torch.from_numpy(frame).cuda()
    boxes = [(0, 20, 50, 244, 274), (0, 0, 0, 260, 300)]
    got = preprocess_device.face_crops(stack, boxes, (224, 224)).cpu().numpy()
    assert np.array_equal(got[0], frame[0, 50:274, 20:244])                            # 224 x 224 -> 224 x 224: the identity
    assert np.array_equal(got[1], preprocess.resize_linear_u8(frame[0], 224, 224))     # shrink, no antialiasing
    # into a slice of a larger batch, and a slice that is not 16-byte aligned (5 x 9 x 3 = 135 bytes per face: the byte path)
    for oh, ow in ((224, 224), (5, 9)):
        batch = torch.full((4, oh, ow, 3), 7, dtype=torch.uint8, device="cuda")
        preprocess_device.face_crops(stack, boxes, (oh, ow), out=batch[1:3])
        b = batch.cpu().numpy()
        assert (b[0] == 7).all() and (b[3] == 7).all()
        for i, (f, x1, y1, x2, y2) in enumerate(boxes):
            assert np.array_equal(b[1 + i], preprocess.resize_linear_u8(frame[f, y1:y2, x1:x2], ow, oh))
    empty = preprocess_device.face_crops(stack, np.zeros((0, 5), np.int32), (224, 224))
    assert tuple(empty.shape) == (0, 224, 224, 3)
    for bad in ([(0, 0, 0, 261, 300)], [(1, 0, 0, 10, 10)], [(0, 5, 5, 5, 9)]):        # refused before any launch
        with pytest.raises(ValueError):
            preprocess_device.face_crops(stack, bad, (224, 224))
    with pytest.raises(ValueError):
        preprocess_device.face_crops(stack.cpu(), boxes, (224, 224))


# ---- process_images ------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def fip():
    from hse_facerec_tf_amd import FacialImageProcessing
    return FacialImageProcessing(mtcnn_detector=True, minsize=32, latency_plan=False)


@pytest.fixture(scope="module")
def photo():
    return opl.imread_rgb(TEST_IMAGE)


@pytest.fixture(scope="module")
def frames(photo):
    """BGR, as cv2.imread gives them: the eight same-size variants, then one frame of another size (a pass of its own)."""
    rgb = variants(photo) + [np.ascontiguousarray(photo[40:520, 100:700])]
    return [np.ascontiguousarray(f[..., ::-1]) for f in rgb]


@pytest.fixture(scope="module")
def host_path(fip, frames):
    out = fip.process_images(frames)
    counts = [len(r[0]) for r in out]
    print("faces per frame:", counts)
    assert max(counts[:8]) >= 4 and min(counts[:8]) == 0 and counts[8] > 0, counts
    return out


def assert_same_results(got, want):
    assert len(got) == len(want)
    for i, (g, w) in enumerate(zip(got, want)):
        assert g[0] == w[0], i                                                         # boxes: lists of ints
        assert np.array_equal(np.asarray(g[1]), np.asarray(w[1])), i                   # points
        assert len(g[2]) == len(w[2]) == len(g[3]) == len(g[4]) == len(w[0])
        for a, b in zip(g[2], w[2]):
            assert a == b, i                                                           # ages
        for k in (3, 4):                                                               # genders, features: the same bits
            for a, b in zip(g[k], w[k]):
                assert a.dtype == b.dtype == np.float32 and np.array_equal(a.view(np.uint32), b.view(np.uint32)), (i, k)


def test_process_images_with_device_crops_equals_the_host_crops(fip, frames, host_path, monkeypatch):
    from hse_facerec_tf_amd import preprocess, preprocess_device
    calls = {"device": [], "host": []}
    real_device, real_host = preprocess_device.face_crops, preprocess_device.preprocess_faces_cv
    monkeypatch.setattr(preprocess_device, "face_crops", lambda stack, boxes, *a, **k: (calls["device"].append(len(boxes)),
                                                                                       real_device(stack, boxes, *a, **k))[1])
    monkeypatch.setattr(preprocess_device, "preprocess_faces_cv", lambda crops, *a, **k: (calls["host"].append(len(crops)),
                                                                                         real_host(crops, *a, **k))[1])
    got, crops = fip.process_images(frames, device_crops=True, return_crops=True)
    counts = [len(r[0]) for r in host_path]
    # one launch for the pass of eight frames, whatever the box sizes; the lone frame took the single-frame call and the host crops
    assert calls == {"device": [sum(counts[:8])], "host": [counts[8]]}, calls
    assert len({(b[2] - b[0], b[3] - b[1]) for r in host_path[:8] for b in r[0]}) > 4   # ... and the boxes do differ in size
    assert_same_results(got, host_path)
    assert_same_results(fip.process_images(frames, device_crops=True), host_path)
    assert_same_results(fip.process_images(frames, max_frames=3, device_crops=True), host_path)
    # sizes that alternate: the faces of the same-size pass do not stand together in the batch
    mixed = [frames[0], frames[8], frames[3], frames[4]]
    assert_same_results(fip.process_images(mixed, device_crops=True), fip.process_images(mixed))
    assert [c.shape for c in crops] == [(n, 224, 224, 3) for n in counts]
    for draw, (bboxes, *_), c in zip(frames, host_path, crops):
        rgb = draw[..., ::-1]
        assert c.dtype == np.uint8
        for (x1, y1, x2, y2), face in zip(bboxes, c):
            assert np.array_equal(face, preprocess.resize_linear_u8(rgb[y1:y2, x1:x2], 224, 224))
    # the host path hands back the same crops
    _, crops_host = fip.process_images(frames, return_crops=True)
    assert all(np.array_equal(a, b) for a, b in zip(crops, crops_host))
    assert fip.process_images([], device_crops=True, return_crops=True) == ([], [])


def test_device_crops_need_the_byte_path(fip, frames, monkeypatch):
    monkeypatch.setattr(fip, "device_preprocess", False)
    with pytest.raises(ValueError, match="device_crops"):
        fip.process_images(frames[:2], device_crops=True)


# ---- the sequential loops of process_photos.py, over process_image ------------------------------------------------------------------
def sequential_process_image(fip, draw, config):
    """process_photos.py:31-43, with the crops in RGB."""
    from hse_facerec_tf_amd import preprocess
    bboxes, _, ages, genders, feats = fip.process_image(draw)
    rgb = draw[..., ::-1]
    images = [preprocess.resize_linear_u8(rgb[y1:y2, x1:x2], 224, 224) for (x1, y1, x2, y2) in bboxes]
    center = any((x2 - x1) / draw.shape[1] >= config.min_face_width_percent / 100 for (x1, y1, x2, y2) in bboxes)
    return images, ages, genders, feats, center


def normalized(features):
    import torch
    from hse_facerec_tf_amd import ops
    return ops.l2_normalize(torch.from_numpy(np.stack(features).astype(np.float32)).cuda())


def sequential_clustering(features, born, mdates, all_indices, min_size, check_dates, config):
    """process_photos.py:45-77 with cluster_faces for the distance matrix and get_facial_clusters."""
    from hse_facerec_tf_amd import clustering
    if len(all_indices) < min_size:
        return []
    clusters = clustering.cluster_faces(normalized(features), config.distance_threshold, born_years=born,
                                        photo_years=[mdates[i].tm_year for i in all_indices], all_indices=all_indices)
    good = []
    for c in clusters:
        ok = len(c) >= min_size
        if ok and check_dates:
            times = [calendar.timegm(mdates[all_indices[i]]) for i in c]
            ok = int((max(times) - min(times)) / DAY) >= config.min_days_difference
        if ok:
            good.append(c)
    return good


def test_process_album_equals_the_sequential_loop(fip, frames, photo):
    from hse_facerec_tf_amd import album
    config = album.AlbumConfig()
    turned = np.ascontiguousarray(np.rot90(photo, 1)[..., ::-1])                     # upright again after the quarter turn clockwise
    photos = frames + [turned, np.zeros((300, 400, 3), np.uint8)]
    mdates = [time.gmtime(T0 + i * 17 * 3600) for i in range(len(photos))]             # eleven photos over a week
    # the sequential loop: process_photos.py:238-258
    images, genders, feats, born, all_indices, private, passes = [], [], [], [], [], [], []
    for i, full_photo in enumerate(photos):
        facial_images, ages, g, f, center = sequential_process_image(fip, full_photo, config)
        n_pass = 1
        if len(facial_images) == 0:
            facial_images, ages, g, f, center = sequential_process_image(fip, np.ascontiguousarray(np.rot90(full_photo, -1)), config)
            n_pass = 2
            if len(facial_images) == 0:
                facial_images, ages, g, f, center = sequential_process_image(fip, np.ascontiguousarray(np.rot90(full_photo, 1)), config)
                n_pass = 3
        passes.append(n_pass if facial_images else 0)
        if center:
            private.append(i)
        images.extend(facial_images)
        genders.extend(g)
        feats.extend(f)
        all_indices.extend([i] * len(ages))
        photo_year = mdates[i].tm_year + (mdates[i].tm_mon - 1) / 12
        born.extend(photo_year - (age - 0.5) for age in ages)
    assert passes[9] == 2 and passes[10] == 0 and passes.count(1) >= 3, passes        # the turned photo is found in the retry pass only
    clusters = sequential_clustering(feats, born, mdates, all_indices, config.min_photos, True, config)
    assert len(clusters) >= 2, clusters
    g = np.array([float(x[0]) for x in genders])
    want_genders = ['male' if album.dempster_shafer_gender(g[c]) == 0 else 'female' for c in clusters]
    want_ages = [int(np.median(np.array(born)[c])) for c in clusters]
    want_private = sorted({all_indices[e] for c in clusters for e in c} | set(private))
    want_public = [i for i in range(len(photos)) if i not in want_private]
    for device_crops in (True, False):
        got = album.process_album(fip, photos, mdates, config=config, device_crops=device_crops)
        assert got.all_indices == all_indices
        assert got.clusters == clusters
        assert got.cluster_genders == want_genders and got.cluster_ages == want_ages
        assert got.private_photos == want_private and got.public_photos == want_public
        assert len(got.facial_images) == len(images) and all(np.array_equal(a, b) for a, b in zip(got.facial_images, images))
    assert 10 in want_public


def test_process_album_reads_paths_and_takes_no_photos(fip):
    from hse_facerec_tf_amd import album, preprocess
    decoded = np.ascontiguousarray(preprocess.imread_rgb(TEST_IMAGE)[..., ::-1])
    mdates = [time.gmtime(T0), time.gmtime(T0 + 3 * DAY)]
    a = album.process_album(fip, [TEST_IMAGE, decoded], mdates)
    assert a.all_indices == [0] * 4 + [1] * 4 and a.clusters == []                     # two photos: no cluster of min_photos = 3
    assert a.private_photos in ([0, 1], []) and sorted(a.private_photos + a.public_photos) == [0, 1]
    assert all(np.array_equal(x, y) for x, y in zip(a.facial_images[:4], a.facial_images[4:]))
    empty = album.process_album(fip, [], [])
    assert empty.clusters == [] and empty.all_indices == [] and empty.public_photos == []
    with pytest.raises(ValueError):
        album.process_album(fip, [decoded], [])


# ---- the cluster logic on planted clusters -------------------------------------------------------------------------------------------
def planted():
    """Five identities of six faces on the unit sphere: 0 is two tight triples 0.3 apart, with one face of each triple in ONE photo;
    1-3 are plain; 4 is photographed within one day.  -> features [30, 64], born years, genders, all_indices, mdates."""
    rng = np.random.RandomState(42)
    centers = np.linalg.qr(rng.standard_normal((64, 64)))[0][:6]
    feats, born, genders = [], [], []
    for ident in range(5):
        for k in range(6):
            c = centers[ident]
            if ident == 0:
                c = c + 0.15 * centers[5] * (1 if k % 2 == 0 else -1)                  # faces 0, 2, 4 and faces 1, 3, 5
            x = c + 0.004 * rng.standard_normal(64)
            feats.append(x / np.linalg.norm(x))
            born.append(1975.0 + 6 * ident + 0.1 * k)
            genders.append(np.array([0.92 - 0.01 * k if ident % 2 == 0 else 0.08 + 0.02 * k], np.float32))
    all_indices = [0, 0] + list(range(1, 29))                                        # faces 0 and 1 share photo 0
    seconds = []
    for photo_index in range(29):
        face = photo_index + 1 if photo_index else 0
        ident, k = divmod(face, 6)
        seconds.append(T0 + (k * 7 * 3600 if ident == 4 else k * DAY + ident * 3600))
    return np.array(feats, np.float32), np.array(born), genders, all_indices, [time.gmtime(s) for s in seconds]


def reference_distance_matrix(features, born, mdates, all_indices):
    """feature_distance of process_photos.py:46-59, in fp64."""
    x = features.astype(np.float64)
    dist = np.sqrt(((x[:, None, :] - x[None, :, :]) ** 2).sum(axis=2))
    years = np.array([mdates[i].tm_year for i in all_indices], np.float64)
    max_year = np.maximum(years[:, None], years[None, :])
    ai, aj = max_year - born[:, None], max_year - born[None, :]
    return np.clip(dist + 0.1 * (ai - aj) ** 2 / (ai + aj), 0, None)


def test_perform_clustering_and_summaries_on_planted_clusters():
    import torch
    from hse_facerec_tf_amd import album, clustering
    feats, born, genders, all_indices, mdates = planted()
    config = album.AlbumConfig()
    faces = lambda ident: list(range(6 * ident, 6 * ident + 6))
    split = [[0, 2, 4], [1, 3, 5]]                                                     # the same-photo split of identity 0
    everything = sorted(split + [faces(i) for i in (1, 2, 3, 4)], key=lambda c: (-len(c), c[0]))
    for x in (feats, torch.from_numpy(feats).cuda()):                                  # host features, and features that stay on the device
        assert album.perform_clustering(x, born, mdates, all_indices, 3, False, config) == everything
        assert album.perform_clustering(x, born, mdates, all_indices, 3, True, config) == [c for c in everything if c != faces(4)]
        assert album.perform_clustering(x, born, mdates, all_indices, 4, True, config) == [faces(1), faces(2), faces(3)]
    # the reference's own route: the N x N matrix of feature_distance through get_facial_clusters, then is_good_cluster's length rule
    D = reference_distance_matrix(feats, born, mdates, all_indices)
    dense = clustering.get_facial_clusters(D, config.distance_threshold, all_indices, 3)
    assert [c for c in dense if len(c) >= 3] == everything
    for method in ("average", "complete"):
        assert album.perform_clustering(feats, born, mdates, all_indices, 3, False, config._replace(method=method)) == everything
    kept = album.perform_clustering(feats, born, mdates, all_indices, 3, True, config)
    raw = (feats.astype(np.float64) * (1.0 + np.arange(30)[:, None])).astype(np.float32)     # un-normalised features of the same faces
    summary = album.summarize_clusters(kept, genders, born, raw, year=2019 + 2 / 12)
    g = np.array([float(x[0]) for x in genders])
    for c, s in zip(kept, summary):
        assert s.gender == float(np.median(g[c])) and s.born_year == float(np.median(born[c]))
        assert np.array_equal(s.feature, raw[c].astype(np.float64).mean(axis=0).astype(np.float32))
        assert s.ds_gender == (0 if (c[0] // 6) % 2 == 0 else 1)
        assert s.age == int(2019 + 2 / 12 - (np.median(born[c]) - 0.5))


# ---- the video loop ------------------------------------------------------------------------------------------------------------------
def test_process_video_equals_the_sequential_loop(fip, frames):
    from hse_facerec_tf_amd import album
    config = album.AlbumConfig()._replace(min_frames=3)
    blank, faces = frames[4], [frames[0], frames[3], frames[7], frames[6]]
    video = [blank] * 9 + [faces[k % 4] for k in range(12)] + [blank] * 6 + [frames[0]] * 3
    assert len(video) == 30
    mdate = time.gmtime(T0)
    video_year = mdate.tm_year + (mdate.tm_mon - 1) / 12
    # the sequential loop: process_photos.py:85-118
    counter, delta_counter, frame_count = 0, 5, 0
    processed, deltas, images, born, genders, feats, all_indices = [], [], [], [], [], [], []
    for k, draw in enumerate(video):
        counter += 1
        if counter % delta_counter != 0:
            continue
        facial_images, ages, g, f, _ = sequential_process_image(fip, draw, config)
        processed.append(k)
        images.extend(facial_images)
        genders.extend(g)
        feats.extend(f)
        all_indices.extend([frame_count] * len(ages))
        born.extend(video_year - (age - 0.5) for age in ages)
        frame_count += 1
        delta_counter = 5 if len(ages) == 0 else 3
        deltas.append(delta_counter)
    assert sum(a != b for a, b in zip(deltas, deltas[1:])) >= 3, deltas               # the rule changes its step several times
    clusters = sequential_clustering(feats, born, [mdate] * frame_count, all_indices, config.min_frames, False, config)
    assert len(clusters) >= 1, clusters                                               # min_frames is low enough for a cluster to survive
    g = np.array([float(x[0]) for x in genders])
    for kw in (dict(device_crops=True), dict(device_crops=False), dict(max_frames=4), dict()):
        got = album.process_video(fip, iter(video), mdate, config=config, **kw)
        assert got.processed_indices == processed
        assert got.clusters == clusters and got.video_has_faces
        assert all(np.array_equal(a, images[c[0]]) for a, c in zip(got.cluster_images, clusters))
        assert got.cluster_ages == [int(video_year - (np.median(np.array(born)[c]) - 0.5)) for c in clusters]
        assert got.cluster_genders == [float(np.median(g[c])) for c in clusters]
        for a, c in zip(got.cluster_features, clusters):
            assert np.array_equal(a, np.stack(feats)[c].astype(np.float64).mean(axis=0).astype(np.float32))
    none = album.process_video(fip, [blank] * 12, mdate, config=config)
    assert none.processed_indices == [4, 9] and not none.video_has_faces and none.clusters == [] and none.cluster_images == []
    # rotation 90 / 270: a frame stored a quarter turn counter-clockwise / clockwise comes out upright
    upright = album.process_video(fip, [frames[0]] * 6, mdate, config=config._replace(min_frames=1))
    for rotation, turns in ((90, 1), (270, -1)):
        turned = [np.ascontiguousarray(np.rot90(frames[0], turns))] * 6
        got = album.process_video(fip, turned, mdate, rotation=rotation, config=config._replace(min_frames=1))
        assert got.processed_indices == upright.processed_indices == [4, 5]              # counter 5, and with faces found, counter 6
        assert got.clusters == upright.clusters and len(got.clusters) >= 4
        assert all(np.array_equal(a, b) for a, b in zip(got.cluster_features, upright.cluster_features))
