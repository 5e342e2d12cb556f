"""The reference's album organiser (age_gender_identity/process_photos.py) on the package's device paths: every photo and every video
of an album through ``FacialImageProcessing.process_images`` (batched MTCNN, faces cut from the frame stack on the device, the age /
gender net), the faces clustered with the age term and the same-photo split (``clustering.cluster_faces``), clusters kept that are
large enough and span enough days, a gender per cluster by Dempster-Shafer fusion, a birth year per cluster, and the photos split
into private and public.

No file or video I/O here beyond reading photo paths with the package's decoder: frames come in as arrays or iterables, dates as
``time.struct_time`` (what the reference takes from ``time.gmtime(os.path.getmtime(f))``) or POSIX seconds, and writing the cluster
folders is left to the caller (``AlbumResult`` holds what process_photos.py:333-358 writes).
"""
from __future__ import annotations

import calendar
import time
from typing import Iterable, List, NamedTuple, Optional, Sequence

import numpy as np

from . import _lib, clustering, preprocess, preprocess_device

# process_images(device_crops=...) of both loops when the caller does not say: decided by tools/album_time.py on an MI355X
# (profiles/album_time.txt, README "Album organiser"): the device crops are used where the engine takes bytes
DEVICE_CROPS_DEFAULT = True
# process_images(device_frames=...) of both loops when the caller does not say: decided by the same run against device_crops alone --
# faster by more than the spread between repetitions at 8, 16 and 32 frames per call (0.44 against 0.78 ms per frame at 16) and the
# 64-photo album not slower (43 against 113 ms) -- so the frames are turned and converted on the device where the detector can read a
# stack and the device crops are in use
DEVICE_FRAMES_DEFAULT = True
# process_images(mixed_sizes=...) of both loops when the caller does not say.  The rule, applied by tools/mtcnn_ragged_time.py in the last
# line of profiles/mtcnn_ragged_time.txt: True if detect_batch(mixed_sizes=True) is faster than one single-frame call per frame by more than
# the spread between repetitions at 4, 8 and 16 frames of different sizes per call AND the 64-photo album of 64 sizes is not slower by more
# than its spread; otherwise False.  Measured on an MI355X: 0.51 / 0.37 / 0.30 against 1.55 / 1.52 / 1.45 ms per frame (spreads 0.12 / 0.004 /
# 0.013) and the album 86 against 150 ms -- so the frames whose size nothing shares go through mixed-size passes where the detector has them
MIXED_SIZES_DEFAULT = True
# process_images(mixed_device=...) of both loops when the caller does not say.  The rule, applied by tools/mixed_device_time.py in the last
# line of profiles/mixed_device_time.txt: True if process_images(mixed_sizes=True, device_frames=True, mixed_device=True) is faster than the
# same call without mixed_device by more than the spread between repetitions at 4, 8 and 16 frames of different sizes per call at BOTH
# rotations 0 and 90 AND the 64-photo album of 64 sizes is not slower by more than its spread; otherwise False.  Measured on an MI355X:
# 0.67 / 0.49 / 0.38 against 1.11 / 0.91 / 0.76 ms per frame at rotation 0 (spreads 0.009 / 0.008 / 0.004), 0.63 / 0.47 / 0.37 against 2.71 /
# 2.60 / 2.48 at rotation 90 (spreads 0.28 / 0.36 / 0.13) and the album 43 against 82 ms (spread 18) -- so the frames and the faces of the
# mixed-size passes stay on the device where those passes and the device crops or frames are in use
MIXED_DEVICE_DEFAULT = True
# perform_clustering(split=...) of both loops when the caller does not say.  The rule, applied by tools/same_photo_split_time.py in the last
# line of profiles/same_photo_split_time.txt: True if cluster_faces(all_indices=..., split="device") is faster than split="host" by more
# than the spread between repetitions on 9164 faces of 1680 identities (the gallery-scale case) AND not slower by more than the spread on
# a 129-face, 6-cluster album; otherwise False.  Measured on an MI355X: 52.5 against 201.9 ms on the gallery (spread 5.5; the split
# alone 3.5 ms of device time against 158 ms of host time) and 1.12 against 2.05 ms on the album (spread 0.03) -- so the clusters of both
# loops are split in one device pass
SPLIT_DEVICE_DEFAULT = True

DECISION_TEMPLATES = ((0.875, 0.125), (0.353, 0.647))      # process_photos.py:209: rows = classes (male, female), columns = (p, 1 - p)


class AlbumConfig(NamedTuple):
    """The values of the reference's config.txt (process_photos.py:374-381)."""
    min_days_difference: int = 2
    min_photos: int = 3
    min_frames: int = 10
    distance_threshold: float = 0.82
    min_face_width_percent: float = 7
    method: str = "single"             # clustering.cluster_faces' method


class ClusterSummary(NamedTuple):
    gender: float                      # median of the members' male probabilities
    born_year: float                   # median of the members' birth years
    feature: np.ndarray                # mean of the members' un-normalised features, float32
    ds_gender: int                     # dempster_shafer_gender of the members: 0 = male
    age: Optional[int]                 # a video's int(year - (born_year - 0.5)); None without ``year``


class VideoResult(NamedTuple):
    """process_video's five results (process_photos.py:156) and what they were made from."""
    cluster_images: List[np.ndarray]   # the first face of every cluster, RGB uint8 [h, w, 3]
    cluster_ages: List[int]
    cluster_genders: List[float]
    cluster_features: List[np.ndarray]
    video_has_faces: bool
    processed_indices: List[int]       # the frames the skip rule processed, 0-based
    clusters: List[List[int]]          # indices into the faces of the processed frames, in frame order


class AlbumResult(NamedTuple):
    clusters: List[List[int]]          # face indices
    cluster_genders: List[str]         # 'male' / 'female', by Dempster-Shafer fusion
    cluster_ages: List[int]            # int(median birth year): what the reference calls cluster_ages and writes into its folder names
    all_indices: List[int]             # the file (photo, then video) of every face
    facial_images: List[np.ndarray]    # every face resized, RGB uint8 [h, w, 3]
    private_photos: List[int]
    public_photos: List[int]


# ---- Dempster-Shafer fusion (process_photos.py:160-217) -------------------------------------------------------------------------------
def dempster_shafer_log_beliefs(male_probs) -> np.ndarray:
    """The two summed log beliefs final_decision compares (index 0 = male), in fp64: per face the proximities
    1 / (1 + ||template_j - (p, 1 - p)||) normalised to sum 1 (calculate_proximity), then compute_b's
    log(prox_j) + log(1 - prox_k) - log(1 - prox_j * (1 - (1 - prox_k))) for the other class k, summed over the faces."""
    p = np.asarray(male_probs, dtype=np.float64)
    p = p.reshape(p.shape[0], -1)[:, 0] if p.size else p.reshape(0)
    dt = np.asarray(DECISION_TEMPLATES, dtype=np.float64)
    preds = np.stack([p, 1.0 - p], axis=1)                                           # [n, 2]
    dist = np.sqrt(((dt[None, :, :] - preds[:, None, :]) ** 2).sum(axis=2))          # [n, class]
    prox = 1.0 / (1.0 + dist)
    prox = prox / prox.sum(axis=1, keepdims=True)
    other = 1.0 - prox[:, ::-1]                                                      # the one (1 - prox_k), k != j
    beliefs = np.log(prox) + np.log(other) - np.log(1.0 - prox * (1.0 - other))
    return beliefs.sum(axis=0)


def dempster_shafer_gender(male_probs) -> int:
    """calculate_proximity + compute_b + final_decision for the male probabilities of a cluster's faces (scalars or the net's [1]
    arrays) -> 0 for male, 1 for female.  An exact tie goes to 1, as ``argsort()[::-1][0]`` gives."""
    m = dempster_shafer_log_beliefs(male_probs)
    return int(m.argsort()[::-1][0])


# ---- dates ---------------------------------------------------------------------------------------------------------------------------
def _struct(mdate) -> time.struct_time:
    return mdate if isinstance(mdate, time.struct_time) else time.gmtime(float(mdate))


def _fractional_year(mdate) -> float:
    m = _struct(mdate)
    return m.tm_year + (m.tm_mon - 1) / 12                                           # process_photos.py:81, :257


# ---- perform_clustering (process_photos.py:45-77) -----------------------------------------------------------------------------------
def perform_clustering(features, born_years, mdates, all_indices, min_size: int, check_dates: bool = True,
                       config: AlbumConfig = AlbumConfig(), device=None, split: Optional[str] = None) -> List[List[int]]:
    """Clusters of face indices: ``clustering.cluster_faces`` at config.distance_threshold with the age term (photo year = the integer
    tm_year of the face's file, as the reference uses) and the same-photo split, then is_good_cluster -- at least ``min_size`` faces
    and, with ``check_dates``, photos that span at least config.min_days_difference days.  ``features``: [n, d] L2-normalised, NumPy
    or a CUDA tensor (it stays on the device); ``mdates``: per FILE, struct_time or POSIX seconds; ``all_indices``: the file of every face.
    Fewer faces than ``min_size`` give [].  cluster_faces' ValueError for a face whose year minus birth year is not positive passes
    through unchanged.  ``split`` ('host' or 'device': cluster_faces' keyword, where the same-photo split runs) is passed on only when
    given.

    The day span is floor((max - min) / 86400) of the files' POSIX times.  The reference takes both dates through local-time
    ``mktime`` and subtracts the datetimes; the two agree wherever no daylight-saving change lies between the two dates."""
    all_indices = [int(i) for i in all_indices]
    n = len(all_indices)
    if n < min_size:
        return []
    dates = [_struct(m) for m in mdates]
    photo_years = [dates[i].tm_year for i in all_indices]
    clusters = clustering.cluster_faces(features, config.distance_threshold, born_years=born_years, photo_years=photo_years,
                                        all_indices=all_indices, min_cluster_size=min_size, device=device, method=config.method,
                                        **({} if split is None else dict(split=split)))
    posix = [calendar.timegm(d) for d in dates]

    def is_good_cluster(cluster):
        res = len(cluster) >= min_size
        if res and check_dates:
            times = [posix[all_indices[i]] for i in cluster]
            res = (max(times) - min(times)) // 86400 >= config.min_days_difference
        return res
    return [c for c in clusters if is_good_cluster(c)]


def summarize_clusters(clusters, genders, born_years, features, year: Optional[float] = None) -> List[ClusterSummary]:
    """Per cluster (process_photos.py:145-153, :323-331): the median gender, the median birth year, the mean of the members'
    UN-normalised features (accumulated in fp64, returned as float32), the Dempster-Shafer gender, and with ``year`` (a video's
    fractional year) the video's int(year - (median_born - 0.5)).  On the host: the clusters are small."""
    g = np.asarray(genders, dtype=np.float64)
    g = g.reshape(g.shape[0], -1)[:, 0] if g.size else g.reshape(0)
    born = np.asarray(born_years, dtype=np.float64).reshape(-1)
    feats = np.asarray(features)
    out = []
    for cluster in clusters:
        idx = np.asarray(cluster, dtype=np.int64)
        median_born = float(np.median(born[idx]))
        out.append(ClusterSummary(gender=float(np.median(g[idx])), born_year=median_born,
                                  feature=feats[idx].astype(np.float64).mean(axis=0).astype(np.float32),
                                  ds_gender=dempster_shafer_gender(g[idx]),
                                  age=None if year is None else int(year - (median_born - 0.5))))
    return out


def split_private_public(clusters, all_indices, private_indices, n_files: int):
    """process_photos.py:345-346: private = the files of the clustered faces and the files with a large-enough face; public = the
    rest.  -> (private, public), both sorted."""
    private = {int(all_indices[i]) for c in clusters for i in c} | {int(i) for i in private_indices}
    return sorted(private), [i for i in range(int(n_files)) if i not in private]


# ---- the video loop (process_photos.py:80-156) ---------------------------------------------------------------------------------------
def video_frame_schedule(face_counts) -> List[int]:
    """The frame-skip rule of process_photos.py:86-118 -> the 0-based indices of the frames it processes.  The counter starts at 0 and
    is incremented per grabbed frame; a frame is processed when counter % delta == 0; delta starts at 5 and becomes 3 after a processed
    frame with faces, 5 after one without.  ``face_counts[k]``: the number of faces frame k yields IF it is processed; only entries of
    frames the rule reaches are read (every one of them has a counter divisible by 3 or 5), the others may hold anything."""
    processed, delta = [], 5
    for k in range(len(face_counts)):
        counter = k + 1
        if counter % delta != 0:
            continue
        processed.append(k)
        delta = 5 if int(face_counts[k]) == 0 else 3
    return processed


def _use_device_crops(img_processing, device_crops: Optional[bool]) -> bool:
    if device_crops is not None:
        return bool(device_crops)
    return bool(DEVICE_CROPS_DEFAULT and img_processing.device_preprocess and img_processing.sess.accepts_u8)


def _use_device_frames(img_processing, device_frames: Optional[bool], use_device_crops: bool) -> bool:
    """(Unasked, the device frames follow the device crops they imply: a caller who turned those off keeps the host path.)"""
    if device_frames is not None:
        return bool(device_frames)
    supported = getattr(img_processing, "device_frames_supported", None)          # process_images' own rule
    return bool(DEVICE_FRAMES_DEFAULT and use_device_crops and supported is not None and supported())


def _use_mixed_sizes(img_processing, mixed_sizes: Optional[bool]) -> bool:
    """(Unasked, the mixed-size passes need a detector that has them: an MTCNNDetector with its box logic on the device.)"""
    if mixed_sizes is not None:
        return bool(mixed_sizes)
    detector = getattr(img_processing, "detector", None)
    return bool(MIXED_SIZES_DEFAULT and getattr(detector, "detect_ragged", None) is not None and getattr(detector, "device_boxes", False))


def _use_device_split(device_split: Optional[bool]) -> bool:
    """(Unasked, the same-photo split follows SPLIT_DEVICE_DEFAULT.)"""
    return bool(SPLIT_DEVICE_DEFAULT if device_split is None else device_split)


def _split_keyword(use_device_split: bool) -> dict:
    """perform_clustering's ``split`` keyword, present only when the device split is in use."""
    return dict(split="device") if use_device_split else {}


def _use_mixed_device(img_processing, mixed_device: Optional[bool], use_mixed_sizes: bool, use_device_crops: bool, use_device_frames: bool) -> bool:
    """(Unasked, the device stages of the mixed-size passes follow those passes and the device crops or frames they extend, and need a
    detector that detects from a packed buffer.)"""
    if mixed_device is not None:
        return bool(mixed_device)
    detector = getattr(img_processing, "detector", None)
    return bool(MIXED_DEVICE_DEFAULT and use_mixed_sizes and (use_device_crops or use_device_frames)
                and getattr(detector, "detect_packed", None) is not None and getattr(detector, "device_boxes", False))


def _device_switches(img_processing, device_crops, device_frames, mixed_sizes, mixed_device):
    """The device switches of both loops, each decided by its _use_* rule -> (device_crops, device_frames, mixed): ``mixed`` holds
    process_images' ``mixed_sizes`` and ``mixed_device`` keywords, each present only when it is in use."""
    use_device = _use_device_crops(img_processing, device_crops)
    use_frames = _use_device_frames(img_processing, device_frames, use_device)
    mixed = dict(mixed_sizes=True) if _use_mixed_sizes(img_processing, mixed_sizes) else {}
    if _use_mixed_device(img_processing, mixed_device, bool(mixed), use_device, use_frames):
        mixed["mixed_device"] = True
    return use_device, use_frames, mixed


def _normalized_on_device(features: Sequence[np.ndarray], device):
    """[n, d] raw features -> their L2-normalised rows as a CUDA tensor (ops.l2_normalize); they stay there for the clustering."""
    from . import ops
    torch = _lib.require_gpu()
    x = torch.from_numpy(np.ascontiguousarray(np.stack(features), dtype=np.float32)).to(_lib.cuda_device(device))
    with _lib.on_device(x):
        return ops.l2_normalize(x)


def process_video(img_processing, frames: Iterable[np.ndarray], mdate, rotation: int = 0, config: AlbumConfig = AlbumConfig(),
                  max_frames: int = 32, device_crops: Optional[bool] = None, device_frames: Optional[bool] = None,
                  mixed_sizes: Optional[bool] = None, mixed_device: Optional[bool] = None,
                  device_split: Optional[bool] = None) -> VideoResult:
    """process_photos.py:80-156 for the BGR uint8 frames of a video, in grab order.  Whether frame k is processed depends on the faces
    of earlier frames, but only counters divisible by 3 or 5 can ever be: those candidate frames run through
    ``process_images`` in windows of ``max_frames`` (batched detector passes), the rule is then replayed on the host over the face
    counts (video_frame_schedule), and the faces of frames the rule skips are dropped before clustering -- the result is that of the
    sequential loop.  Clusters need config.min_frames faces; no date rule.  ``rotation`` (0, 90 or 270: :102-107) is applied by
    process_images, on the device with ``device_frames`` (None: DEVICE_FRAMES_DEFAULT where the configuration allows it).
    ``mixed_sizes`` (None: MIXED_SIZES_DEFAULT where the detector has ragged passes): frames whose size no other frame of their
    call shares are detected together (process_images(mixed_sizes=True)); the keyword is passed on only when it is in use.
    ``mixed_device`` (None: MIXED_DEVICE_DEFAULT where those passes and the device crops or frames are in use): those passes' frames and
    crops stay on the device (process_images(mixed_device=True)); passed on only when it is in use, too.
    ``device_split`` (None: SPLIT_DEVICE_DEFAULT): the same-photo split of the clusters runs in one device pass
    (perform_clustering(split="device")); passed on only when it is in use, too."""
    rotation = preprocess_device.check_rotation(rotation)
    video_year = _fractional_year(mdate)
    use_device, use_frames, mixed = _device_switches(img_processing, device_crops, device_frames, mixed_sizes, mixed_device)
    per_frame = {}                     # candidate frame index -> (ages, genders, features, crops)
    n_frames = 0

    def flush(window):
        if not window:
            return
        res, crops = img_processing.process_images([f for _, f in window], max_frames=max_frames, device_crops=use_device, return_crops=True,
                                                   rotation=rotation, device_frames=use_frames, **mixed)
        for (k, _), (_, _, ages, genders, feats), c in zip(window, res, crops):
            per_frame[k] = (ages, genders, feats, c)

    window = []
    for k, draw in enumerate(frames):
        n_frames = k + 1
        if (k + 1) % 3 == 0 or (k + 1) % 5 == 0:
            window.append((k, np.asarray(draw)))
            if len(window) == max_frames:
                flush(window)
                window = []
    flush(window)
    counts = [len(per_frame[k][0]) if k in per_frame else 0 for k in range(n_frames)]
    processed = video_frame_schedule(counts)
    images, born, genders, features, indices = [], [], [], [], []
    for frame_count, k in enumerate(processed):
        ages, g, feats, crops = per_frame[k]
        images.extend(crops)
        genders.extend(g)
        features.extend(feats)
        indices.extend([frame_count] * len(ages))
        born.extend(video_year - (age - 0.5) for age in ages)
    clusters = []
    if len(indices) >= max(config.min_frames, 1):
        clusters = perform_clustering(_normalized_on_device(features, img_processing.sess.device), born, [mdate] * len(processed), indices,
                                      config.min_frames, False, config, **_split_keyword(_use_device_split(device_split)))
    summary = summarize_clusters(clusters, genders, born, features, year=video_year) if clusters else []
    return VideoResult([images[c[0]] for c in clusters], [s.age for s in summary], [s.gender for s in summary], [s.feature for s in summary],
                       len(clusters) > 0, processed, clusters)


# ---- the album (process_photos.py:219-358) -------------------------------------------------------------------------------------------
def has_center_face(bboxes, width: int, config: AlbumConfig = AlbumConfig()) -> bool:
    """process_photos.py:41 on process_image's padded boxes: some face at least min_face_width_percent of the frame wide."""
    return any((x2 - x1) / width >= config.min_face_width_percent / 100 for (x1, y1, x2, y2) in (b[0:4] for b in bboxes))


def _as_bgr(photo) -> np.ndarray:
    if isinstance(photo, (str, bytes)) or hasattr(photo, "__fspath__"):
        return np.ascontiguousarray(preprocess.imread_rgb(photo)[..., ::-1])         # cv2.imread's channel order
    return np.asarray(photo)


def process_album(img_processing, photos, mdates, videos=(), config: AlbumConfig = AlbumConfig(), max_frames: int = 32,
                  device_crops: Optional[bool] = None, device_frames: Optional[bool] = None, mixed_sizes: Optional[bool] = None,
                  mixed_device: Optional[bool] = None, device_split: Optional[bool] = None) -> AlbumResult:
    """process_photos.py:219-358.  ``photos``: BGR uint8 arrays or paths, ``mdates`` their dates; ``videos``: (frames, mdate) or
    (frames, mdate, rotation) per video, frames as process_video takes them.  Pass 1 runs every photo, pass 2 the quarter turns
    clockwise of the photos without a face, pass 3 the quarter turns counter-clockwise of those still without one (:241-247) -- each pass
    through ``process_images`` in calls of a few detector passes.  The faces' features are L2-normalised on the device and stay there
    until the clustering is done; born years follow :257-258; a video contributes its clusters' faces, with the cluster means as
    features (:284-297).  Then perform_clustering with config.min_photos and the date rule, the summaries, and the private / public
    split (:345-346) over the files (photos, then videos).  The quarter turns of passes 2 and 3 and of a turned video are made by
    process_images(rotation=...): on the device, in the launch that converts the frames to RGB, with ``device_frames`` (None:
    DEVICE_FRAMES_DEFAULT where the configuration allows it).  ``mixed_sizes`` (None: MIXED_SIZES_DEFAULT where the detector has ragged
    passes): the photos of a call whose size no other shares -- most of a real album -- are detected together in mixed-size passes
    (process_images(mixed_sizes=True)) instead of one by one; it goes to the videos too, and the keyword is passed on only when it is
    in use, so an ``img_processing`` written without it keeps working.  ``mixed_device`` (None: MIXED_DEVICE_DEFAULT where those passes
    and the device crops or frames are in use): the frames and the crops of those passes stay on the device
    (process_images(mixed_device=True)); it goes to the videos too and is passed on only when it is in use.  ``device_split`` (None:
    SPLIT_DEVICE_DEFAULT): the same-photo split of the clusters runs in one device pass (perform_clustering(split="device")); it goes to
    the videos too and is passed on only when it is in use."""
    photos = list(photos)
    mdates = list(mdates)
    videos = list(videos)
    if len(mdates) != len(photos):
        raise ValueError("%d photos, %d dates" % (len(photos), len(mdates)))
    for video in videos:
        preprocess_device.check_rotation(video[2] if len(video) > 2 else 0)
    use_device, use_frames, mixed = _device_switches(img_processing, device_crops, device_frames, mixed_sizes, mixed_device)
    use_split = _use_device_split(device_split)       # decided once, for the album's clusters and for its videos'
    # a video gets the decision itself; the keyword is left out only where it is off and off is what process_video would choose anyway
    video_split = dict(device_split=use_split) if use_split or SPLIT_DEVICE_DEFAULT else {}
    n_photos = len(photos)
    found = [None] * n_photos          # per photo: (ages, genders, features, crops, has_center_face)
    call = 4 * max_frames              # frames per process_images call: bounds the frame stacks held on the device at one time

    def run_pass(todo, rotation):
        for a in range(0, len(todo), call):
            part = todo[a:a + call]
            draws = [_as_bgr(photos[i]) for i in part]
            res, crops = img_processing.process_images(draws, max_frames=max_frames, device_crops=use_device, return_crops=True,
                                                       rotation=rotation, device_frames=use_frames, **mixed)
            for i, d, (bboxes, _, ages, genders, feats), c in zip(part, draws, res, crops):
                found[i] = (ages, genders, feats, c, has_center_face(bboxes, d.shape[0] if rotation else d.shape[1], config))   # the turned width

    todo = list(range(n_photos))
    for rotation in (0, 90, 270):
        if todo:
            run_pass(todo, rotation)
        todo = [i for i in todo if len(found[i][0]) == 0]
    images, genders, features, born, all_indices, private = [], [], [], [], [], []
    for i in range(n_photos):
        ages, g, feats, crops, center = found[i]
        if center:
            private.append(i)
        images.extend(crops)
        genders.extend(float(np.asarray(x).reshape(-1)[0]) for x in g)
        features.extend(feats)
        all_indices.extend([i] * len(ages))
        photo_year = _fractional_year(mdates[i])
        born.extend(photo_year - (age - 0.5) for age in ages)
    for j, video in enumerate(videos):
        frames, vdate = video[0], video[1]
        v = process_video(img_processing, frames, vdate, video[2] if len(video) > 2 else 0, config, max_frames, use_device, use_frames,
                          "mixed_sizes" in mixed, "mixed_device" in mixed, **video_split)
        if v.video_has_faces:
            private.append(n_photos + j)
        images.extend(v.cluster_images)
        genders.extend(v.cluster_genders)
        features.extend(v.cluster_features)
        all_indices.extend([n_photos + j] * len(v.cluster_ages))
        photo_year = _fractional_year(vdate)
        born.extend(photo_year - (age - 0.5) for age in v.cluster_ages)
    all_dates = mdates + [v[1] for v in videos]
    clusters = []
    if len(all_indices) >= max(config.min_photos, 1):
        clusters = perform_clustering(_normalized_on_device(features, img_processing.sess.device), born, all_dates, all_indices,
                                      config.min_photos, True, config, **_split_keyword(use_split))
    summary = summarize_clusters(clusters, genders, born, features) if clusters else []
    private_photos, public_photos = split_private_public(clusters, all_indices, private, len(all_dates))
    return AlbumResult(clusters, ['male' if s.ds_gender == 0 else 'female' for s in summary], [int(s.born_year) for s in summary],
                       all_indices, images, private_photos, public_photos)
