"""CPU suite: the album organiser without a GPU -- the names libhsefr_album.so exports and its argument checks before any device work
(what holds for every library is in tests/test_libraries_cpu.py), the Dempster-Shafer fusion against values recorded from the reference (tests/golden/album_reference.npz,
tools/record_album_golden.py), the video frame-skip rule against the reference's loop written out here, the date rule, the cluster
summaries and the private / public split on hand-made data."""
import calendar
import ctypes
import os
import time

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "album_reference.npz")


# ---- the library -----------------------------------------------------------------------------------------------------------------
def test_header_library_and_binding_agree():
    from hse_facerec_tf_amd import _lib
    assert sorted(_lib.ALBUM_SIGNATURES) == ["hsefr_album_face_crops", "hsefr_album_last_error_string", "hsefr_album_version"]
    assert "HSEFR_KNOB" not in open(os.path.join(ROOT, "hse_facerec_tf_amd", "csrc", "album.hip")).read()


def test_face_crops_checks_its_arguments_without_a_gpu():
    from hse_facerec_tf_amd import _lib
    L = _lib.album_lib()
    buf = ctypes.create_string_buffer(4096)
    p = ctypes.cast(buf, ctypes.c_void_p).value

    def call(boxes, n_frames=2, h=10, w=12, frames=p, out=p, oh=8, ow=8, table=True):
        t = np.ascontiguousarray(boxes, dtype=np.int32).reshape(-1, 5)
        rc = L.hsefr_album_face_crops(frames, n_frames, h, w, t.ctypes.data if table else None, t.shape[0], out, oh, ow, None)
        return rc, _lib.album_last_error()
    good = [1, 2, 3, 12, 10]
    bad = {"empty in x": ([0, 5, 3, 5, 6], "empty"), "reversed in x": ([0, 6, 3, 5, 6], "empty"), "empty in y": ([0, 2, 4, 6, 4], "empty"),
           "left of the frame": ([0, -1, 0, 4, 4], "outside"), "above the frame": ([0, 0, -1, 4, 4], "outside"),
           "right of the frame": ([0, 2, 3, 13, 10], "outside"), "below the frame": ([0, 2, 3, 12, 11], "outside"),
           "frame index too large": ([2, 2, 3, 12, 10], "frame"), "negative frame index": ([-1, 2, 3, 12, 10], "frame")}
    for what, (box, word) in bad.items():
        for table in ([box], [good, box], [box, good]):                    # wherever the bad row stands
            rc, msg = call(table)
            assert rc == _lib.ERR_INVALID and word in msg, (what, rc, msg)
        with pytest.raises(ValueError):
            _lib.album_check(rc, "hsefr_album_face_crops")
    for kw in (dict(frames=None), dict(out=None), dict(table=False)):
        rc, msg = call([good], **kw)
        assert rc == _lib.ERR_INVALID and "null" in msg, (kw, rc, msg)
    for kw in (dict(oh=0), dict(ow=-1), dict(h=0), dict(n_frames=0)):
        rc, msg = call([good], **kw)
        assert rc == _lib.ERR_INVALID, (kw, rc, msg)
    # m == 0: a no-op that returns 0, whatever the pointers
    assert L.hsefr_album_face_crops(None, 0, 0, 0, None, 0, None, 0, 0, None) == 0
    assert L.hsefr_album_face_crops(p, 2, 10, 12, None, 0, p, 8, 8, None) == 0


# ---- Dempster-Shafer fusion ----------------------------------------------------------------------------------------------------------
def golden_cases():
    z = np.load(GOLDEN)
    assert sorted(z.files) == ["beliefs", "decisions", "lengths", "probs"]          # data only
    at = np.concatenate([[0], np.cumsum(z["lengths"])])
    return [(z["probs"][at[i]:at[i + 1]], z["beliefs"][i], int(z["decisions"][i])) for i in range(len(z["lengths"]))]


def test_dempster_shafer_gender_equals_the_reference():
    from hse_facerec_tf_amd import album
    cases = golden_cases()
    assert len(cases) >= 100 and {len(p) for p, _, _ in cases} >= set(range(1, 51))
    assert {d for _, _, d in cases} == {0, 1}
    undecided = 0
    for probs, beliefs, decision in cases:
        got = album.dempster_shafer_log_beliefs(probs)
        assert got.dtype == np.float64 and got.shape == (2,)
        assert np.all(np.abs(got - beliefs) <= 1e-12 * np.abs(beliefs)), (probs, got, beliefs)
        if abs(beliefs[0] - beliefs[1]) > 1e-9:
            assert album.dempster_shafer_gender(probs) == decision, (probs, beliefs)
            assert album.dempster_shafer_gender([np.array([p], np.float32) for p in probs]) == decision        # the net's [1] arrays
        else:
            undecided += 1
    assert undecided <= 0.05 * len(cases), undecided


def test_dempster_shafer_tie_goes_to_index_one(monkeypatch):
    from hse_facerec_tf_amd import album
    monkeypatch.setattr(album, "dempster_shafer_log_beliefs", lambda p: np.array([-1.5, -1.5]))
    assert album.dempster_shafer_gender([0.5]) == 1
    monkeypatch.undo()
    assert album.dempster_shafer_gender([0.9, 0.8]) == 0 and album.dempster_shafer_gender([0.1]) == 1


# ---- the frame-skip rule -------------------------------------------------------------------------------------------------------------
def literal_loop(face_counts):
    """process_photos.py:85-118 with the grab and the detector replaced by the list."""
    processed = []
    counter = 0
    delta_counter = 5
    for k in range(len(face_counts)):
        counter += 1
        if counter % delta_counter != 0:
            continue
        ages = [0] * face_counts[k]
        processed.append(k)
        delta_counter = 5 if len(ages) == 0 else 3
    return processed


def test_video_frame_schedule_is_the_reference_loop():
    from hse_facerec_tf_amd import album
    rng = np.random.RandomState(5)
    sequences = [[0] * 40, [2] * 40, [0] * 9 + [1] * 12 + [0] * 19, [1 if k % 7 < 3 else 0 for k in range(61)], [], [3], [0] * 4, [1] * 5]
    sequences += [list(rng.randint(0, 2, n)) for n in (17, 30, 64, 100)]
    for counts in sequences:
        want = literal_loop(counts)
        assert album.video_frame_schedule(counts) == want, counts
        assert all((k + 1) % 3 == 0 or (k + 1) % 5 == 0 for k in want)
        # entries of frames the rule never reaches are not read
        masked = [c if k in want else None for k, c in enumerate(counts)]
        assert album.video_frame_schedule(masked) == want
    assert album.video_frame_schedule([0] * 40) == [4, 9, 14, 19, 24, 29, 34, 39]
    assert album.video_frame_schedule([2] * 40) == [4] + list(range(5, 40, 3))
    got = album.video_frame_schedule([0] * 9 + [1] * 12 + [0] * 19)               # 5 -> 3 -> 5
    assert got[:3] == [4, 9, 11] and got == literal_loop([0] * 9 + [1] * 12 + [0] * 19)


# ---- the date rule -------------------------------------------------------------------------------------------------------------------
DAY = 86400
T0 = calendar.timegm((2019, 6, 10, 12, 0, 0))


def date_rule_album(monkeypatch, album):
    """Two planted clusters over six photos: faces 0-2 in photos that span one day, faces 3-5 in photos that span two."""
    mdates = [time.gmtime(T0 + s) for s in (0, 3600, DAY + 3600, 0, DAY, 2 * DAY)]
    seen = {}

    def fake_cluster_faces(features, distance_threshold, born_years=None, photo_years=None, all_indices=None, min_cluster_size=1,
                           device=None, method="single"):
        seen.update(threshold=distance_threshold, years=list(photo_years), indices=list(all_indices), method=method)
        return [c for c in ([0, 1, 2], [3, 4, 5], [6]) if len(c) >= min_cluster_size and c[-1] < len(all_indices)]
    monkeypatch.setattr(album.clustering, "cluster_faces", fake_cluster_faces)
    return mdates, seen


def test_date_rule(monkeypatch):
    from hse_facerec_tf_amd import album
    mdates, seen = date_rule_album(monkeypatch, album)
    feats, born, idx = np.zeros((6, 8), np.float32), [1990.0] * 6, [0, 1, 2, 3, 4, 5]
    cfg = album.AlbumConfig()
    assert (cfg.min_days_difference, cfg.min_photos, cfg.min_frames, cfg.distance_threshold, cfg.min_face_width_percent, cfg.method) == \
        (2, 3, 10, 0.82, 7, "single")
    assert album.perform_clustering(feats, born, mdates, idx, 3, True, cfg) == [[3, 4, 5]]         # one day dropped, two days kept
    assert seen == dict(threshold=0.82, years=[2019] * 6, indices=idx, method="single")
    assert album.perform_clustering(feats, born, mdates, idx, 3, False, cfg) == [[0, 1, 2], [3, 4, 5]]
    assert album.perform_clustering(feats, born, mdates, idx, 3, True, cfg._replace(min_days_difference=1)) == [[0, 1, 2], [3, 4, 5]]
    # 2 days less one second is one day
    short = mdates[:5] + [time.gmtime(T0 + 2 * DAY - 1)]
    assert album.perform_clustering(feats, born, short, idx, 3, True, cfg) == []
    # POSIX seconds are taken like struct_time
    assert album.perform_clustering(feats, born, [calendar.timegm(m) for m in mdates], idx, 3, True, cfg) == [[3, 4, 5]]
    # fewer faces than min_size: [] without clustering
    seen.clear()
    assert album.perform_clustering(feats[:2], born[:2], mdates, idx[:2], 3, True, cfg) == []
    assert seen == {}


def test_cluster_faces_errors_pass_through():
    from hse_facerec_tf_amd import album
    mdates = [time.gmtime(T0)] * 3
    with pytest.raises(ValueError, match="photo_year - born_year > 0"):
        album.perform_clustering(np.zeros((3, 8), np.float32), [1990.0, 2019.5, 1980.0], mdates, [0, 1, 2], 2, False)


# ---- summaries -----------------------------------------------------------------------------------------------------------------------
def test_summarize_clusters():
    from hse_facerec_tf_amd import album
    genders = [np.array([g], np.float32) for g in (0.9, 0.2, 0.7, 0.95, 0.1, 0.3, 0.8)]
    born = [1990.25, 1985.0, 1991.75, 1989.5, 2001.0, 2003.5, 1990.0]
    rng = np.random.RandomState(3)
    feats = (rng.standard_normal((7, 16)) * 1e4).astype(np.float32)
    feats[0, 0], feats[2, 0], feats[3, 0], feats[6, 0] = 16777216.0, 1.0, 1.0, 1.0          # a float32 running sum loses the ones
    clusters = [[0, 2, 3, 6], [1, 4, 5]]
    s = album.summarize_clusters(clusters, genders, born, feats)
    g32 = np.array([float(g[0]) for g in genders])
    assert s[0].gender == float(np.median(g32[[0, 2, 3, 6]])) and s[1].gender == float(g32[1])            # even and odd counts
    assert s[0].born_year == (1990.0 + 1990.25) / 2 and s[1].born_year == 2001.0
    for c, got in zip(clusters, s):
        want = np.sum(feats[c].astype(np.float64), axis=0) / len(c)
        assert got.feature.dtype == np.float32 and np.array_equal(got.feature, want.astype(np.float32))
        assert got.age is None
    assert s[0].feature[0] == np.float32((16777216.0 + 3.0) / 4)
    assert [x.ds_gender for x in s] == [0, 1]
    v = album.summarize_clusters(clusters, genders, born, feats, year=2019 + 5 / 12)
    assert [x.age for x in v] == [int(2019 + 5 / 12 - (1990.125 - 0.5)), int(2019 + 5 / 12 - (2001.0 - 0.5))] == [29, 18]
    assert album.summarize_clusters([], genders, born, feats) == []


def test_private_public_rule():
    from hse_facerec_tf_amd import album
    all_indices = [0, 0, 1, 3, 3, 4, 6, 7]                       # the file of every face; files 2 and 5 have no face
    clusters = [[0, 2, 3], [5, 7]]                               # files 0, 1, 3 and 4, 7
    private, public = album.split_private_public(clusters, all_indices, [5, 0], 9)
    assert private == [0, 1, 3, 4, 5, 7] and public == [2, 6, 8]
    assert album.split_private_public([], all_indices, [], 3) == ([], [0, 1, 2])
    assert album.has_center_face([[0, 0, 7, 50]], 100) and not album.has_center_face([[0, 0, 6, 50], [10, 0, 16, 9]], 100)
    assert not album.has_center_face([], 100)
