"""CPU suite: the same-photo split's library without a GPU -- the names libhsefr_split.so exports and the limits of its header (what
holds for every library is in tests/test_libraries_cpu.py), compiled with libhsefr.so's flags against the shared distance headers,
every refused argument of hsefr_split_groups before any device work, clustering.group_table, the ``split`` keyword of the two entry points and of the album, and the host restatement the GPU suite compares with against scipy."""
import ctypes
import os
import re

import numpy as np
import pytest

import build_table
import group_split_cases as cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "hse_facerec_tf_amd", "csrc")
HEADER = os.path.join(ROOT, "include", "hsefr_split.h")
NAMES = ["hsefr_split_groups", "hsefr_split_last_error", "hsefr_split_version"]


# ---- the library -----------------------------------------------------------------------------------------------------------------
def test_header_library_and_binding_agree():
    from hse_facerec_tf_amd import _lib, ops
    assert sorted(_lib.SPLIT_SIGNATURES) == NAMES
    assert "HSEFR_KNOB" not in open(os.path.join(CSRC, "group_split.hip")).read()
    header = open(HEADER).read()
    # the argument count of the one call is the header's
    args = re.search(r"int hsefr_split_groups\((.*?)\);", re.sub(r"/\*.*?\*/", "", header, flags=re.S), flags=re.S).group(1)
    assert len(args.split(",")) == len(_lib.SPLIT_SIGNATURES["hsefr_split_groups"][1]) == 16
    # the class limits and the counts' order are the header's
    limits = {k: int(v) for k, v in re.findall(r"#define HSEFR_SPLIT_(WAVE_MAX|LDS_MAX|STATS) (\d+)", header)}
    assert (limits["WAVE_MAX"], limits["LDS_MAX"]) == (ops.SPLIT_WAVE_MAX, ops.SPLIT_LDS_MAX) == (cases.WAVE_MAX, cases.LDS_MAX)
    assert limits["STATS"] == len(ops.SPLIT_STATS) == 5
    for limit in (cases.WAVE_MAX, cases.LDS_MAX):                                      # the GPU suite stands on both sides of each
        assert {limit - 1, limit, limit + 1} <= set(cases.SIZES)


def test_the_library_compiles_the_shared_distance_with_the_main_librarys_flags():
    """The features path splits on the bits the clusters were formed by because feat_tile is written once (linkage_scan.h over
    mfma_dot.h) and compiled here with libhsefr.so's own flags."""
    src = open(os.path.join(CSRC, "group_split.hip")).read()
    assert '#include "linkage_scan.h"' in src and "link::feat_tile(" in src and "link::better(" in src
    assert not re.search(r"__device__[^;{]*\bfeat_tile\(", src) and "mfma_f32_32x32x2f32" not in src      # called, not written again
    table = build_table.rows()
    assert table["split"]["srcs"] == ["group_split.hip"] and table["split"]["flags"] == table["hsefr"]["flags"]
    assert build_table.stale_against("split", "linkage_scan.h", "mfma_dot.h", "common.h", "include/hsefr.h", "include/hsefr_split.h")
    assert table["split"]["lint"] == "1"


# ---- argument checks before any device work ------------------------------------------------------------------------------------------
@pytest.fixture()
def host():
    """A host buffer whose address stands in for every device pointer: no call below reaches a launch."""
    from hse_facerec_tf_amd import _lib
    buf = ctypes.create_string_buffer(4096)
    return _lib, _lib.split_lib(), ctypes.cast(buf, ctypes.c_void_p).value, buf


def test_split_groups_checks_its_arguments_without_a_gpu(host):
    _lib, L, p, _ = host
    good = np.array([0, 3, 4, 10], dtype=np.int64)
    KEEP = object()

    def call(x=p, n=10, d=8, born=None, year=None, dense=None, members=p + 512, offsets=good, groups=KEEP, photo=p + 1024, penalty=100.0,
             cut=50.0, sublabel=p + 1536):
        groups = len(offsets) - 1 if groups is KEEP else groups
        return L.hsefr_split_groups(x, n, d, born, year, dense, members, None if offsets is None else offsets.ctypes.data, groups, photo,
                                    penalty, cut, sublabel, None, None, None)

    def refused(rc, word):
        msg = _lib.split_last_error()
        assert rc == _lib.ERR_INVALID and "split_groups" in msg and word in msg, (rc, msg, word)
    assert call(groups=0) == 0                                                          # nothing to do
    for n in (0, -1):
        refused(call(n=n), "n=")
    refused(call(dense=p + 2048), "exactly one")
    refused(call(x=None), "exactly one")
    for d in (0, 4, 12, -8):
        refused(call(d=d), "multiple of 8")
    refused(call(born=p + 2048), "come together")
    refused(call(year=p + 2048), "come together")
    refused(call(x=None, dense=p + 2048, born=p + 2560, year=p + 3072), "features path")
    refused(call(members=None), "null members")
    refused(call(offsets=None, groups=3), "null offsets")
    refused(call(photo=None), "null photo")
    refused(call(sublabel=None), "null sublabel")
    refused(call(groups=-1), "groups=-1")
    refused(call(offsets=np.array([1, 3, 4], dtype=np.int64)), "start at 1")
    refused(call(offsets=np.array([1], dtype=np.int64), groups=0), "start at 1")    # a bad table is refused when empty too
    for table in ([0, 3, 3, 10], [0, 5, 4, 10], [0, 0], [0, -2]):
        refused(call(offsets=np.array(table, dtype=np.int64)), "strictly increase")
    refused(call(offsets=np.array([0, 5, 1 << 31], dtype=np.int64)), "2^31")
    refused(call(offsets=np.array([0, 5, (1 << 40) + 7], dtype=np.int64)), "2^31")
    for penalty in (float("nan"), float("inf"), -float("inf"), -1.0):
        refused(call(penalty=penalty), "penalty")
    for cut in (float("nan"), float("inf"), -float("inf")):
        refused(call(cut=cut), "cut")
    with pytest.raises(ValueError, match="strictly increase"):
        _lib.split_check(call(offsets=np.array([0, 3, 3], dtype=np.int64)), "hsefr_split_groups")


# ---- the group table -------------------------------------------------------------------------------------------------------------------
def test_group_table_is_groups_order():
    from hse_facerec_tf_amd import clustering
    rs = np.random.RandomState(0)
    for n, classes in ((1, 1), (7, 7), (50, 4), (300, 40), (300, 1)):
        labels = rs.randint(0, classes, n) * 11 - 40                                   # not dense, some negative
        if classes == n:
            labels = rs.permutation(n)                                                 # singletons only
        members, offsets = clustering.group_table(labels)
        groups = clustering._groups(labels)
        assert members.dtype == np.int32 and offsets.dtype == np.int64
        assert offsets[0] == 0 and offsets[-1] == n and len(offsets) == len(groups) + 1 and (np.diff(offsets) > 0).all()
        for g, want in enumerate(groups):
            assert np.array_equal(members[offsets[g]:offsets[g + 1]], want)
        firsts = members[offsets[:-1]]
        assert (np.diff(firsts) > 0).all()                                             # ordered by their smallest member
        assert sorted(members.tolist()) == list(range(n))
    members, offsets = clustering.group_table(["b", "a", "b", "c", "a"])               # compared for equality only
    assert members.tolist() == [0, 2, 1, 4, 3] and offsets.tolist() == [0, 2, 4, 5]
    members, offsets = clustering.group_table(np.zeros(5))                             # one group
    assert members.tolist() == [0, 1, 2, 3, 4] and offsets.tolist() == [0, 5]
    members, offsets = clustering.group_table([])
    assert len(members) == 0 and offsets.tolist() == [0]


# ---- the keywords ------------------------------------------------------------------------------------------------------------------------
def no_device(monkeypatch):
    from hse_facerec_tf_amd import _lib

    def refuse(*a, **k):
        raise AssertionError("device work")
    for name in ("require_gpu", "lib", "split_lib", "cuda_device"):
        monkeypatch.setattr(_lib, name, refuse)


def test_a_bad_split_raises_before_any_device_work(monkeypatch):
    from hse_facerec_tf_amd import album, clustering
    no_device(monkeypatch)
    D = cases.integer_matrix(6, 0)
    X = np.eye(6, 8, dtype=np.float32)
    for method in clustering.CLUSTER_METHODS:
        for bad in ("bogus", None, True, "Device"):
            with pytest.raises(ValueError, match="split"):
                clustering.get_facial_clusters(D, 2, [0, 0, 1, 2, 3, 4], method=method, split=bad)
            with pytest.raises(ValueError, match="split"):
                clustering.cluster_faces(X, 1.0, all_indices=[0, 0, 1, 2, 3, 4], method=method, split=bad)
    with pytest.raises(ValueError, match="split"):
        album.perform_clustering(X, [1990.0] * 6, [0.0] * 6, list(range(6)), 1, False, split="bogus")
    assert clustering.SPLIT_CHOICES == ("host", "device")


def test_split_is_ignored_where_all_indices_is(monkeypatch):
    from hse_facerec_tf_amd import clustering
    no_device(monkeypatch)
    calls = []
    monkeypatch.setattr(clustering, "split_same_photo", lambda *a, **k: calls.append("split") or [])
    monkeypatch.setattr(clustering, "_split_on_device", lambda *a, **k: calls.append("split") or [])
    monkeypatch.setattr(clustering, "dbscan_dense", lambda *a, **k: (np.array([0, 1]), np.array([0, 0, -1, 1, 1, 1])))
    monkeypatch.setattr(clustering, "dbscan", lambda *a, **k: (np.array([0, 1]), np.array([0, 0, -1, 1, 1, 1])))
    monkeypatch.setattr(clustering, "rank_order_dense", lambda *a, **k: ([[3, 4, 5], [0, 1]], 2))
    monkeypatch.setattr(clustering, "rank_order", lambda *a, **k: ([[3, 4, 5], [0, 1]], 2))
    D, X, photos = cases.integer_matrix(6, 0), np.eye(6, 8, dtype=np.float32), [0, 0, 1, 1, 1, 2]
    for split in clustering.SPLIT_CHOICES:
        assert clustering.get_facial_clusters(D, 2, photos, method="dbscan", split=split) == [[3, 4, 5], [0, 1]]
        assert clustering.get_facial_clusters(D, 2, photos, method="rankorder", split=split) == [[3, 4, 5], [0, 1]]
        assert clustering.cluster_faces(X, 1.0, all_indices=photos, method="dbscan", split=split) == [[3, 4, 5], [0, 1]]
        assert clustering.cluster_faces(X, 1.0, all_indices=photos, method="rankorder", split=split) == [[3, 4, 5], [0, 1]]
    assert calls == []


def test_the_album_passes_the_keyword_on_only_when_it_is_in_use(monkeypatch):
    """A cluster_faces written without ``split`` keeps working with the album unless the device split is asked for or is the default."""
    from hse_facerec_tf_amd import album, clustering
    seen, real = [], clustering.cluster_faces

    def old_cluster_faces(features, distance_threshold, born_years=None, photo_years=None, all_indices=None, min_cluster_size=1, device=None,
                          method="single", **kw):
        seen.append(kw)
        return [[0, 1, 2]]
    monkeypatch.setattr(clustering, "cluster_faces", old_cluster_faces)
    X = np.eye(3, 8, dtype=np.float32)
    args = (X, [1990.0] * 3, [0.0, 1e6, 2e6], [0, 1, 2], 3, False)
    album.perform_clustering(*args)
    album.perform_clustering(*args, split="device")
    album.perform_clustering(*args, split="host")
    assert seen == [{}, {"split": "device"}, {"split": "host"}]
    for default in (False, True):
        monkeypatch.setattr(album, "SPLIT_DEVICE_DEFAULT", default)
        assert album._use_device_split(None) is default
        assert album._use_device_split(True) is True and album._use_device_split(False) is False
    assert album._split_keyword(True) == {"split": "device"} and album._split_keyword(False) == {}
    assert isinstance(album.SPLIT_DEVICE_DEFAULT, bool)
    import inspect
    for fn in (album.process_album, album.process_video):
        assert inspect.signature(fn).parameters["device_split"].default is None
    assert inspect.signature(album.perform_clustering).parameters["split"].default is None
    for fn in (clustering.get_facial_clusters, real):
        assert inspect.signature(fn).parameters["split"].default == "host"


class OneFacePerFrame:
    """An img_processing that finds one face in every frame (no device, no detector)."""
    device_preprocess = False

    class sess:
        accepts_u8, device = False, None

    def process_images(self, draws, max_frames=32, device_crops=False, return_crops=False, rotation=0, device_frames=False, **kw):
        res = [([(0, 0, 20, 20, 1.0)], [None], [30.0], [np.array([0.5], np.float32)], [np.ones(8, np.float32)]) for _ in draws]
        return (res, [np.zeros((1, 224, 224, 3), np.uint8) for _ in draws]) if return_crops else res


@pytest.mark.parametrize("default", [False, True])
def test_the_albums_choice_reaches_its_videos(monkeypatch, default):
    """process_album decides once where the same-photo split runs: its own clusters and its videos' clusters get the same answer, the
    caller's word against the default included."""
    from hse_facerec_tf_amd import album
    monkeypatch.setattr(album, "SPLIT_DEVICE_DEFAULT", default)
    monkeypatch.setattr(album, "_normalized_on_device", lambda features, device: np.stack(features))
    seen = []

    def fake_perform_clustering(features, born_years, mdates, all_indices, min_size, check_dates=True, config=None, device=None, **kw):
        seen.append(("album" if check_dates else "video", kw))
        return []
    monkeypatch.setattr(album, "perform_clustering", fake_perform_clustering)
    photos, dates = [np.zeros((40, 50, 3), np.uint8)] * 4, [1.6e9 + 86400.0 * i for i in range(4)]
    video = ([np.zeros((30, 30, 3), np.uint8)] * 60, 1.6e9)
    for asked, want in ((False, {}), (True, {"split": "device"}), (None, {"split": "device"} if default else {})):
        del seen[:]
        album.process_album(OneFacePerFrame(), photos, dates, videos=[video], **({} if asked is None else dict(device_split=asked)))
        assert seen == [("video", want), ("album", want)], (asked, default, seen)
        del seen[:]
        album.process_video(OneFacePerFrame(), video[0], video[1], **({} if asked is None else dict(device_split=asked)))
        assert seen == [("video", want)], (asked, default, seen)
    # a process_video written without the keyword keeps working while the device split is off everywhere
    if not default:
        real = album.process_video
        monkeypatch.setattr(album, "process_video", lambda fip, frames, mdate, rotation, config, max_frames, dc, df, ms, md:
                            real(fip, frames, mdate, rotation, config, max_frames, dc, df, ms, md))
        del seen[:]
        album.process_album(OneFacePerFrame(), photos, dates, videos=[video])
        assert seen == [("video", {}), ("album", {})]


def test_split_same_photo_of_no_faces_is_no_clusters():
    from hse_facerec_tf_amd import clustering
    assert clustering.split_same_photo([], [], features=np.zeros((0, 8), np.float32)) == []
    assert clustering.split_same_photo(np.zeros(0, int), np.zeros(0, int), dist_matrix=np.zeros((0, 0))) == []


def test_the_default_is_the_records_verdict():
    """album.SPLIT_DEVICE_DEFAULT is what the last line of profiles/same_photo_split_time.txt says."""
    from hse_facerec_tf_amd import album
    last = open(os.path.join(ROOT, "profiles", "same_photo_split_time.txt")).read().strip().splitlines()[-1]
    verdict = re.match(r"# rule: album\.SPLIT_DEVICE_DEFAULT = (True|False) ", last)
    assert verdict, last
    assert album.SPLIT_DEVICE_DEFAULT == (verdict.group(1) == "True")


# ---- the host restatement the GPU suite compares with ----------------------------------------------------------------------------------
def test_the_host_chain_is_scipys_partition_on_the_gpu_suites_tied_groups():
    """A guard on the GPU suite's REFERENCE, not on the feature (it passes without the library): complete_linkage_labels, which the
    device sublabels are compared with, is scipy's partition on the tied groups that suite uses, and those groups give every chain class
    work."""
    members, offsets, n = cases.grouping(cases.SIZES, 5, sum(cases.SIZES) + 77, True)
    D = cases.integer_matrix(n, 6)
    photo = cases.photos_with_shared(members, offsets, n, 7)
    P_of = lambda g: cases.host_P(D, members[offsets[g]:offsets[g + 1]], photo)      # noqa: E731
    want, chained = cases.expected_sublabels(P_of, offsets)
    for g in range(len(offsets) - 1):
        assert np.array_equal(want[offsets[g]:offsets[g + 1]], cases.scipy_partition(P_of(g))), g
    k = np.diff(offsets)
    assert chained[k > cases.WAVE_MAX].all() and chained[k <= cases.WAVE_MAX].any()    # every chain class has work
    assert cases.expected_stats(offsets, chained)[1:3] == [int(chained[k <= cases.LDS_MAX].sum()), int((k > cases.LDS_MAX).sum())]
    P = P_of(len(k) - 1)
    assert np.array_equal(P, P.T) and set(np.unique(P[~np.eye(len(P), dtype=bool)])) <= {1, 2, 3, 4, 5, 101, 102, 103, 104, 105}
