"""CPU suite: the device stages of a mixed-size pass without a GPU -- the names libhsefr_mixed.so exports and its table's layout (what
holds for every library is in tests/test_libraries_cpu.py), the per-pixel bodies it shares with album.hip and frames.hip, every refused argument of its two entry points and of their Python wrappers before any device
work, PackedFrames' layout, which side of a quarter turn takes which path for the shapes the GPU suite uses, and the album's keyword."""
import ctypes
import os
import re

import numpy as np
import pytest

import build_table

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "hse_facerec_tf_amd", "csrc")
HEADER = os.path.join(ROOT, "include", "hsefr_mixed.h")
NAMES = ["hsefr_mixed_face_crops", "hsefr_mixed_frames_prepare", "hsefr_mixed_last_error_string", "hsefr_mixed_version"]
# the shapes of tests/test_mixed_gpu.py
SHAPES = [(72, 132), (64, 48), (66, 40), (40, 70), (37, 53), (68, 36), (5, 7), (1, 9), (9, 1), (66, 129), (12, 12)]


# ---- the library -----------------------------------------------------------------------------------------------------------------
def test_header_library_and_binding_agree():
    from hse_facerec_tf_amd import _lib
    assert sorted(_lib.MIXED_SIGNATURES) == NAMES
    assert "HSEFR_KNOB" not in open(os.path.join(CSRC, "mixed_frames.hip")).read()


def test_the_table_has_the_headers_layout():
    from hse_facerec_tf_amd import mtcnn_ragged as mr
    body, size = re.search(r"typedef struct \{([^}]*)\} hsefr_mixed_frame;\s*/\* (\d+) bytes \*/", open(HEADER).read(), flags=re.S).groups()
    fields = [f.strip() for decl in re.findall(r"(?:int64_t|int32_t)\s+([^;]+);", body) for f in decl.split(",")]
    assert fields == list(mr.MIXED_FRAME_DT.names) == ["offset", "h", "w"]
    assert mr.MIXED_FRAME_DT.itemsize == int(size) == 16
    assert [mr.MIXED_FRAME_DT.fields[f][1] for f in fields] == [0, 8, 12]


def test_the_libraries_compile_the_shared_per_pixel_bodies():
    """The byte identity with libhsefr_album.so and libhsefr_frames.so rests on it: the bodies live in the two headers, and the old
    sources and the new one include them instead of holding a copy."""
    cv, px = open(os.path.join(CSRC, "cv_linear_px.h")).read(), open(os.path.join(CSRC, "frames_px.h")).read()
    cv_bodies, px_bodies = ("linear_tap", "linear_blend"), ("unpack4", "pack4", "store_px4", "load_pixel", "store_pixel", "swap_02")
    for body in cv_bodies:
        assert re.search(r"__device__[^;{]*\b%s\(" % body, cv), body
    for body in px_bodies:
        assert re.search(r"__device__[^;{]*\b%s\(" % body, px), body
    assert re.search(r"struct[^;{]*\bPx4\s*\{", px) and "s_nop 1" in px                  # the 12-byte unit and its store's guard
    assert "fp contract(off)" in cv
    for source, headers in (("album.hip", ["cv_linear_px.h"]), ("frames.hip", ["frames_px.h"]),
                            ("mixed_frames.hip", ["cv_linear_px.h", "frames_px.h"])):
        src = open(os.path.join(CSRC, source)).read()
        for h in headers:
            assert '#include "%s"' % h in src, (source, h)
        for body in cv_bodies + px_bodies:
            assert not re.search(r"__device__[^;{]*\b%s\(" % body, src), (source, body)       # called, not defined again
        assert not re.search(r"struct[^;{]*\bPx4\s*\{", src), source
    # each is rebuilt when a header it includes changes, and the crops' taps round twice in both libraries
    assert build_table.stale_against("album", "cv_linear_px.h", "include/hsefr_album.h")
    assert build_table.stale_against("frames", "frames_px.h", "include/hsefr_frames.h")
    assert build_table.stale_against("mixed", "cv_linear_px.h", "frames_px.h", "include/hsefr_mixed.h")
    table = build_table.rows()
    assert "-ffp-contract=off" in table["mixed"]["flags"] and "-ffp-contract=off" in table["album"]["flags"]
    assert "-ffp-contract=off" not in table["hsefr"]["flags"] and "-ffp-contract=off" not in table["frames"]["flags"]
    assert [f for f in table["mixed"]["flags"] if f != "-ffp-contract=off"] == table["hsefr"]["flags"] == table["frames"]["flags"]
    assert table["mixed"]["flags"] == table["album"]["flags"] and table["mixed"]["srcs"] == ["mixed_frames.hip"]


# ---- argument checks before any device work ------------------------------------------------------------------------------------------
def table_of(rows):
    from hse_facerec_tf_amd.mtcnn_ragged import MIXED_FRAME_DT
    return np.array(rows, MIXED_FRAME_DT)


@pytest.fixture()
def host():
    """A host buffer whose address stands in for every device pointer: no call below reaches a launch."""
    from hse_facerec_tf_amd import _lib
    buf = ctypes.create_string_buffer(4096)
    return _lib, _lib.mixed_lib(), ctypes.cast(buf, ctypes.c_void_p).value, buf


def refused(_lib, rc, status, word):
    msg = _lib.mixed_last_error()
    assert rc == status and word in msg, (rc, msg, word)


def test_frames_prepare_checks_its_arguments_without_a_gpu(host):
    _lib, L, p, _ = host
    good = table_of([(0, 4, 5), (60, 2, 3)])                                           # 60 and 18 bytes

    def call(src=p, dst=p + 2048, nbytes=78, table=good, n=None, rotation=90, swap=1):
        return L.hsefr_mixed_frames_prepare(src, dst, nbytes, None if table is None else table.ctypes.data, len(table) if n is None else n,
                                            rotation, swap, None)
    assert call(n=0) == 0 and call(n=0, src=None, dst=None, table=None) == 0           # nothing to do: OK, whatever the pointers
    for rotation in (1, 180, -90, 360):
        refused(_lib, call(rotation=rotation), _lib.ERR_INVALID, "rotation")
        refused(_lib, call(rotation=rotation, n=0), _lib.ERR_INVALID, "rotation")    # a bad scalar is refused for an empty table too
    refused(_lib, call(n=-1), _lib.ERR_INVALID, "negative size")
    refused(_lib, call(nbytes=-1), _lib.ERR_INVALID, "negative size")
    refused(_lib, call(src=None), _lib.ERR_INVALID, "null source")
    refused(_lib, call(dst=None), _lib.ERR_INVALID, "null destination")
    refused(_lib, call(table=None, n=2), _lib.ERR_INVALID, "null table")
    for rotation in (90, 270):
        refused(_lib, call(dst=p, rotation=rotation), _lib.ERR_INVALID, "in place")
    refused(_lib, call(nbytes=77), _lib.ERR_INVALID, "past the buffer")               # the last frame ends one byte behind it
    refused(_lib, call(table=table_of([(0, 4, 5), (-1, 2, 3)])), _lib.ERR_INVALID, "offset -1")
    for h, w in ((0, 3), (3, 0), (-2, 3)):
        refused(_lib, call(table=table_of([(0, h, w)])), _lib.ERR_INVALID, "bad frame size")
    refused(_lib, call(table=table_of([(0, 30000, 30000)]), nbytes=1 << 40), _lib.ERR_UNSUPPORTED, "too large")
    # overlaps: by one byte, a frame inside another, the same frame twice, and rows that are not in offset order
    for rows in ([(0, 4, 5), (59, 2, 3)], [(0, 4, 5), (3, 1, 1)], [(0, 4, 5), (0, 4, 5)], [(60, 2, 3), (100, 1, 1), (59, 1, 1)]):
        refused(_lib, call(table=table_of(rows), nbytes=4096), _lib.ERR_INVALID, "overlap")
    with pytest.raises(ValueError, match="overlap"):
        _lib.mixed_check(call(table=table_of([(0, 4, 5), (59, 2, 3)])), "hsefr_mixed_frames_prepare")
    with pytest.raises(NotImplementedError, match="too large"):
        _lib.mixed_check(call(table=table_of([(0, 30000, 30000)]), nbytes=1 << 40), "hsefr_mixed_frames_prepare")


def test_face_crops_checks_its_arguments_without_a_gpu(host):
    _lib, L, p, _ = host
    frames = table_of([(0, 10, 12), (360, 40, 50)])                                    # a small frame, then a larger one

    def call(src=p, nbytes=6360, table=frames, n=None, boxes=((1, 0, 0, 50, 40),), m=None, out=p + 2048, oh=8, ow=8):
        rows = np.ascontiguousarray(boxes, dtype=np.int32).reshape(-1, 5)
        return L.hsefr_mixed_face_crops(src, nbytes, None if table is None else table.ctypes.data, len(table) if n is None else n,
                                        rows.ctypes.data if len(rows) else None, len(rows) if m is None else m, out, oh, ow, None)
    assert call(boxes=()) == 0 and call(boxes=(), src=None, table=None, n=0, out=None, oh=0) == 0
    assert L.hsefr_mixed_face_crops(None, -5, None, -1, None, 0, None, 0, 0, None) == 0        # m = 0: OK, whatever else it was given
    refused(_lib, call(m=-1), _lib.ERR_INVALID, "m = -1")
    refused(_lib, call(src=None), _lib.ERR_INVALID, "null frames")
    refused(_lib, call(out=None), _lib.ERR_INVALID, "null out")
    refused(_lib, call(table=None, n=2), _lib.ERR_INVALID, "null table")
    refused(_lib, L.hsefr_mixed_face_crops(p, 6360, frames.ctypes.data, 2, None, 1, p, 8, 8, None), _lib.ERR_INVALID, "null boxes")
    refused(_lib, call(n=-1), _lib.ERR_INVALID, "negative size")
    for oh, ow in ((0, 8), (8, 0), (-1, 8)):
        refused(_lib, call(oh=oh, ow=ow), _lib.ERR_INVALID, "bad output size")
    refused(_lib, call(nbytes=6359), _lib.ERR_INVALID, "past the buffer")
    refused(_lib, call(table=table_of([(0, 10, 12), (359, 40, 50)])), _lib.ERR_INVALID, "overlap")
    # a box is checked against ITS frame: these lie inside the larger frame 1 and outside frame 0 (10 x 12)
    for box in ((0, 0, 0, 13, 10), (0, 0, 0, 12, 11), (0, 5, 5, 50, 40), (0, -1, 0, 5, 5), (0, 0, -1, 5, 5)):
        refused(_lib, call(boxes=(box,)), _lib.ERR_INVALID, "outside the 12 x 10 frame 0")
    refused(_lib, call(boxes=((1, 0, 0, 51, 40),)), _lib.ERR_INVALID, "outside the 50 x 40 frame 1")
    refused(_lib, call(boxes=((1, 0, 0, 5, 5), (2, 0, 0, 5, 5))), _lib.ERR_INVALID, "box 1 names frame 2 of 2")        # frame n_frames
    refused(_lib, call(boxes=((-1, 0, 0, 5, 5),)), _lib.ERR_INVALID, "names frame -1")
    refused(_lib, call(boxes=((0, 0, 0, 5, 5),), n=0), _lib.ERR_INVALID, "names frame 0 of 0")
    for box in ((1, 5, 5, 5, 9), (1, 5, 5, 9, 5), (1, 9, 5, 5, 9)):
        refused(_lib, call(boxes=(box,)), _lib.ERR_INVALID, "is empty")
    refused(_lib, call(oh=4000, ow=97), _lib.ERR_UNSUPPORTED, "tap tables")           # oh + ow = 4097
    with pytest.raises(ValueError, match="outside"):
        _lib.mixed_check(call(boxes=((0, 0, 0, 13, 10),)), "hsefr_mixed_face_crops")
    with pytest.raises(NotImplementedError, match="tap tables"):
        _lib.mixed_check(call(oh=4096, ow=1), "hsefr_mixed_face_crops")


def test_the_wrappers_raise_before_any_device_work():
    """Host tensors stand in: every call is refused before a device is asked for."""
    import torch
    from hse_facerec_tf_amd import preprocess_device as pd
    buf = torch.zeros(100, dtype=torch.uint8)
    for fn in (lambda x, **kw: pd.prepare_packed(x, [(2, 3)], **kw), lambda x, **kw: pd.face_crops_packed(x, [(2, 3)], [[0, 0, 0, 1, 1]], (4, 4), **kw)):
        with pytest.raises(ValueError, match="not ndarray"):
            fn(np.zeros(100, np.uint8))
        with pytest.raises(ValueError, match="uint8 1-D"):
            fn(buf.float())
        with pytest.raises(ValueError, match="uint8 1-D"):
            fn(buf.reshape(10, 10))
        with pytest.raises(ValueError, match="contiguous"):
            fn(buf[::2])
        with pytest.raises(ValueError, match="CUDA"):
            fn(buf)
    with pytest.raises(ValueError, match="rotation"):
        pd.prepare_packed(buf, [(2, 3)], rotation=180)


def test_process_images_refuses_mixed_device_without_its_companions():
    from hse_facerec_tf_amd.facial_analysis import FacialImageProcessing

    class Sess:
        accepts_u8 = True

    class Proc:
        device_preprocess, sess, detector = True, Sess(), None

        def device_frames_supported(self):
            raise AssertionError("checked before the keyword's own rule")
    frames = [np.zeros((40, 40, 3), np.uint8)]
    with pytest.raises(ValueError, match="mixed_device needs mixed_sizes"):
        FacialImageProcessing.process_images(Proc(), frames, device_frames=True, mixed_device=True)
    with pytest.raises(ValueError, match="mixed_device needs device_crops=True or device_frames=True"):
        FacialImageProcessing.process_images(Proc(), frames, mixed_sizes=True, mixed_device=True)

    class Proc2(Proc):
        def device_frames_supported(self):
            return True
    with pytest.raises(ValueError, match="detect_packed"):                              # a detector without the packed entry
        FacialImageProcessing.process_images(Proc2(), frames, mixed_sizes=True, device_crops=True, mixed_device=True)
    assert FacialImageProcessing._packed_kw(False) == {} and FacialImageProcessing._packed_kw(True) == {"packed_sources": True}


# ---- the layout ---------------------------------------------------------------------------------------------------------------------------
def test_packed_frames_offsets_are_the_plans():
    import torch
    from hse_facerec_tf_amd import mtcnn
    from hse_facerec_tf_amd.mtcnn_ragged import PackedFrames, frame_table, packed_offsets
    for shapes in (SHAPES, [(37, 53), (64, 48)], [(588, 784), (784, 588), (90, 200)], [(5, 7)]):
        plan = mtcnn.ragged_plan(shapes, 32, 0.709)
        data = torch.arange(plan.frames_bytes + 5, dtype=torch.int64).to(torch.uint8)
        packed = PackedFrames(data, shapes)
        assert packed.offsets.dtype == np.int64 and np.array_equal(packed.offsets, plan.frames["offset"])
        assert packed.shapes == plan.shapes and packed.nbytes == plan.frames_bytes and len(packed) == len(shapes)
        t = packed.table
        assert np.array_equal(t["offset"], plan.frames["offset"]) and np.array_equal(t["h"], plan.frames["h"]) and np.array_equal(t["w"], plan.frames["w"])
        for i, (h, w) in enumerate(shapes):
            view = packed.frame(i)
            assert tuple(view.shape) == (h, w, 3) and view.data_ptr() == data.data_ptr() + int(packed.offsets[i])
    assert len(packed_offsets([])) == 0 and len(frame_table([])) == 0
    with pytest.raises(ValueError, match="buffer has"):
        PackedFrames(torch.zeros(104, dtype=torch.uint8), [(5, 7)])
    with pytest.raises(ValueError, match="bad size"):
        PackedFrames(torch.zeros(104, dtype=torch.uint8), [(0, 7)])
    with pytest.raises(ValueError, match="1-D"):
        PackedFrames(torch.zeros((5, 7, 3), dtype=torch.uint8), [(5, 7)])


def test_the_gpu_suites_shapes_take_every_path():
    """Which side of a quarter turn takes the 12-byte path is decided per frame from its address and its size (csrc/mixed_frames.hip):
    for the GPU suite's list on a 4-byte aligned buffer, as the issue states it."""
    from hse_facerec_tf_amd import mtcnn
    off = [int(o) for o in mtcnn.ragged_plan(SHAPES, 32, 0.709).frames["offset"]]
    assert [o % 4 for o in off] == [0, 0, 0, 0, 0, 3, 3, 0, 3, 2, 0]
    load = [o % 4 == 0 and w % 4 == 0 for o, (h, w) in zip(off, SHAPES)]
    store = [o % 4 == 0 and h % 4 == 0 for o, (h, w) in zip(off, SHAPES)]
    both = [s for s, a, b in zip(SHAPES, load, store) if a and b]
    assert both == [(72, 132), (64, 48), (12, 12)]
    assert [s for s, a, b in zip(SHAPES, load, store) if a and not b] == [(66, 40)]
    assert [s for s, a, b in zip(SHAPES, load, store) if b and not a] == [(40, 70)]
    assert (68, 36) not in both and 68 % 4 == 0 and 36 % 4 == 0                         # the sizes would do, the offset does not
    assert [s for s in SHAPES if s[0] > 64 and s[1] > 64 and s[0] % 64 and s[1] % 64] == [(72, 132), (66, 129)]      # tiles both ways, cut edges
    assert sum(h * w for h, w in [(37, 53), (64, 48)]) == 5033 and 5033 % 4 == 1        # the rotation-0 tail


# ---- the album's keyword ---------------------------------------------------------------------------------------------------------------
class StandIn:
    """An img_processing that records what process_album / process_video hand to process_images and finds no face."""
    device_preprocess = True

    class sess:
        accepts_u8, device = True, None

    def __init__(self, detector=None, takes_keyword=True):
        self.detector, self.calls, self.takes_keyword = detector, [], takes_keyword

    def device_frames_supported(self):
        return True

    def process_images(self, draws, max_frames=32, device_crops=False, return_crops=False, rotation=0, device_frames=False, **kw):
        if not self.takes_keyword and "mixed_device" in kw:
            raise TypeError("process_images() got an unexpected keyword argument 'mixed_device'")
        self.calls.append(dict(kw))
        res = [([], [], [], [], []) for _ in draws]
        return (res, [np.empty((0, 224, 224, 3), np.uint8) for _ in draws]) if return_crops else res


class Packed:
    device_boxes = True

    def detect_ragged(self, frames):
        return []

    def detect_packed(self, packed):
        return []


def test_the_album_passes_the_keyword_on_only_when_it_is_in_use(monkeypatch):
    from hse_facerec_tf_amd import album
    assert album.MIXED_DEVICE_DEFAULT in (True, False)
    photos, dates = [np.zeros((40, 50, 3), np.uint8), np.zeros((50, 40, 3), np.uint8)], [1.6e9] * 2
    video = ([np.zeros((30, 30, 3), np.uint8)] * 6, 1.6e9 + 86400.0)

    def keywords(proc, **kw):
        album.process_album(proc, photos, dates, videos=[video], **kw)
        assert len(proc.calls) == 4                                                     # three passes over the photos, one video window
        assert all(c == proc.calls[0] for c in proc.calls)                              # the video gets what the photos get
        return proc.calls[0]
    # asked: the caller's word, whatever the default and the detector
    assert keywords(StandIn(Packed()), mixed_device=True) == dict(mixed_sizes=True, mixed_device=True)
    assert keywords(StandIn(Packed()), mixed_device=False) == dict(mixed_sizes=True)
    assert keywords(StandIn(None), mixed_sizes=True, mixed_device=True) == dict(mixed_sizes=True, mixed_device=True)
    # unasked: the default, and then only where the mixed-size passes, the device crops or frames and a detector with detect_packed are
    for default in (False, True):
        monkeypatch.setattr(album, "MIXED_DEVICE_DEFAULT", default)
        on = dict(mixed_sizes=True, mixed_device=True) if default and album.MIXED_SIZES_DEFAULT else \
            (dict(mixed_sizes=True) if album.MIXED_SIZES_DEFAULT else {})
        assert keywords(StandIn(Packed())) == on
        assert "mixed_device" not in keywords(StandIn(Packed()), mixed_sizes=False)
        assert "mixed_device" not in keywords(StandIn(Packed()), mixed_sizes=True, device_crops=False, device_frames=False)
        assert "mixed_device" not in keywords(StandIn(None), mixed_sizes=True)
        assert keywords(StandIn(Packed(), takes_keyword=False), mixed_device=False) == (dict(mixed_sizes=True) if album.MIXED_SIZES_DEFAULT else {})
    # an img_processing written without the keyword keeps working as long as nobody asks for it
    monkeypatch.setattr(album, "MIXED_DEVICE_DEFAULT", False)
    assert "mixed_device" not in keywords(StandIn(Packed(), takes_keyword=False))
    with pytest.raises(TypeError, match="mixed_device"):
        album.process_album(StandIn(Packed(), takes_keyword=False), photos, dates, mixed_device=True)
    assert album._use_mixed_device(StandIn(Packed()), None, True, True, True) is False
    assert album._use_mixed_device(StandIn(Packed()), True, False, False, False) is True
