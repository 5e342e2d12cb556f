"""CPU suite: the frame front end without a GPU -- the names libhsefr_frames.so exports (what holds for every library is in
tests/test_libraries_cpu.py), every refused argument combination returns a status and a message before any device work, the input
rules of preprocess_device.prepare_frames, and the rotation rule of process_images and of both album functions."""
import ctypes
import os

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["hsefr_frames_last_error_string", "hsefr_frames_prepare", "hsefr_frames_version"]


# ---- the library -----------------------------------------------------------------------------------------------------------------
def test_header_library_and_binding_agree():
    from hse_facerec_tf_amd import _lib
    assert sorted(_lib.FRAMES_SIGNATURES) == NAMES
    assert "HSEFR_KNOB" not in open(os.path.join(ROOT, "hse_facerec_tf_amd", "csrc", "frames.hip")).read()


def test_prepare_checks_its_arguments_without_a_gpu():
    from hse_facerec_tf_amd import _lib
    L = _lib.frames_lib()
    buf = ctypes.create_string_buffer(4096)
    p = ctypes.cast(buf, ctypes.c_void_p).value
    q = p + 2048

    def call(src=p, dst=q, n=2, h=10, w=12, rotation=0, swap_rb=1):
        rc = L.hsefr_frames_prepare(src, dst, n, h, w, rotation, swap_rb, None)
        return rc, _lib.frames_last_error()
    refused = [(dict(rotation=r), _lib.ERR_INVALID, "rotation") for r in (180, 1, -90, 360, 45)]
    refused += [(dict(n=-1), _lib.ERR_INVALID, "n = -1")]
    refused += [(kw, _lib.ERR_INVALID, "frame size") for kw in (dict(h=0), dict(w=0), dict(h=-3), dict(w=-1), dict(h=0, w=0))]
    # 3 h w >= 2^31: at the bound, past it, and where the product wraps around in 32 bits
    refused += [(kw, _lib.ERR_UNSUPPORTED, "too large") for kw in (dict(h=32768, w=21846), dict(h=1 << 16, w=1 << 16), dict(h=46341, w=46341),
                                                                   dict(h=(1 << 31) - 1, w=(1 << 31) - 1))]
    refused += [(dict(src=None), _lib.ERR_INVALID, "null source"), (dict(dst=None), _lib.ERR_INVALID, "null destination"),
                (dict(src=None, dst=None), _lib.ERR_INVALID, "null")]
    refused += [(dict(dst=p, rotation=r), _lib.ERR_INVALID, "in place") for r in (90, 270)]
    for kw, status, word in refused:
        for extra in (dict(), dict(swap_rb=0), dict(n=1)):
            rc, msg = call(**dict(extra, **kw))
            assert rc == status and word in msg, (kw, extra, rc, msg)
    # a bad argument is refused for an empty stack too
    for kw in (dict(rotation=180), dict(h=0), dict(h=32768, w=21846)):
        rc, msg = call(n=0, **kw)
        assert rc != 0 and msg, (kw, rc, msg)
    with pytest.raises(ValueError, match="rotation 180"):
        _lib.frames_check(call(rotation=180)[0], "hsefr_frames_prepare")
    with pytest.raises(NotImplementedError, match="too large"):
        _lib.frames_check(call(h=32768, w=21846)[0], "hsefr_frames_prepare")
    # the largest frame below the bound passes the checks (n == 0: nothing is launched)
    assert call(n=0, h=32768, w=21845)[0] == 0
    # n == 0: a no-op that returns 0, whatever the pointers, at every rotation
    for rotation in (0, 90, 270):
        assert call(n=0, rotation=rotation)[0] == 0
        assert call(n=0, src=None, dst=None, rotation=rotation)[0] == 0
        assert call(n=0, dst=p, rotation=rotation)[0] == 0


# ---- the Python face ---------------------------------------------------------------------------------------------------------------
def test_prepare_frames_refuses_bad_input_before_any_launch(monkeypatch):
    import torch
    from hse_facerec_tf_amd import _lib, preprocess_device
    monkeypatch.setattr(_lib, "frames_lib", lambda: pytest.fail("the library was reached"))
    good = torch.zeros((2, 6, 8, 3), dtype=torch.uint8)
    with pytest.raises(ValueError, match="CUDA"):
        preprocess_device.prepare_frames(good)                                         # a host tensor
    with pytest.raises(ValueError, match="tensor"):
        preprocess_device.prepare_frames(good.numpy())                                 # a host array
    for bad in (good.float(), good.to(torch.int8), good[0], good[..., :2], torch.zeros((2, 6, 8, 4), dtype=torch.uint8),
                torch.zeros((2, 3, 6, 8), dtype=torch.uint8)):
        with pytest.raises(ValueError, match="uint8 \\[n, h, w, 3\\]"):
            preprocess_device.prepare_frames(bad)
    for view in (good[:, ::2], good[:, :, 1:], good.permute(0, 2, 1, 3), torch.zeros((2, 6, 8, 4), dtype=torch.uint8)[..., :3]):
        assert not view.is_contiguous()
        with pytest.raises(ValueError, match="contiguous"):
            preprocess_device.prepare_frames(view)
    for rotation in (180, 1, -90, 360, None, "90", 90.5):
        with pytest.raises(ValueError, match="rotation"):
            preprocess_device.prepare_frames(good, rotation=rotation)
    assert [preprocess_device.check_rotation(r) for r in (0, 90, 270)] == [0, 90, 270]


def test_the_host_turn_is_the_reference_transpose_and_flip():
    from hse_facerec_tf_amd import preprocess_device
    x = np.random.RandomState(2).randint(0, 256, (5, 7, 3)).astype(np.uint8)
    t = np.transpose(x, (1, 0, 2))
    assert preprocess_device.turn_frame(x, 0) is x
    cw, ccw = preprocess_device.turn_frame(x, 90), preprocess_device.turn_frame(x, 270)
    assert np.array_equal(cw, t[:, ::-1]) and np.array_equal(ccw, t[::-1])             # cv2.flip(., 1): around the y axis; (., 0): the x axis
    assert cw.shape == ccw.shape == (7, 5, 3) and cw.flags.c_contiguous and ccw.flags.c_contiguous
    with pytest.raises(ValueError, match="rotation"):
        preprocess_device.turn_frame(x, 180)


def test_rotation_180_is_refused_before_any_work():
    from hse_facerec_tf_amd import album
    from hse_facerec_tf_amd.facial_analysis import FacialImageProcessing

    class Untouchable:
        def __getattr__(self, name):
            pytest.fail("the processing object was used (%s)" % name)

    def frames():
        pytest.fail("a frame was read")
        yield
    with pytest.raises(ValueError, match="rotation"):
        FacialImageProcessing.process_images(Untouchable(), frames(), rotation=180)
    with pytest.raises(ValueError, match="rotation"):
        FacialImageProcessing.process_images(Untouchable(), frames(), rotation=180, device_frames=True)
    with pytest.raises(ValueError, match="rotation"):
        album.process_video(Untouchable(), frames(), 0.0, rotation=180)
    with pytest.raises(ValueError, match="rotation"):
        album.process_album(Untouchable(), [], [], videos=[(frames(), 0.0), (frames(), 0.0, 180)])
    assert album.DEVICE_FRAMES_DEFAULT in (True, False) and album.DEVICE_CROPS_DEFAULT is True
