"""CPU suite: the frame front end without a GPU -- the ABI of libhsefr_frames.so (include/hsefr_frames.h, the library's dynamic symbols and
_lib.FRAMES_SIGNATURES agree; gfx950 only; the ISA lint; every refused argument combination returns a status and a message before
any device work), the input rules of preprocess_device.prepare_frames, the rotation rule of process_images and of both album
functions, and the two other libraries' headers untouched."""
import ctypes
import importlib.util
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "hsefr_frames.h")
NAMES = ["hsefr_frames_last_error_string", "hsefr_frames_prepare", "hsefr_frames_version"]


def declared(header, prefix):
    src = re.sub(r"/\*.*?\*/", "", open(header).read(), flags=re.S)
    return sorted(set(re.findall(r"\b(%s[a-z0-9_]+)\s*\(" % prefix, src)))


# ---- the library -----------------------------------------------------------------------------------------------------------------
def test_header_library_and_binding_agree():
    from hse_facerec_tf_amd import _lib
    assert declared(HEADER, "hsefr_frames_") == NAMES
    assert os.path.exists(_lib.FRAMES_LIB_PATH), "run __graft_entry__.build() first"
    assert os.path.basename(_lib.FRAMES_LIB_PATH) == os.environ.get("HSEFR_FRAMES_LIB", "libhsefr_frames.so")
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.FRAMES_LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = sorted(l.split()[-1] for l in out.splitlines() if " T " in l and not l.split()[-1].startswith(("_init", "_fini")))
    assert exported == NAMES
    assert sorted(_lib.FRAMES_SIGNATURES) == NAMES
    L = _lib.frames_lib()
    assert L.hsefr_frames_version() == 100
    assert int(re.search(r"#define HSEFR_FRAMES_VERSION (\d+)", open(HEADER).read()).group(1)) == 100
    assert _lib.frames_lib() is L                                                       # loaded once


def test_the_other_two_libraries_are_untouched():
    from hse_facerec_tf_amd import _lib
    for header in ("hsefr.h", "hsefr_album.h"):
        assert "hsefr_frames_" not in open(os.path.join(ROOT, "include", header)).read(), header
    assert not [n for n in list(_lib.SIGNATURES) + list(_lib.ALBUM_SIGNATURES) if n.startswith("hsefr_frames")]
    assert sorted(_lib.ALBUM_SIGNATURES) == declared(os.path.join(ROOT, "include", "hsefr_album.h"), "hsefr_album_")
    assert os.path.getsize(_lib.LIB_PATH) < 4_000_000
    assert "HSEFR_KNOB" not in open(os.path.join(ROOT, "hse_facerec_tf_amd", "csrc", "frames.hip")).read()
    for lib in (_lib.LIB_PATH, _lib.ALBUM_LIB_PATH):                                    # neither exports a name of the third
        out = subprocess.run(["nm", "-D", "--defined-only", lib], capture_output=True, text=True, check=True).stdout
        assert "hsefr_frames_" not in out, lib


def test_frames_code_object_targets_gfx950_only():
    from hse_facerec_tf_amd import _lib
    blob = open(_lib.FRAMES_LIB_PATH, "rb").read()
    assert b"gfx950" in blob
    for other in (b"gfx942", b"gfx90a", b"sm_90", b"gfx1100"):
        assert other not in blob


def test_frames_device_code_passes_the_isa_lint():
    if not os.path.exists("/opt/rocm/lib/llvm/bin/llvm-objdump"):
        pytest.skip("no llvm-objdump on this machine")
    spec = importlib.util.spec_from_file_location("isa_lint", os.path.join(ROOT, "tools", "isa_lint.py"))
    lint = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(lint)
    from hse_facerec_tf_amd import _lib
    findings, n_symbols, n_stores = lint.lint(_lib.FRAMES_LIB_PATH)
    # the vector forms of both kernels: swap_kernel<true>, and the three turn_kernel instances with a 12-byte side
    assert n_symbols >= 6 and n_stores >= 3, "the lint did not see the kernels and their 12-byte stores"
    assert findings == []


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
