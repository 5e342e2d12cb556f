"""Device-side image preparation: the resize + BGR + mean steps of
facerec_test.py:80-112 and facial_analysis.py:95-107 on the GPU, bit-exact with PIL / OpenCV's 8-bit paths.

Host work here is table building only (per-axis taps and integer weights, cached per size pair); the
pixels are resampled by hsefr_preprocess_pil_u8 / hsefr_preprocess_cv_u8.
"""
from __future__ import annotations

import ctypes
import math
from functools import lru_cache
from typing import Sequence, Tuple

import numpy as np

from . import _lib
from .preprocess import IMAGENET_CAFFE_BGR_MEAN, VGGFACE2_BGR_MEAN

COLOR_BGR_MEAN_F64, COLOR_RGB_UNIT, COLOR_BGR_MEAN_F32, COLOR_NONE_U8 = 0, 1, 2, 3
_PRECISION_BITS = 32 - 8 - 2      # Pillow: Resample.c


def pil_bilinear_coeffs(in_size: int, out_size: int) -> Tuple[np.ndarray, np.ndarray, np.ndarray, int]:
    """Pillow's precompute_coeffs + normalize_coeffs_8bpc for the BILINEAR filter (support 1.0):
    -> (first tap [out], tap count [out], int32 weights [out, ksize], ksize)."""
    scale = in_size / out_size
    filterscale = max(scale, 1.0)
    support = 1.0 * filterscale
    ksize = int(math.ceil(support)) * 2 + 1
    xmin = np.zeros(out_size, np.int32)
    cnt = np.zeros(out_size, np.int32)
    kk = np.zeros((out_size, ksize), np.float64)
    ss = 1.0 / filterscale
    for xx in range(out_size):
        center = (xx + 0.5) * scale
        lo = int(center - support + 0.5)
        lo = max(lo, 0)
        hi = int(center + support + 0.5)
        hi = min(hi, in_size)
        n = hi - lo
        ww = 0.0
        for x in range(n):
            a = (x + lo - center + 0.5) * ss
            w = 1.0 - abs(a) if abs(a) < 1.0 else 0.0
            kk[xx, x] = w
            ww += w
        if ww != 0.0:
            kk[xx, :n] /= ww
        xmin[xx], cnt[xx] = lo, n
    # normalize_coeffs_8bpc: round half away from zero into 22-bit fixed point
    ik = np.where(kk < 0, (kk * (1 << _PRECISION_BITS) - 0.5), (kk * (1 << _PRECISION_BITS) + 0.5)).astype(np.int64).astype(np.int32)
    return xmin, cnt, ik, ksize


def cv_linear_taps(in_size: int, out_size: int) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
    """OpenCV resize INTER_LINEAR, 8-bit: (index0, index1, 11-bit weight of index1) per output coordinate."""
    pos = ((np.arange(out_size, dtype=np.float64) + 0.5) * (in_size / out_size) - 0.5).astype(np.float32)
    base = np.floor(pos).astype(np.int64)
    frac = pos - base.astype(np.float32)
    edge = (base < 0) | (base >= in_size - 1)
    base = np.clip(base, 0, in_size - 1)
    frac = np.where(edge, np.float32(0), frac)
    nxt = np.minimum(base + 1, in_size - 1)
    w1 = np.rint(frac * np.float32(2048)).astype(np.int32)
    return base.astype(np.int32), nxt.astype(np.int32), w1


def _tight(xmin, cnt, coef, ksize):
    """Pillow sizes its table rows for ceil(support) * 2 + 1 taps; the rows hold at most floor(2 * support) + 1 (250 -> 192:
    three of five).  The device kernels loop over the table WIDTH (zero weights included), so hand them the tight table."""
    k = max(1, int(cnt.max()))
    return xmin, cnt, np.ascontiguousarray(coef[:, :k]), k


@lru_cache(maxsize=64)
def _pil_tables_dev(H: int, W: int, oh: int, ow: int, device_index: int):
    torch = _lib.require_gpu()
    dev = torch.device("cuda", device_index)
    xm, xc, xk, xks = _tight(*pil_bilinear_coeffs(W, ow))
    ym, yc, yk, yks = _tight(*pil_bilinear_coeffs(H, oh))
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    return (t(xm), t(xc), t(xk), xks, t(ym), t(yc), t(yk), yks)


@lru_cache(maxsize=256)
def _cv_tables_dev(H: int, W: int, oh: int, ow: int, device_index: int):
    torch = _lib.require_gpu()
    dev = torch.device("cuda", device_index)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    return tuple(t(a) for a in cv_linear_taps(W, ow)) + tuple(t(a) for a in cv_linear_taps(H, oh))


def _mean_array(imageNetUtilsMean: bool):
    m = IMAGENET_CAFFE_BGR_MEAN if imageNetUtilsMean else VGGFACE2_BGR_MEAN
    return (ctypes.c_double * 3)(float(m[0]), float(m[1]), float(m[2]))


def _as_u8_cuda(imgs, device=None):
    torch = _lib.require_gpu()
    if isinstance(imgs, np.ndarray):
        imgs = torch.from_numpy(np.ascontiguousarray(imgs, dtype=np.uint8)).to(_lib.cuda_device(device))
    elif device is not None and imgs.is_cuda and imgs.device != _lib.cuda_device(device):
        raise ValueError("images are on %s, expected %s" % (imgs.device, _lib.cuda_device(device)))
    if imgs.dtype != torch.uint8 or imgs.dim() != 4 or imgs.shape[3] != 3 or not imgs.is_cuda:
        raise ValueError("images must be a uint8 [n,H,W,3] RGB batch")
    return imgs.contiguous()


def preprocess_pil(imgs, out_hw: Tuple[int, int], convert2BGR: bool = True, imageNetUtilsMean: bool = True, device=None,
                   raw_u8: bool = False):
    """facerec_test.py:93-110 for a batch of same-size decoded RGB images -> CUDA float32 [n,oh,ow,3].
    A NumPy batch is uploaded to ``device`` (default: the current one); a CUDA batch stays where it is.
    raw_u8: stop after misc.imresize (:93) -- CUDA uint8 [n,oh,ow,3], RGB, for Engine.forward_u8, whose first kernel does the
    float conversion, channel reversal and mean subtraction (:95-106) inside its window load."""
    torch = _lib.require_gpu()
    x = _as_u8_cuda(imgs, device)
    n, H, W, _ = x.shape
    oh, ow = int(out_hw[0]), int(out_hw[1])
    if raw_u8 and (H, W) == (oh, ow):
        return x                      # Pillow's resize to the same size is the identity (coefficients 1.0)
    xm, xc, xk, xks, ym, yc, yk, yks = _pil_tables_dev(H, W, oh, ow, x.device.index or 0)
    tmp = torch.empty((n, H, ow, 3), dtype=torch.uint8, device=x.device)
    out = torch.empty((n, oh, ow, 3), dtype=torch.uint8 if raw_u8 else torch.float32, device=x.device)
    mode = COLOR_NONE_U8 if raw_u8 else (COLOR_BGR_MEAN_F64 if convert2BGR else COLOR_RGB_UNIT)
    with _lib.on_device(x):
        _lib.check(_lib.lib().hsefr_preprocess_pil_u8(x.data_ptr(), tmp.data_ptr(), out.data_ptr(), n, H, W, oh, ow, xm.data_ptr(),
                                                      xc.data_ptr(), xk.data_ptr(), xks, ym.data_ptr(), yc.data_ptr(), yk.data_ptr(),
                                                      yks, mode, _mean_array(imageNetUtilsMean), _lib.current_stream_ptr()),
                   "hsefr_preprocess_pil_u8")
    return out


def preprocess_cv(imgs, out_hw: Tuple[int, int], device=None, raw_u8: bool = False):
    """facial_analysis.py:95-107 (cv2.resize -> float32 -> BGR -> ImageNet-Caffe mean) for a same-size batch.
    raw_u8: stop after cv2.resize (:95) -- CUDA uint8 [n,oh,ow,3] RGB for Engine.forward_u8."""
    torch = _lib.require_gpu()
    x = _as_u8_cuda(imgs, device)
    n, H, W, _ = x.shape
    oh, ow = int(out_hw[0]), int(out_hw[1])
    if raw_u8 and (H, W) == (oh, ow):
        return x
    out = torch.empty((n, oh, ow, 3), dtype=torch.uint8 if raw_u8 else torch.float32, device=x.device)
    if (H, W) == (oh, ow):
        tabs = [None] * 6
    else:
        tabs = [t.data_ptr() for t in _cv_tables_dev(H, W, oh, ow, x.device.index or 0)]
    with _lib.on_device(x):
        _lib.check(_lib.lib().hsefr_preprocess_cv_u8(x.data_ptr(), out.data_ptr(), n, H, W, oh, ow, *tabs, COLOR_NONE_U8 if raw_u8 else COLOR_BGR_MEAN_F32,
                                                     _mean_array(True), _lib.current_stream_ptr()), "hsefr_preprocess_cv_u8")
    return out


def preprocess_faces_cv(crops: Sequence[np.ndarray], out_hw: Tuple[int, int], device=None, raw_u8: bool = False):
    """Variable-size face crops (process_image's per-box crops): grouped by size, one launch per group,
    results returned in input order as one CUDA float32 [n,oh,ow,3] tensor on ``device`` (raw_u8: the resized RGB bytes,
    uint8, for Engine.forward_u8)."""
    torch = _lib.require_gpu()
    oh, ow = out_hw
    dev = _lib.cuda_device(device)
    groups = {}
    for i, c in enumerate(crops):
        groups.setdefault(c.shape[:2], []).append(i)
    if len(groups) == 1:       # one face, or faces of one size: the resize kernel's own output, no scatter (two launches and an index upload less)
        return preprocess_cv(np.stack([np.ascontiguousarray(c, dtype=np.uint8) for c in crops]), out_hw, dev, raw_u8=raw_u8)
    out = torch.empty((len(crops), oh, ow, 3), dtype=torch.uint8 if raw_u8 else torch.float32, device=dev)
    for (h, w), idx in groups.items():
        batch = np.stack([np.ascontiguousarray(crops[i], dtype=np.uint8) for i in idx])
        out[torch.tensor(idx, device=dev)] = preprocess_cv(batch, out_hw, dev, raw_u8=raw_u8)
    return out


def face_crops(frames, boxes, out_hw: Tuple[int, int], out=None):
    """Every box of a stack of frames cut and resized in ONE launch (libhsefr_album.so, csrc/album.hip): ``frames`` a CUDA uint8
    [n, h, w, 3] stack (the one a detector pass uploaded), ``boxes`` host int32 [m, 5] rows (frame, x1, y1, x2, y2) with x2, y2
    exclusive -> CUDA uint8 [m, oh, ow, 3] with out[i] = cv2.resize(frames[f][y1:y2, x1:x2], (ow, oh)) byte for byte, channel order
    kept.  The library checks every box before any device work (ValueError) and uploads the table itself: one upload, whatever the box
    sizes.  ``out``: a contiguous CUDA uint8 [m, oh, ow, 3] tensor to write into (a slice of a larger batch)."""
    torch = _lib.require_gpu()
    if not (hasattr(frames, "is_cuda") and frames.is_cuda and frames.dtype == torch.uint8 and frames.dim() == 4 and frames.shape[3] == 3
            and frames.is_contiguous()):
        raise ValueError("frames must be a contiguous CUDA uint8 [n, h, w, 3] stack")
    table = np.ascontiguousarray(boxes, dtype=np.int32)
    if table.ndim != 2 or table.shape[1] != 5:
        raise ValueError("boxes must be [m, 5] rows of (frame, x1, y1, x2, y2), got shape %r" % (table.shape,))
    m, oh, ow = table.shape[0], int(out_hw[0]), int(out_hw[1])
    if out is None:
        out = torch.empty((m, oh, ow, 3), dtype=torch.uint8, device=frames.device)
    elif not (out.is_cuda and out.device == frames.device and out.dtype == torch.uint8 and tuple(out.shape) == (m, oh, ow, 3)
              and out.is_contiguous()):
        raise ValueError("out must be a contiguous uint8 [%d, %d, %d, 3] tensor on %s" % (m, oh, ow, frames.device))
    n, h, w, _ = frames.shape
    with _lib.on_device(frames):
        _lib.album_check(_lib.album_lib().hsefr_album_face_crops(frames.data_ptr(), n, h, w, table.ctypes.data, m, out.data_ptr(), oh, ow,
                                                                 _lib.current_stream_ptr()), "hsefr_album_face_crops")
    return out


FRAME_ROTATIONS = (0, 90, 270)


def check_rotation(rotation) -> int:
    """0, 90 or 270 (degrees clockwise), as process_photos.py turns a photo or a video frame; anything else is a ValueError."""
    if rotation not in FRAME_ROTATIONS:
        raise ValueError("rotation must be 0, 90 or 270, not %r" % (rotation,))
    return int(rotation)


def turn_frame(frame: np.ndarray, rotation: int) -> np.ndarray:
    """The host turn (process_photos.py:102-107): cv2.flip(cv2.transpose(x), 1) is a quarter turn clockwise (90), flip 0 a quarter
    turn counter-clockwise (270); a contiguous copy, or the frame itself for 0."""
    rotation = check_rotation(rotation)
    if rotation == 90:
        return np.ascontiguousarray(np.rot90(frame, -1))
    if rotation == 270:
        return np.ascontiguousarray(np.rot90(frame, 1))
    return frame


def prepare_frames(stack, rotation: int = 0, swap_rb: bool = True, out=None):
    """A stack of frames as decoded, turned upright and converted, in ONE launch (libhsefr_frames.so, csrc/frames.hip): ``stack`` a
    contiguous CUDA uint8 [n, h, w, 3] tensor -> CUDA uint8 [n, h, w, 3] for rotation 0, [n, w, h, 3] for 90 (np.rot90(x, -1) per
    frame, a quarter turn clockwise) and 270 (np.rot90(x, 1)), with channels 0 and 2 exchanged when ``swap_rb`` (BGR <-> RGB), byte for
    byte.  ``out``: a contiguous CUDA uint8 tensor of that shape to write into (a slice of a larger tensor will do); ``out=stack`` with
    rotation 0 runs in place.  ValueError before any launch for a host tensor, a wrong dtype or shape, a non-contiguous stack, a bad
    rotation and an ``out`` that does not fit."""
    import torch
    rotation = check_rotation(rotation)
    if not isinstance(stack, torch.Tensor):
        raise ValueError("stack must be a CUDA uint8 [n, h, w, 3] tensor, not %s" % type(stack).__name__)
    if stack.dtype != torch.uint8 or stack.dim() != 4 or stack.shape[3] != 3:
        raise ValueError("stack must be a uint8 [n, h, w, 3] tensor, got %s %r" % (stack.dtype, tuple(stack.shape)))
    if not stack.is_contiguous():
        raise ValueError("stack must be contiguous")
    if not stack.is_cuda:
        raise ValueError("stack must be a CUDA tensor (the caller uploads the decoded frames)")
    n, h, w, _ = (int(s) for s in stack.shape)
    shape = (n, h, w, 3) if rotation == 0 else (n, w, h, 3)
    if out is None:
        out = torch.empty(shape, dtype=torch.uint8, device=stack.device)
    elif not (getattr(out, "is_cuda", False) and out.device == stack.device and out.dtype == torch.uint8 and tuple(out.shape) == shape
              and out.is_contiguous()):
        raise ValueError("out must be a contiguous uint8 %r tensor on %s" % (shape, stack.device))
    if rotation != 0 and out.data_ptr() == stack.data_ptr() and n > 0:
        raise ValueError("a quarter turn cannot run in place")
    if n == 0 or h == 0 or w == 0:
        return out
    with _lib.on_device(stack):
        _lib.frames_check(_lib.frames_lib().hsefr_frames_prepare(stack.data_ptr(), out.data_ptr(), n, h, w, rotation, 1 if swap_rb else 0,
                                                                  _lib.current_stream_ptr()), "hsefr_frames_prepare")
    return out


def _packed_args(packed, shapes, offsets, what: str):
    """The checks prepare_packed and face_crops_packed share -> the host frame table (mtcnn_ragged.MIXED_FRAME_DT)."""
    import torch
    from .mtcnn_ragged import frame_table
    if not isinstance(packed, torch.Tensor):
        raise ValueError("%s must be a CUDA uint8 1-D tensor, not %s" % (what, type(packed).__name__))
    if packed.dtype != torch.uint8 or packed.dim() != 1:
        raise ValueError("%s must be a uint8 1-D tensor, got %s %r" % (what, packed.dtype, tuple(packed.shape)))
    if not packed.is_contiguous():
        raise ValueError("%s must be contiguous" % what)
    if not packed.is_cuda:
        raise ValueError("%s must be a CUDA tensor (the caller uploads the frames)" % what)
    shapes = [(int(h), int(w)) for h, w in shapes]
    for f, (h, w) in enumerate(shapes):
        if h < 1 or w < 1 or h * w * 3 >= 1 << 31:
            raise ValueError("frame %d: bad size %d x %d" % (f, h, w))
    if offsets is not None and len(offsets) != len(shapes):
        raise ValueError("%d offsets for %d frames" % (len(offsets), len(shapes)))
    table = frame_table(shapes, offsets)
    ends = table["offset"] + table["h"].astype(np.int64) * table["w"] * 3
    if len(table) and (int(table["offset"].min()) < 0 or int(ends.max()) > int(packed.shape[0])):
        raise ValueError("the frames do not fit %s of %d bytes (they end at byte %d)" % (what, int(packed.shape[0]), int(ends.max())))
    return table


def prepare_packed(packed, shapes, rotation: int = 0, swap_rb: bool = True, out=None, offsets=None):
    """prepare_frames for frames of DIFFERENT sizes packed in one buffer, in ONE launch (libhsefr_mixed.so, csrc/mixed_frames.hip):
    ``packed`` a contiguous CUDA uint8 1-D tensor that holds frame i as [h, w, 3] (``shapes[i]``, the SOURCE shapes) at byte
    ``offsets[i]`` (default: back to back in list order, mtcnn.ragged_plan's layout) -> a CUDA uint8 tensor of the same length with
    frame i at the same offset, as [h, w, 3] for rotation 0 and as [w, h, 3] for 90 (np.rot90(x, -1)) and 270 (np.rot90(x, 1)), with
    channels 0 and 2 exchanged when ``swap_rb``, byte for byte.  Bytes outside the frames are not written (those of a fresh ``out`` are
    undefined).  ``out``: a tensor like ``packed`` to write into; ``out=packed`` with rotation 0 runs in place.  ValueError before any
    launch for a host tensor, a wrong dtype or shape, frames that do not fit or overlap, a bad rotation and an ``out`` that does not
    fit."""
    import torch
    rotation = check_rotation(rotation)
    table = _packed_args(packed, shapes, offsets, "packed")
    if out is None:
        out = torch.empty_like(packed)
    elif not (isinstance(out, torch.Tensor) and out.is_cuda and out.device == packed.device and out.dtype == torch.uint8
              and tuple(out.shape) == tuple(packed.shape) and out.is_contiguous()):
        raise ValueError("out must be a contiguous uint8 %r tensor on %s" % (tuple(packed.shape), packed.device))
    if rotation != 0 and out.data_ptr() == packed.data_ptr() and len(table):
        raise ValueError("a quarter turn cannot run in place")
    if len(table) == 0:
        return out
    with _lib.on_device(packed):
        _lib.mixed_check(_lib.mixed_lib().hsefr_mixed_frames_prepare(packed.data_ptr(), out.data_ptr(), int(packed.shape[0]), table.ctypes.data,
                                                                      len(table), rotation, 1 if swap_rb else 0, _lib.current_stream_ptr()),
                         "hsefr_mixed_frames_prepare")
    return out


def face_crops_packed(packed, shapes, boxes, out_hw: Tuple[int, int], out=None, offsets=None):
    """face_crops for frames of DIFFERENT sizes packed in one buffer, in ONE launch (libhsefr_mixed.so): ``packed`` and ``offsets`` as
    prepare_packed takes them, ``shapes`` the (h, w) of the frames as they stand in the buffer, ``boxes`` host int32 [m, 5] rows
    (frame, x1, y1, x2, y2) with x2, y2 exclusive, checked against their own frame -> CUDA uint8 [m, oh, ow, 3] with
    out[i] = cv2.resize(frame[y1:y2, x1:x2], (ow, oh)) byte for byte.  ``out``: a contiguous CUDA uint8 [m, oh, ow, 3] tensor to write
    into (a slice of a larger batch).  ValueError before any launch for bad arguments."""
    import torch
    table = _packed_args(packed, shapes, offsets, "packed")
    rows = np.ascontiguousarray(boxes, dtype=np.int32)
    if rows.ndim != 2 or rows.shape[1] != 5:
        raise ValueError("boxes must be [m, 5] rows of (frame, x1, y1, x2, y2), got shape %r" % (rows.shape,))
    m, oh, ow = rows.shape[0], int(out_hw[0]), int(out_hw[1])
    if oh < 1 or ow < 1:
        raise ValueError("bad output size %d x %d" % (oh, ow))
    if out is None:
        out = torch.empty((m, oh, ow, 3), dtype=torch.uint8, device=packed.device)
    elif not (isinstance(out, torch.Tensor) and out.is_cuda and out.device == packed.device and out.dtype == torch.uint8
              and tuple(out.shape) == (m, oh, ow, 3) and out.is_contiguous()):
        raise ValueError("out must be a contiguous uint8 [%d, %d, %d, 3] tensor on %s" % (m, oh, ow, packed.device))
    if m == 0:
        return out
    with _lib.on_device(packed):
        _lib.mixed_check(_lib.mixed_lib().hsefr_mixed_face_crops(packed.data_ptr(), int(packed.shape[0]), table.ctypes.data, len(table),
                                                                  rows.ctypes.data, m, out.data_ptr(), oh, ow, _lib.current_stream_ptr()),
                         "hsefr_mixed_face_crops")
    return out


def face_crops_from(source, boxes, out_hw: Tuple[int, int], out=None):
    """The faces of one detector pass cut from whatever that pass left on the device: face_crops for a CUDA uint8 [n, h, w, 3] stack
    (a same-size pass), face_crops_packed for a mtcnn_ragged.PackedFrames (a mixed-size pass).  ``boxes``, ``out_hw`` and ``out`` as both
    take them."""
    from .mtcnn_ragged import PackedFrames
    if isinstance(source, PackedFrames):
        return face_crops_packed(source.data, source.shapes, boxes, out_hw, out=out)
    return face_crops(source, boxes, out_hw, out=out)
