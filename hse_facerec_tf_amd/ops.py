"""Per-kernel Python entry points: torch CUDA tensors in, torch CUDA tensors out, through the
C ABI of libhsefr (include/hsefr.h "Per-kernel entry points").  Used by the unit parity tests
and by the identification stage; the engine calls the same launchers internally."""
from __future__ import annotations

import ctypes
import math
from typing import Optional, Tuple

import numpy as np

from . import _lib
from .lowering import ACT_NONE, ACT_RELU, ACT_RELU6, ACT_SIGMOID, tf_same_padding  # noqa: F401


def _device_guarded(fn):
    """Run the launch with the device of the first CUDA tensor argument current (stream + launch target = the
    device that owns the pointers); mixing devices in one call is an error, not a memory fault."""
    import functools

    @functools.wraps(fn)
    def wrapper(*args, **kw):
        devs = [a.device for a in list(args) + list(kw.values()) if hasattr(a, "is_cuda") and a.is_cuda]
        if not devs:
            return fn(*args, **kw)
        if any(d != devs[0] for d in devs):
            raise ValueError("%s: tensors live on different devices: %s" % (fn.__name__, sorted({str(d) for d in devs})))
        with _lib.on_device(devs[0]):
            return fn(*args, **kw)
    return wrapper


def _f32c(t, name):
    torch = _lib.require_gpu()
    if not (t.is_cuda and t.dtype == torch.float32 and t.is_contiguous()):
        raise ValueError("%s must be a contiguous float32 CUDA tensor" % name)
    return t


def _same(h: int, w: int, k: int, stride: int) -> Tuple[int, int, int, int]:
    oh, pt = tf_same_padding(h, k, stride)
    ow, pl = tf_same_padding(w, k, stride)
    return oh, ow, pt, pl


@_device_guarded
def conv3x3_c3(x, w_hwio, shift, stride: int = 2, act: int = ACT_RELU6):
    """Conv2D 3x3 SAME over a 3-channel NHWC image + shift + act (graph nodes #30-34)."""
    torch = _lib.require_gpu()
    _f32c(x, "x"), _f32c(w_hwio, "w"), _f32c(shift, "shift")
    n, h, w, c = x.shape
    if c != 3 or tuple(w_hwio.shape[:3]) != (3, 3, 3):
        raise ValueError("conv3x3_c3 wants x [n,h,w,3] and w [3,3,3,cout]")
    cout = w_hwio.shape[3]
    oh, ow, pt, pl = _same(h, w, 3, stride)
    y = torch.empty((n, oh, ow, cout), dtype=torch.float32, device=x.device)
    _lib.check(_lib.lib().hsefr_conv_c3_bias_act(x.data_ptr(), w_hwio.data_ptr(), shift.data_ptr(), y.data_ptr(),
                                                 n, h, w, 3, 3, stride, pt, pl, oh, ow, cout, act,
                                                 _lib.current_stream_ptr()), "hsefr_conv_c3_bias_act")
    return y


@_device_guarded
def dwconv3x3(x, w_hwc, scale, shift, stride: int = 1, act: int = ACT_RELU6):
    """DepthwiseConv2dNative 3x3 SAME + scale + shift + act (graph nodes #35-39,#44)."""
    torch = _lib.require_gpu()
    _f32c(x, "x"), _f32c(w_hwc, "w"), _f32c(scale, "scale"), _f32c(shift, "shift")
    n, h, w, c = x.shape
    oh, ow, pt, pl = _same(h, w, 3, stride)
    y = torch.empty((n, oh, ow, c), dtype=torch.float32, device=x.device)
    _lib.check(_lib.lib().hsefr_dwconv3x3_bn_relu6(x.data_ptr(), w_hwc.data_ptr(), scale.data_ptr(), shift.data_ptr(),
                                                   y.data_ptr(), n, h, w, c, stride, pt, pl, oh, ow, act,
                                                   _lib.current_stream_ptr()), "hsefr_dwconv3x3_bn_relu6")
    return y


def split_rows_encode(x, a_log2: int = 12):
    """fp32 [..., c] (c % 32 == 0) -> the split-row image of it as a float16 tensor [..., c/32, 2, 32] ([..., 0, :] = hi,
    [..., 1, :] = lo), computed with torch ops exactly as the kernels do: v = x * 2^a_log2, hi = f16(v), lo = f16(v - hi).
    A reference / container helper for tests; the product path writes this format in dwconv.hip."""
    torch = _lib.require_gpu()
    c = x.shape[-1]
    v = (x.float() * float(2 ** a_log2)).reshape(tuple(x.shape[:-1]) + (c // 32, 32))
    hi = v.to(torch.float16)
    lo = (v - hi.float()).to(torch.float16)
    return torch.stack([hi, lo], dim=-2).contiguous()


def split_rows_decode(xs, a_log2: int = 12):
    """Inverse view of split rows: float16 [..., c/32, 2, 32] -> fp32 [..., c] = (hi + lo) / 2^a_log2 (exact in fp32
    for values the split represents exactly; otherwise within 2^-22 relative)."""
    v = xs[..., 0, :].float() + xs[..., 1, :].float()
    return (v / float(2 ** a_log2)).reshape(tuple(xs.shape[:-3]) + (xs.shape[-3] * 32,))


@_device_guarded
def dwconv3x3_split(x, w_hwc, scale, shift, stride: int = 1, act: int = ACT_RELU6, a_log2: int = 12):
    """dwconv3x3 with its result stored PRE-SPLIT for the GEMM behind it (csrc/dwconv.hip SPLIT): float16 tensor
    [n, oh, ow, c/32, 2, 32] (same bytes as the fp32 tensor)."""
    torch = _lib.require_gpu()
    _f32c(x, "x"), _f32c(w_hwc, "w"), _f32c(scale, "scale"), _f32c(shift, "shift")
    n, h, w, c = x.shape
    oh, ow, pt, pl = _same(h, w, 3, stride)
    y = torch.empty((n, oh, ow, max(c // 32, 0), 2, 32), dtype=torch.float16, device=x.device)
    _lib.check(_lib.lib().hsefr_dwconv3x3_bn_relu6_split(x.data_ptr(), w_hwc.data_ptr(), scale.data_ptr(), shift.data_ptr(),
                                                         y.data_ptr(), n, h, w, c, stride, pt, pl, oh, ow, act, a_log2,
                                                         _lib.current_stream_ptr()), "hsefr_dwconv3x3_bn_relu6_split")
    return y


@_device_guarded
def pwconv1x1_presplit(xs, w_t, shift, act: int = ACT_RELU6, a_log2: int = 12, prepared=None):
    """1x1 conv + shift + act on PRE-SPLIT activations xs = float16 [..., k/32, 2, 32] (csrc/pwconv_ps.hip); weights as for
    pwconv1x1_f16split (a_log2 must be the exponent xs was split with)."""
    torch = _lib.require_gpu()
    _f32c(shift, "shift")
    if not (xs.is_cuda and xs.dtype == torch.float16 and xs.is_contiguous() and xs.dim() >= 3 and tuple(xs.shape[-2:]) == (2, 32)):
        raise ValueError("xs must be a contiguous float16 CUDA tensor [..., k/32, 2, 32]")
    d_img, d_ds = prepared if prepared is not None else split_weights_device(w_t, xs.device, a_log2)
    k = xs.shape[-3] * 32
    cout = d_img.shape[0]
    m = xs.numel() // (2 * k)
    y = torch.empty(tuple(xs.shape[:-3]) + (cout,), dtype=torch.float32, device=xs.device)
    _lib.check(_lib.lib().hsefr_pwconv1x1_presplit(xs.data_ptr(), d_img.data_ptr(), d_ds.data_ptr(), shift.data_ptr(), y.data_ptr(),
                                                   m, k, cout, act, _lib.current_stream_ptr()), "hsefr_pwconv1x1_presplit")
    return y


@_device_guarded
def pwconv1x1_presplit_gap(xs, w_t, shift, act: int = ACT_RELU6, a_log2: int = 12, prepared=None):
    """pwconv1x1_presplit with the global average pool in its epilogue (csrc/pwconv_ps.hip): xs = split rows [n, h, w, k/32, 2, 32]
    with 33 <= h * w <= 288 -> fp32 [n, cout] means; the pointwise tensor is never written."""
    torch = _lib.require_gpu()
    _f32c(shift, "shift")
    if not (xs.is_cuda and xs.dtype == torch.float16 and xs.is_contiguous() and xs.dim() == 6 and tuple(xs.shape[-2:]) == (2, 32)):
        raise ValueError("xs must be a contiguous float16 CUDA tensor [n, h, w, k/32, 2, 32]")
    d_img, d_ds = prepared if prepared is not None else split_weights_device(w_t, xs.device, a_log2)
    n, h, w = int(xs.shape[0]), int(xs.shape[1]), int(xs.shape[2])
    k, cout = xs.shape[3] * 32, d_img.shape[0]
    y = torch.empty((n, cout), dtype=torch.float32, device=xs.device)
    _lib.check(_lib.lib().hsefr_pwconv1x1_presplit_gap(xs.data_ptr(), d_img.data_ptr(), d_ds.data_ptr(), shift.data_ptr(), y.data_ptr(),
                                                       n * h * w, k, cout, act, h * w, _lib.current_stream_ptr()), "hsefr_pwconv1x1_presplit_gap")
    return y


@_device_guarded
def pwconv1x1_presplit_dw(xs, w_t, shift, dw_w_hwc, dw_scale, dw_shift, act: int = ACT_RELU6, a_log2: int = 12, out_log2: int = 12, prepared=None,
                          dw_stride: int = 1):
    """pwconv1x1_presplit with the NEXT block's depthwise 3x3 / stride 1 / SAME + scale + shift + ReLU6 in its epilogue
    (csrc/pwconv_ps.hip, DW = true).  xs = split rows [n, h, w, k/32, 2, 32] with h * w <= 288; dw_w_hwc [3, 3, cout].
    Returns the depthwise result as split rows [n, h/s, w/s, cout/32, 2, 32] scaled by 2^out_log2 (split_rows_decode); dw_stride 2
    (12x12 maps only) is TF SAME on an even map: no top / left padding."""
    torch = _lib.require_gpu()
    _f32c(shift, "shift"), _f32c(dw_w_hwc, "dw_w"), _f32c(dw_scale, "dw_scale"), _f32c(dw_shift, "dw_shift")
    if not (xs.is_cuda and xs.dtype == torch.float16 and xs.is_contiguous() and xs.dim() == 6 and tuple(xs.shape[-2:]) == (2, 32)):
        raise ValueError("xs must be a contiguous float16 CUDA tensor [n, h, w, k/32, 2, 32]")
    d_img, d_ds = prepared if prepared is not None else split_weights_device(w_t, xs.device, a_log2)
    n, h, w = int(xs.shape[0]), int(xs.shape[1]), int(xs.shape[2])
    k, cout = xs.shape[3] * 32, d_img.shape[0]
    if tuple(dw_w_hwc.shape) != (3, 3, cout) or dw_scale.numel() != cout or dw_shift.numel() != cout:
        raise ValueError("depthwise operands must be [3,3,%d], [%d], [%d]" % (cout, cout, cout))
    amp = float(2 ** out_log2)
    consts = torch.cat([dw_w_hwc.reshape(9, cout), (dw_scale * amp).reshape(1, cout), (dw_shift * amp).reshape(1, cout)]).contiguous()
    ys = torch.empty((n, h // dw_stride, w // dw_stride, cout // 32, 2, 32), dtype=torch.float16, device=xs.device)
    _lib.check(_lib.lib().hsefr_pwconv1x1_presplit_dw(xs.data_ptr(), d_img.data_ptr(), d_ds.data_ptr(), shift.data_ptr(), consts.data_ptr(),
                                                      ys.data_ptr(), n * h * w, k, cout, act, w, h * w, dw_stride, out_log2,
                                                      _lib.current_stream_ptr()),
               "hsefr_pwconv1x1_presplit_dw")
    return ys


@_device_guarded
def pwconv1x1(x, w_t, shift, act: int = ACT_RELU6):
    """1x1 conv + shift + act on NHWC x [..., k]; w_t is the TF kernel transposed: [cout, k]."""
    torch = _lib.require_gpu()
    _f32c(x, "x"), _f32c(w_t, "w_t"), _f32c(shift, "shift")
    k = x.shape[-1]
    cout = w_t.shape[0]
    m = x.numel() // k
    y = torch.empty(tuple(x.shape[:-1]) + (cout,), dtype=torch.float32, device=x.device)
    _lib.check(_lib.lib().hsefr_pwconv1x1_bias_relu6(x.data_ptr(), w_t.data_ptr(), shift.data_ptr(), y.data_ptr(),
                                                     m, k, cout, act, _lib.current_stream_ptr()),
               "hsefr_pwconv1x1_bias_relu6")
    return y


def split_weights_device(w_t, device, a_log2: int = 12):
    """Host-side split of a pointwise kernel [cout, k] into the device image + descale the f16-split GEMM takes."""
    torch = _lib.require_gpu()
    from . import lowering
    w_np = w_t.detach().cpu().numpy() if hasattr(w_t, "detach") else w_t
    img, descale = lowering.split_pointwise_weights(w_np, a_log2)
    return torch.from_numpy(img.view(np.int16)).to(device), torch.from_numpy(descale).to(device)


@_device_guarded
def pwconv1x1_f16split(x, w_t, shift, act: int = ACT_RELU6, a_log2: int = 12, prepared=None):
    """1x1 conv + shift + act with split-f16 products (fp32-grade, csrc/pwconv_f16s.hip).  PRECONDITION:
    |x| * 2^a_log2 < 32768 (a ReLU6 producer with the default 12).  w_t [cout, k] fp32 is split on the host
    (or pass prepared=split_weights_device(...))."""
    torch = _lib.require_gpu()
    _f32c(x, "x"), _f32c(shift, "shift")
    d_img, d_ds = prepared if prepared is not None else split_weights_device(w_t, x.device, a_log2)
    k = x.shape[-1]
    cout = d_img.shape[0]
    m = x.numel() // k
    y = torch.empty(tuple(x.shape[:-1]) + (cout,), dtype=torch.float32, device=x.device)
    _lib.check(_lib.lib().hsefr_pwconv1x1_f16split(x.data_ptr(), d_img.data_ptr(), d_ds.data_ptr(), shift.data_ptr(),
                                                   y.data_ptr(), m, k, cout, a_log2, act, _lib.current_stream_ptr()),
               "hsefr_pwconv1x1_f16split")
    return y


@_device_guarded
def dwpw_f16split(x, w_hwc, dscale, dshift, wp_t, pshift, stride: int = 1, act: int = ACT_RELU6, a_log2: int = 12, prepared=None):
    """One MobileNet block in one kernel, any c % 32 == 0 / cout % 64 == 0: depthwise 3x3 SAME + scale + shift + ReLU6 ->
    pointwise 1x1 + shift + act with split-f16 products (csrc/dwpw_f16s.hip).  wp_t [cout, c] fp32 is split on the host."""
    torch = _lib.require_gpu()
    for t, nm in ((x, "x"), (w_hwc, "w"), (dscale, "dscale"), (dshift, "dshift"), (pshift, "pshift")):
        _f32c(t, nm)
    d_img, d_ds = prepared if prepared is not None else split_weights_device(wp_t, x.device, a_log2)
    n, h, w, c = x.shape
    cout = d_img.shape[0]
    oh, ow, pt, pl = _same(h, w, 3, stride)
    y = torch.empty((n, oh, ow, cout), dtype=torch.float32, device=x.device)
    _lib.check(_lib.lib().hsefr_dwpw_f16split(x.data_ptr(), w_hwc.data_ptr(), dscale.data_ptr(), dshift.data_ptr(), d_img.data_ptr(),
                                              d_ds.data_ptr(), pshift.data_ptr(), y.data_ptr(), n, h, w, c, stride, pt, pl, oh, ow,
                                              cout, a_log2, act, _lib.current_stream_ptr()), "hsefr_dwpw_f16split")
    return y


@_device_guarded
def pwblk_f16split(x, w2_t, shift2, w_hwc, dscale, dshift, w3_t, shift3, act: int = ACT_RELU6, a_log2: int = 12, a_log2_blk: int = 12, segs: int = 0,
                   prepared2=None, prepared3=None):
    """pwconv1x1_f16split (+ ReLU6) -> dwpw_f16split (stride 1) as one row-streaming launch, bit for bit the two calls
    (csrc/pwblk_stream.hip: 64 -> 128 -> 128 channels on rows of at most 48 pixels; other shapes run as the two launches).  x [n,h,w,cin];
    w2_t [cmid, cin], w3_t [cout, cmid] fp32 are split on the host (or pass prepared2 / prepared3 = split_weights_device(...)).
    segs: 0 = automatic, s > 0 = s row segments per image -- the result does not depend on it."""
    torch = _lib.require_gpu()
    for t, nm in ((x, "x"), (shift2, "shift2"), (w_hwc, "w"), (dscale, "dscale"), (dshift, "dshift"), (shift3, "shift3")):
        _f32c(t, nm)
    img2, ds2 = prepared2 if prepared2 is not None else split_weights_device(w2_t, x.device, a_log2)
    img3, ds3 = prepared3 if prepared3 is not None else split_weights_device(w3_t, x.device, a_log2_blk)
    n, h, w, cin = x.shape
    cmid, cout = img2.shape[0], img3.shape[0]
    if tuple(w_hwc.shape) != (3, 3, cmid) or dscale.numel() != cmid or dshift.numel() != cmid or shift2.numel() != cmid or shift3.numel() != cout:
        raise ValueError("depthwise operands must be [3,3,%d], [%d], [%d]; shifts [%d], [%d]" % (cmid, cmid, cmid, cmid, cout))
    y = torch.empty((n, h, w, cout), dtype=torch.float32, device=x.device)
    covered = cin == 64 and cmid == 128 and cout == 128 and w <= 48
    mid = None if covered else torch.empty((n, h, w, cmid), dtype=torch.float32, device=x.device)
    _lib.check(_lib.lib().hsefr_pwblk_f16split(x.data_ptr(), img2.data_ptr(), ds2.data_ptr(), shift2.data_ptr(), w_hwc.data_ptr(), dscale.data_ptr(),
                                               dshift.data_ptr(), img3.data_ptr(), ds3.data_ptr(), shift3.data_ptr(),
                                               None if mid is None else mid.data_ptr(), y.data_ptr(), n, h, w, cin, cmid, cout, a_log2, a_log2_blk,
                                               act, segs, _lib.current_stream_ptr()), "hsefr_pwblk_f16split")
    return y


@_device_guarded
def stem_fused(x, conv_w, conv_shift, w_hwc, dscale, dshift, wp_t, pshift, act: int = ACT_RELU6, a_log2: int = 12, prepared=None):
    """The MobileNet stem in one kernel (csrc/stem_fused.hip): conv 3x3/2 SAME 3->32 + shift + ReLU6 -> depthwise 3x3/1 +
    scale + shift + ReLU6 -> pointwise 32->64 + shift + act.  conv_w TF HWIO [3,3,3,32], w_hwc [3,3,32], wp_t [64,32]."""
    torch = _lib.require_gpu()
    if not hasattr(_lib.lib(), "hsefr_stem_fused"):
        raise NotImplementedError("round 1's fused stem is part of DEVELOPMENT builds of the library only (HSEFR_LIB=libhsefr_dev.so)")
    for t, nm in ((x, "x"), (conv_w, "conv_w"), (conv_shift, "conv_shift"), (w_hwc, "w"), (dscale, "dscale"), (dshift, "dshift"),
                  (pshift, "pshift")):
        _f32c(t, nm)
    d_img, d_ds = prepared if prepared is not None else split_weights_device(wp_t, x.device, a_log2)
    n, h, w, c = x.shape
    if c != 3 or tuple(conv_w.shape) != (3, 3, 3, 32) or tuple(w_hwc.shape) != (3, 3, 32) or d_img.shape[0] != 64:
        raise NotImplementedError("stem_fused covers 3 -> 32 -> 64 channels")
    oh, ow, pt, pl = _same(h, w, 3, 2)
    y = torch.empty((n, oh, ow, 64), dtype=torch.float32, device=x.device)
    _lib.check(_lib.lib().hsefr_stem_fused(x.data_ptr(), conv_w.data_ptr(), conv_shift.data_ptr(), w_hwc.data_ptr(), dscale.data_ptr(),
                                           dshift.data_ptr(), d_img.data_ptr(), d_ds.data_ptr(), pshift.data_ptr(), y.data_ptr(),
                                           n, h, w, pt, pl, oh, ow, a_log2, act, _lib.current_stream_ptr()), "hsefr_stem_fused")
    return y


@_device_guarded
def stem2_fused(x, conv_w, conv_shift, w1_hwc, d1scale, d1shift, wp_t, pshift, w2_hwc, d2scale, d2shift, act: int = ACT_RELU6,
                a_log2: int = 12, prepared=None):
    """Stem + the depthwise of block 2 in one kernel (csrc/stem2_fused.hip): conv 3x3/2 3->32 -> depthwise 3x3/1 -> pointwise
    32->64 (all + ReLU6) -> depthwise 3x3/2 + scale + shift + act.  w2_hwc [3,3,64]; output [n, ceil(h/4), ceil(w/4), 64]."""
    torch = _lib.require_gpu()
    for t, nm in ((x, "x"), (conv_w, "conv_w"), (conv_shift, "conv_shift"), (w1_hwc, "w1"), (d1scale, "d1scale"), (d1shift, "d1shift"),
                  (pshift, "pshift"), (w2_hwc, "w2"), (d2scale, "d2scale"), (d2shift, "d2shift")):
        _f32c(t, nm)
    d_img, d_ds = prepared if prepared is not None else split_weights_device(wp_t, x.device, a_log2)
    n, h, w, c = x.shape
    if c != 3 or tuple(conv_w.shape) != (3, 3, 3, 32) or tuple(w1_hwc.shape) != (3, 3, 32) or d_img.shape[0] != 64 or \
            tuple(w2_hwc.shape) != (3, 3, 64):
        raise NotImplementedError("stem2_fused covers 3 -> 32 -> 64 channels")
    h1, w1, pt, pl = _same(h, w, 3, 2)
    oh2, ow2, pt2, pl2 = _same(h1, w1, 3, 2)
    y = torch.empty((n, oh2, ow2, 64), dtype=torch.float32, device=x.device)
    _lib.check(_lib.lib().hsefr_stem2_fused(x.data_ptr(), conv_w.data_ptr(), conv_shift.data_ptr(), w1_hwc.data_ptr(), d1scale.data_ptr(),
                                            d1shift.data_ptr(), d_img.data_ptr(), d_ds.data_ptr(), pshift.data_ptr(), w2_hwc.data_ptr(),
                                            d2scale.data_ptr(), d2shift.data_ptr(), y.data_ptr(), n, h, w, pt, pl, h1, w1, pt2, pl2,
                                            oh2, ow2, a_log2, act, _lib.current_stream_ptr()), "hsefr_stem2_fused")
    return y


@_device_guarded
def stem3_fused(x, conv_w, conv_shift, w1_hwc, d1scale, d1shift, wp_t, pshift, w2_hwc, d2scale, d2shift, act: int = ACT_RELU6,
                a_log2: int = 12, in_log2: int = 7, prepared=None, overflow=None):
    """stem2_fused for an input with the declared bound |x| < 2^(15 - in_log2) (csrc/stem3_fused.hip): conv1 on the f16 MFMA
    from two-term splits.  overflow: optional int32 CUDA tensor [1] that is OR-ed with 1 when a value breaks the bound."""
    torch = _lib.require_gpu()
    from . import lowering
    for t, nm in ((x, "x"), (conv_shift, "conv_shift"), (w1_hwc, "w1"), (d1scale, "d1scale"), (d1shift, "d1shift"),
                  (pshift, "pshift"), (w2_hwc, "w2"), (d2scale, "d2scale"), (d2shift, "d2shift")):
        _f32c(t, nm)
    d_img, d_ds = prepared if prepared is not None else split_weights_device(wp_t, x.device, a_log2)
    n, h, w, c = x.shape
    cw = conv_w.detach().cpu().numpy() if hasattr(conv_w, "detach") else np.asarray(conv_w)
    if c != 3 or tuple(cw.shape) != (3, 3, 3, 32) or tuple(w1_hwc.shape) != (3, 3, 32) or d_img.shape[0] != 64 or tuple(w2_hwc.shape) != (3, 3, 64):
        raise NotImplementedError("stem3_fused covers 3 -> 32 -> 64 channels")
    cw_t = np.zeros((32, 32), np.float32)
    cw_t[:, :27] = cw.reshape(27, 32).T
    cimg, cds = lowering.split_pointwise_weights(cw_t, in_log2)
    d_cimg = torch.from_numpy(cimg.view(np.int16)).to(x.device)
    d_cds = torch.from_numpy(cds).to(x.device)
    h1, w1, pt, pl = _same(h, w, 3, 2)
    oh2, ow2, pt2, pl2 = _same(h1, w1, 3, 2)
    y = torch.empty((n, oh2, ow2, 64), dtype=torch.float32, device=x.device)
    _lib.check(_lib.lib().hsefr_stem3_fused(x.data_ptr(), d_cimg.data_ptr(), d_cds.data_ptr(), conv_shift.data_ptr(), w1_hwc.data_ptr(),
                                            d1scale.data_ptr(), d1shift.data_ptr(), d_img.data_ptr(), d_ds.data_ptr(), pshift.data_ptr(),
                                            w2_hwc.data_ptr(), d2scale.data_ptr(), d2shift.data_ptr(), y.data_ptr(),
                                            None if overflow is None else overflow.data_ptr(), n, h, w, pt, pl, h1, w1, pt2, pl2,
                                            oh2, ow2, in_log2, a_log2, act, _lib.current_stream_ptr()), "hsefr_stem3_fused")
    return y


def stem5_stream(*args, **kw):
    """stem4_fused's four layers, operands and bits as the streaming kernel of round 4 (csrc/stem5_stream.hip): same arguments."""
    return stem4_fused(*args, _entry="hsefr_stem5_stream", **kw)


@_device_guarded
def stem4_fused(x, conv_w, conv_shift, w1_hwc, d1scale, d1shift, wp_t, pshift, w2_hwc, d2scale, d2shift, act: int = ACT_RELU6,
                a_log2: int = 12, in_log2: int = 7, prepared=None, overflow=None, u8_mean_bgr=None, _entry: str = "hsefr_stem4_fused"):
    """stem3_fused for inputs whose edges are multiples of 4 (csrc/stem4_fused.hip): no im2col, conv1's operands straight from
    the f16 window.  x float32 [n,h,w,3] within the declared bound -- or, with u8_mean_bgr, the RESIZED image as uint8 RGB
    [n,h,w,3]: float conversion, channel reversal and the BGR mean are folded into the constants (in_log2 is then 0)."""
    torch = _lib.require_gpu()
    from . import lowering
    for t, nm in ((conv_shift, "conv_shift"), (w1_hwc, "w1"), (d1scale, "d1scale"), (d1shift, "d1shift"),
                  (pshift, "pshift"), (w2_hwc, "w2"), (d2scale, "d2scale"), (d2shift, "d2shift")):
        _f32c(t, nm)
    u8 = u8_mean_bgr is not None
    if u8:
        if x.dtype != torch.uint8 or not x.is_cuda or not x.is_contiguous():
            raise ValueError("x: expected a contiguous uint8 CUDA tensor")
    else:
        _f32c(x, "x")
    d_img, d_ds = prepared if prepared is not None else split_weights_device(wp_t, x.device, a_log2)
    n, h, w, c = x.shape
    cw = conv_w.detach().cpu().numpy() if hasattr(conv_w, "detach") else np.asarray(conv_w)
    if c != 3 or tuple(cw.shape) != (3, 3, 3, 32) or tuple(w1_hwc.shape) != (3, 3, 32) or d_img.shape[0] != 64 or tuple(w2_hwc.shape) != (3, 3, 64):
        raise NotImplementedError("stem4_fused covers 3 -> 32 -> 64 channels")
    if u8:
        img4, ds4 = lowering.stem4_conv_image(cw, 0, reverse_channels=True)
        sh = lowering.stem4_u8_shifts(cw, conv_shift.detach().cpu().numpy(), u8_mean_bgr)
        d_sh = torch.from_numpy(sh).to(x.device)
        in_log2 = 0
    else:
        img4, ds4 = lowering.stem4_conv_image(cw, in_log2)
        d_sh = conv_shift
    d_cimg = torch.from_numpy(img4.view(np.int16)).to(x.device)
    d_cds = torch.from_numpy(ds4).to(x.device)
    y = torch.empty((n, h // 4, w // 4, 64), dtype=torch.float32, device=x.device)
    _lib.check(getattr(_lib.lib(), _entry)(x.data_ptr(), 1 if u8 else 0, d_cimg.data_ptr(), d_cds.data_ptr(), d_sh.data_ptr(), w1_hwc.data_ptr(),
                                            d1scale.data_ptr(), d1shift.data_ptr(), d_img.data_ptr(), d_ds.data_ptr(), pshift.data_ptr(),
                                            w2_hwc.data_ptr(), d2scale.data_ptr(), d2shift.data_ptr(), y.data_ptr(),
                                            None if overflow is None else overflow.data_ptr(), n, h, w, in_log2, a_log2, act,
                                            _lib.current_stream_ptr()), _entry)
    return y


@_device_guarded
def dwpw_fused(x, w_hwc, dscale, dshift, wp_t, pshift, stride: int = 1):
    """One early MobileNet block in one kernel: depthwise 3x3 SAME + scale + shift + ReLU6 -> pointwise 1x1 + shift +
    ReLU6 (graph nodes #35-#49).  c in {32, 64}, cout in {64, 128}; wp_t is the pointwise kernel transposed [cout, c]."""
    torch = _lib.require_gpu()
    for t, nm in ((x, "x"), (w_hwc, "w"), (dscale, "dscale"), (dshift, "dshift"), (wp_t, "wp_t"), (pshift, "pshift")):
        _f32c(t, nm)
    n, h, w, c = x.shape
    cout = wp_t.shape[0]
    oh, ow, pt, pl = _same(h, w, 3, stride)
    y = torch.empty((n, oh, ow, cout), dtype=torch.float32, device=x.device)
    _lib.check(_lib.lib().hsefr_dwpw_fused(x.data_ptr(), w_hwc.data_ptr(), dscale.data_ptr(), dshift.data_ptr(), wp_t.data_ptr(),
                                           pshift.data_ptr(), y.data_ptr(), n, h, w, c, stride, pt, pl, oh, ow, cout,
                                           _lib.current_stream_ptr()), "hsefr_dwpw_fused")
    return y


@_device_guarded
def gap(x):
    torch = _lib.require_gpu()
    _f32c(x, "x")
    n, h, w, c = x.shape
    y = torch.empty((n, c), dtype=torch.float32, device=x.device)
    _lib.check(_lib.lib().hsefr_gap(x.data_ptr(), y.data_ptr(), n, h * w, c, _lib.current_stream_ptr()), "hsefr_gap")
    return y


@_device_guarded
def dense(x, w, bias=None, act: int = ACT_NONE):
    torch = _lib.require_gpu()
    _f32c(x, "x"), _f32c(w, "w")
    n, k = x.shape
    cout = w.shape[1]
    y = torch.empty((n, cout), dtype=torch.float32, device=x.device)
    _lib.check(_lib.lib().hsefr_dense(x.data_ptr(), w.data_ptr(), None if bias is None else _f32c(bias, "bias").data_ptr(),
                                      y.data_ptr(), n, k, cout, act, _lib.current_stream_ptr()), "hsefr_dense")
    return y


@_device_guarded
def softmax(x):
    torch = _lib.require_gpu()
    _f32c(x, "x")
    n, c = x.shape
    y = torch.empty_like(x)
    _lib.check(_lib.lib().hsefr_softmax(x.data_ptr(), y.data_ptr(), n, c, _lib.current_stream_ptr()), "hsefr_softmax")
    return y


@_device_guarded
def heads_fused(x, w1, b1, wa, ba, wg, bg):
    """The age / gender heads in one launch (hsefr_heads_fused; facial_analysis.py:109): x [n,k] -> (hidden [n,256] = relu(x.w1 + b1),
    logits [n,a] = hidden.wa + ba, age_probs = softmax(logits), gender [n,1] = sigmoid(hidden.wg + bg)); w1 [k,256], wa [256,a], wg [256,1]."""
    torch = _lib.require_gpu()
    for t, nm in ((x, "x"), (w1, "w1"), (b1, "b1"), (wa, "wa"), (ba, "ba"), (wg, "wg"), (bg, "bg")):
        _f32c(t, nm)
    n, k = x.shape
    a = wa.shape[1]
    if tuple(w1.shape) != (k, 256) or wa.shape[0] != 256 or tuple(wg.shape) != (256, 1):
        raise ValueError("heads_fused: w1 [k,256], wa [256,a], wg [256,1]")
    hidden = torch.empty((n, 256), dtype=torch.float32, device=x.device)
    logits = torch.empty((n, a), dtype=torch.float32, device=x.device)
    probs = torch.empty((n, a), dtype=torch.float32, device=x.device)
    gender = torch.empty((n, 1), dtype=torch.float32, device=x.device)
    _lib.check(_lib.lib().hsefr_heads_fused(x.data_ptr(), w1.data_ptr(), b1.data_ptr(), wa.data_ptr(), ba.data_ptr(), wg.data_ptr(), bg.data_ptr(),
                                            hidden.data_ptr(), logits.data_ptr(), probs.data_ptr(), gender.data_ptr(), n, k, a,
                                            _lib.current_stream_ptr()), "hsefr_heads_fused")
    return hidden, logits, probs, gender


@_device_guarded
def l2_normalize(x):
    """preprocessing.normalize(X, norm='l2') (facerec_test.py:401)."""
    torch = _lib.require_gpu()
    _f32c(x, "x")
    n, d = x.shape
    y = torch.empty_like(x)
    _lib.check(_lib.lib().hsefr_l2_normalize(x.data_ptr(), y.data_ptr(), n, d, _lib.current_stream_ptr()),
               "hsefr_l2_normalize")
    return y


@_device_guarded
def nn1(queries, gallery):
    """Index (int32) and squared L2 distance of each query's nearest gallery row."""
    torch = _lib.require_gpu()
    _f32c(queries, "queries"), _f32c(gallery, "gallery")
    nq, d = queries.shape
    ng = gallery.shape[0]
    if gallery.shape[1] != d:
        raise ValueError("queries are %d-D, gallery is %d-D" % (d, gallery.shape[1]))
    idx = torch.empty((nq,), dtype=torch.int32, device=queries.device)
    dist = torch.empty((nq,), dtype=torch.float32, device=queries.device)
    _lib.check(_lib.lib().hsefr_nn1(queries.data_ptr(), gallery.data_ptr(), nq, ng, d, idx.data_ptr(), dist.data_ptr(),
                                    _lib.current_stream_ptr()), "hsefr_nn1")
    return idx, dist


def _int_arg(name, v, least, greatest=None, says=None) -> int:
    """``v`` as an int: a real integer (no bool) in least..greatest.  ``says``: the one message (a %r for ``v``) of a site that has one."""
    if isinstance(v, bool) or not isinstance(v, (int, np.integer)):
        raise ValueError(says % (v,) if says else "%s must be an integer, got %r" % (name, v))
    if v < least or (greatest is not None and v > greatest):
        raise ValueError(says % (v,) if says else "%s=%d must be %s" % (name, v, "at least %d" % least if greatest is None
                                                                            else "in %d..%d" % (least, greatest)))
    return int(v)


def _number_arg(name, v, finite=None, also=""):
    """``v``: a number (no bool); with ``finite`` given it is positive too, and below infinity where ``finite`` is True."""
    if isinstance(v, bool) or not isinstance(v, (int, float, np.integer, np.floating)):
        raise ValueError("%s must be a number%s, got %r" % (name, also, v))
    if finite is not None and not (v > 0 and (np.isfinite(v) or not finite)):
        raise ValueError("%s=%r must be positive%s" % (name, v, " and finite" if finite else ""))


def _labels_arg(torch, labels, n, like, where="x's device"):
    """``labels``: a contiguous int32 tensor of ``n`` values on the device of ``like`` (``where`` in the site's words)."""
    if labels.dtype != torch.int32 or not labels.is_contiguous() or tuple(labels.shape) != (n,) or labels.device != like.device:
        raise ValueError("labels must be a contiguous int32 tensor of %d values on %s" % (n, where))


def _typed(t, dtype, name, what, shape=None, like=None):
    """``t``: a contiguous CUDA tensor of ``dtype`` (``what`` in words) -- of ``shape`` and on the device of ``like`` (x), where given."""
    if not (hasattr(t, "is_cuda") and t.is_cuda and t.dtype == dtype and t.is_contiguous()
            and (shape is None or tuple(t.shape) == shape) and (like is None or t.device == like.device)):
        raise ValueError("%s must be a contiguous %s CUDA tensor%s%s" % (name, what, "" if shape is None else " of shape %s" % (shape,),
                                                                         "" if like is None else " on x's device"))
    return t


KNN_MAX_K = 16     # hsefr_knn's largest k (the selection kernel's per-lane list)


def check_n_neighbors(k, ng=None) -> int:
    """hsefr_knn's range of k, raised as ValueError before the library is called (scikit-learn raises for k > n_samples_fit too)."""
    k = _int_arg("n_neighbors", k, 1, KNN_MAX_K)
    if ng is not None and k > ng:
        raise ValueError("n_neighbors=%d exceeds the %d gallery rows" % (k, ng))
    return k


METRICS = {"l2": 0, "chi2": 1, "kl": 2}     # the k-NN distances: squared L2 (hsefr_nn1 / hsefr_knn), HSEFR_METRIC_CHI2, HSEFR_METRIC_KL


def check_metric(metric) -> str:
    """The distances of the k-NN searches, raised as ValueError before the library is loaded: "l2", or the study's chi2dist ("chi2") and
    KL_dist ("kl") of facerec_test.py:157-164."""
    if not isinstance(metric, str) or metric not in METRICS:
        raise ValueError("metric=%r must be 'l2', 'chi2' (sum (x - y)^2 / (x + y)) or 'kl' (sum (x + 0.001) log((x + 0.001) / (y + 0.001)))"
                         % (metric,))
    return metric


def _pad4(torch, t):
    """``t`` with zero columns up to a multiple of 4: neutral under both metrics (chi2's (0, 0) term is 0, kl's a (log a - log a))."""
    pad = (-t.shape[1]) % 4
    return torch.nn.functional.pad(t, (0, pad)).contiguous() if pad else t


@_device_guarded
def metric_distances(x, y=None, metric: str = "chi2"):
    """The matrix [n, m] (float32) of chi2dist or KL_dist (facerec_test.py:157-164) between the rows of x [n,d] (the first argument of
    the reference's callable) and of y [m,d] (default: x itself) -- hsefr_metric_dist: equal rows are at exactly 0, a NaN sum comes
    back as +inf."""
    if check_metric(metric) == "l2":
        raise ValueError("metric='l2' is ops.pairwise_distances; metric_distances takes 'chi2' or 'kl'")
    torch = _lib.require_gpu()
    _f32c(x, "x")
    if y is None:
        y = x
    else:
        _f32c(y, "y")
        if y.shape[1] != x.shape[1]:
            raise ValueError("x is %d-D, y is %d-D" % (x.shape[1], y.shape[1]))
    if x.shape[1] < 1:
        raise ValueError("x has no columns")
    xp = _pad4(torch, x)
    yp = xp if y is x else _pad4(torch, y)
    n, d = xp.shape
    m = yp.shape[0]
    out = torch.empty((n, m), dtype=torch.float32, device=x.device)
    _lib.check(_lib.lib().hsefr_metric_dist(xp.data_ptr(), yp.data_ptr(), n, m, d, METRICS[metric], out.data_ptr(),
                                            _lib.current_stream_ptr()), "hsefr_metric_dist")
    return out


@_device_guarded
def knn(queries, gallery, k: int, labels=None, metric: str = "l2"):
    """The k nearest gallery rows of each query, sorted by (squared L2 distance, gallery index) -- exact ties to the lowest index --
    and, with ``labels`` (int32 [ng]), their majority label, equal counts to the smallest label value (hsefr_knn).
    Returns (index [nq,k] int32, dist2 [nq,k] float32, pred [nq] int32 or None).
    ``metric`` "chi2" or "kl": the same search under chi2dist / KL_dist with the query as the callable's first argument
    (hsefr_knn_metric); the distances returned are then the metric's own values."""
    k = check_n_neighbors(k, gallery.shape[0])               # before anything touches a device
    metric = check_metric(metric)
    torch = _lib.require_gpu()
    _f32c(queries, "queries"), _f32c(gallery, "gallery")
    nq, d = queries.shape
    ng = gallery.shape[0]
    if gallery.shape[1] != d:
        raise ValueError("queries are %d-D, gallery is %d-D" % (d, gallery.shape[1]))
    pred = None
    if labels is not None:
        _labels_arg(torch, labels, ng, gallery, "the gallery's device")
        pred = torch.empty((nq,), dtype=torch.int32, device=queries.device)
    idx = torch.empty((nq, k), dtype=torch.int32, device=queries.device)
    dist = torch.empty((nq, k), dtype=torch.float32, device=queries.device)
    tail = (idx.data_ptr(), dist.data_ptr(), labels.data_ptr() if labels is not None else None,
            pred.data_ptr() if pred is not None else None, _lib.current_stream_ptr())
    if metric == "l2":
        _lib.check(_lib.lib().hsefr_knn(queries.data_ptr(), gallery.data_ptr(), nq, ng, d, k, *tail), "hsefr_knn")
    else:
        if d < 1:
            raise ValueError("queries have no columns")
        queries, gallery = _pad4(torch, queries), _pad4(torch, gallery)
        _lib.check(_lib.lib().hsefr_knn_metric(queries.data_ptr(), gallery.data_ptr(), nq, ng, int(queries.shape[1]), k, METRICS[metric],
                                               *tail), "hsefr_knn_metric")
    return idx, dist, pred


PCA_MAX_K = 256    # hsefr_pca_fit's largest component count (the largest the reference names)


def check_pca_components(k, n=None, d=None) -> int:
    """hsefr_pca_fit's range of k, raised as ValueError before the library is called: 1 <= k <= min(n - 1, d, 256) (with k = min(n, d)
    scikit-learn's last component has zero variance and an arbitrary direction)."""
    k = _int_arg("pca_components", k, 1, PCA_MAX_K)
    if n is not None and k > n - 1:
        raise ValueError("pca_components=%d exceeds n - 1 for the %d rows to fit on" % (k, n))
    if d is not None and k > d:
        raise ValueError("pca_components=%d exceeds the %d features" % (k, d))
    return k


@_device_guarded
def pca_fit(x, k: int, max_iter: int = 1000):
    """PCA(n_components=k).fit(x) as a deterministic fp64 computation on the device (hsefr_pca_fit): x [n,d] float32 ->
    (mean [d], components [k,d], explained_variance [k]) float64 device tensors and info = {"iterations", "converged"}.  The sign of
    each component is scikit-learn 1.7's (its entry of largest magnitude is positive).  A fit that stops at ``max_iter`` is returned
    with converged False: the caller decides."""
    k = check_pca_components(k, x.shape[0], x.shape[1])      # before anything touches a device
    max_iter = _int_arg("max_iter", max_iter, 1, says="max_iter must be a positive integer, got %r")
    torch = _lib.require_gpu()
    _f32c(x, "x")
    n, d = x.shape
    mean = torch.empty((d,), dtype=torch.float64, device=x.device)
    components = torch.empty((k, d), dtype=torch.float64, device=x.device)
    variance = torch.empty((k,), dtype=torch.float64, device=x.device)
    info = torch.zeros((2,), dtype=torch.int32, device=x.device)
    _lib.check(_lib.lib().hsefr_pca_fit(x.data_ptr(), n, d, k, int(max_iter), mean.data_ptr(), components.data_ptr(), variance.data_ptr(),
                                        info.data_ptr(), _lib.current_stream_ptr()), "hsefr_pca_fit")
    iterations, converged = info.cpu().tolist()
    return mean, components, variance, {"iterations": int(iterations), "converged": bool(converged)}


@_device_guarded
def pca_transform(x, mean, components):
    """(x - mean) . components^T accumulated in fp64 and rounded once to float32 (hsefr_pca_transform): [n, k rounded up to a multiple
    of 8], the padding columns zero -- the width ops.nn1 / ops.knn want, and zero columns change no distance."""
    torch = _lib.require_gpu()
    _f32c(x, "x")
    n, d = x.shape
    _typed(mean, torch.float64, "mean", "float64", (d,))
    _typed(components, torch.float64, "components", "float64", (components.shape[0], d))
    k = check_pca_components(int(components.shape[0]), None, d)
    ld = (k + 7) // 8 * 8
    z = torch.empty((n, ld), dtype=torch.float32, device=x.device)
    _lib.check(_lib.lib().hsefr_pca_transform(x.data_ptr(), n, d, k, mean.data_ptr(), components.data_ptr(), z.data_ptr(), ld,
                                              _lib.current_stream_ptr()), "hsefr_pca_transform")
    return z


# hsefr_linear_svm_fit's limits (include/hsefr.h)
LINEAR_SVM_MAX_N, LINEAR_SVM_MAX_D, LINEAR_SVM_MAX_CLASSES, LINEAR_SVM_MAX_ELEMS = 1 << 20, 1 << 14, 1 << 16, 1 << 30


def check_linear_svm_args(n, d, n_classes, C=1.0, tol=1e-10, max_iter=1000) -> None:
    """hsefr_linear_svm_fit's argument ranges, raised as ValueError before the library or a device is touched."""
    for name, v, least in (("n", n, 1), ("d", d, 1), ("n_classes", n_classes, 2), ("max_iter", max_iter, 1)):
        _int_arg(name, v, least)
    if n > LINEAR_SVM_MAX_N or d > LINEAR_SVM_MAX_D or n_classes > LINEAR_SVM_MAX_CLASSES or n * (d + 1) > LINEAR_SVM_MAX_ELEMS:
        raise ValueError("n=%d d=%d n_classes=%d over the limits n <= %d, d <= %d, n_classes <= %d, n (d + 1) <= %d"
                         % (n, d, n_classes, LINEAR_SVM_MAX_N, LINEAR_SVM_MAX_D, LINEAR_SVM_MAX_CLASSES, LINEAR_SVM_MAX_ELEMS))
    _number_arg("C", C), _number_arg("tol", tol)                # both types before either range
    _number_arg("C", C, finite=True), _number_arg("tol", tol, finite=False)


@_device_guarded
def linear_svm_fit(x, labels, n_classes: int, C: float = 1.0, tol: float = 1e-10, max_iter: int = 1000):
    """LinearSVC(C=C).fit(x, labels) solved to the optimum of its objective, a deterministic fp64 computation on the device
    (hsefr_linear_svm_fit): x [n,d] float32, labels [n] int32 codes in 0..n_classes-1 -> (coef [K',d], intercept [K']) float64 device
    tensors, K' = n_classes or 1 for two classes (the row of class 1), and info = {"iterations", "converged", "hessian_products"}.
    A class is converged when |grad f_k| <= tol |grad f_k(0)|; a fit that stops at ``max_iter`` is returned with converged False: the
    caller decides.  A label code out of range raises ValueError."""
    if getattr(x, "ndim", 0) != 2:
        raise ValueError("x must be [n, d]")
    check_linear_svm_args(int(x.shape[0]), int(x.shape[1]), n_classes, C, tol, max_iter)      # before anything touches a device
    torch = _lib.require_gpu()
    _f32c(x, "x")
    n, d = x.shape
    _labels_arg(torch, labels, n, x)
    rows = 1 if n_classes == 2 else int(n_classes)
    coef = torch.empty((rows, d), dtype=torch.float64, device=x.device)
    intercept = torch.empty((rows,), dtype=torch.float64, device=x.device)
    info = torch.zeros((3,), dtype=torch.int32, device=x.device)
    _lib.check(_lib.lib().hsefr_linear_svm_fit(x.data_ptr(), n, d, labels.data_ptr(), int(n_classes), float(C), float(tol), int(max_iter),
                                               coef.data_ptr(), intercept.data_ptr(), info.data_ptr(), _lib.current_stream_ptr()),
               "hsefr_linear_svm_fit")
    iterations, converged, products = info.cpu().tolist()
    return coef, intercept, {"iterations": int(iterations), "converged": bool(converged), "hessian_products": int(products)}


@_device_guarded
def linear_svm_decision(x, coef, intercept):
    """LinearSVC.decision_function: x . coef^T + intercept accumulated in fp64 (hsefr_linear_svm_decision): [n, K'] float64."""
    torch = _lib.require_gpu()
    _f32c(x, "x")
    n, d = x.shape
    rows = int(coef.shape[0]) if getattr(coef, "ndim", 0) == 2 else 0
    _typed(coef, torch.float64, "coef", "float64", (rows, d), x)
    _typed(intercept, torch.float64, "intercept", "float64", (rows,), x)
    out = torch.empty((n, rows), dtype=torch.float64, device=x.device)
    _lib.check(_lib.lib().hsefr_linear_svm_decision(x.data_ptr(), n, d, coef.data_ptr(), intercept.data_ptr(), rows, out.data_ptr(),
                                                    _lib.current_stream_ptr()), "hsefr_linear_svm_decision")
    return out


@_device_guarded
def linear_svm_predict(decision):
    """LinearSVC.predict on decision values [n, K'] float64 (hsefr_linear_svm_predict): int32 [n], the column of the largest value with
    exact ties to the lowest index (np.argmax); K' = 1: decision > 0."""
    torch = _lib.require_gpu()
    if not (decision.is_cuda and decision.dtype == torch.float64 and decision.is_contiguous() and decision.ndim == 2):
        raise ValueError("decision must be a contiguous float64 CUDA tensor [n, K']")
    n, rows = decision.shape
    pred = torch.empty((n,), dtype=torch.int32, device=decision.device)
    _lib.check(_lib.lib().hsefr_linear_svm_predict(decision.data_ptr(), n, rows, pred.data_ptr(), _lib.current_stream_ptr()),
               "hsefr_linear_svm_predict")
    return pred


# hsefr_rbf_svm_*'s limits (include/hsefr.h)
RBF_SVM_MAX_N, RBF_SVM_MAX_D, RBF_SVM_MAX_CLASSES, RBF_SVM_MAX_PROBES, RBF_SVM_MAX_DECISIONS = 1 << 14, 1 << 14, 1 << 12, 1 << 20, 1 << 27


def check_rbf_svm_args(n, d, n_classes, C=1.0, gamma="scale", tol=1e-10, max_iter=100000) -> None:
    """hsefr_rbf_svm_fit's argument ranges, raised as ValueError before the library or a device is touched.  ``gamma`` is "scale" or a
    positive finite number."""
    for name, v, least in (("n", n, 2), ("d", d, 1), ("n_classes", n_classes, 2), ("max_iter", max_iter, 1)):
        _int_arg(name, v, least)
    if n > RBF_SVM_MAX_N or d > RBF_SVM_MAX_D or n_classes > RBF_SVM_MAX_CLASSES or n_classes > n:
        raise ValueError("n=%d d=%d n_classes=%d over the limits n <= %d, d <= %d, n_classes <= min(n, %d)"
                         % (n, d, n_classes, RBF_SVM_MAX_N, RBF_SVM_MAX_D, RBF_SVM_MAX_CLASSES))
    _number_arg("C", C, finite=True), _number_arg("tol", tol, finite=True)
    if not (isinstance(gamma, str) and gamma == "scale"):
        _number_arg("gamma", gamma, finite=True, also=" or 'scale'")


def _rbf_svm_model(torch, x, labels, n_classes, gamma, dual_coef, rho):
    """The fitted model's tensors as hsefr_rbf_svm_decision / _predict want them."""
    if getattr(x, "ndim", 0) != 2:
        raise ValueError("x must be [n, d]")
    check_rbf_svm_args(int(x.shape[0]), int(x.shape[1]), n_classes, gamma=gamma)
    if isinstance(gamma, str):
        raise ValueError("gamma must be the number the model was fitted with (ops.rbf_svm_gamma)")
    _f32c(x, "x")
    n, K = int(x.shape[0]), int(n_classes)
    _labels_arg(torch, labels, n, x)
    _typed(dual_coef, torch.float64, "dual_coef", "float64", (K - 1, n), x)
    _typed(rho, torch.float64, "rho", "float64", (K * (K - 1) // 2,), x)


def _rbf_svm_probes(q, x, limit_pairs=None):
    if getattr(q, "ndim", 0) != 2 or getattr(x, "ndim", 0) != 2 or q.shape[1] != x.shape[1]:
        raise ValueError("q must be [nq, d] with the d of x")
    nq = int(q.shape[0])
    if nq < 1 or nq > RBF_SVM_MAX_PROBES:
        raise ValueError("nq=%d must be in 1..%d" % (nq, RBF_SVM_MAX_PROBES))
    if limit_pairs is not None and nq * limit_pairs > RBF_SVM_MAX_DECISIONS:
        raise ValueError("nq=%d probes x %d pairs over the limit of %d decision values: rbf_svm_predict labels the probes without them"
                         % (nq, limit_pairs, RBF_SVM_MAX_DECISIONS))
    return nq


@_device_guarded
def rbf_svm_gamma(x, d_used=None) -> float:
    """SVC(gamma='scale')'s value 1 / (d_used * Var(x[:, :d_used])) from an fp64 pass over x [n,d] float32 on the device
    (hsefr_rbf_svm_gamma_scale); 1.0 where the variance is 0.  ``d_used`` (default d) leaves out the zero columns ops.pca_transform pads
    with."""
    if getattr(x, "ndim", 0) != 2:
        raise ValueError("x must be [n, d]")
    n, d = int(x.shape[0]), int(x.shape[1])
    d_used = _int_arg("d_used", d if d_used is None else d_used, 1, d, says="d_used=%%r must be an integer in 1..%d" % d)
    if n < 1 or n > RBF_SVM_MAX_PROBES or d > RBF_SVM_MAX_D:
        raise ValueError("n=%d d=%d outside 1 <= n <= %d, d <= %d" % (n, d, RBF_SVM_MAX_PROBES, RBF_SVM_MAX_D))
    torch = _lib.require_gpu()
    _f32c(x, "x")
    gamma = torch.empty((1,), dtype=torch.float64, device=x.device)
    _lib.check(_lib.lib().hsefr_rbf_svm_gamma_scale(x.data_ptr(), n, d, int(d_used), gamma.data_ptr(), _lib.current_stream_ptr()),
               "hsefr_rbf_svm_gamma_scale")
    return float(gamma.cpu()[0])


@_device_guarded
def rbf_svm_fit(x, labels, n_classes: int, gamma, C: float = 1.0, tol: float = 1e-10, max_iter: int = 100000):
    """SVC(C=C, gamma=gamma).fit(x, labels) -- libsvm's one-vs-one C-SVC with the RBF kernel -- solved to the optimum of every pair's
    dual, a deterministic fp64 computation on the device (hsefr_rbf_svm_fit): x [n,d] float32, labels [n] int32 codes in
    0..n_classes-1 in any row order, gamma a positive number (ops.rbf_svm_gamma gives 'scale') -> (dual_coef [n_classes-1, n], rho
    [n_classes (n_classes-1)/2]) float64 device tensors in libsvm's sv_coef layout and pair order, and info = {"iterations",
    "converged", "pairs_at_max_iter"}.  A pair is converged at m(a) - M(a) <= tol; a fit in which a pair stops at ``max_iter`` is
    returned with converged False: the caller decides.  A label code out of range or a class without a row raises ValueError."""
    if getattr(x, "ndim", 0) != 2:
        raise ValueError("x must be [n, d]")
    check_rbf_svm_args(int(x.shape[0]), int(x.shape[1]), n_classes, C, gamma, tol, max_iter)      # before anything touches a device
    if isinstance(gamma, str):
        raise ValueError("gamma must be a number here: ops.rbf_svm_gamma(x) gives SVC's 'scale'")
    torch = _lib.require_gpu()
    _f32c(x, "x")
    n, d = x.shape
    K = int(n_classes)
    _labels_arg(torch, labels, n, x)
    dual_coef = torch.empty((K - 1, n), dtype=torch.float64, device=x.device)
    rho = torch.empty((K * (K - 1) // 2,), dtype=torch.float64, device=x.device)
    info = torch.zeros((3,), dtype=torch.int32, device=x.device)
    _lib.check(_lib.lib().hsefr_rbf_svm_fit(x.data_ptr(), n, d, labels.data_ptr(), K, float(gamma), float(C), float(tol), int(max_iter),
                                            dual_coef.data_ptr(), rho.data_ptr(), info.data_ptr(), _lib.current_stream_ptr()),
               "hsefr_rbf_svm_fit")
    iterations, converged, capped = info.cpu().tolist()
    return dual_coef, rho, {"iterations": int(iterations), "converged": bool(converged), "pairs_at_max_iter": int(capped)}


@_device_guarded
def rbf_svm_decision(q, x, labels, n_classes: int, gamma, dual_coef, rho):
    """SVC.decision_function(decision_function_shape='ovo') of the probes q [nq,d] (hsefr_rbf_svm_decision): [nq, K (K-1)/2] float64 in
    libsvm's pair order, at most 2^27 values -- the tests' window into the model; rbf_svm_predict never stores them."""
    K = int(n_classes) if isinstance(n_classes, (int, np.integer)) and not isinstance(n_classes, bool) else 0
    nq = _rbf_svm_probes(q, x, K * (K - 1) // 2)
    torch = _lib.require_gpu()
    _rbf_svm_model(torch, x, labels, n_classes, gamma, dual_coef, rho)
    _f32c(q, "q")
    n, d = x.shape
    out = torch.empty((nq, K * (K - 1) // 2), dtype=torch.float64, device=x.device)
    _lib.check(_lib.lib().hsefr_rbf_svm_decision(q.data_ptr(), nq, x.data_ptr(), n, d, labels.data_ptr(), K, float(gamma),
                                                 dual_coef.data_ptr(), rho.data_ptr(), out.data_ptr(), _lib.current_stream_ptr()),
               "hsefr_rbf_svm_decision")
    return out


@_device_guarded
def rbf_svm_predict(q, x, labels, n_classes: int, gamma, dual_coef, rho, return_votes: bool = True):
    """SVC.predict of the probes q [nq,d] (hsefr_rbf_svm_predict): (pred [nq] int32, votes [nq, K] int32 or None).  A pair's decision
    > 0 votes for its first class, anything else for its second; the label is the first class with the most votes (libsvm)."""
    nq = _rbf_svm_probes(q, x)
    torch = _lib.require_gpu()
    _rbf_svm_model(torch, x, labels, n_classes, gamma, dual_coef, rho)
    _f32c(q, "q")
    n, d = x.shape
    K = int(n_classes)
    pred = torch.empty((nq,), dtype=torch.int32, device=x.device)
    votes = torch.empty((nq, K), dtype=torch.int32, device=x.device) if return_votes else None
    _lib.check(_lib.lib().hsefr_rbf_svm_predict(q.data_ptr(), nq, x.data_ptr(), n, d, labels.data_ptr(), K, float(gamma),
                                                dual_coef.data_ptr(), rho.data_ptr(), pred.data_ptr(),
                                                votes.data_ptr() if votes is not None else None, _lib.current_stream_ptr()),
               "hsefr_rbf_svm_predict")
    return pred, votes


# hsefr_forest_*'s limits (include/hsefr_forest.h)
FOREST_MAX_N, FOREST_MAX_D, FOREST_MAX_CLASSES, FOREST_MAX_TREES, FOREST_MAX_DEPTH = 65535, 4096, 2048, 1024, 24
FOREST_MAX_CANDIDATES, FOREST_MAX_PROBES, FOREST_MAX_SLAB_BYTES, FOREST_SORT_TILE = 1 << 28, 1 << 24, 1 << 32, 4096
FOREST_INFO_BAD_LABEL, FOREST_INFO_NOT_FINITE, FOREST_INFO_INTERNAL = 1, 2, 4      # HSEFR_FOREST_INFO_*


def forest_node_capacity(n: int, max_depth: int) -> int:
    """The worst case of one tree, the stride of a fitted forest's node arrays: min(2^(max_depth + 1) - 1, 2 n - 1)."""
    return min((1 << (max_depth + 1)) - 1, 2 * n - 1)


def check_random_forest_args(n, d, n_classes, n_trees=100, max_depth=10, max_features="sqrt", bootstrap=True, seed=0) -> int:
    """hsefr_forest_fit's argument ranges, raised as ValueError before the library or a device is touched.  Returns max_features as a
    number: "sqrt" is max(1, int(sqrt(d))) as in scikit-learn."""
    for name, v, least in (("n", n, 1), ("d", d, 1), ("n_classes", n_classes, 2), ("n_trees", n_trees, 1), ("max_depth", max_depth, 1)):
        _int_arg(name, v, least)
    if isinstance(max_features, str):
        if max_features != "sqrt":
            raise ValueError("max_features=%r must be 'sqrt' or an integer in 1..d" % (max_features,))
        mf = max(1, int(np.sqrt(d)))
    else:
        mf = _int_arg("max_features", max_features, 1, d, says="max_features=%%r must be 'sqrt' or an integer in 1..d=%d" % d)
    if not isinstance(bootstrap, (bool, np.bool_)):
        raise ValueError("bootstrap must be True or False, got %r" % (bootstrap,))
    _int_arg("seed", seed, 0, (1 << 63) - 1)
    widest = min(1 << (max_depth - 1), n) if max_depth <= FOREST_MAX_DEPTH else 0
    if (n > FOREST_MAX_N or d > FOREST_MAX_D or n_classes > FOREST_MAX_CLASSES or n_trees > FOREST_MAX_TREES or max_depth > FOREST_MAX_DEPTH
            or n_trees * widest * mf > FOREST_MAX_CANDIDATES):
        raise ValueError("n=%d d=%d n_classes=%d n_trees=%d max_depth=%d max_features=%d over the limits n <= %d, d <= %d, n_classes <= %d, "
                         "n_trees <= %d, max_depth <= %d, n_trees min(2^(max_depth-1), n) max_features <= %d"
                         % (n, d, n_classes, n_trees, max_depth, mf, FOREST_MAX_N, FOREST_MAX_D, FOREST_MAX_CLASSES, FOREST_MAX_TREES,
                            FOREST_MAX_DEPTH, FOREST_MAX_CANDIDATES))
    slab = n_trees * mf * 2 * n * 8 if n > FOREST_SORT_TILE else 0
    if slab > FOREST_MAX_SLAB_BYTES:
        raise ValueError("n=%d rows exceed one sort tile of %d, and n_trees=%d x max_features=%d x 2 n keys of 8 bytes are %d bytes of sort "
                         "space, over the limit of %d" % (n, FOREST_SORT_TILE, n_trees, mf, slab, FOREST_MAX_SLAB_BYTES))
    return mf


class RandomForest:
    """A forest as hsefr_forest_predict reads it: device tensors, a tree's slice at [tree] of each.  feature int32 [T, M] (-1: a leaf),
    threshold float64 [T, M], left / right int32 [T, M] (node indices inside the tree), weight int32 [T, M] (a node's weighted row
    count), leaf_begin / leaf_len int32 [T, M] (leaves: a slice of the tree's list), leaf_class / leaf_count int32 [T, L], n_nodes
    int32 [T]; n_classes and n_features are numbers."""
    ARRAYS = ("feature", "threshold", "left", "right", "weight", "leaf_begin", "leaf_len", "leaf_class", "leaf_count", "n_nodes")

    def __init__(self, n_classes, n_features, **arrays):
        self.n_classes, self.n_features = int(n_classes), int(n_features)
        for name in self.ARRAYS:
            setattr(self, name, arrays[name])

    @property
    def n_trees(self) -> int:
        return int(self.feature.shape[0])

    @property
    def node_capacity(self) -> int:
        return int(self.feature.shape[1])

    @property
    def leaf_capacity(self) -> int:
        return int(self.leaf_class.shape[1])

    @property
    def device(self):
        return self.feature.device


@_device_guarded
def random_forest_fit(x, labels, n_classes: int, n_trees: int = 100, max_depth: int = 10, max_features="sqrt", bootstrap: bool = True,
                      seed: int = 0) -> RandomForest:
    """The forest of include/hsefr_forest.h fitted on the device (hsefr_forest_fit): x [n,d] float32, labels [n] int32 codes in
    0..n_classes-1 -> a RandomForest.  The defaults are the reference's 'rf' row, RandomForestClassifier(n_estimators=100,
    max_depth=10); the forest is a pure function of its arguments (tests/random_forest_ref.py restates it, and the device equals that
    bit for bit).  A label code out of range or a value of x that is not finite raises ValueError (checked on the device during the
    fit, read back once)."""
    if getattr(x, "ndim", 0) != 2:
        raise ValueError("x must be [n, d]")
    mf = check_random_forest_args(int(x.shape[0]), int(x.shape[1]), n_classes, n_trees, max_depth, max_features, bootstrap, seed)
    torch = _lib.require_gpu()
    _f32c(x, "x")
    n, d = int(x.shape[0]), int(x.shape[1])
    _labels_arg(torch, labels, n, x)
    T, M = int(n_trees), forest_node_capacity(n, int(max_depth))
    L = _lib.forest_lib()
    need = int(L.hsefr_forest_workspace_bytes(n, d, T, int(max_depth), mf))
    if need == 0:
        _lib.forest_check(_lib.ERR_UNSUPPORTED, "hsefr_forest_workspace_bytes")
    i32 = dict(dtype=torch.int32, device=x.device)
    arrays = {name: torch.empty((T, M), **i32) for name in ("feature", "left", "right", "weight", "leaf_begin", "leaf_len")}
    arrays["threshold"] = torch.empty((T, M), dtype=torch.float64, device=x.device)
    arrays["leaf_class"], arrays["leaf_count"] = torch.empty((T, n), **i32), torch.empty((T, n), **i32)
    arrays["n_nodes"] = torch.empty((T,), **i32)
    info = torch.empty((4,), **i32)
    workspace = torch.empty(((need + 7) // 8,), dtype=torch.int64, device=x.device)
    a = arrays
    _lib.forest_check(L.hsefr_forest_fit(x.data_ptr(), n, d, labels.data_ptr(), int(n_classes), T, int(max_depth), mf, int(bool(bootstrap)),
                                         int(seed), M, a["feature"].data_ptr(), a["threshold"].data_ptr(), a["left"].data_ptr(),
                                         a["right"].data_ptr(), a["weight"].data_ptr(), a["leaf_begin"].data_ptr(), a["leaf_len"].data_ptr(),
                                         a["leaf_class"].data_ptr(), a["leaf_count"].data_ptr(), a["n_nodes"].data_ptr(), info.data_ptr(),
                                         workspace.data_ptr(), need, _lib.current_stream_ptr()), "hsefr_forest_fit")
    bits = int(info.cpu()[0])                       # the one read-back: it also keeps the workspace alive until the fit has run
    if bits & FOREST_INFO_BAD_LABEL:
        raise ValueError("labels (int32 [%d]) hold a code outside 0..n_classes-1 = %d" % (n, int(n_classes) - 1))
    if bits & FOREST_INFO_NOT_FINITE:
        raise ValueError("x (float32 [%d, %d]) holds a NaN or an infinity: the forest wants finite features" % (n, d))
    if bits:
        raise _lib.HsefrError("hsefr_forest_fit: an index left its bound on the device (info %d); the forest is not usable" % bits)
    return RandomForest(n_classes, d, **arrays)


def _forest_arrays(torch, forest):
    """The ten arrays of a RandomForest as hsefr_forest_predict reads them: dtype, shape, device and contiguity of each, so that a forest
    built by hand cannot be read out of bounds."""
    feature = forest.feature
    if not (hasattr(feature, "is_cuda") and feature.is_cuda and feature.ndim == 2 and feature.shape[0] >= 1 and feature.shape[1] >= 1):
        raise ValueError("forest.feature must be a contiguous int32 CUDA tensor [n_trees, node_capacity], got %s"
                         % (tuple(getattr(feature, "shape", ())),))
    T, M = int(feature.shape[0]), int(feature.shape[1])
    lists = forest.leaf_class
    L = int(lists.shape[1]) if getattr(lists, "ndim", 0) == 2 and lists.shape[1] >= 1 else -1
    for name in RandomForest.ARRAYS:
        dtype = torch.float64 if name == "threshold" else torch.int32
        shape = (T,) if name == "n_nodes" else (T, L) if name in ("leaf_class", "leaf_count") else (T, M)
        t = getattr(forest, name)
        if not (hasattr(t, "is_cuda") and t.is_cuda and t.dtype == dtype and t.is_contiguous() and tuple(t.shape) == shape
                and t.device == feature.device) or L < 1:
            raise ValueError("forest.%s must be a contiguous %s CUDA tensor of shape %s on %s, got %s %s on %s%s"
                             % (name, "float64" if name == "threshold" else "int32", "[n_trees, leaf_capacity >= 1]" if L < 1 else shape,
                                feature.device, getattr(t, "dtype", type(t).__name__), tuple(getattr(t, "shape", ())), getattr(t, "device", "the host"),
                                "" if not hasattr(t, "is_contiguous") or t.is_contiguous() else ", not contiguous"))
    if not (2 <= forest.n_classes <= FOREST_MAX_CLASSES and 1 <= forest.n_features <= FOREST_MAX_D and T <= FOREST_MAX_TREES):
        raise ValueError("n_classes=%d n_features=%d n_trees=%d outside 2 <= n_classes <= %d, 1 <= n_features <= %d, n_trees <= %d"
                         % (forest.n_classes, forest.n_features, T, FOREST_MAX_CLASSES, FOREST_MAX_D, FOREST_MAX_TREES))


def _forest_probes(torch, forest, q):
    if getattr(q, "ndim", 0) != 2 or int(q.shape[1]) != forest.n_features:
        raise ValueError("q must be [nq, d] with the forest's d = %d, got shape %s" % (forest.n_features, tuple(getattr(q, "shape", ()))))
    nq = int(q.shape[0])
    if nq < 1 or nq > FOREST_MAX_PROBES:
        raise ValueError("nq=%d must be in 1..%d" % (nq, FOREST_MAX_PROBES))
    _f32c(q, "q")
    if q.device != forest.device:
        raise ValueError("q (float32 [%d, %d]) lives on %s, the forest on %s" % (nq, forest.n_features, q.device, forest.device))
    return nq


def _forest_predict(forest, q, want_proba):
    if not isinstance(forest, RandomForest):
        raise ValueError("forest must be a RandomForest (ops.random_forest_fit or ops.random_forest_from_sklearn), got %s" % type(forest).__name__)
    torch = _lib.require_gpu()
    _forest_arrays(torch, forest)
    nq = _forest_probes(torch, forest, q)
    proba = torch.empty((nq, forest.n_classes), dtype=torch.float64, device=q.device) if want_proba else None
    pred = torch.empty((nq,), dtype=torch.int32, device=q.device)
    f = forest
    _lib.forest_check(_lib.forest_lib().hsefr_forest_predict(
        q.data_ptr(), nq, f.n_features, f.n_classes, f.n_trees, f.node_capacity, f.leaf_capacity, f.feature.data_ptr(), f.threshold.data_ptr(),
        f.left.data_ptr(), f.right.data_ptr(), f.weight.data_ptr(), f.leaf_begin.data_ptr(), f.leaf_len.data_ptr(), f.leaf_class.data_ptr(),
        f.leaf_count.data_ptr(), proba.data_ptr() if proba is not None else None, pred.data_ptr(), _lib.current_stream_ptr()),
        "hsefr_forest_predict")
    return proba, pred


@_device_guarded
def random_forest_predict_proba(forest, q):
    """predict_proba of the probes q [nq,d] float32 (hsefr_forest_predict): ([nq, n_classes] float64, [nq] int32 labels).  A class's
    value is (sum over trees of its share of the probe's leaf) / n_trees, added in tree order in fp64."""
    return _forest_predict(forest, q, True)


@_device_guarded
def random_forest_predict(forest, q):
    """predict of the probes q [nq,d] float32: int32 [nq], the class of the largest probability, equal values to the lowest class.  A
    probe that met an index out of range in a forest from elsewhere is labelled -1."""
    return _forest_predict(forest, q, False)[1]


def random_forest_from_sklearn(estimator, device=None) -> RandomForest:
    """A fitted RandomForestClassifier or DecisionTreeClassifier (single output) copied into a RandomForest on ``device``: scikit-learn's
    own node order, its fp64 thresholds, and a leaf's class fractions x weighted_n_node_samples as integer counts (scikit-learn's
    bootstrap weights are counts)."""
    # the fitted attributes are all that is read (tree_, estimators_, n_classes_, n_features_in_, n_outputs_): scikit-learn itself is
    # not imported, here or anywhere else in the package's device paths
    trees = [estimator] if hasattr(estimator, "tree_") else list(getattr(estimator, "estimators_", ()))
    if not trees or not all(hasattr(t, "tree_") for t in trees) or getattr(estimator, "n_outputs_", 0) != 1:
        raise ValueError("estimator must be a fitted single-output RandomForestClassifier or DecisionTreeClassifier, got %s"
                         % type(estimator).__name__)
    C, d = int(estimator.n_classes_), int(estimator.n_features_in_)
    if C < 2 or C > FOREST_MAX_CLASSES or d > FOREST_MAX_D or len(trees) > FOREST_MAX_TREES:
        raise ValueError("n_classes=%d d=%d n_trees=%d outside 2 <= n_classes <= %d, d <= %d, n_trees <= %d"
                         % (C, d, len(trees), FOREST_MAX_CLASSES, FOREST_MAX_D, FOREST_MAX_TREES))
    leaves = []
    for t in trees:
        tr = t.tree_
        is_leaf = tr.children_left < 0
        counts = tr.value[:, 0, :] * tr.weighted_n_node_samples[:, None]
        whole = np.rint(counts)
        if np.abs(counts - whole)[is_leaf].max() > 1e-6:
            raise ValueError("a leaf's class fractions x weighted_n_node_samples are not integer counts: fractional sample weights "
                             "are not supported")
        node, cls = np.nonzero((whole > 0) & is_leaf[:, None])          # by node, then by class
        leaves.append((node, cls, whole[node, cls].astype(np.int32), is_leaf))
    T, M, L = len(trees), max(t.tree_.node_count for t in trees), max(1, max(len(node) for node, _, _, _ in leaves))
    a = {name: np.full((T, M), -1, dtype=np.int32) for name in ("feature", "left", "right", "weight", "leaf_begin", "leaf_len")}
    a["threshold"] = np.zeros((T, M), dtype=np.float64)
    a["leaf_class"], a["leaf_count"] = np.full((T, L), -1, dtype=np.int32), np.zeros((T, L), dtype=np.int32)
    a["n_nodes"] = np.zeros((T,), dtype=np.int32)
    for i, (t, (node, cls, cnt, is_leaf)) in enumerate(zip(trees, leaves)):
        tr = t.tree_
        m = tr.node_count
        a["n_nodes"][i] = m
        a["feature"][i, :m] = np.where(is_leaf, -1, tr.feature)
        a["threshold"][i, :m] = np.where(is_leaf, 0.0, tr.threshold)
        a["left"][i, :m], a["right"][i, :m] = tr.children_left, tr.children_right
        a["weight"][i, :m] = np.rint(tr.weighted_n_node_samples).astype(np.int32)
        per_node = np.bincount(node, minlength=m).astype(np.int32)
        begin = np.concatenate([[0], np.cumsum(per_node)[:-1]]).astype(np.int32)
        a["leaf_begin"][i, :m], a["leaf_len"][i, :m] = np.where(is_leaf, begin, -1), np.where(is_leaf, per_node, -1)
        a["leaf_class"][i, :len(cls)], a["leaf_count"][i, :len(cls)] = cls, cnt
    torch = _lib.require_gpu()
    dev = _lib.cuda_device(device)
    return RandomForest(C, d, **{name: torch.from_numpy(v).to(dev) for name, v in a.items()})


@_device_guarded
def conv2d_direct(x, w_hwio, bias=None, alpha=None, stride: int = 1, padding: str = "VALID"):
    """Generic Conv2D + BiasAdd + optional PReLU (MTCNN nets).  padding: 'VALID' | 'SAME' (TensorFlow rule)."""
    torch = _lib.require_gpu()
    _f32c(x, "x"), _f32c(w_hwio, "w")
    n, h, w, c = x.shape
    kh, kw, wc, cout = w_hwio.shape
    if wc != c:
        raise ValueError("kernel expects %d input channels, tensor has %d" % (wc, c))
    if padding == "SAME":
        oh, pt = tf_same_padding(h, kh, stride)
        ow, pl = tf_same_padding(w, kw, stride)
    else:
        oh, ow, pt, pl = (h - kh) // stride + 1, (w - kw) // stride + 1, 0, 0
    y = torch.empty((n, max(oh, 0), max(ow, 0), cout), dtype=torch.float32, device=x.device)
    if y.numel():
        _lib.check(_lib.lib().hsefr_conv2d_direct(x.data_ptr(), w_hwio.data_ptr(), None if bias is None else bias.data_ptr(),
                                                  None if alpha is None else alpha.data_ptr(), y.data_ptr(), n, h, w, c, oh, ow,
                                                  cout, kh, kw, stride, pt, pl, _lib.current_stream_ptr()), "hsefr_conv2d_direct")
    return y


@_device_guarded
def conv2d_f32(x, w_hwio, scale=None, shift=None, stride: int = 1, pad: int = 0, res=None, act: int = ACT_NONE, mfma: bool = False):
    """General Conv2D in exact fp32 + per-channel scale / shift + optional residual + activation (the fp32-grade mode of the
    ResNet-style graphs).  x [n,h,w,c], w_hwio [kh,kw,c,cout] with cout % 4 == 0, symmetric zero padding `pad`.
    mfma: the implicit GEMM on the fp32 matrix pipe (csrc/conv_f32_mfma.hip, cout % 64 == 0; what the engine runs when it covers
    the layer) instead of the vector-FMA direct convolution."""
    torch = _lib.require_gpu()
    _f32c(x, "x"), _f32c(w_hwio, "w")
    n, h, w, c = x.shape
    kh, kw, wc, cout = w_hwio.shape
    if wc != c:
        raise ValueError("kernel expects %d input channels, tensor has %d" % (wc, c))
    oh, ow = (h + 2 * pad - kh) // stride + 1, (w + 2 * pad - kw) // stride + 1
    if oh <= 0 or ow <= 0:
        raise ValueError("kernel %dx%d does not fit a %dx%d tensor padded by %d" % (kh, kw, h, w, pad))
    y = torch.empty((n, oh, ow, cout), dtype=torch.float32, device=x.device)
    if res is not None and tuple(_f32c(res, "res").shape) != tuple(y.shape):
        raise ValueError("residual shape %r, output shape %r" % (tuple(res.shape), tuple(y.shape)))
    for v, name in ((scale, "scale"), (shift, "shift")):
        if v is not None and _f32c(v, name).numel() != cout:
            raise ValueError("%s has %d elements for %d output channels" % (name, v.numel(), cout))
    fn = _lib.lib().hsefr_conv2d_f32_mfma if mfma else _lib.lib().hsefr_conv2d_f32
    _lib.check(fn(x.data_ptr(), w_hwio.data_ptr(), None if scale is None else scale.data_ptr(),
                                           None if shift is None else shift.data_ptr(), None if res is None else res.data_ptr(),
                                           y.data_ptr(), n, h, w, c, oh, ow, cout, kh, kw, stride, pad, pad, act,
                                           _lib.current_stream_ptr()), "hsefr_conv2d_f32")
    return y


@_device_guarded
def maxpool(x, k: int, stride: int, padding: str = "SAME"):
    torch = _lib.require_gpu()
    _f32c(x, "x")
    n, h, w, c = x.shape
    if padding == "SAME":
        oh, pt = tf_same_padding(h, k, stride)
        ow, pl = tf_same_padding(w, k, stride)
    else:
        oh, ow, pt, pl = (h - k) // stride + 1, (w - k) // stride + 1, 0, 0
    y = torch.empty((n, max(oh, 0), max(ow, 0), c), dtype=torch.float32, device=x.device)
    if y.numel():
        _lib.check(_lib.lib().hsefr_maxpool_f32(x.data_ptr(), y.data_ptr(), n, h, w, c, oh, ow, k, stride, pt, pl,
                                                _lib.current_stream_ptr()), "hsefr_maxpool_f32")
    return y


@_device_guarded
def pairwise_distances(x, y=None):
    """sklearn pairwise_distances(X[, Y]) (euclidean) -> CUDA float32 [n, m] (facial_clustering_test.py:396)."""
    torch = _lib.require_gpu()
    _f32c(x, "x")
    y = x if y is None else _f32c(y, "y")
    n, d = x.shape
    m = y.shape[0]
    out = torch.empty((n, m), dtype=torch.float32, device=x.device)
    _lib.check(_lib.lib().hsefr_pairwise_dist(x.data_ptr(), y.data_ptr(), n, m, d, out.data_ptr(), _lib.current_stream_ptr()),
               "hsefr_pairwise_dist")
    return out


def _dist_source(who, x, dense, born, year):
    """The distance source of the clustering entry points, checked for ``who``: exactly one of x [n,d] float32 (zero columns pad d to a
    multiple of 8, which changes no distance; born / year float32 [n] optional) and dense [n,n] float64
    -> (the padded x, which must outlive the call; n; the device; the C call's leading arguments x, n, d, born, year, dense)."""
    torch = _lib.require_gpu()
    if (x is None) == (dense is None):
        raise ValueError("%s: pass exactly one of x and dense" % who)
    if (born is None) != (year is None):
        raise ValueError("%s: born and year come together" % who)
    d = 0
    if x is not None:
        _f32c(x, "x")
        if x.dim() != 2:
            raise ValueError("x must be [n, d]")
        n, d = x.shape
        if d % 8:
            x = torch.nn.functional.pad(x, (0, 8 - d % 8)).contiguous()
            d = x.shape[1]
        for v, name in ((born, "born"), (year, "year")):
            if v is not None and _f32c(v, name).numel() != n:
                raise ValueError("%s has %d elements for %d rows" % (name, v.numel(), n))
    else:
        if born is not None:
            raise ValueError("%s: the age term belongs to the features path" % who)
        if not (dense.is_cuda and dense.dtype == torch.float64 and dense.is_contiguous() and dense.dim() == 2
                and dense.shape[0] == dense.shape[1]):
            raise ValueError("dense must be a contiguous square float64 CUDA tensor")
        n = dense.shape[0]
    if n < 1:
        raise ValueError("%s: no points" % who)
    ptr = lambda t: None if t is None else t.data_ptr()  # noqa: E731
    return x, n, (x if x is not None else dense).device, (ptr(x), n, d, ptr(born), ptr(year), ptr(dense))


@_device_guarded
def single_linkage_edges(x=None, dense=None, born=None, year=None):
    """The minimum spanning tree behind single linkage (hsefr_single_linkage) -> (edge_a int32, edge_b int32, edge_h float64), n - 1 CUDA
    tensors each, edge_a < edge_b, round by round.  Exactly one source: x [n,d] float32 features (zero columns pad d to a multiple of 8,
    which changes no distance) with optional born / year float32 [n] (the age term of process_photos.py:46-51), or dense [n,n] float64
    distances read as their upper triangle.  Asynchronous on the current stream."""
    torch = _lib.require_gpu()
    x, n, dev, src = _dist_source("single_linkage_edges", x, dense, born, year)
    m = max(n - 1, 1)
    ea = torch.full((m,), -1, dtype=torch.int32, device=dev)
    eb = torch.full((m,), -1, dtype=torch.int32, device=dev)
    eh = torch.empty((m,), dtype=torch.float64, device=dev)
    _lib.check(_lib.lib().hsefr_single_linkage(*src, ea.data_ptr(), eb.data_ptr(), eh.data_ptr(), _lib.current_stream_ptr()),
               "hsefr_single_linkage")
    return ea[:n - 1], eb[:n - 1], eh[:n - 1]


LINK_METHODS = {"average": 0, "complete": 1, "weighted": 2}     # HSEFR_LINK_AVERAGE / _COMPLETE / _WEIGHTED


@_device_guarded
def hier_linkage_merges(x=None, dense=None, born=None, year=None, method="average"):
    """Average, complete or weighted linkage (hsefr_hier_linkage) -> (merge_a int32, merge_b int32, merge_h float64, merge_round int32),
    n - 1 CUDA tensors each: merge_a < merge_b are the points whose clusters merged at height merge_h in round merge_round (the cluster
    lives on in merge_a's slot).  The sources are single_linkage_edges': x [n,d] float32 features (zero columns pad d to a multiple of 8)
    with optional born / year float32 [n], or dense [n,n] float64 distances read as their upper triangle.  Needs 8 n^2 bytes of device
    workspace; returns with the current stream synchronised (the host checks the cluster count once per batch of rounds)."""
    torch = _lib.require_gpu()
    if method not in LINK_METHODS:
        raise ValueError("hier_linkage_merges: method %r is not one of %s" % (method, ", ".join(sorted(LINK_METHODS))))
    x, n, dev, src = _dist_source("hier_linkage_merges", x, dense, born, year)
    m = max(n - 1, 1)
    ma = torch.full((m,), -1, dtype=torch.int32, device=dev)
    mb = torch.full((m,), -1, dtype=torch.int32, device=dev)
    mh = torch.empty((m,), dtype=torch.float64, device=dev)
    mr = torch.full((m,), -1, dtype=torch.int32, device=dev)
    _lib.check(_lib.lib().hsefr_hier_linkage(*src, LINK_METHODS[method], ma.data_ptr(), mb.data_ptr(), mh.data_ptr(), mr.data_ptr(),
                                             _lib.current_stream_ptr()), "hsefr_hier_linkage")
    return ma[:n - 1], mb[:n - 1], mh[:n - 1], mr[:n - 1]


GEOM_METHODS = {"centroid": 0, "median": 1, "ward": 2}     # HSEFR_GEOM_CENTROID / _MEDIAN / _WARD
GEOM_LDS_MAX = 128      # HSEFR_GEOM_LDS_MAX: the largest n centroid / median run as one launch of one workgroup


@_device_guarded
def geom_linkage_merges(x=None, dense=None, born=None, year=None, method="ward", return_matrix=False, return_counts=False):
    """Centroid, median or Ward linkage (hsefr_geom_linkage, libhsefr_geom.so) -> (merge_a int32, merge_b int32, merge_h float64,
    merge_round int32), n - 1 CUDA tensors each, merge_a < merge_b the points whose clusters merged at height merge_h.  'ward' runs
    hier_linkage_merges' rounds: the cluster lives on in merge_a's slot and merge_round is the round (clustering.linkage_from_merges
    makes Z).  'centroid' and 'median' merge the least pair step by step: the cluster lives on in merge_b's slot, the records are in
    merge order with heights that may fall, and merge_round is the step (clustering.linkage_from_sequence makes Z).  The sources are
    hier_linkage_merges'.  With ``return_matrix`` also the float64 CUDA tensor [n, n] of the working matrix as first built (diagonal
    +inf); with ``return_counts`` also a host int64 [2] = (records written, radicands clamped at zero), read back.  Needs 8 n^2 bytes of
    device workspace.  'ward' returns with the current stream synchronised; the other two are asynchronous unless the counts are read."""
    torch = _lib.require_gpu()
    if method not in GEOM_METHODS:
        raise ValueError("geom_linkage_merges: method %r is not one of %s" % (method, ", ".join(sorted(GEOM_METHODS))))
    x, n, dev, src = _dist_source("geom_linkage_merges", x, dense, born, year)
    m = max(n - 1, 1)
    ma = torch.full((m,), -1, dtype=torch.int32, device=dev)
    mb = torch.full((m,), -1, dtype=torch.int32, device=dev)
    mh = torch.empty((m,), dtype=torch.float64, device=dev)
    mr = torch.full((m,), -1, dtype=torch.int32, device=dev)
    W = torch.full((n, n), float("inf"), dtype=torch.float64, device=dev) if return_matrix else None
    counts = torch.zeros((2,), dtype=torch.int64, device=dev) if return_counts else None
    ptr = lambda t: None if t is None else t.data_ptr()  # noqa: E731
    _lib.geom_check(_lib.geom_lib().hsefr_geom_linkage(*src, GEOM_METHODS[method], ma.data_ptr(), mb.data_ptr(), mh.data_ptr(), mr.data_ptr(),
                                                       ptr(W), ptr(counts), _lib.current_stream_ptr()), "hsefr_geom_linkage")
    out = (ma[:n - 1], mb[:n - 1], mh[:n - 1], mr[:n - 1])
    if return_matrix:
        out += (W,)
    if return_counts:
        out += (counts.cpu().numpy(),)
    return out


# include/hsefr_shift.h: HSEFR_SHIFT_MAX_N, _MAX_D, _D_MULTIPLE, _MAX_ITER, HSEFR_SHIFT_DIST2_ULPS(d) = d + SHIFT_DIST2_ULPS_PLUS and the
# words of info
SHIFT_MAX_N, SHIFT_MAX_D, SHIFT_D_MULTIPLE, SHIFT_MAX_ITER, SHIFT_DIST2_ULPS_PLUS = 65535, 4096, 4, 10000, 8
SHIFT_INFO = ("centers", "n_iter", "distinct", "max_iter", "nonfinite", "internal", "work", "reserved")


def mean_shift_distance_bound(d, bandwidth, norm_a=1.0, norm_b=1.0):
    """The header's bound of the membership decision (include/hsefr_shift.h): with rows of norms <= norm_a and norm_b in d dimensions,
    hsefr_shift_fit decides |a - b| <= bandwidth exactly wherever | |a - b| - bandwidth | exceeds this."""
    return (d + SHIFT_DIST2_ULPS_PLUS) * 2.0 ** -53 * ((norm_a + norm_b) ** 2 + bandwidth ** 2) / bandwidth


def _shift_rows(t, name):
    """[n, d] float32 CUDA -> the same with zero columns padding d to a multiple of 4 (they change no distance and no mean)"""
    torch = _lib.require_gpu()
    _f32c(t, name)
    if t.dim() != 2 or t.shape[0] < 1 or t.shape[1] < 1:
        raise ValueError("%s must be [n, d] with n, d >= 1" % name)
    if t.shape[1] % SHIFT_D_MULTIPLE:
        t = torch.nn.functional.pad(t, (0, SHIFT_D_MULTIPLE - t.shape[1] % SHIFT_D_MULTIPLE)).contiguous()
    return t


@_device_guarded
def mean_shift_fit(x, bandwidth, max_iter=300, info=None, workspace=None):
    """sklearn.cluster.MeanShift(bandwidth=bandwidth, max_iter=max_iter).fit(x) (hsefr_shift_fit, libhsefr_shift.so) for x [n, d] float32
    CUDA -> (cluster_centers float64 [k, d], intensity int32 [k], labels int32 [n], label_dist float64 [n], info), CUDA tensors but
    info, a host dict of SHIFT_INFO's names read back.  fp64 on the device; zero columns pad d to a multiple of 4.  ``info``: an int32 CUDA
    tensor [8] to receive the words (it holds them also when the call raises: info[4] = 1 with the ValueError of a non-finite feature);
    ``workspace``: a uint8 CUDA tensor to use instead of a fresh one (ValueError if it is too small).  Returns with the current stream
    synchronised."""
    torch = _lib.require_gpu()
    xp = _shift_rows(x, "x")
    n, d = xp.shape
    dev = xp.device
    L = _lib.shift_lib()
    need = L.hsefr_shift_workspace_bytes(n, d)
    if workspace is None:
        workspace = torch.empty((max(need, 16),), dtype=torch.uint8, device=dev)
    elif not (workspace.is_cuda and workspace.dtype == torch.uint8 and workspace.is_contiguous() and workspace.device == dev):
        raise ValueError("workspace must be a contiguous uint8 CUDA tensor on x's device")
    if info is None:
        info = torch.zeros((8,), dtype=torch.int32, device=dev)
    elif not (info.is_cuda and info.dtype == torch.int32 and info.is_contiguous() and info.numel() == 8 and info.device == dev):
        raise ValueError("info must be a contiguous int32 CUDA tensor of 8 words on x's device")
    centers = torch.empty((n, d), dtype=torch.float64, device=dev)
    intensity = torch.empty((n,), dtype=torch.int32, device=dev)
    labels = torch.empty((n,), dtype=torch.int32, device=dev)
    dist = torch.empty((n,), dtype=torch.float64, device=dev)
    _lib.shift_check(L.hsefr_shift_fit(xp.data_ptr(), n, d, float(bandwidth), int(max_iter), centers.data_ptr(), intensity.data_ptr(),
                                       labels.data_ptr(), dist.data_ptr(), info.data_ptr(), workspace.data_ptr(), workspace.numel(),
                                       _lib.current_stream_ptr()), "hsefr_shift_fit")
    words = dict(zip(SHIFT_INFO, (int(v) for v in info.cpu().numpy())))
    k = words["centers"]
    return centers[:k, :x.shape[1]], intensity[:k], labels, dist, words


@_device_guarded
def mean_shift_assign(q, centers):
    """MeanShift.predict (hsefr_shift_assign): q [nq, d] float32 CUDA, centers [k, d] float64 CUDA -> (labels int32 [nq]: the nearest centre,
    the lowest index among equal distances; dist float64 [nq]).  Asynchronous on the current stream."""
    torch = _lib.require_gpu()
    if not (centers.is_cuda and centers.dtype == torch.float64 and centers.dim() == 2 and centers.shape[0] >= 1):
        raise ValueError("centers must be a float64 CUDA tensor [k, d] with k >= 1")
    if q.dim() != 2 or q.shape[1] != centers.shape[1]:
        raise ValueError("q must be [nq, %d] as the centres" % centers.shape[1])
    qp = _shift_rows(q, "q")
    nq, d = qp.shape
    cp = centers.contiguous()
    if cp.shape[1] != d:
        cp = torch.nn.functional.pad(cp, (0, d - cp.shape[1])).contiguous()
    labels = torch.empty((nq,), dtype=torch.int32, device=qp.device)
    dist = torch.empty((nq,), dtype=torch.float64, device=qp.device)
    _lib.shift_check(_lib.shift_lib().hsefr_shift_assign(qp.data_ptr(), nq, d, cp.data_ptr(), cp.shape[0], labels.data_ptr(), dist.data_ptr(),
                                                         _lib.current_stream_ptr()), "hsefr_shift_assign")
    return labels, dist


# include/hsefr_affinity.h: HSEFR_AFFINITY_MAX_N, _MAX_D, _D_MULTIPLE, _MAX_ITER, _MAX_CONVERGENCE_ITER, HSEFR_AFFINITY_SIM_ULPS(d) = d +
# AFFINITY_SIM_ULPS_PLUS, HSEFR_AFFINITY_MSG_ULPS(n, d) = n (d + AFFINITY_MSG_ULPS_PLUS) and the words of info
AFFINITY_MAX_N, AFFINITY_MAX_D, AFFINITY_D_MULTIPLE, AFFINITY_MAX_ITER, AFFINITY_MAX_CONVERGENCE_ITER = 16384, 4096, 4, 10000, 64
AFFINITY_SIM_ULPS_PLUS, AFFINITY_MSG_ULPS_PLUS = 8, 24
AFFINITY_INFO = ("clusters", "n_iter", "converged", "equal", "nonfinite", "internal", "reserved6", "reserved7")


def affinity_message_bound(n, d, s_max):
    """The header's first-order bound (include/hsefr_affinity.h) of how far A_kk + R_kk, a member sum or an assignment's similarity of
    hsefr_affinity_fit can lie from scikit-learn's on fp64 input: n points of d features, similarities and preference within s_max."""
    return n * (d + AFFINITY_MSG_ULPS_PLUS) * 2.0 ** -53 * s_max


@_device_guarded
def affinity_propagation_fit(x=None, S=None, damping=0.5, max_iter=200, convergence_iter=15, preference=None, seed=0, info=None,
                             workspace=None):
    """sklearn.cluster.AffinityPropagation(damping=, max_iter=, convergence_iter=, preference=).fit on fp64 input (libhsefr_affinity.so):
    exactly one of ``x`` [n, d] float32 CUDA features (hsefr_affinity_fit: S = -|x_i - x_j|^2 in fp64, zero columns pad d to a multiple
    of 4) and ``S`` [n, n] float64 CUDA similarities, which may be asymmetric (hsefr_affinity_fit_dense: affinity="precomputed") ->
    (exemplars int32 [K] ascending, labels int32 [n], diag float64 [n]: the final A_kk + R_kk, preference: a float, info), CUDA tensors
    but the last two; info is a host dict of AFFINITY_INFO's names.  ``preference`` None: the median of the similarities, exact.
    ``seed`` >= 0: the header's hash noise (what decides exact ties; scikit-learn's is unseeded); None: no noise.  ``info``: an int32 CUDA
    tensor [8] to receive the words (it holds them also when the call raises); ``workspace``: a uint8 CUDA tensor to use instead of a
    fresh one.  Neither input is written.  Returns with the current stream synchronised."""
    torch = _lib.require_gpu()
    if (x is None) == (S is None):
        raise ValueError("affinity_propagation_fit takes exactly one of x and S")
    L = _lib.affinity_lib()
    if x is not None:
        src = _shift_rows(x, "x")
        n, d = src.shape
    else:
        if not (S.is_cuda and S.dtype == torch.float64 and S.dim() == 2 and S.shape[0] == S.shape[1] and S.shape[0] >= 1):
            raise ValueError("S must be a square float64 CUDA tensor [n, n] with n >= 1")
        src = S.contiguous()
        n, d = src.shape[0], AFFINITY_D_MULTIPLE
    dev = src.device
    need = L.hsefr_affinity_workspace_bytes(n, d)
    if workspace is None:
        workspace = torch.empty((max(need, 16),), dtype=torch.uint8, device=dev)
    elif not (workspace.is_cuda and workspace.dtype == torch.uint8 and workspace.is_contiguous() and workspace.device == dev):
        raise ValueError("workspace must be a contiguous uint8 CUDA tensor on the input's device")
    if info is None:
        info = torch.zeros((8,), dtype=torch.int32, device=dev)
    elif not (info.is_cuda and info.dtype == torch.int32 and info.is_contiguous() and info.numel() == 8 and info.device == dev):
        raise ValueError("info must be a contiguous int32 CUDA tensor of 8 words on the input's device")
    exemplars = torch.empty((n,), dtype=torch.int32, device=dev)
    labels = torch.empty((n,), dtype=torch.int32, device=dev)
    diag = torch.empty((n,), dtype=torch.float64, device=dev)
    pref = torch.empty((1,), dtype=torch.float64, device=dev)
    tail = (float(damping), int(max_iter), int(convergence_iter), float("nan") if preference is None else float(preference),
            -1 if seed is None else int(seed), exemplars.data_ptr(), labels.data_ptr(), diag.data_ptr(), pref.data_ptr(), info.data_ptr(),
            workspace.data_ptr(), workspace.numel(), _lib.current_stream_ptr())
    if x is not None:
        _lib.affinity_check(L.hsefr_affinity_fit(src.data_ptr(), n, d, *tail), "hsefr_affinity_fit")
    else:
        _lib.affinity_check(L.hsefr_affinity_fit_dense(src.data_ptr(), n, *tail), "hsefr_affinity_fit_dense")
    words = dict(zip(AFFINITY_INFO, (int(v) for v in info.cpu().numpy())))
    return exemplars[:words["clusters"]], labels, diag, float(pref.item()), words


@_device_guarded
def dbscan_labels(x=None, dense=None, born=None, year=None, eps=0.5, min_samples=5):
    """DBSCAN with scikit-learn's labels (hsefr_dbscan) -> (labels int32 [n], core uint8 [n]) CUDA tensors: clusters 0, 1, ... in
    order of their smallest core index, -1 for noise.  The sources are single_linkage_edges': x [n,d] float32 features (zero columns
    pad d to a multiple of 8) with optional born / year float32 [n], or dense [n,n] float64 distances read as their upper triangle.
    O(n) device workspace, no N x N matrix on the features path.  Asynchronous on the current stream."""
    torch = _lib.require_gpu()
    x, n, dev, src = _dist_source("dbscan_labels", x, dense, born, year)
    labels = torch.empty((n,), dtype=torch.int32, device=dev)
    core = torch.empty((n,), dtype=torch.uint8, device=dev)
    # min_samples above n + 1 makes no point core, as n + 1 does (the C argument is an int)
    _lib.check(_lib.lib().hsefr_dbscan(*src, float(eps), int(min(min_samples, n + 1)), labels.data_ptr(), core.data_ptr(),
                                       _lib.current_stream_ptr()), "hsefr_dbscan")
    return labels, core


@_device_guarded
def rank_order_labels(x=None, dense=None, born=None, year=None, norm_threshold=0.9, rank_threshold=14, thresholds=None):
    """Rank-order clustering (hsefr_rank_order) -> (labels int32 [n] CUDA tensor, iterations int): labels[i] is the smallest face index of
    face i's final cluster.  The sources are hier_linkage_merges': x [n,d] float32 features (zero columns pad d to a multiple of 8) with
    optional born / year float32 [n], or dense [n,n] float64 distances read as their upper triangle with the diagonal counted as 0.
    With ``thresholds`` = a sequence of (norm, rank) pairs (hsefr_rank_order_sweep) -> (labels int32 [pairs, n], list of iterations):
    the working matrix and the face lists are built once for the whole sequence.  Needs 8 n^2 bytes of device workspace (16 n^2 for
    a sequence of more than one pair); returns with the current stream synchronised (the host reads the cluster count every iteration)."""
    torch = _lib.require_gpu()
    x, n, dev, src = _dist_source("rank_order_labels", x, dense, born, year)
    sweep = thresholds is not None
    pairs = [(float(a), float(b)) for a, b in thresholds] if sweep else [(float(norm_threshold), float(rank_threshold))]
    if not pairs:
        raise ValueError("rank_order_labels: no threshold pairs")
    labels = torch.empty((len(pairs), n), dtype=torch.int32, device=dev)
    thr = (ctypes.c_double * (2 * len(pairs)))(*[v for pair in pairs for v in pair])
    iters = (ctypes.c_int * len(pairs))()
    _lib.check(_lib.lib().hsefr_rank_order_sweep(*src, thr, len(pairs), labels.data_ptr(), iters, _lib.current_stream_ptr()),
               "hsefr_rank_order")
    return (labels, list(iters)) if sweep else (labels[0], int(iters[0]))


SPLIT_WAVE_MAX, SPLIT_LDS_MAX = 32, 128      # HSEFR_SPLIT_WAVE_MAX / _LDS_MAX: the largest group of the two LDS chain classes
SPLIT_STATS = ("early", "lds", "global", "merges", "bad_members")      # HSEFR_SPLIT_STAT_*


@_device_guarded
def split_groups(members, offsets, photo, x=None, dense=None, born=None, year=None, penalty=100.0, cut=50.0, return_distances=False,
                 return_stats=False):
    """Complete linkage inside every group of points, cut at ``cut``, with ``penalty`` between two points of one photo
    (hsefr_split_groups, libhsefr_split.so): the reference's same-photo split for all clusters of a clustering in one call ->
    sublabel int32 CUDA tensor [len(members)]: sublabel[offsets[g] + a] is clustering.complete_linkage_labels(P_g, cut)[a] for the matrix
    P_g[a][b] = w(m_a, m_b) + penalty * [photo[m_a] == photo[m_b]] of group g's members m = members[offsets[g]:offsets[g + 1]], in the
    order given.  members int32 CUDA tensor; offsets a HOST int64 sequence [groups + 1] from 0, strictly increasing, to len(members)
    (clustering.group_table makes both); photo int32 CUDA tensor [n].  The sources are hier_linkage_merges': x [n,d] float32 features
    (zero columns pad d to a multiple of 8) with optional born / year float32 [n] -- w is then the distance the clusterings use, feat_tile's,
    widened to fp64 -- or dense [n,n] float64 read as its upper triangle and left as it is.  With ``return_distances`` also the float64
    CUDA tensor of every group's P as first built, row-major, group after group (diagonals unspecified); with ``return_stats`` also the
    call's five counts as a host int64 array in SPLIT_STATS order, read back (the one synchronisation), and a member outside [0, n)
    raises ValueError then.  Without it the call is asynchronous on the current stream and such a member's group comes back as -1."""
    torch = _lib.require_gpu()
    x, n, dev, src = _dist_source("split_groups", x, dense, born, year)
    _typed(members, torch.int32, "members", "int32")
    _typed(photo, torch.int32, "photo", "int32")
    off = np.ascontiguousarray(offsets, dtype=np.int64).reshape(-1)
    if members.dim() != 1 or photo.dim() != 1 or photo.shape[0] != n:
        raise ValueError("split_groups: members [m] and photo [n = %d] are vectors, got %r and %r" % (n, tuple(members.shape), tuple(photo.shape)))
    if len(off) < 1 or int(off[-1]) != members.shape[0] or (members.shape[0] == 0 and len(off) != 1):
        raise ValueError("split_groups: %d offsets ending at %s for %d members" % (len(off), off[-1] if len(off) else None, members.shape[0]))
    if not (math.isfinite(penalty) and penalty >= 0 and math.isfinite(cut)):
        raise ValueError("split_groups: penalty=%r must be finite and >= 0, cut=%r finite" % (penalty, cut))
    m = members.shape[0]
    sublabel = torch.empty((m,), dtype=torch.int32, device=dev)
    counts = np.diff(off)
    dist = torch.empty((int((counts * counts).sum()),), dtype=torch.float64, device=dev) if return_distances else None
    stats = torch.empty((len(SPLIT_STATS),), dtype=torch.int64, device=dev) if return_stats else None
    ptr = lambda t: None if t is None else t.data_ptr()  # noqa: E731
    if m:                                             # (no members: no groups, nothing to do)
        _lib.split_check(_lib.split_lib().hsefr_split_groups(*src, members.data_ptr(), off.ctypes.data, len(off) - 1, photo.data_ptr(),
                                                             float(penalty), float(cut), sublabel.data_ptr(), ptr(dist), ptr(stats),
                                                             _lib.current_stream_ptr()), "hsefr_split_groups")
    out = (sublabel,) + ((dist,) if return_distances else ())
    if return_stats:
        host = stats.cpu().numpy() if m else np.zeros(len(SPLIT_STATS), dtype=np.int64)
        if host[4]:
            raise ValueError("split_groups: %d member(s) outside [0, %d)" % (int(host[4]), n))
        out += (host,)
    return out if len(out) > 1 else sublabel


SCORES_MAX_N = 65536       # HSEFR_SCORES_MAX_N


@_device_guarded
def flat_cuts(order, gaps, thresholds):
    """fcluster(Z, t, 'distance') for every t of ``thresholds`` from one dendrogram (hsefr_flat_cuts) -> labels int32 [rows, n] CUDA
    tensor: labels[r, order[p]] = 1 + the number of gaps before position p that exceed thresholds[r] (a gap equal to the threshold
    stays joined).  order int32 [n] = the leaves in dendrogram order (a permutation of 0 .. n - 1), gaps float64 [n - 1], thresholds
    float64 [rows], all CUDA tensors (clustering._cut_order makes the first two from Z).  Asynchronous on the current stream."""
    torch = _lib.require_gpu()
    _typed(order, torch.int32, "order", "int32")
    _typed(gaps, torch.float64, "gaps", "float64")
    _typed(thresholds, torch.float64, "thresholds", "float64")
    if order.dim() != 1 or gaps.dim() != 1 or thresholds.dim() != 1:
        raise ValueError("flat_cuts: order [n], gaps [n - 1] and thresholds [rows] are vectors")
    n, rows = order.shape[0], thresholds.shape[0]
    if n < 1 or rows < 1 or gaps.shape[0] != n - 1:
        raise ValueError("flat_cuts: %d leaves, %d gaps, %d thresholds" % (n, gaps.shape[0], rows))
    labels = torch.zeros((rows, n), dtype=torch.int32, device=order.device)
    _lib.check(_lib.lib().hsefr_flat_cuts(order.data_ptr(), gaps.data_ptr() if n > 1 else None, n, thresholds.data_ptr(), rows,
                                          labels.data_ptr(), _lib.current_stream_ptr()), "hsefr_flat_cuts")
    return labels


@_device_guarded
def partition_scores(y_true, labels):
    """The counts and sums behind the clustering study's statistics (hsefr_partition_scores) -> (counts int64 [rows, 8], stats float64
    [rows, 6]) CUDA tensors, one row per labelling: y_true int32 [n] and labels int32 [rows, n] (or [n] for one row) CUDA tensors, any
    values, a negative label being a cluster of its own.  counts = classes, clusters, clusters of at least 2, non-negative clusters,
    non-zero cells, sum n_ij^2, sum a_i^2, sum b_j^2; stats = H_true, H_pred, MI, EMI, sum n_ij^2 / a_i / n, sum n_ij^2 / b_j / n
    (clustering.scores_from_counts turns a row into the scores).  Bit-identical from run to run, every row independent of the others.
    n <= SCORES_MAX_N.  Asynchronous on the current stream."""
    torch = _lib.require_gpu()
    _typed(y_true, torch.int32, "y_true", "int32")
    _typed(labels, torch.int32, "labels", "int32")
    if labels.dim() == 1:
        labels = labels[None]
    if y_true.dim() != 1 or labels.dim() != 2 or labels.shape[1] != y_true.shape[0]:
        raise ValueError("partition_scores: y_true [n] and labels [rows, n], got %r and %r" % (tuple(y_true.shape), tuple(labels.shape)))
    rows, n = labels.shape
    if n < 1 or rows < 1 or n > SCORES_MAX_N:
        raise ValueError("partition_scores: n=%d (1 .. %d), rows=%d (at least 1)" % (n, SCORES_MAX_N, rows))
    counts = torch.empty((rows, 8), dtype=torch.int64, device=y_true.device)
    stats = torch.empty((rows, 6), dtype=torch.float64, device=y_true.device)
    _lib.check(_lib.lib().hsefr_partition_scores(y_true.data_ptr(), labels.data_ptr(), n, rows, counts.data_ptr(), stats.data_ptr(),
                                                 _lib.current_stream_ptr()), "hsefr_partition_scores")
    return counts, stats


# ---- bf16 ResNet-50 kernels -------------------------------------------------------------------------
def _bf16c(t, name):
    torch = _lib.require_gpu()
    if not (t.is_cuda and t.dtype == torch.bfloat16 and t.is_contiguous()):
        raise ValueError("%s must be a contiguous bfloat16 CUDA tensor" % name)
    return t


def bf16_from_bits(bits_u16, device=None):
    """NumPy uint16 bf16 bit patterns -> CUDA bfloat16 tensor (a container; no arithmetic)."""
    torch = _lib.require_gpu()
    import numpy as np
    return torch.from_numpy(np.ascontiguousarray(bits_u16).view(np.int16)).to(_lib.cuda_device(device)).view(torch.bfloat16)


@_device_guarded
def conv_bf16(x, w_packed, scale, shift, kh: int, kw: int, stride: int = 1, pad: int = 0, res=None, act: int = ACT_RELU):
    """x [n,h,w,c] bf16; w_packed [cout, kh*kw*c] bf16 (resnet50.pack_conv_weight); -> [n,oh,ow,cout] bf16."""
    torch = _lib.require_gpu()
    _bf16c(x, "x"), _bf16c(w_packed, "w"), _f32c(scale, "scale"), _f32c(shift, "shift")
    n, h, w, c = x.shape
    cout = w_packed.shape[0]
    oh, ow = (h + 2 * pad - kh) // stride + 1, (w + 2 * pad - kw) // stride + 1
    y = torch.empty((n, oh, ow, cout), dtype=torch.bfloat16, device=x.device)
    _lib.check(_lib.lib().hsefr_conv_bf16(x.data_ptr(), w_packed.data_ptr(), scale.data_ptr(), shift.data_ptr(),
                                          None if res is None else _bf16c(res, "res").data_ptr(), y.data_ptr(),
                                          n, h, w, c, oh, ow, cout, kh, kw, stride, pad, pad, act,
                                          _lib.current_stream_ptr()), "hsefr_conv_bf16")
    return y


@_device_guarded
def conv1x1_proj_bf16(x, w_packed, scale, shift, x2, w2_packed, scale2, shift2, stride2: int = 1, act: int = ACT_RELU):
    """The increase layer of a ResNet stage's first block with its projected shortcut in one launch (hsefr_conv1x1_proj_bf16):
    act(bf16(scale * x.w + shift) + bf16(scale2 * x2[::stride2, ::stride2].w2 + shift2)).  x [n,oh,ow,c] bf16, w_packed [cout,c],
    x2 [n,h2,w2,c2] bf16 (the block input), w2_packed [cout,c2] -> [n,oh,ow,cout] bf16."""
    torch = _lib.require_gpu()
    _bf16c(x, "x"), _bf16c(w_packed, "w"), _f32c(scale, "scale"), _f32c(shift, "shift")
    _bf16c(x2, "x2"), _bf16c(w2_packed, "w2"), _f32c(scale2, "scale2"), _f32c(shift2, "shift2")
    n, oh, ow, c = x.shape
    n2, h2, w2, c2 = x2.shape
    cout = w_packed.shape[0]
    if n2 != n or tuple(w2_packed.shape) != (cout, c2) or w_packed.shape[1] != c:
        raise ValueError("conv1x1_proj_bf16: inconsistent shapes")
    y = torch.empty((n, oh, ow, cout), dtype=torch.bfloat16, device=x.device)
    _lib.check(_lib.lib().hsefr_conv1x1_proj_bf16(x.data_ptr(), w_packed.data_ptr(), scale.data_ptr(), shift.data_ptr(), x2.data_ptr(),
                                                  w2_packed.data_ptr(), scale2.data_ptr(), shift2.data_ptr(), y.data_ptr(), n, oh, ow, c, cout,
                                                  c2, stride2, h2, w2, act, _lib.current_stream_ptr()), "hsefr_conv1x1_proj_bf16")
    return y


@_device_guarded
def conv1x1_sres_bf16(x, w_packed, scale, shift, res, res_stride: int = 2, act: int = ACT_RELU):
    """A 1x1 convolution whose residual is a stride view of a larger map (hsefr_conv1x1_sres_bf16):
    act(bf16(scale * x.w + shift) + res[:, ::res_stride, ::res_stride, :][:, :oh, :ow]).  x [n,oh,ow,c], res [n,h2,w2,cout] bf16."""
    torch = _lib.require_gpu()
    _bf16c(x, "x"), _bf16c(w_packed, "w"), _f32c(scale, "scale"), _f32c(shift, "shift"), _bf16c(res, "res")
    n, oh, ow, c = x.shape
    n2, h2, w2, cout = res.shape
    if n2 != n or tuple(w_packed.shape) != (cout, c):
        raise ValueError("conv1x1_sres_bf16: inconsistent shapes")
    y = torch.empty((n, oh, ow, cout), dtype=torch.bfloat16, device=x.device)
    _lib.check(_lib.lib().hsefr_conv1x1_sres_bf16(x.data_ptr(), w_packed.data_ptr(), scale.data_ptr(), shift.data_ptr(), res.data_ptr(), y.data_ptr(),
                                                  n, oh, ow, c, cout, res_stride, h2, w2, act, _lib.current_stream_ptr()), "hsefr_conv1x1_sres_bf16")
    return y


def conv1x1_pair_bf16(x, w1_packed, scale1, shift1, w2_packed, scale2, shift2, res=None, x2=None, wp_packed=None, scale_p=None, shift_p=None,
                      act1: int = ACT_RELU, act2: int = ACT_RELU, y1_sub2: bool = False):
    """A bottleneck's increase layer and the next bottleneck's reduce layer in one launch (hsefr_conv1x1_pair_bf16):
    y1 = act1(bf16(scale1 * x.w1 + shift1) + R), R = res or bf16(scale_p * x2.wp + shift_p);  y2 = act2(bf16(scale2 * y1.w2 + shift2)).
    x [n,h,w,c] bf16, w1_packed [cout1,c], res [n,h,w,cout1] | x2 [n,h,w,c2] with wp_packed [cout1,c2], w2_packed [cout2,cout1]
    -> (y1 [n,h,w,cout1], y2 [n,h,w,cout2]) bf16.  y1_sub2: y1 is stored at even rows / columns only, [n,(h+1)//2,(w+1)//2,cout1]
    (hsefr_conv1x1_pair_sub2_bf16)."""
    torch = _lib.require_gpu()
    _bf16c(x, "x"), _bf16c(w1_packed, "w1"), _f32c(scale1, "scale1"), _f32c(shift1, "shift1")
    _bf16c(w2_packed, "w2"), _f32c(scale2, "scale2"), _f32c(shift2, "shift2")
    n, h, w, c = x.shape
    cout1, cout2 = w1_packed.shape[0], w2_packed.shape[0]
    if w1_packed.shape[1] != c or w2_packed.shape[1] != cout1:
        raise ValueError("conv1x1_pair_bf16: inconsistent shapes")
    c2 = 0
    if res is not None:
        _bf16c(res, "res")
        if tuple(res.shape) != (n, h, w, cout1) or x2 is not None:
            raise ValueError("conv1x1_pair_bf16: res must be [n,h,w,cout1], and exclusive with the projected shortcut")
    else:
        _bf16c(x2, "x2"), _bf16c(wp_packed, "wp"), _f32c(scale_p, "scale_p"), _f32c(shift_p, "shift_p")
        c2 = x2.shape[3]
        if tuple(x2.shape[:3]) != (n, h, w) or tuple(wp_packed.shape) != (cout1, c2):
            raise ValueError("conv1x1_pair_bf16: the projected shortcut reads the same pixels")
    y1 = torch.empty((n, (h + 1) // 2, (w + 1) // 2, cout1) if y1_sub2 else (n, h, w, cout1), dtype=torch.bfloat16, device=x.device)
    y2 = torch.empty((n, h, w, cout2), dtype=torch.bfloat16, device=x.device)
    ptr = lambda t: 0 if t is None else t.data_ptr()
    if y1_sub2:
        _lib.check(_lib.lib().hsefr_conv1x1_pair_sub2_bf16(x.data_ptr(), w1_packed.data_ptr(), scale1.data_ptr(), shift1.data_ptr(), ptr(res), ptr(x2),
                                                           ptr(wp_packed), ptr(scale_p), ptr(shift_p), y1.data_ptr(), w2_packed.data_ptr(),
                                                           scale2.data_ptr(), shift2.data_ptr(), y2.data_ptr(), n, h, w, c, cout1, cout2, c2, act1, act2,
                                                           _lib.current_stream_ptr()), "hsefr_conv1x1_pair_sub2_bf16")
        return y1, y2
    _lib.check(_lib.lib().hsefr_conv1x1_pair_bf16(x.data_ptr(), w1_packed.data_ptr(), scale1.data_ptr(), shift1.data_ptr(), ptr(res), ptr(x2),
                                                  ptr(wp_packed), ptr(scale_p), ptr(shift_p), y1.data_ptr(), w2_packed.data_ptr(),
                                                  scale2.data_ptr(), shift2.data_ptr(), y2.data_ptr(), n * h * w, c, cout1, cout2, c2, act1, act2,
                                                  _lib.current_stream_ptr()), "hsefr_conv1x1_pair_bf16")
    return y1, y2


@_device_guarded
def stem7x7_bf16(x, w_packed, scale, shift, act: int = ACT_RELU):
    torch = _lib.require_gpu()
    _f32c(x, "x"), _bf16c(w_packed, "w")
    n, h, w, c = x.shape
    oh, ow = (h + 6 - 7) // 2 + 1, (w + 6 - 7) // 2 + 1
    y = torch.empty((n, oh, ow, 64), dtype=torch.bfloat16, device=x.device)
    _lib.check(_lib.lib().hsefr_stem7x7_bf16(x.data_ptr(), w_packed.data_ptr(), scale.data_ptr(), shift.data_ptr(),
                                             y.data_ptr(), n, h, w, oh, ow, act, _lib.current_stream_ptr()),
               "hsefr_stem7x7_bf16")
    return y


@_device_guarded
def stem7x7_pool_bf16(x, w_packed, scale, shift, ceil_mode: bool = True, pool_pad: int = 0):
    """conv1 7x7/2 pad 3 (3 -> 64) + scale + shift + ReLU + max-pool 3x3/2 in one kernel: x [n,h,w,3] fp32 -> [n,ph,pw,64] bf16.
    ceil_mode / pool_pad as in maxpool3x3s2_bf16 (Caffe ceil mode pads 0; pool_pad 1 = an explicit Pad(1) + VALID pool)."""
    torch = _lib.require_gpu()
    _f32c(x, "x"), _bf16c(w_packed, "w"), _f32c(scale, "scale"), _f32c(shift, "shift")
    n, h, w, c = x.shape
    if c != 3 or tuple(w_packed.shape) != (64, 256):
        raise ValueError("stem7x7_pool: x must be [n,h,w,3] and the weight image [64,256]")
    oh, ow = (h - 1) // 2 + 1, (w - 1) // 2 + 1
    if ceil_mode:
        ph, pw = -(-(oh + 2 * pool_pad - 3) // 2) + 1, -(-(ow + 2 * pool_pad - 3) // 2) + 1
    else:
        ph, pw = (oh + 2 * pool_pad - 3) // 2 + 1, (ow + 2 * pool_pad - 3) // 2 + 1
    y = torch.empty((n, ph, pw, 64), dtype=torch.bfloat16, device=x.device)
    _lib.check(_lib.lib().hsefr_stem7x7_pool_bf16(x.data_ptr(), w_packed.data_ptr(), scale.data_ptr(), shift.data_ptr(), y.data_ptr(),
                                                  n, h, w, ph, pw, pool_pad, pool_pad, _lib.current_stream_ptr()), "hsefr_stem7x7_pool_bf16")
    return y


@_device_guarded
def maxpool3x3s2_bf16(x, ceil_mode: bool = True):
    torch = _lib.require_gpu()
    _bf16c(x, "x")
    n, h, w, c = x.shape
    if ceil_mode:
        oh, ow = -(-(h - 3) // 2) + 1, -(-(w - 3) // 2) + 1
    else:
        oh, ow = (h - 3) // 2 + 1, (w - 3) // 2 + 1
    y = torch.empty((n, oh, ow, c), dtype=torch.bfloat16, device=x.device)
    _lib.check(_lib.lib().hsefr_maxpool3x3s2_bf16(x.data_ptr(), y.data_ptr(), n, h, w, c, oh, ow, 0, 0,
                                                  _lib.current_stream_ptr()), "hsefr_maxpool3x3s2_bf16")
    return y


@_device_guarded
def gap_bf16(x):
    torch = _lib.require_gpu()
    _bf16c(x, "x")
    n, h, w, c = x.shape
    y = torch.empty((n, c), dtype=torch.float32, device=x.device)
    _lib.check(_lib.lib().hsefr_gap_bf16(x.data_ptr(), y.data_ptr(), n, h * w, c, _lib.current_stream_ptr()),
               "hsefr_gap_bf16")
    return y
