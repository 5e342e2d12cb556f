"""The plan of a mixed-size MTCNN pass and its maps on the device (libhsefr_ragged.so, include/hsefr_ragged.h).

``MTCNNDetector.detect_batch`` shares a launch sequence among frames of ONE size.  A ragged pass takes frames of any sizes: every
(frame, pyramid level) pair is an *item* with its own dimensions, all items of a P-Net layer stand back to back in one packed buffer,
and one launch per layer covers the list.  ``ragged_plan`` is the host side of that: a pure function of the frames' shapes that lays
out the buffers and builds the tables the kernels read -- the frame table, the item table of the pyramid, per P-Net layer each item's
dimensions, 64-bit offsets and first workgroup plus the workgroup -> item map, and the stage-1 table.  Nothing here needs a GPU
until ``RaggedPlan.to_device``.
"""
from __future__ import annotations

from typing import List, Sequence, Tuple

import numpy as np

from . import _lib

THREADS = 256                      # threads of a workgroup of the ragged kernels (csrc/mtcnn_ragged.hip)
LEVEL_LDS_MAX = 64 * 1024          # the row form of the pyramid kernel fits its LDS in this (csrc/area_resize.hip)
XCELL_BYTES = 24                   # sizeof(XCell), csrc/area_resize_px.h

# the tables of include/hsefr_ragged.h
FRAME_DT = np.dtype([("offset", "<i8"), ("h", "<i4"), ("w", "<i4"), ("first_item", "<i4"), ("n_items", "<i4")])
LEVEL_DT = np.dtype([("frame", "<i4"), ("dh", "<i4"), ("dw", "<i4"), ("rows", "<i4"), ("level_off", "<i8"), ("first_block", "<i4"), ("hoff", "<i4")])
MAP_DT = np.dtype([("in_off", "<i8"), ("out_off", "<i8"), ("ih", "<i4"), ("iw", "<i4"), ("oh", "<i4"), ("ow", "<i4"), ("first_block", "<i4"),
                   ("reserved", "<i4")])
CELLS_DT = np.dtype([("cell_off", "<i8"), ("scale", "<f8"), ("w", "<i4"), ("h", "<i4")])
assert (FRAME_DT.itemsize, LEVEL_DT.itemsize, MAP_DT.itemsize, CELLS_DT.itemsize) == (24, 32, 40, 24)

# P-Net as the plan sees it (models/mtcnn.pb, pnet/*): (kind, k, stride, output channels of the ops that read this layer's input).
# conv4-1 (2 channels, then the softmax) and conv4-2 (4 channels) both read conv3's maps and share the last entry's tables.
PNET_LAYERS = (("conv", 3, 1, (10,)), ("pool", 2, 2, (10,)), ("conv", 3, 1, (16,)), ("conv", 3, 1, (32,)), ("conv", 1, 1, (2, 4)))
PNET_CHANNELS = (3, 10, 10, 16, 32, 2 + 2 + 4)      # floats per pixel held for each layer state (the last: conv4-1, its softmax, conv4-2)


def conv_co(cout: int) -> int:
    """Output channels per thread of hsefr_ragged_conv2d for ``cout`` channels: the widest of 4 / 2 / 1 that divides it (what
    hsefr_conv2d_direct picks for aligned weights; the bits do not depend on it)."""
    return 4 if cout % 4 == 0 else (2 if cout % 2 == 0 else 1)


def pyramid_scales(h: int, w: int, minsize: int, factor: float) -> List[float]:
    """The scales of a frame's image pyramid (facial_analysis.py:489-499) as a function of the detector's two constants:
    MTCNNDetector.pyramid_scales is this."""
    m = 12.0 / minsize
    side = min(h, w) * m
    scales, k = [], 0
    while side >= 12:
        scales.append(m * np.power(factor, k))
        side *= factor
        k += 1
    return scales


def level_sizes(h: int, w: int, minsize: int, factor: float) -> List[Tuple[float, int, int]]:
    """[(scale, hs, ws)] of a frame's pyramid: the level sizes every MTCNNDetector path resamples to."""
    return [(s, int(np.ceil(h * s)), int(np.ceil(w * s))) for s in pyramid_scales(h, w, minsize, factor)]


def layer_dims(d0: np.ndarray, d1: np.ndarray, layers=PNET_LAYERS) -> List[Tuple[np.ndarray, np.ndarray]]:
    """The map sizes of every layer state from the level sizes: VALID convolutions shrink by k - 1, a SAME pooling gives ceil(d / stride)."""
    out = [(np.asarray(d0, np.int64), np.asarray(d1, np.int64))]
    for kind, k, stride, _ in layers:
        a, b = out[-1]
        if kind == "conv":
            if stride != 1:
                raise NotImplementedError("a ragged convolution has stride 1")
            out.append((a - k + 1, b - k + 1))
        else:
            out.append((-(-a // stride), -(-b // stride)))
    return out


def block_map(threads: np.ndarray) -> Tuple[np.ndarray, np.ndarray]:
    """Items of ``threads`` threads each, padded to whole workgroups -> (first workgroup of every item int32 [n], item of every
    workgroup int32 [n_blocks])."""
    blocks = -(-np.asarray(threads, np.int64) // THREADS)
    first = np.concatenate([[0], np.cumsum(blocks)[:-1]]) if len(blocks) else np.zeros(0, np.int64)
    if len(blocks) and int(first[-1] + blocks[-1]) >= 1 << 31:
        raise ValueError("a ragged pass of %d workgroups is too large" % int(first[-1] + blocks[-1]))
    return first.astype(np.int32), np.repeat(np.arange(len(blocks), dtype=np.int32), blocks)


def map_tables(in_dims, out_dims, threads_per_pixel: int):
    """The tables of one ragged layer over items packed back to back: in_dims / out_dims = (d0 [n], d1 [n]) -> (maps MAP_DT [n],
    block_item int32 [n_blocks], input pixels, output pixels).  Offsets are the running sums of the sizes, in int64."""
    ih, iw = (np.asarray(a, np.int64) for a in in_dims)
    oh, ow = (np.asarray(a, np.int64) for a in out_dims)
    n = len(ih)
    if n and (min(ih.min(), iw.min()) < 1 or min(oh.min(), ow.min()) < 1):
        raise ValueError("a ragged item without pixels")
    maps = np.zeros(n, MAP_DT)
    in_px, out_px = ih * iw, oh * ow
    maps["in_off"] = np.concatenate([[0], np.cumsum(in_px)[:-1]]) if n else 0
    maps["out_off"] = np.concatenate([[0], np.cumsum(out_px)[:-1]]) if n else 0
    maps["ih"], maps["iw"], maps["oh"], maps["ow"] = ih, iw, oh, ow
    maps["first_block"], block_item = block_map(out_px * int(threads_per_pixel))
    return maps, block_item, int(in_px.sum()), int(out_px.sum())


def _level_form(sh: int, sw: int, dh: int, dw: int) -> Tuple[int, int, int]:
    """(rows, hoff, LDS bytes) of a pyramid level: launch_area_level_batch's choice between its two kernel forms (area_resize.hip) --
    the general decimation case row by row where its LDS fits, a thread per pixel otherwise.  Both give the same bits."""
    fx, fy = sw / dw, sh / dh
    if fx >= 1.0 and fy >= 1.0 and not (sh == dh and sw == dw):
        eps = 2.220446049250313e-16
        integer = abs(fx - np.rint(fx)) < eps and abs(fy - np.rint(fy)) < eps
        hoff = (dw * XCELL_BYTES + 15) & ~15
        lds = hoff + (int(fy) + 3) * dw * 3 * 4
        if not integer and lds <= LEVEL_LDS_MAX:
            return 1, hoff, lds
    return 0, 0, 0


def frame_workspace_bytes(h: int, w: int, minsize: int, factor: float, layers=PNET_LAYERS, channels=PNET_CHANNELS) -> int:
    """What one frame adds to a ragged pass's workspace: its bytes and the float32 maps of all its levels at every P-Net layer."""
    sizes = level_sizes(h, w, minsize, factor)
    total = int(h) * int(w) * 3
    if sizes:
        dims = layer_dims(np.array([ws for _, _, ws in sizes]), np.array([hs for _, hs, _ in sizes]), layers)
        total += 4 * sum(int((a * b).sum()) * c for (a, b), c in zip(dims, channels))
    return total


class RaggedPlan:
    """What ragged_plan returns.
      shapes          the frames' (h, w);  n_frames, n_items
      frames          FRAME_DT [n_frames]: byte offset of the frame in the packed buffer (frames back to back), h, w, its items
      frames_bytes    bytes of the packed frame buffer
      levels          LEVEL_DT [n_items]: the item table -- frame, level size (dh, dw), kernel form, 64-bit element offset of the level,
                      first workgroup; every frame's pyramid_scales levels in order
      scales          float64 [n_items]
      level_block_item int32 [level_blocks], level_lds: the pyramid launch
      dims            per layer state g = 0 .. len(layers): (d0 [n_items], d1 [n_items]) -- the maps as the nets see them, (W', H')
      pixels          per layer state: pixels of the packed buffer
      layers          per P-Net layer: dict(kind, k, stride, tpp, maps MAP_DT [n_items], block_item int32 [n_blocks])
      cells           CELLS_DT [n_items]: the stage-1 table over the last layer state
      workspace_bytes frames_bytes + the float32 maps of every layer state (the sum of frame_workspace_bytes over the frames)"""


def ragged_plan(shapes: Sequence[Tuple[int, int]], minsize: int, factor: float, layers=PNET_LAYERS, channels=PNET_CHANNELS) -> RaggedPlan:
    """The plan of ONE ragged pass over frames of the given (h, w), in list order.  A frame without a pyramid level has no items."""
    p = RaggedPlan()
    p.shapes = tuple((int(h), int(w)) for h, w in shapes)
    p.minsize, p.factor = minsize, factor
    p.n_frames = len(p.shapes)
    p.frames = np.zeros(p.n_frames, FRAME_DT)
    item_frame, item_dh, item_dw, scales = [], [], [], []
    at = 0
    for f, (h, w) in enumerate(p.shapes):
        if h < 1 or w < 1 or h * w * 3 >= 1 << 31:
            raise ValueError("frame %d: bad size %d x %d" % (f, h, w))
        sizes = level_sizes(h, w, minsize, factor)
        p.frames[f] = (at, h, w, len(scales), len(sizes))
        at += h * w * 3
        for s, hs, ws in sizes:
            item_frame.append(f), item_dh.append(hs), item_dw.append(ws), scales.append(float(s))
    p.frames_bytes = at
    p.n_items = n = len(scales)
    p.scales = np.asarray(scales, np.float64)
    dh, dw = np.asarray(item_dh, np.int64), np.asarray(item_dw, np.int64)
    # the pyramid: a workgroup per destination row or per 256 pixels
    p.levels = np.zeros(n, LEVEL_DT)
    forms = [_level_form(p.shapes[f][0], p.shapes[f][1], int(a), int(b)) for f, a, b in zip(item_frame, dh, dw)]
    rows = np.array([r for r, _, _ in forms], np.int64)
    p.levels["frame"], p.levels["dh"], p.levels["dw"], p.levels["rows"] = item_frame, dh, dw, rows
    p.levels["hoff"] = [hoff for _, hoff, _ in forms]
    p.levels["level_off"] = (np.concatenate([[0], np.cumsum(dh * dw * 3)[:-1]]) if n else 0)
    p.levels["first_block"], p.level_block_item = block_map(np.where(rows != 0, dh * THREADS, dh * dw))
    p.level_lds = max([lds for _, _, lds in forms], default=0)
    # the layers: the nets see a level as (W', H')
    p.dims = layer_dims(dw, dh, layers)
    p.pixels = [int((a * b).sum()) for a, b in p.dims]
    p.layers = []
    for g, (kind, k, stride, couts) in enumerate(layers):
        tpps = {c // conv_co(c) for c in couts} if kind == "conv" else {channels[g]}
        if len(tpps) != 1:
            raise NotImplementedError("the ops of layer %d need different thread counts" % g)
        tpp = tpps.pop()
        maps, block_item, _, _ = map_tables(p.dims[g], p.dims[g + 1], tpp)
        p.layers.append(dict(kind=kind, k=k, stride=stride, tpp=tpp, maps=maps, block_item=block_item))
    p.cells = np.zeros(n, CELLS_DT)
    last0, last1 = p.dims[-1]
    p.cells["cell_off"] = (np.concatenate([[0], np.cumsum(last0 * last1)[:-1]]) if n else 0)
    p.cells["scale"], p.cells["w"], p.cells["h"] = p.scales, last0, last1
    p.workspace_bytes = p.frames_bytes + 4 * sum(px * c for px, c in zip(p.pixels, channels))
    return p


# the frame table of include/hsefr_mixed.h (libhsefr_mixed.so reads it from the host)
MIXED_FRAME_DT = np.dtype([("offset", "<i8"), ("h", "<i4"), ("w", "<i4")])
assert MIXED_FRAME_DT.itemsize == 16


def packed_offsets(shapes: Sequence[Tuple[int, int]]) -> np.ndarray:
    """The byte offsets of uint8 [h, w, 3] frames packed back to back in list order, int64: ragged_plan's ``frames["offset"]``."""
    sizes = np.array([int(h) * int(w) * 3 for h, w in shapes], np.int64)
    return np.concatenate([[0], np.cumsum(sizes)[:-1]]).astype(np.int64) if len(sizes) else np.zeros(0, np.int64)


def frame_table(shapes: Sequence[Tuple[int, int]], offsets=None) -> np.ndarray:
    """MIXED_FRAME_DT [n]: the host table libhsefr_mixed.so takes, for frames of the given (h, w) at ``offsets`` (default: back to back)."""
    table = np.zeros(len(shapes), MIXED_FRAME_DT)
    table["offset"] = packed_offsets(shapes) if offsets is None else np.asarray(offsets, np.int64)
    if len(shapes):
        table["h"], table["w"] = [int(h) for h, _ in shapes], [int(w) for _, w in shapes]
    return table


class PackedFrames:
    """The frames of a mixed-size pass on the device: ``data`` a contiguous uint8 1-D buffer (CUDA for every consumer) that holds
    frame i as [h, w, 3] at byte ``offsets[i]``; ``shapes`` the (h, w) of the frames AS THEY STAND in the buffer (after
    preprocess_device.prepare_packed turned them: the turned sizes); ``offsets`` int64, the frames back to back in list order -- the
    layout of ragged_plan, whose ``frames["offset"]`` they equal.  ``frame(i)`` is a [h, w, 3] view of frame i."""

    def __init__(self, data, shapes: Sequence[Tuple[int, int]]):
        self.shapes = tuple((int(h), int(w)) for h, w in shapes)
        for f, (h, w) in enumerate(self.shapes):
            if h < 1 or w < 1 or h * w * 3 >= 1 << 31:
                raise ValueError("frame %d: bad size %d x %d" % (f, h, w))
        self.offsets = packed_offsets(self.shapes)
        self.nbytes = int(sum(h * w * 3 for h, w in self.shapes))
        if not (hasattr(data, "dim") and data.dim() == 1 and str(data.dtype) == "torch.uint8" and data.is_contiguous()):
            raise ValueError("data must be a contiguous uint8 1-D tensor")
        if int(data.shape[0]) < self.nbytes:
            raise ValueError("the frames take %d bytes, the buffer has %d" % (self.nbytes, int(data.shape[0])))
        self.data = data

    def __len__(self) -> int:
        return len(self.shapes)

    @property
    def table(self) -> np.ndarray:
        return frame_table(self.shapes, self.offsets)

    def frame(self, i: int):
        h, w = self.shapes[i]
        at = int(self.offsets[i])
        return self.data[at:at + h * w * 3].reshape(h, w, 3)


class DevicePlan:
    """A RaggedPlan's tables on the device: ONE upload of all of them (sections aligned to 16 bytes), addressed by pointer."""

    def __init__(self, plan: RaggedPlan, device):
        torch = _lib.require_gpu()
        self.plan = plan
        sections = [plan.frames, plan.levels, plan.level_block_item, plan.cells]
        for layer in plan.layers:
            sections += [layer["maps"], layer["block_item"]]
        at, offs, parts = 0, [], []
        for a in sections:
            b = np.ascontiguousarray(a).view(np.uint8).reshape(-1)
            pad = (-len(b)) % 16
            offs.append(at)
            parts += [b, np.zeros(pad, np.uint8)]
            at += len(b) + pad
        self.tables = torch.from_numpy(np.concatenate(parts) if at else np.zeros(16, np.uint8)).to(device)
        base = self.tables.data_ptr()
        ptr = [base + o for o in offs]
        self.frames, self.levels, self.level_block_item, self.cells = ptr[:4]
        self.layers = [(ptr[4 + 2 * g], ptr[5 + 2 * g]) for g in range(len(plan.layers))]


class RaggedMaps:
    """The maps of one P-Net layer state of a ragged pass: ``data`` CUDA float32 [pixels * c], item after item, each [d0, d1, c].
    _DeviceNet runs its compiled program on this as on a tensor: the three ops P-Net is made of."""

    def __init__(self, dplan: DevicePlan, g: int, c: int, data):
        self.dplan, self.g, self.c, self.data = dplan, g, c, data

    def _layer(self, kind: str, k: int, stride: int, tpp: int):
        plan = self.dplan.plan
        if self.g >= len(plan.layers):
            raise NotImplementedError("the ragged plan has no layer %d" % self.g)
        layer = plan.layers[self.g]
        if (layer["kind"], layer["k"], layer["stride"], layer["tpp"]) != (kind, k, stride, tpp):
            raise NotImplementedError("layer %d of the ragged plan is %s %d/%d with %d threads per pixel, the graph asks for %s %d/%d with %d"
                                      % (self.g, layer["kind"], layer["k"], layer["stride"], layer["tpp"], kind, k, stride, tpp))
        return plan, layer, self.dplan.layers[self.g]

    def conv2d(self, w_hwio, bias, alpha, stride: int, padding: str) -> "RaggedMaps":
        torch = _lib.require_gpu()
        kh, kw, wc, cout = (int(d) for d in w_hwio.shape)
        if wc != self.c:
            raise ValueError("kernel expects %d input channels, the maps have %d" % (wc, self.c))
        if kh != kw:
            raise NotImplementedError("a ragged convolution has a square kernel")
        if padding != "VALID" and kh != 1:
            raise NotImplementedError("a ragged convolution is VALID")
        co = conv_co(cout)
        plan, layer, (d_maps, d_blocks) = self._layer("conv", kh, stride, cout // co)
        y = torch.empty(plan.pixels[self.g + 1] * cout, dtype=torch.float32, device=self.data.device)
        _lib.ragged_check(_lib.ragged_lib().hsefr_ragged_conv2d(
            self.data.data_ptr(), plan.pixels[self.g], w_hwio.data_ptr(), None if bias is None else bias.data_ptr(),
            None if alpha is None else alpha.data_ptr(), y.data_ptr(), plan.pixels[self.g + 1], d_maps, plan.n_items, d_blocks,
            len(layer["block_item"]), self.c, cout, kh, kw, stride, 0, 0, co, _lib.current_stream_ptr()), "hsefr_ragged_conv2d")
        return RaggedMaps(self.dplan, self.g + 1, cout, y)

    def maxpool(self, k: int, stride: int, padding: str) -> "RaggedMaps":
        torch = _lib.require_gpu()
        if padding != "SAME":
            raise NotImplementedError("a ragged pooling is SAME")
        plan, layer, (d_maps, d_blocks) = self._layer("pool", k, stride, self.c)
        y = torch.empty(plan.pixels[self.g + 1] * self.c, dtype=torch.float32, device=self.data.device)
        _lib.ragged_check(_lib.ragged_lib().hsefr_ragged_maxpool(
            self.data.data_ptr(), plan.pixels[self.g], y.data_ptr(), plan.pixels[self.g + 1], d_maps, plan.n_items, d_blocks,
            len(layer["block_item"]), self.c, k, stride, _lib.current_stream_ptr()), "hsefr_ragged_maxpool")
        return RaggedMaps(self.dplan, self.g + 1, self.c, y)

    def softmax(self) -> "RaggedMaps":
        """Over the channels of every pixel: hsefr_softmax is row-wise, so it runs on the packed [pixels, c] buffer as it is."""
        from . import ops
        return RaggedMaps(self.dplan, self.g, self.c, ops.softmax(self.data.reshape(-1, self.c)).reshape(-1))

    def item(self, i: int):
        """Item i as the tensor the single-frame path holds: [1, d0, d1, c] (a view)."""
        d0, d1 = (int(a[i]) for a in self.dplan.plan.dims[self.g])
        first = int(sum(int(a) * int(b) for a, b in zip(self.dplan.plan.dims[self.g][0][:i], self.dplan.plan.dims[self.g][1][:i])))
        return self.data[first * self.c:(first + d0 * d1) * self.c].reshape(1, d0, d1, self.c)
