"""MTCNN face detection on libhsefr: the step before the age/gender path.

Replaces ``FacialImageProcessing.load_mtcnn`` / ``mtcnn_detect_faces`` (facial_analysis.py:334-352, 478-604).
The three nets of the reference's ``mtcnn.pb`` (P-Net fully convolutional over an image pyramid, R-Net on 24x24
crops, O-Net on 48x48 crops) are read with the TF-free GraphDef reader and executed by a small device-side graph
walker that fuses the patterns the file is made of:

    BiasAdd(Conv2D | MatMul) [+ Relu(v) + alpha * -Relu(-v)]   -> hsefr_conv2d_direct (bias + PReLU fused; a MatMul is
                                                                 the VALID conv spanning the flattened map)
    MaxPool                                                     -> hsefr_maxpool_f32
    RealDiv(Exp(x - Max(x)), Sum(Exp(..)))                      -> hsefr_softmax over the last axis

The image pyramid and the R-Net / O-Net crops (cv2.resize INTER_AREA, facial_analysis.py:507,546,575) are cut on the device
from ONE upload of the frame (csrc/area_resize.hip: hsefr_mtcnn_pyramid_level / hsefr_mtcnn_crops, normalisation and the
(W,H) transposition fused in); every P-Net level is launched before the first result is read back.  The box bookkeeping
(threshold, NMS over a few hundred boxes, regression, squaring, window clipping) is host NumPy, written to give the
reference's numbers including its conventions: boxes are 1-based inclusive, ``np.fix`` truncation.
``device_resize=False`` keeps the round-1 path (host resizes through preprocess.resize_area).
``MTCNNDetector.detect_batch`` runs same-size frames through that launch sequence together (the ``*_batch`` entry points of
include/hsefr.h; the single-frame call with the box logic on the device is such a pass of ONE frame), each frame's result bit for bit
its single-frame result.  ``MTCNNDetector.detect_ragged`` runs frames of ANY sizes
through one pass (include/hsefr_ragged.h, mtcnn_ragged.py: one list of (frame, level) items, one launch per P-Net layer), with the same
bits; ``detect_batch(mixed_sizes=True)`` sends the frames that are alone in their size group through such passes.
"""
from __future__ import annotations

import os
from typing import Dict, List, Optional, Tuple

import numpy as np

from . import _lib, mtcnn_ragged, ops, preprocess
from .graphdef import Graph, GraphNode, read_graph
from .mtcnn_ragged import DevicePlan, PackedFrames, RaggedMaps, RaggedPlan, frame_workspace_bytes, ragged_plan  # noqa: F401  (ragged_plan: part of this module's face)

MTCNN_PB = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "models", "mtcnn.pb")


class _DeviceNet:
    """Evaluate tensors of a small frozen CNN on the GPU, fusing bias / PReLU / softmax sub-graphs."""

    def __init__(self, graph: Graph, device=None):
        torch = _lib.require_gpu()
        self.g = graph
        self._torch = torch
        self.device = _lib.cuda_device(device)
        self._const: Dict[str, object] = {}
        self._programs: Dict[tuple, tuple] = {}

    def _dev(self, node: GraphNode, reshape=None):
        key = node.name + ("" if reshape is None else str(reshape))
        t = self._const.get(key)
        if t is None:
            a = np.ascontiguousarray(self._const_np(node), dtype=np.float32)
            if reshape is not None:
                a = a.reshape(reshape)
            t = self._torch.from_numpy(a).to(self.device)
            self._const[key] = t
        return t

    def _const_np(self, node: GraphNode) -> np.ndarray:
        while node.op == "Identity":
            node = self.g.data_inputs(node)[0][0]
        if node.op != "Const":
            raise NotImplementedError("expected a constant at %s" % node.name)
        return self.g.const_value(node)

    def _is_const(self, node: GraphNode) -> bool:
        while node.op == "Identity":
            node = self.g.data_inputs(node)[0][0]
        return node.op == "Const"

    def _ins(self, node: GraphNode) -> List[GraphNode]:
        return [n for n, _ in self.g.data_inputs(node)]

    # -- pattern matchers ---------------------------------------------------------------------------------
    def _match_prelu(self, node: GraphNode):
        """Add(Relu(v), Mul(alpha, Neg(Relu(Neg(v))))) -> (v, alpha) or None."""
        if node.op not in ("Add", "AddV2"):
            return None
        a, b = self._ins(node)
        for pos, neg in ((a, b), (b, a)):
            if pos.op != "Relu" or neg.op != "Mul":
                continue
            v = self._ins(pos)[0]
            m0, m1 = self._ins(neg)
            for alpha, chain in ((m0, m1), (m1, m0)):
                if not self._is_const(alpha) or chain.op != "Neg":
                    continue
                r = self._ins(chain)[0]
                if r.op != "Relu":
                    continue
                ng = self._ins(r)[0]
                if ng.op == "Neg" and self._ins(ng)[0].name == v.name:
                    return v, alpha
        return None

    def _match_softmax(self, node: GraphNode):
        """RealDiv(Exp(Sub(x, Max(x))), Sum(Exp(Sub(x, Max(x))))) -> x or None."""
        if node.op != "RealDiv":
            return None
        e, s = self._ins(node)
        if e.op != "Exp" or s.op != "Sum" or self._ins(s)[0].name != e.name:
            return None
        sub = self._ins(e)[0]
        if sub.op != "Sub":
            return None
        x, mx = self._ins(sub)
        if mx.op != "Max" or self._ins(mx)[0].name != x.name:
            return None
        return x

    # -- evaluation ------------------------------------------------------------------------------------------
    # The graph is walked ONCE per (fetches, input) pair: pattern matching, attribute parsing and constant uploads produce a linear
    # program of (output name, callable, input names); every later run just executes it (round 3: the recursive interpreter of
    # rounds 1-2 re-matched the PReLU / softmax sub-graphs on every call -- 0.5 ms of host time per frame for ~60 launches).
    def run(self, fetches: List[str], input_name: str, x):
        key = (tuple(fetches), input_name)
        prog = self._programs.get(key)
        in_name = self.g.get_tensor_by_name(input_name)[0].name
        if prog is None:
            steps: List[Tuple[str, object, Tuple[str, ...]]] = []
            done = {in_name}
            outs = []
            for f in fetches:
                node = self.g.get_tensor_by_name(f)[0]
                self._compile(node, steps, done)
                outs.append(node.name)
            prog = self._programs[key] = (steps, outs)
        steps, outs = prog
        vals: Dict[str, object] = {in_name: x}
        for name, fn, ins in steps:
            vals[name] = fn(*[vals[i] for i in ins])
        return [vals[o] for o in outs]

    def _compile(self, node: GraphNode, steps, done) -> None:
        if node.name in done:
            return
        fn, srcs = self._compile_node(node)
        for sn in srcs:
            self._compile(sn, steps, done)
        steps.append((node.name, fn, tuple(sn.name for sn in srcs)))
        done.add(node.name)

    def _compile_linear(self, node: GraphNode, alpha_node: Optional[GraphNode]):
        """node = BiasAdd(Conv2D | MatMul) (or a bare Conv2D/MatMul): one fused kernel launch."""
        bias = None
        if node.op == "BiasAdd":
            lin, bnode = self._ins(node)
            bias = self._dev(bnode)
        else:
            lin = node
        alpha = None if alpha_node is None else self._dev(alpha_node)
        src, wnode = self._ins(lin)
        if lin.op == "Conv2D":
            stride, padding, wdev = lin.attr_ints("strides")[1], lin.attr_s("padding"), self._dev(wnode)
            # (the maps of a ragged pass run the same step with the same weight tensors: one launch over all their items)
            return (lambda xin: xin.conv2d(wdev, bias, alpha, stride, padding) if isinstance(xin, RaggedMaps)
                    else ops.conv2d_direct(xin, wdev, bias, alpha, stride, padding)), [src]
        if lin.op == "MatMul":
            w = self._const_np(wnode)
            cout = int(w.shape[1])
            wdev = self._dev(wnode, (1, 1, w.shape[0], w.shape[1]))

            def matmul(xin):
                n = xin.shape[0]
                flat = xin.reshape(n, 1, 1, -1).contiguous()
                return ops.conv2d_direct(flat, wdev, bias, alpha, 1, "VALID").reshape(n, cout)
            return matmul, [src]
        raise NotImplementedError("%s: op %s" % (lin.name, lin.op))

    def _compile_node(self, node: GraphNode):
        """-> (callable(*input tensors), [input nodes])."""
        op = node.op
        pr = self._match_prelu(node)
        if pr is not None:
            return self._compile_linear(pr[0], pr[1])
        sm = self._match_softmax(node)
        if sm is not None:
            return (lambda x: x.softmax() if isinstance(x, RaggedMaps)
                    else ops.softmax(x.reshape(-1, x.shape[-1]).contiguous()).reshape(x.shape)), [sm]
        if op in ("BiasAdd", "Conv2D", "MatMul"):
            return self._compile_linear(node, None)
        if op == "MaxPool":
            k, st, padding = node.attr_ints("ksize")[1], node.attr_ints("strides")[1], node.attr_s("padding")
            return (lambda x: x.maxpool(k, st, padding) if isinstance(x, RaggedMaps) else ops.maxpool(x, k, st, padding)), [self._ins(node)[0]]
        if op == "Reshape":
            shape = [int(d) for d in self._const_np(self._ins(node)[1]).reshape(-1)]
            return (lambda x: x.reshape(shape).contiguous()), [self._ins(node)[0]]
        if op == "Identity":
            return (lambda x: x), [self._ins(node)[0]]
        raise NotImplementedError("MTCNN graph walker: no kernel for op %s (%s)" % (op, node.name))


# ---- box utilities (facial_analysis.py:354-476 semantics) -------------------------------------------------------
def _iou_suppress(boxes: np.ndarray, threshold: float, use_min: bool) -> np.ndarray:
    """Greedy NMS by descending score; overlap = IoU, or intersection / smaller area ('Min')."""
    if boxes.size == 0:
        return np.empty((0,), np.int64)
    x1, y1, x2, y2, score = (boxes[:, i] for i in range(5))
    area = (x2 - x1 + 1) * (y2 - y1 + 1)
    # the reference: `I = np.argsort(s)`, pick I[-1] (facial_analysis.py:398-403).  Among bit-equal scores (softmax saturated
    # to 1.0f on clear faces) NumPy's default sort leaves lists of <= 16 elements -- the usual R-/O-Net list -- in ascending
    # index order, so the HIGHEST index is picked first.  A stable sort makes that the rule for every list size; the device
    # kernel (csrc/mtcnn_post.hip make_key) uses the same rule.
    order = np.argsort(score.astype(np.float32), kind="stable")
    keep = []
    while order.size:
        top, rest = order[-1], order[:-1]
        keep.append(top)
        iw = np.maximum(0.0, np.minimum(x2[top], x2[rest]) - np.maximum(x1[top], x1[rest]) + 1)
        ih = np.maximum(0.0, np.minimum(y2[top], y2[rest]) - np.maximum(y1[top], y1[rest]) + 1)
        inter = iw * ih
        ov = inter / (np.minimum(area[top], area[rest]) if use_min else (area[top] + area[rest] - inter))
        order = rest[ov <= threshold]
    return np.asarray(keep, np.int64)


def _regress(boxes: np.ndarray, reg: np.ndarray) -> np.ndarray:
    out = boxes.copy()
    w = boxes[:, 2] - boxes[:, 0] + 1
    h = boxes[:, 3] - boxes[:, 1] + 1
    out[:, 0] = boxes[:, 0] + reg[:, 0] * w
    out[:, 1] = boxes[:, 1] + reg[:, 1] * h
    out[:, 2] = boxes[:, 2] + reg[:, 2] * w
    out[:, 3] = boxes[:, 3] + reg[:, 3] * h
    return out


def _square(boxes: np.ndarray) -> np.ndarray:
    out = boxes.copy()
    w = boxes[:, 2] - boxes[:, 0]
    h = boxes[:, 3] - boxes[:, 1]
    side = np.maximum(w, h)
    out[:, 0] = boxes[:, 0] + w * 0.5 - side * 0.5
    out[:, 1] = boxes[:, 1] + h * 0.5 - side * 0.5
    out[:, 2] = out[:, 0] + side
    out[:, 3] = out[:, 1] + side
    return out


def _crop_windows(boxes: np.ndarray, img_w: int, img_h: int):
    """1-based inclusive source window of each box clipped to the frame, and where it lands in the box-sized tile."""
    bw = (boxes[:, 2] - boxes[:, 0] + 1).astype(np.int32)
    bh = (boxes[:, 3] - boxes[:, 1] + 1).astype(np.int32)
    x1, y1 = boxes[:, 0].astype(np.int32), boxes[:, 1].astype(np.int32)
    x2, y2 = boxes[:, 2].astype(np.int32), boxes[:, 3].astype(np.int32)
    tx1, ty1 = np.ones_like(x1), np.ones_like(y1)
    tx2, ty2 = bw.copy(), bh.copy()
    over = x2 > img_w
    tx2[over] = img_w - x2[over] + bw[over]
    x2 = np.where(over, img_w, x2)
    over = y2 > img_h
    ty2[over] = img_h - y2[over] + bh[over]
    y2 = np.where(over, img_h, y2)
    under = x1 < 1
    tx1[under] = 2 - x1[under]
    x1 = np.where(under, 1, x1)
    under = y1 < 1
    ty1[under] = 2 - y1[under]
    y1 = np.where(under, 1, y1)
    return bw, bh, x1, y1, x2, y2, tx1, ty1, tx2, ty2


# ---- the four stage bodies of the cascade on the host (facial_analysis.py:505-603) -----------------------------------------------
# Pure functions of the nets' outputs in the layout the nets give them (a P-Net map is [W', H'], an R-/O-Net output [n, channels]):
# the detector's host path and its overflow fallback run these, csrc/mtcnn_post.hip computes the same lists on the device.
def _crop_table(boxes: np.ndarray, img_w: int, img_h: int) -> np.ndarray:
    """int32 [m, 8] = {x1, y1, x2, y2, tx1, ty1, bw, bh}, the rows hsefr_mtcnn_crops takes."""
    if boxes.shape[0] == 0:
        return np.empty((0, 8), np.int32)
    bw, bh, x1, y1, x2, y2, tx1, ty1, _, _ = _crop_windows(boxes, img_w, img_h)
    return np.stack([x1, y1, x2, y2, tx1, ty1, bw, bh], axis=1).astype(np.int32)


def stage1_level(prob: np.ndarray, reg: np.ndarray, scale: float, thr: float) -> np.ndarray:
    """One pyramid level: prob [W', H'] float32 (the face channel), reg [W', H', 4] float32 -> rows [k, 9] = x1, y1, x2, y2,
    score, 4 regressions of the cells at or above ``thr`` that survive the 0.5 NMS, in pick order."""
    xi, yi = np.nonzero(prob >= thr)
    if xi.size == 0:
        return np.empty((0, 9))
    score = prob[xi, yi]
    # the reference flips the regression maps when exactly one cell fires (:383-387)
    rr = reg[prob.shape[0] - 1 - xi, yi] if xi.size == 1 else reg[xi, yi]
    cell = np.stack([xi, yi], axis=1)
    boxes = np.hstack([np.fix((2 * cell + 1) / scale), np.fix((2 * cell + 12) / scale), score[:, None], rr])
    return boxes[_iou_suppress(boxes, 0.5, False)]


def stage1_finish(found: np.ndarray, img_w: int, img_h: int) -> Tuple[np.ndarray, np.ndarray]:
    """Every level's rows [n, 9] -> boxes [m, 5] after the 0.7 NMS, the P-Net regression, squaring and truncation, and their
    crop table [m, 8]."""
    boxes = np.asarray(found, np.float64)
    if boxes.shape[0] == 0:
        return np.empty((0, 5)), np.empty((0, 8), np.int32)
    boxes = boxes[_iou_suppress(boxes, 0.7, False)]
    rw, rh = boxes[:, 2] - boxes[:, 0], boxes[:, 3] - boxes[:, 1]
    boxes = np.stack([boxes[:, 0] + boxes[:, 5] * rw, boxes[:, 1] + boxes[:, 6] * rh, boxes[:, 2] + boxes[:, 7] * rw,
                      boxes[:, 3] + boxes[:, 8] * rh, boxes[:, 4]], axis=1)
    boxes = _square(boxes)
    boxes[:, 0:4] = np.fix(boxes[:, 0:4]).astype(np.int32)
    return boxes, _crop_table(boxes, img_w, img_h)


def stage2_finish(boxes_in: np.ndarray, prob: np.ndarray, reg: np.ndarray, thr: float, img_w: int, img_h: int) -> Tuple[np.ndarray, np.ndarray]:
    """R-Net's prob [n, 2] and reg [n, 4] on the stage-1 boxes [n, 5] -> int32 boxes [m, 5] (scores above ``thr``, 0.7 NMS,
    regression, squaring; the whole row truncated, score column included, as the reference's np.fix does) and their crop table."""
    boxes = np.asarray(boxes_in)
    score = prob[:, 1]
    ok = np.nonzero(score > thr)[0]
    boxes = np.hstack([boxes[ok, 0:4], score[ok][:, None]])
    reg = reg[ok]
    if boxes.shape[0] == 0:
        return np.empty((0, 5)), np.empty((0, 8), np.int32)
    keep = _iou_suppress(boxes, 0.7, False)
    boxes = _square(_regress(boxes[keep], reg[keep]))
    boxes = np.fix(boxes).astype(np.int32)
    return boxes, _crop_table(boxes, img_w, img_h)


def stage3_finish(boxes_in: np.ndarray, prob: np.ndarray, reg: np.ndarray, pts: np.ndarray, thr: float) -> Tuple[np.ndarray, np.ndarray]:
    """O-Net's prob [n, 2], reg [n, 4] and landmarks pts [n, 10] on the stage-2 boxes [n, 5] -> boxes [m, 5] float64 (regressed,
    then the 0.7 'Min' NMS) and landmarks [m, 10] float32 in frame pixels, taken relative to the boxes BEFORE the regression."""
    boxes = np.asarray(boxes_in)
    score = prob[:, 1]
    ok = np.nonzero(score > thr)[0]
    points = pts[ok].T                                           # [10, n]
    reg = reg[ok]
    boxes = np.hstack([boxes[ok, 0:4], score[ok][:, None]])
    bw = boxes[:, 2] - boxes[:, 0] + 1
    bh = boxes[:, 3] - boxes[:, 1] + 1
    points[0:5, :] = bw[None, :] * points[0:5, :] + boxes[:, 0][None, :] - 1
    points[5:10, :] = bh[None, :] * points[5:10, :] + boxes[:, 1][None, :] - 1
    if boxes.shape[0]:
        boxes = _regress(boxes, reg)
        keep = _iou_suppress(boxes, 0.7, True)
        boxes, points = boxes[keep], points[:, keep]
    return boxes, np.ascontiguousarray(points.T)


# ---- bookkeeping of the batched entry points (pure functions: tests/test_mtcnn_batch_cpu.py) ----------------------------------------
def plan_passes(shapes, max_frames: int) -> List[Tuple[Tuple[int, int], List[int]]]:
    """The passes of ``MTCNNDetector.detect_batch`` over frames of the given (h, w): frames of one size form a group (groups in the
    order their first frame appears, a group's frames in list order), a group runs in passes of at most ``max_frames`` frames.
    -> [((h, w), [indices into the list])]; every index appears exactly once."""
    max_frames = int(max_frames)
    if max_frames < 1:
        raise ValueError("max_frames must be at least 1, not %d" % max_frames)
    groups: Dict[Tuple[int, int], List[int]] = {}
    for i, hw in enumerate(shapes):
        groups.setdefault((int(hw[0]), int(hw[1])), []).append(i)
    return [(hw, idx[a:a + max_frames]) for hw, idx in groups.items() for a in range(0, len(idx), max_frames)]


def plan_mixed_passes(shapes, max_frames: int, max_bytes: int = 4 << 30, minsize: int = 32,
                      factor: float = 0.709) -> List[Tuple[Optional[Tuple[int, int]], List[int]]]:
    """The passes of ``detect_batch(mixed_sizes=True)``: the same-size groups of two or more frames stay the passes plan_passes gives,
    -> ((h, w), [indices]); the frames left alone in their group are gathered, in list order, into ragged passes -> (None, [indices])
    of at most ``max_frames`` frames whose planned workspace (mtcnn_ragged.frame_workspace_bytes, summed; ``minsize`` and ``factor``
    are the detector's) is at most ``max_bytes`` -- a pass closes before the frame that would exceed either limit, and a frame that
    exceeds ``max_bytes`` alone stands alone.  A ragged pass of ONE frame is the single-frame call: ((h, w), [index]), what
    plan_passes gives.  So is a lone frame without a pyramid level, which needs no launch and joins no pass.  Same-size passes come
    first, then the ragged passes, then the single frames, each in list order; every index appears exactly once."""
    max_bytes = int(max_bytes)
    shapes = [(int(hw[0]), int(hw[1])) for hw in shapes]
    passes: List[Tuple[Optional[Tuple[int, int]], List[int]]] = []
    lone: List[int] = []
    for hw, idx in plan_passes(shapes, max_frames):
        if len(idx) > 1:
            passes.append((hw, idx))
        else:
            lone.append(idx[0])                # (a group's last pass may be a single frame too: it is alone in ITS pass)
    lone.sort()
    singles: List[int] = []                    # frames that take the single-frame call
    ragged: List[List[int]] = []
    used = 0
    for i in lone:
        h, w = shapes[i]
        need = frame_workspace_bytes(h, w, minsize, factor)
        if need == h * w * 3:                  # no pyramid level: no launch, nothing to share
            singles.append(i)
            continue
        if not ragged or len(ragged[-1]) >= int(max_frames) or used + need > max_bytes:
            ragged.append([])
            used = 0
        ragged[-1].append(i)
        used += need
    singles += [g[0] for g in ragged if len(g) == 1]
    passes += [(None, g) for g in ragged if len(g) > 1]
    passes += [(shapes[i], [i]) for i in sorted(singles)]
    return passes


def split_by_counts(items, counts) -> List[list]:
    """A flat list that holds ``counts[0]`` items of frame 0, then ``counts[1]`` of frame 1, ... -> one list per frame."""
    items = list(items)
    if sum(int(c) for c in counts) != len(items):
        raise ValueError("%d items for counts that sum to %d" % (len(items), sum(int(c) for c in counts)))
    out, at = [], 0
    for c in counts:
        out.append(items[at:at + int(c)])
        at += int(c)
    return out


def empty_detection() -> Tuple[np.ndarray, np.ndarray]:
    """What detect_batch returns for a frame without faces."""
    return np.empty((0, 5), np.float64), np.empty((10, 0), np.float32)


class MTCNNDetector:
    """callable(img_rgb_uint8) -> (bounding_boxes [n,5] = x1,y1,x2,y2,score; points [10,n])."""

    THRESHOLDS = (0.6, 0.7, 0.9)       # facial_analysis.py:481
    FACTOR = 0.709                     # :483

    def __init__(self, mtcnn_pb: Optional[str] = None, minsize: int = 32, device=None, device_resize: bool = True,
                 device_boxes: Optional[bool] = None):
        """device_resize: pyramid levels and crops resampled on the GPU (csrc/area_resize.hip); device_boxes (default: as
        device_resize): candidate generation, NMS, box regression, squaring, crop windows and landmarks on the GPU too
        (csrc/mtcnn_post.hip) -- the host then only reads three box counts per frame."""
        torch = _lib.require_gpu()
        self._torch = torch
        self.minsize = minsize
        self.device_resize = device_resize
        self.device_boxes = device_resize if device_boxes is None else bool(device_boxes)
        if self.device_boxes and not device_resize:
            raise ValueError("device_boxes needs device_resize (the crops are cut from the frame on the device)")
        self.host_fallbacks = 0            # frames redone on the host because a candidate list overflowed
        self.ragged_passes = 0             # mixed-size passes detect_batch(mixed_sizes=True) ran, and the frames in them
        self.ragged_frames = 0
        self._ragged_plans: Dict[tuple, DevicePlan] = {}      # (shapes, minsize) -> the plan and its tables on the device
        self._work = None                  # cap-sized work tensors of the device box logic, allocated once (_work_tensors)
        self.device = _lib.cuda_device(device)
        self.net = _DeviceNet(read_graph(mtcnn_pb or MTCNN_PB), self.device)

    # the three sess.run lambdas of load_mtcnn (:347-349)
    def pnet(self, img):
        return self.net.run(['pnet/conv4-2/BiasAdd:0', 'pnet/prob1:0'], 'pnet/input:0', img)

    def rnet(self, img):
        return self.net.run(['rnet/conv5-2/conv5-2:0', 'rnet/prob1:0'], 'rnet/input:0', img)

    def onet(self, img):
        return self.net.run(['onet/conv6-2/conv6-2:0', 'onet/conv6-3/conv6-3:0', 'onet/prob1:0'], 'onet/input:0', img)

    def pyramid_scales(self, h: int, w: int) -> List[float]:
        return mtcnn_ragged.pyramid_scales(h, w, self.minsize, self.FACTOR)

    def _to_device(self, a: np.ndarray):
        return self._torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(self.device)

    def _level_device(self, frame, h: int, w: int, hs: int, ws: int):
        """One pyramid level of the uploaded frame (``frame``: CUDA uint8 [h, w, 3] -- an argument, not detector state, so one
        detector can serve several threads), normalised and transposed: CUDA float32 [1, ws, hs, 3]."""
        torch = self._torch
        out = torch.empty((1, ws, hs, 3), dtype=torch.float32, device=self.device)
        with _lib.on_device(out):
            _lib.check(_lib.lib().hsefr_mtcnn_pyramid_level(frame.data_ptr(), out.data_ptr(), h, w, hs, ws,
                                                            _lib.current_stream_ptr()), "hsefr_mtcnn_pyramid_level")
        return out

    def _stage1(self, img: np.ndarray, frame=None) -> np.ndarray:
        h, w = img.shape[:2]
        found = [np.empty((0, 9))]
        sizes = mtcnn_ragged.level_sizes(h, w, self.minsize, self.FACTOR)
        maps = []
        for _, hs, ws in sizes:                                      # launch every level first ...
            if self.device_resize:
                x = self._level_device(frame, h, w, hs, ws)
            else:
                level = (preprocess.resize_area(img, ws, hs) - 127.5) * 0.0078125
                x = self._to_device(np.transpose(level, (1, 0, 2))[None])           # nets see (W, H)
            maps.append(self.pnet(x))
        for (scale, _, _), (reg_t, prob_t) in zip(sizes, maps):      # ... then read the maps back
            prob = prob_t[0, :, :, 1].cpu().numpy()                  # [W', H']
            reg = reg_t[0].cpu().numpy()                             # [W', H', 4]
            found.append(stage1_level(prob, reg, scale, self.THRESHOLDS[0]))
        return np.concatenate(found, axis=0)

    def _crops(self, img: np.ndarray, boxes: np.ndarray, size: int, frame=None):
        h, w = img.shape[:2]
        bw, bh, x1, y1, x2, y2, tx1, ty1, tx2, ty2 = _crop_windows(boxes, w, h)
        if self.device_resize:
            torch = self._torch
            n = boxes.shape[0]
            tab = np.stack([x1, y1, x2, y2, tx1, ty1, bw, bh], axis=1).astype(np.int32)
            d_tab = torch.from_numpy(np.ascontiguousarray(tab)).to(self.device)
            out = torch.empty((n, size, size, 3), dtype=torch.float32, device=self.device)
            with _lib.on_device(out):
                _lib.check(_lib.lib().hsefr_mtcnn_crops(frame.data_ptr(), d_tab.data_ptr(), out.data_ptr(), h, w, n, size,
                                                        _lib.current_stream_ptr()), "hsefr_mtcnn_crops")
            return out
        out = np.zeros((boxes.shape[0], size, size, 3))
        for k in range(boxes.shape[0]):
            tile = np.zeros((int(bh[k]), int(bw[k]), 3))
            tile[ty1[k] - 1:ty2[k], tx1[k] - 1:tx2[k], :] = img[y1[k] - 1:y2[k], x1[k] - 1:x2[k], :]
            out[k] = preprocess.resize_area(tile, size, size)
        out = (out - 127.5) * 0.0078125
        return self._to_device(np.transpose(out, (0, 2, 1, 3)))      # [n, W, H, 3]

    # ---- the cascade with its box logic on the device, one frame or many per pass (csrc/mtcnn_post.hip, the *_batch entries) -------------
    def _work_tensors(self, cap: int, n_frames: int):
        """The [frames, cap, .] lists of the device box logic, allocated once per detector and thread and grown to the largest pass
        seen (work on one stream is ordered, so a pass may overwrite what the previous pass of the same thread left; a pass takes the
        first n_frames frames' rows, which are contiguous)."""
        import threading
        torch, dev = self._torch, self.device
        if self._work is None:
            self._work = threading.local()
        wk = self._work
        if getattr(wk, "cap", None) != cap or wk.frames < n_frames:
            wk.cap, wk.frames = cap, n_frames
            wk.found = torch.empty((n_frames, cap, 9), dtype=torch.float64, device=dev)
            wk.boxes = [torch.empty((n_frames, cap, 5), dtype=torch.float64, device=dev) for _ in range(3)]
            wk.tab = torch.empty((n_frames, cap, 8), dtype=torch.int32, device=dev)
            wk.points = torch.empty((n_frames, cap, 10), dtype=torch.float32, device=dev)
        return wk

    def _detect_pass(self, imgs: List[np.ndarray], stack_out: Optional[list] = None) -> List[Optional[Tuple[np.ndarray, np.ndarray]]]:
        """One pass over same-size frames: the launches of the cascade, each covering every frame, and three read-backs.  Per
        frame (boxes, points), or None where that frame's candidate list overflowed (the caller redoes that frame alone).
        ``stack_out``: a list that receives the pass's uploaded frame stack (CUDA uint8 [frames, h, w, 3]), for a caller that cuts
        the faces from it on the device.  The single-frame call is a pass of one (__call__).

        A frame's result does not depend on the pass it stands in: the pyramid, the crops and the box logic compute a frame's values
        from that frame's data by the same operations (the kernels take the frame as a grid index); the nets run on the stacked levels
        and on the concatenated crop lists, and conv2d_direct, maxpool_f32 and softmax (csrc/smallnet.hip) compute each output element
        from its own image alone in a fixed FMA order, so a row's values do not depend on the batch it stands in
        (tests/test_mtcnn_batch_gpu.py checks both)."""
        stack = self._torch.from_numpy(np.stack(imgs)).to(self.device)     # one upload per pass
        if stack_out is not None:
            stack_out.append(stack)
        return self._detect_stack_body(stack)

    def detect_stack(self, stack) -> List[Optional[Tuple[np.ndarray, np.ndarray]]]:
        """_detect_pass for a pass whose frames are on the device already: ``stack`` a contiguous CUDA uint8 RGB [frames, h, w, 3]
        tensor on the detector's device (preprocess_device.prepare_frames writes one).  Nothing is uploaded; the launches, the
        read-backs and the results are those of _detect_pass on the same frames.  Per frame (boxes, points), or None where that frame's
        candidate list overflowed (the caller redoes that frame alone: ``self(stack[row].cpu().numpy())``).  A stack of frames too small
        for a pyramid level gives empty detections without a launch.  Needs ``device_boxes``."""
        torch = self._torch
        if not self.device_boxes:
            raise ValueError("detect_stack needs a detector with device_boxes")
        if not (isinstance(stack, torch.Tensor) and stack.is_cuda and stack.dtype == torch.uint8 and stack.dim() == 4 and stack.shape[3] == 3
                and stack.is_contiguous()):
            raise ValueError("detect_stack takes a contiguous CUDA uint8 RGB stack [frames, H, W, 3]")
        if stack.device != self.device:
            raise ValueError("the stack is on %s, the detector on %s" % (stack.device, self.device))
        if stack.shape[0] == 0 or not self.pyramid_scales(int(stack.shape[1]), int(stack.shape[2])):
            return [empty_detection() for _ in range(int(stack.shape[0]))]
        return self._detect_stack_body(stack)

    def _detect_stack_body(self, stack, counts: Optional[list] = None) -> List[Optional[Tuple[np.ndarray, np.ndarray]]]:
        """_detect_pass behind its upload (``counts``: see _finish_pass)."""
        torch, L = self._torch, _lib.lib()
        n_frames, h, w = int(stack.shape[0]), int(stack.shape[1]), int(stack.shape[2])
        cap = int(L.hsefr_mtcnn_post_capacity())
        dev = self.device
        results: List[Optional[Tuple[np.ndarray, np.ndarray]]] = [empty_detection() for _ in range(n_frames)]
        with _lib.on_device(stack):
            st = _lib.current_stream_ptr()
            wk = self._work_tensors(cap, n_frames)
            counters = torch.zeros((n_frames, 8), dtype=torch.int32, device=dev)
            found, boxes1, tab = wk.found, wk.boxes[0], wk.tab
            thr = [float(np.float32(t)) for t in self.THRESHOLDS]
            for scale, hs, ws in mtcnn_ragged.level_sizes(h, w, self.minsize, self.FACTOR):
                level = torch.empty((n_frames, ws, hs, 3), dtype=torch.float32, device=dev)
                _lib.check(L.hsefr_mtcnn_pyramid_level_batch(stack.data_ptr(), level.data_ptr(), n_frames, h, w, hs, ws, st),
                           "hsefr_mtcnn_pyramid_level_batch")
                reg_t, prob_t = self.pnet(level)
                reg_t, prob_t = reg_t.contiguous(), prob_t.contiguous()
                _lib.check(L.hsefr_mtcnn_stage1_level_batch(prob_t.data_ptr(), reg_t.data_ptr(), n_frames, int(prob_t.shape[1]), int(prob_t.shape[2]),
                                                            float(scale), thr[0], found.data_ptr(), counters.data_ptr(), st),
                           "hsefr_mtcnn_stage1_level_batch")
            _lib.check(L.hsefr_mtcnn_stage1_finish_batch(found.data_ptr(), counters.data_ptr(), boxes1.data_ptr(), tab.data_ptr(), n_frames, w, h, st),
                       "hsefr_mtcnn_stage1_finish_batch")
            crops_of = lambda tab, d_off, total, size, out: _lib.check(      # noqa: E731
                L.hsefr_mtcnn_crops_batch(stack.data_ptr(), tab.data_ptr(), d_off.data_ptr(), out.data_ptr(), n_frames, h, w, total, size, st),
                "hsefr_mtcnn_crops_batch")
            finish = lambda stage, b_in, d_off, total, prob, reg, pts, t, b_out, tab, points: _lib.check(      # noqa: E731
                L.hsefr_mtcnn_stage_finish_batch(stage, b_in.data_ptr(), d_off.data_ptr(), total, prob.data_ptr(), reg.data_ptr(),
                                                 None if pts is None else pts.data_ptr(), t, b_out.data_ptr(), None if tab is None else tab.data_ptr(),
                                                 None if points is None else points.data_ptr(), counters.data_ptr(), n_frames, w, h, st),
                "hsefr_mtcnn_stage_finish_batch")
            return self._finish_pass(n_frames, counters, wk, results, crops_of, finish, counts)

    def _finish_pass(self, n_frames: int, counters, wk, results, crops_of, finish,
                     counts: Optional[list] = None) -> List[Optional[Tuple[np.ndarray, np.ndarray]]]:
        """A pass behind its stage 1 (run under on_device): the three read-backs, R-Net and O-Net on the concatenated crop lists, the
        results per frame.  ``crops_of(tab, d_off, total, size, out)`` cuts the crops of all frames and ``finish(stage, boxes_in, d_off,
        total, prob, reg, pts, thr, boxes_out, tab, points)`` runs stage 2 / 3 of all frames: the same-size pass and the ragged pass
        differ only in where those two read a frame's place and size.  ``counts``: a list that receives every read-back of the
        counters, int32 [frames, 8] each (columns 1, 2, 3: the boxes stages 1, 2, 3 kept; a stage not reached has 0), for a caller
        that has to know WHERE a frame's cascade emptied (__call__)."""
        torch, dev = self._torch, self.device
        (boxes1, boxes2, boxes3), tab, points3 = wk.boxes, wk.tab, wk.points
        thr = [float(np.float32(t)) for t in self.THRESHOLDS]
        seen = [] if counts is None else counts
        c = counters.cpu().numpy()                                     # read-back 1
        seen.append(c)
        over = c[:, 4] != 0                                            # (only a pyramid level can overflow: later lists are no longer)
        for b in np.nonzero(over)[0]:
            results[int(b)] = None

        def offsets_of(counts):                                        # host scan of the counts just read; a 4(B+1)-byte upload
            counts = np.where(over, 0, counts).astype(np.int64)
            off = np.concatenate([[0], np.cumsum(counts)])
            return int(off[-1]), torch.from_numpy(off.astype(np.int32)).to(dev)

        total, d_off = offsets_of(c[:, 1])
        if total == 0:
            return results
        crops = torch.empty((total, 24, 24, 3), dtype=torch.float32, device=dev)
        crops_of(tab, d_off, total, 24, crops)
        reg_t, prob_t = self.rnet(crops)
        reg_t, prob_t = reg_t.contiguous(), prob_t.contiguous()
        finish(2, boxes1, d_off, total, prob_t, reg_t, None, thr[1], boxes2, tab, None)
        c = counters.cpu().numpy()                                     # read-back 2
        seen.append(c)
        n2 = np.where(over, 0, c[:, 2])
        total, d_off = offsets_of(c[:, 2])
        if total == 0:
            return results
        crops = torch.empty((total, 48, 48, 3), dtype=torch.float32, device=dev)
        crops_of(tab, d_off, total, 48, crops)
        reg_t, pts_t, prob_t = self.onet(crops)
        reg_t, pts_t, prob_t = reg_t.contiguous(), pts_t.contiguous(), prob_t.contiguous()
        finish(3, boxes2, d_off, total, prob_t, reg_t, pts_t, thr[2], boxes3, None, points3)
        # read-back 3: the counts and the first max(n2) rows of every frame's lists (stage 3 keeps at most its n2 inputs) as one copy
        m = int(n2.max())
        packed = torch.cat([counters.view(torch.uint8).reshape(-1), boxes3[:n_frames, :m].contiguous().view(torch.uint8).reshape(-1),
                            points3[:n_frames, :m].contiguous().view(torch.uint8).reshape(-1)]).cpu().numpy()
        at_boxes = n_frames * 32
        at_points = at_boxes + n_frames * m * 40
        c = np.frombuffer(packed, np.int32, n_frames * 8, 0).reshape(n_frames, 8)
        seen.append(c)
        boxes = np.frombuffer(packed, np.float64, n_frames * m * 5, at_boxes).reshape(n_frames, m, 5)
        points = np.frombuffer(packed, np.float32, n_frames * m * 10, at_points).reshape(n_frames, m, 10)
        for b in range(n_frames):
            n3 = int(c[b, 3])
            if results[b] is not None and n3 > 0:
                results[b] = (boxes[b, :n3].copy(), np.ascontiguousarray(points[b, :n3].T))
        return results

    # ---- frames of different sizes in one pass (csrc/mtcnn_ragged.hip, mtcnn_ragged.py) ----------------------------------------------
    RAGGED_PLANS_KEPT = 32             # plans (and their tables on the device) a detector keeps, most recently used last

    def _ragged_device_plan(self, shapes: tuple) -> DevicePlan:
        """The plan of a ragged pass over frames of these shapes with its tables on the device: built and uploaded once per
        (shapes, minsize), then reused (an album's retry passes, a video's frames)."""
        key = (shapes, self.minsize)
        dplan = self._ragged_plans.pop(key, None)
        if dplan is None:
            dplan = DevicePlan(ragged_plan(shapes, self.minsize, self.FACTOR), self.device)
            while len(self._ragged_plans) >= self.RAGGED_PLANS_KEPT:
                self._ragged_plans.pop(next(iter(self._ragged_plans)))
        self._ragged_plans[key] = dplan
        return dplan

    def detect_ragged(self, frames, packed_out: Optional[list] = None) -> List[Optional[Tuple[np.ndarray, np.ndarray]]]:
        """ONE pass over frames of any sizes (uint8 RGB [H, W, 3] each): per frame (boxes [n,5] float64, points [10,n] float32), bit
        for bit what ``self(frame)`` returns (a frame without faces gives shapes (0, 5) and (10, 0)), or None where that frame's
        candidate list overflowed (the caller redoes that frame alone).  Uploads: the frames' bytes packed back to back, the plan's
        tables (once per list of shapes), the two small offset tables of the crop lists; launches: one per P-Net layer over ALL pyramid
        levels of ALL frames (the same-size pass makes one per level), R-Net and O-Net on the concatenated crop lists; the three
        read-backs of the same-size pass.  Needs ``device_boxes``.

        Bit identity with the single-frame call: the pyramid, the crops and the box logic run the one-frame bodies the single-frame
        entries run (csrc/area_resize_px.h, csrc/mtcnn_post_frame.h), with a frame's place and size read from the plan's tables; P-Net
        runs through the program _DeviceNet compiled, with the same weight tensors, each output's FMA chain in conv2d_direct's order
        (tests/test_mtcnn_ragged_gpu.py checks every step and the whole).
        ``packed_out``: a list that receives the pass's uploaded frames as a PackedFrames, for a caller that cuts the faces from them
        on the device (nothing is appended where no frame has a pyramid level: nothing is uploaded then)."""
        if not self.device_boxes:
            raise ValueError("detect_ragged needs a detector with device_boxes")
        imgs = [self._check_frame(f) for f in frames]
        if not imgs:
            return []
        shapes = tuple((int(f.shape[0]), int(f.shape[1])) for f in imgs)
        if self._ragged_device_plan(shapes).plan.n_items == 0:            # no frame has a pyramid level: no upload, no launch
            return [empty_detection() for _ in imgs]
        packed = self._torch.from_numpy(np.concatenate([np.ascontiguousarray(f).reshape(-1) for f in imgs])).to(self.device)      # one upload per pass
        if packed_out is not None:
            packed_out.append(PackedFrames(packed, shapes))
        return self._detect_ragged_body(shapes, packed)

    def detect_packed(self, packed: PackedFrames) -> List[Optional[Tuple[np.ndarray, np.ndarray]]]:
        """detect_ragged for a pass whose frames are on the device already: ``packed`` a PackedFrames of RGB frames on the detector's
        device (preprocess_device.prepare_packed writes one).  Nothing is uploaded but the plan's tables where the list of shapes is new;
        the launches, the read-backs and the results are those of detect_ragged on the same frames.  Per frame (boxes, points), or None
        where that frame's candidate list overflowed (the caller redoes that frame alone: ``self(packed.frame(row).cpu().numpy())``).
        Needs ``device_boxes``."""
        if not self.device_boxes:
            raise ValueError("detect_packed needs a detector with device_boxes")
        if not isinstance(packed, PackedFrames):
            raise ValueError("detect_packed takes a PackedFrames, not %s" % type(packed).__name__)
        if not getattr(packed.data, "is_cuda", False):
            raise ValueError("detect_packed takes frames on the device (a CUDA buffer)")
        if packed.data.device != self.device:
            raise ValueError("the frames are on %s, the detector on %s" % (packed.data.device, self.device))
        if not len(packed):
            return []
        if self._ragged_device_plan(packed.shapes).plan.n_items == 0:
            return [empty_detection() for _ in packed.shapes]
        return self._detect_ragged_body(packed.shapes, packed.data)

    def _detect_ragged_body(self, shapes: tuple, packed) -> List[Optional[Tuple[np.ndarray, np.ndarray]]]:
        """detect_ragged behind its upload: ``packed`` the CUDA uint8 buffer that holds the frames of ``shapes`` back to back."""
        torch, L, R = self._torch, _lib.lib(), _lib.ragged_lib()
        dplan = self._ragged_device_plan(shapes)
        plan = dplan.plan
        n_frames, dev = plan.n_frames, self.device
        results: List[Optional[Tuple[np.ndarray, np.ndarray]]] = [empty_detection() for _ in range(n_frames)]
        cap = int(L.hsefr_mtcnn_post_capacity())
        if int(R.hsefr_ragged_capacity()) != cap:
            raise RuntimeError("libhsefr.so and libhsefr_ragged.so were built from different sources (list capacity %d / %d)"
                               % (cap, int(R.hsefr_ragged_capacity())))
        with _lib.on_device(packed):
            st = _lib.current_stream_ptr()
            wk = self._work_tensors(cap, n_frames)
            counters = torch.zeros((n_frames, 8), dtype=torch.int32, device=dev)
            levels = torch.empty(plan.pixels[0] * 3, dtype=torch.float32, device=dev)
            _lib.ragged_check(R.hsefr_ragged_pyramid(packed.data_ptr(), plan.frames_bytes, dplan.frames, n_frames, dplan.levels, plan.n_items,
                                                     dplan.level_block_item, len(plan.level_block_item), levels.data_ptr(), plan.pixels[0] * 3,
                                                     plan.level_lds, st), "hsefr_ragged_pyramid")
            reg_m, prob_m = self.pnet(RaggedMaps(dplan, 0, 3, levels))
            _lib.ragged_check(R.hsefr_ragged_stage1(prob_m.data.data_ptr(), reg_m.data.data_ptr(), plan.pixels[-1], dplan.frames, n_frames, dplan.cells,
                                                    plan.n_items, float(np.float32(self.THRESHOLDS[0])), wk.found.data_ptr(), counters.data_ptr(),
                                                    wk.boxes[0].data_ptr(), wk.tab.data_ptr(), st), "hsefr_ragged_stage1")
            crops_of = lambda tab, d_off, total, size, out: _lib.ragged_check(      # noqa: E731
                R.hsefr_ragged_crops(packed.data_ptr(), plan.frames_bytes, dplan.frames, n_frames, tab.data_ptr(), d_off.data_ptr(), out.data_ptr(),
                                     cap, total, size, st), "hsefr_ragged_crops")
            finish = lambda stage, b_in, d_off, total, prob, reg, pts, t, b_out, tab, points: _lib.ragged_check(      # noqa: E731
                R.hsefr_ragged_stage_finish(stage, b_in.data_ptr(), d_off.data_ptr(), total, prob.data_ptr(), reg.data_ptr(),
                                            None if pts is None else pts.data_ptr(), t, b_out.data_ptr(), None if tab is None else tab.data_ptr(),
                                            None if points is None else points.data_ptr(), counters.data_ptr(), dplan.frames, n_frames, st),
                "hsefr_ragged_stage_finish")
            return self._finish_pass(n_frames, counters, wk, results, crops_of, finish)

    def _check_frame(self, img) -> np.ndarray:
        """The input rules of __call__."""
        img = np.asarray(img)
        if img.ndim != 3 or img.shape[2] != 3:
            raise ValueError("the detector takes an RGB frame [H, W, 3]")
        if self.device_resize and img.dtype != np.uint8:
            raise ValueError("device_resize takes a uint8 RGB frame [H, W, 3]; construct the detector with device_resize=False "
                             "for %s frames" % img.dtype)
        return img

    def _alone(self, img: np.ndarray) -> Tuple[np.ndarray, np.ndarray]:
        """self(img) with detect_batch's empty shapes."""
        boxes, points = self(img)
        return (boxes, points) if boxes.shape[0] else empty_detection()

    def detect_batch(self, frames, max_frames: int = 32, return_stacks: bool = False, mixed_sizes: bool = False, packed_sources: bool = False):
        """[(boxes [n,5] float64, points [10,n] float32)] in the order of ``frames`` (uint8 RGB [H, W, 3] each), every entry bit for bit
        what ``self(frame)`` returns; a frame without faces gives shapes (0, 5) and (10, 0).  Frames of one size run together, at most
        ``max_frames`` per pass: one upload, the launches of one frame and three read-backs per pass (a pass of ONE frame is the
        single-frame call).  A frame whose candidate list
        overflows the device capacity is redone alone through ``self(frame)`` (counted in ``host_fallbacks``); the others of its pass
        keep their results.  A detector without ``device_boxes`` has no batched path and runs the frames one by one.
        ``return_stacks``: -> (that list, sources), where sources[i] is (stack, row) -- the CUDA uint8 [frames, h, w, 3] stack the
        frame's pass uploaded and the frame's row in it -- or None for a frame that took the single-frame call (a pass of one, a frame
        redone after an overflow, any frame of a detector without ``device_boxes``) or had no pyramid level.
        ``mixed_sizes``: the frames that would take the single-frame call because nothing shares their size run together in ragged
        passes instead (plan_mixed_passes, detect_ragged), with the same results; ``ragged_passes`` and ``ragged_frames`` count them,
        a frame that overflows there is redone alone as above, and ``sources`` stays None for the frames of a ragged pass.
        ``packed_sources`` (with ``return_stacks`` and ``mixed_sizes``): sources[i] of a frame of a ragged pass is (PackedFrames, row)
        instead -- the buffer that pass uploaded and the frame's place in it (preprocess_device.face_crops_packed cuts from it) -- and
        None where the frame was redone alone."""
        imgs = [self._check_frame(f) for f in frames]
        shapes = [f.shape[:2] for f in imgs]
        passes = plan_mixed_passes(shapes, max_frames, minsize=self.minsize, factor=self.FACTOR) if mixed_sizes and self.device_boxes else \
            plan_passes(shapes, max_frames)
        sources: list = [None] * len(imgs)
        if not self.device_boxes:
            alone = [self._alone(f) for f in imgs]
            return (alone, sources) if return_stacks else alone
        results: List[Optional[Tuple[np.ndarray, np.ndarray]]] = [None] * len(imgs)
        for hw, idx in passes:
            group = [imgs[i] for i in idx]
            kept: list = []                                                # receives the pass's frames on the device where the caller asked for them
            if hw is None:                                                 # frames of different sizes: one ragged pass
                self.ragged_passes += 1
                self.ragged_frames += len(idx)
                got = self.detect_ragged(group, kept if return_stacks and packed_sources else None)
            elif not self.pyramid_scales(*hw):                             # smaller than minsize: no level, no launch
                got = [empty_detection() for _ in idx]
            elif len(idx) == 1:                                            # nothing to share: the single-frame call, without the stacking
                got = [self._alone(group[0])]
            else:
                got = self._detect_pass(group, kept) if return_stacks else self._detect_pass(group)
            for row, (i, res) in enumerate(zip(idx, got)):
                results[i] = res if res is not None else self._alone(imgs[i])       # an overflowed frame is redone alone
                if res is not None and kept:
                    sources[i] = (kept[0], row)
        return (results, sources) if return_stacks else results

    def __call__(self, img: np.ndarray) -> Tuple[np.ndarray, np.ndarray]:
        img = self._check_frame(img)   # (the device resampler is OpenCV's 8-bit path; float frames: MTCNNDetector(device_resize=False))
        frame = None
        if self.device_resize:
            frame = self._torch.from_numpy(np.ascontiguousarray(img)).to(self.device)     # local: no per-frame detector state
        if self.device_boxes:              # a pass of one frame (frame[None]: a contiguous view)
            counts: list = []
            res = self._detect_stack_body(frame[None], counts)[0]
            if res is not None:
                n1, n2 = (int(n) for n in counts[-1][0, 1:3])
                if n1 == 0 or n2 == 0:     # this call's own empty results where stage 1 or 2 kept nothing (stage 3: empty_detection())
                    return np.empty((0, 9) if n1 == 0 else (0, 5)), np.array([])
                return res
            self.host_fallbacks += 1
        points = np.array([])
        h, w = img.shape[:2]
        boxes = self._stage1(img, frame)
        if boxes.shape[0]:
            boxes, _ = stage1_finish(boxes, w, h)
        if boxes.shape[0]:
            reg_t, prob_t = self.rnet(self._crops(img, boxes, 24, frame))
            boxes, _ = stage2_finish(boxes, prob_t.cpu().numpy(), reg_t.cpu().numpy(), self.THRESHOLDS[1], w, h)
        if boxes.shape[0]:
            reg_t, pts_t, prob_t = self.onet(self._crops(img, boxes, 48, frame))
            boxes, points = stage3_finish(boxes, prob_t.cpu().numpy(), reg_t.cpu().numpy(), pts_t.cpu().numpy(), self.THRESHOLDS[2])
            points = points.T                                        # [10, n]
        return boxes, points
