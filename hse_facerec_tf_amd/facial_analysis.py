"""Drop-in for the age/gender/identity part of the reference's ``FacialImageProcessing``
(age_gender_identity/facial_analysis.py:36-130,225-294): ``age_gender_fun(img)``,
``process_image(draw)``, ``close()``, ``is_male()`` -- on libhsefr instead of ``tf.Session``.

Face *detection* is the step before the hot path: with ``mtcnn_detector=True`` the MTCNN
cascade of the reference's mtcnn.pb runs on the GPU (hse_facerec_tf_amd/mtcnn.py; facial_analysis.py:334-604);
any other detector (e.g. the OpenCV LBP cascade of :217-222) can be injected as a callable
``detector(img_rgb) -> (bounding_boxes, points)``.

Added for throughput: ``age_gender_batch`` -- all faces of a frame/album in ONE forward (the
reference runs one ``sess.run`` per face, facial_analysis.py:266-271).
"""
from __future__ import annotations

import os
import time
from typing import Callable, List, Optional, Sequence, Tuple

import numpy as np

from . import _lib, preprocess
from .engine import Engine
from .graphdef import read_graph
from .lowering import OUT_AGE, OUT_FEATURES, OUT_GENDER, lower_graph
from .tf_inference import AGE_GENDER_PB


def decode_age(age_preds: np.ndarray, min_age: int = 1):
    """facial_analysis.py:112-124: renormalised expectation over the two most probable age bins."""
    indices = age_preds.argsort()[::-1][:2]
    norm_preds = age_preds[indices] / np.sum(age_preds[indices])
    res_age = min_age
    for age, probab in zip(indices, norm_preds):
        res_age += age * probab
    return res_age, indices, norm_preds


class FacialImageProcessing:
    # minsize: minimum of faces' size
    def __init__(self, print_stat=False, mtcnn_detector=True, minsize=32, model_file: Optional[str] = None,
                 detector: Optional[Callable] = None, max_batch: int = 64, device: Optional[int] = None,
                 device_preprocess: bool = True, latency_plan: bool = True):
        # latency_plan: age_gender_fun / process_image -- the reference's one-face-per-run calls (:93-129, :225-294) -- run the
        # small-batch lowering of the graph (Engine.__init__: one face 0.17 instead of 0.26 ms on the device); age_gender_batch,
        # the bulk entry, keeps the one plan for every batch size unless asked (latency=True).  Results of the two plans differ in
        # the last bits (3e-7 relative; both are tested against the oracle at the same tolerance).
        self.latency_plan = bool(latency_plan)
        self.device_preprocess = device_preprocess
        self.mtcnn_detector = mtcnn_detector
        self.print_stat = print_stat
        self.minsize = minsize
        self.detector = detector
        if detector is None and mtcnn_detector:        # facial_analysis.py:59-61: the MTCNN cascade of mtcnn.pb
            from .mtcnn import MTCNNDetector
            self.detector = MTCNNDetector(minsize=minsize, device=device)
        # facial_analysis.py:45 loads a sibling .pb; the one that ships with the reference checkout is
        # the quantised age_gender_tf2_new-01-0.14-0.92 model.
        self.model_file = model_file or AGE_GENDER_PB
        self.age_gender_fun = self.load_age_gender(self.model_file, max_batch, device)

    def close(self):                          # facial_analysis.py:73-74
        self.sess.close()

    @staticmethod
    def is_male(gender_preds):                # facial_analysis.py:76-81, use_sota=False
        return (gender_preds >= 0.6)

    # ---- facial_analysis.py:83-130 -------------------------------------------------------------
    def load_age_gender(self, model_file, max_batch, device):
        graph = read_graph(model_file)
        outs = {OUT_AGE: 'age_pred/Softmax:0', OUT_GENDER: 'gender_pred/Sigmoid:0',
                OUT_FEATURES: 'global_pooling/Mean:0'}
        for t in outs.values():
            graph.get_tensor_by_name(t)       # KeyError like graph.get_tensor_by_name (:84-86)
        in_node, _ = graph.get_tensor_by_name('input_1:0')
        _, w, h, _ = graph.placeholder_shape(in_node.name)
        self.w, self.h = int(w), int(h)
        # the preprocessing of facial_analysis.py:95-107 (uint8 pixels minus the ImageNet-Caffe BGR mean) bounds the input: |x| < 256
        # ... and lets the engine take the RESIZED BYTES themselves (Engine.forward_u8): the float32 conversion, the channel
        # reversal and the float32 mean of :98-107 are folded into the first kernel's constants
        mean32 = tuple(float(np.float32(m)) for m in preprocess.IMAGENET_CAFFE_BGR_MEAN)
        self.plan = lower_graph(graph, 'input_1:0', outs, (self.w, self.h), input_bound=256.0, u8_mean_bgr=mean32)
        # age_gender_fun is called once per face (:93-129, process_image :225-294): few images per call run the small-batch
        # lowering of the same graph (Engine.__init__)
        small = (lower_graph(graph, 'input_1:0', outs, (self.w, self.h), input_bound=256.0, u8_mean_bgr=mean32, presplit="none")
                 if self.latency_plan else None)
        self.sess = Engine(self.plan, max_batch=max_batch, device=device, small_plan=small)

        def age_gender_fun(img):
            ages, genders, feats = self.age_gender_batch([img], latency=self.latency_plan)
            if self.print_stat:
                print('gender', genders[0])
                print('age', ages[0])
            return ages[0], genders[0], feats[0]
        return age_gender_fun

    def preprocess_face(self, img_rgb_u8: np.ndarray) -> np.ndarray:
        """facial_analysis.py:95-107: cv2.resize -> float32 -> BGR -> ImageNet-Caffe mean."""
        resized = preprocess.resize_linear_u8(img_rgb_u8, self.w, self.h)
        return preprocess.to_model_input(resized, True, True, dtype=np.float32)

    def age_gender_batch(self, faces_rgb_u8: Sequence[np.ndarray], latency: bool = False):
        """-> (ages [float], genders [ndarray[1]], features [ndarray[1024]]) for a list of face crops.
        latency: see Engine.forward (a frame's few faces: process_image and age_gender_fun pass it)."""
        torch = _lib.require_gpu()
        ages, genders, feats = [], [], []
        mb = self.sess.max_batch
        for i in range(0, len(faces_rgb_u8), mb):
            chunk = faces_rgb_u8[i:i + mb]
            if self.device_preprocess and self.sess.accepts_u8:      # cv2.resize on the GPU (integer: same bits), bytes into the net
                from . import preprocess_device
                x8 = preprocess_device.preprocess_faces_cv(chunk, (self.h, self.w), device=self.sess.device, raw_u8=True)
                a, g, fea = self._forward_u8_batch(x8, latency)
            else:
                if self.device_preprocess:  # cv2.resize + BGR + mean on the GPU
                    from . import preprocess_device
                    xd = preprocess_device.preprocess_faces_cv(chunk, (self.h, self.w), device=self.sess.device)
                else:
                    x = np.stack([self.preprocess_face(f) for f in chunk])
                    xd = torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).to(self.sess.device)
                a, g, fea = self._read_back(self.sess.forward(xd, (OUT_FEATURES, OUT_AGE, OUT_GENDER), latency=latency))
            ages.extend(a)
            genders.extend(g)
            feats.extend(fea)
        return ages, genders, feats

    @staticmethod
    def _read_back(r):
        """A forward's three outputs -> (ages, genders, features), a list entry per image: one read-back (three small device-to-host
        copies are three synchronisations), the ages decoded."""
        torch = _lib.require_gpu()
        packed = torch.cat([r["age_probs"], r["gender"], r["features"]], dim=1).cpu().numpy()
        na, ng = r["age_probs"].shape[1], r["gender"].shape[1]
        age_p, gen, fea = packed[:, :na], packed[:, na:na + ng].copy(), packed[:, na + ng:].copy()
        return [decode_age(p)[0] for p in age_p], list(gen), list(fea)

    # ---- facial_analysis.py:210-223 ---------------------------------------------------------------
    def detect_faces(self, img):
        if self.detector is None:
            raise NotImplementedError("no face detector configured: pass detector=callable(img_rgb) -> "
                                      "(bounding_boxes, points); the MTCNN cascade is the step before this path")
        return self.detector(img)

    def detect_faces_batch(self, imgs, max_frames: int = 32, mixed_sizes: bool = False):
        """detect_faces for a list of RGB frames -> [(bounding_boxes, points)] in list order: one call of the detector's
        ``detect_batch`` where it has one (MTCNNDetector: same-size frames share their launches, and with ``mixed_sizes`` the others
        share mixed-size passes), a loop over detect_faces otherwise."""
        batch = getattr(self.detector, "detect_batch", None)
        if batch is None:
            return [self.detect_faces(img) for img in imgs]       # (no detector at all: raises as detect_faces does)
        return batch(imgs, max_frames=max_frames, **self._mixed_kw(mixed_sizes))

    @staticmethod
    def _mixed_kw(mixed_sizes: bool) -> dict:
        """detect_batch's keyword, passed only when it is in use (a detector written without it keeps working)."""
        return dict(mixed_sizes=True) if mixed_sizes else {}

    @staticmethod
    def _packed_kw(mixed_device: bool) -> dict:
        """detect_batch's keyword of mixed_device, passed only when it is in use, as _mixed_kw's."""
        return dict(packed_sources=True) if mixed_device else {}

    # ---- facial_analysis.py:225-294 -----------------------------------------------------------------
    @staticmethod
    def face_boxes(bounding_boxes, img_w: int, img_h: int) -> List[List[int]]:
        """The per-bbox geometry of process_image: int cast, keep x2>x1 and y2>y1, pad 10 px,
        clip to the frame (:233-263)."""
        out = []
        for b in bounding_boxes:
            b = [int(bi) for bi in b]
            x1, y1, x2, y2 = b[0:4]
            if x2 > x1 and y2 > y1:
                dw, dh = 10, 10
                x1, x2 = x1 - dw, x2 + dw
                y1, y2 = y1 - dh, y2 + dh
                box = [x1, y1, x2, y2]
                if box[0] < 0:
                    box[0] = 0
                if box[2] > img_w:
                    box[2] = img_w
                if box[1] < 0:
                    box[1] = 0
                if box[3] > img_h:
                    box[3] = img_h
                out.append(box)
        return out

    @staticmethod
    def _bgr_to_rgb(draw) -> np.ndarray:
        draw = np.asarray(draw)
        # cv2.cvtColor(draw, COLOR_BGR2RGB): plane by plane (np.ascontiguousarray(draw[..., ::-1]) walks a 3-element inner loop with
        # a negative stride: 1.2 ms for a 784x588 frame, a quarter of this call, against 0.3 ms)
        img = np.empty(draw.shape, draw.dtype)
        img[..., 0], img[..., 1], img[..., 2] = draw[..., 2], draw[..., 1], draw[..., 0]
        return img

    def process_image(self, draw, bounding_boxes=None, points=None):
        """draw: BGR uint8 frame, as cv2.imread returns it (:225-226).  Detection runs unless
        ``bounding_boxes`` is supplied.  Returns (bboxes, points, ages, genders, facial_features)."""
        img = self._bgr_to_rgb(draw)
        t = time.time()
        if bounding_boxes is None:
            bounding_boxes, points = self.detect_faces(img)
        elapsed = time.time() - t
        if self.print_stat:
            print('detection elapsed', elapsed)
        img_h, img_w, _ = img.shape
        bboxes = self.face_boxes(bounding_boxes, img_w, img_h)
        crops = [img[y1:y2, x1:x2, :] for (x1, y1, x2, y2) in bboxes]
        t = time.time()
        ages, genders, facial_features = self.age_gender_batch(crops, latency=self.latency_plan) if crops else ([], [], [])
        if self.print_stat:
            print('age gender elapsed', time.time() - t)
        return bboxes, points if points is not None else [], ages, genders, facial_features

    def _forward_u8_batch(self, x8, latency: bool = False):
        """age_gender_batch's forward and read-back for resized faces that are already on the device: ``x8`` CUDA uint8 [m, h, w, 3]
        RGB, in chunks of max_batch (on the bulk plan unless ``latency``) -> (ages, genders, features)."""
        ages, genders, feats = [], [], []
        mb = self.sess.max_batch
        for i in range(0, int(x8.shape[0]), mb):
            a, g, fea = self._read_back(self.sess.forward_u8(x8[i:i + mb], (OUT_FEATURES, OUT_AGE, OUT_GENDER), latency=latency))
            ages.extend(a)
            genders.extend(g)
            feats.extend(fea)
        return ages, genders, feats

    def _resized_faces(self, imgs, all_bboxes, sources):
        """The resized faces of process_images on the device, CUDA uint8 [m, h, w, 3] RGB in list order.  The frames of a detector
        pass (``sources[i]`` = the pass's stack on the device and the frame's row in it) are cut from that stack by ONE launch per pass
        (preprocess_device.face_crops: one [m, 5] table uploaded, no frame and no crop uploaded again, no launch per crop size); the
        frames that took the single-frame call are cut on the host and resized by preprocess_faces_cv, as without device_crops.
        The frames of a mixed-size pass whose source is (PackedFrames, row) -- process_images(mixed_device=True) -- are cut the same
        way from that pass's packed buffer: preprocess_device.face_crops_from takes either kind of source."""
        from . import preprocess_device
        torch = _lib.require_gpu()
        counts = [len(b) for b in all_bboxes]
        starts = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
        x8 = torch.empty((int(starts[-1]), self.h, self.w, 3), dtype=torch.uint8, device=self.sess.device)
        passes, alone = {}, []                      # id(stack) -> (stack, [frame index]) in list order
        for i, src in enumerate(sources):
            if not counts[i]:
                continue
            if src is None:
                alone.append(i)
            else:
                passes.setdefault(id(src[0]), (src[0], []))[1].append(i)
        for source, idx in passes.values():
            table = np.array([[sources[i][1]] + list(box) for i in idx for box in all_bboxes[i]], dtype=np.int32)
            where = np.concatenate([np.arange(starts[i], starts[i + 1]) for i in idx])
            if where[-1] - where[0] + 1 == len(where):            # the pass's faces stand together in the batch: written in place
                preprocess_device.face_crops_from(source, table, (self.h, self.w), out=x8[int(where[0]):int(where[-1]) + 1])
            else:
                x8[torch.from_numpy(where).to(x8.device)] = preprocess_device.face_crops_from(source, table, (self.h, self.w))
        if alone:
            crops = [imgs[i][y1:y2, x1:x2, :] for i in alone for (x1, y1, x2, y2) in all_bboxes[i]]
            where = np.concatenate([np.arange(starts[i], starts[i + 1]) for i in alone])
            x8[torch.from_numpy(where).to(x8.device)] = preprocess_device.preprocess_faces_cv(crops, (self.h, self.w), device=self.sess.device,
                                                                                           raw_u8=True)
        return x8

    def device_frames_supported(self) -> bool:
        """process_images(device_frames=True)'s rule: the byte path (device_preprocess and an engine that accepts bytes) and a detector
        that can detect from a stack on the device -- it has ``detect_stack`` and keeps its box logic on the device (``device_boxes``:
        an MTCNNDetector without it has the method but no batched path to run it on)."""
        return bool(self.device_preprocess and self.sess.accepts_u8 and getattr(self.detector, "detect_stack", None) is not None
                    and getattr(self.detector, "device_boxes", False))

    def _detect_device_frames(self, draws, rotation: int, max_frames: int, mixed_sizes: bool = False, mixed_device: bool = False):
        """process_images' detection with device_frames: the frames grouped by their TURNED size (mtcnn.plan_passes); a group of two or
        more is stacked as decoded (BGR, unrotated), uploaded, turned and converted by ONE launch (preprocess_device.prepare_frames; in
        place for rotation 0, and a quarter turn's raw stack is dropped as soon as the prepared one is written) and detected from that
        stack (MTCNNDetector.detect_stack).  -> (imgs, shapes, detections, sources): ``sources`` as detect_batch(return_stacks=True)
        gives them; ``imgs[i]`` the frame's turned RGB host array where it took the single-frame call -- a frame alone in its size group
        (converted on the host, as without device_frames) and a frame whose candidate list overflowed (read back from its row of the
        prepared stack) -- and None for the others, whose pixels the host never touches; ``shapes[i]`` the turned (h, w).
        ``mixed_sizes``: the frames alone in their size group are converted on the host as before and then detected TOGETHER, in the
        detector's mixed-size passes (detect_batch(mixed_sizes=True)), instead of one by one.
        ``mixed_device`` (with ``mixed_sizes``): those frames get what the same-size groups get -- the passes are planned here
        (mtcnn.plan_mixed_passes over the TURNED shapes, the plan detect_batch makes), a pass's frames are concatenated as decoded,
        uploaded once, turned and converted by ONE launch (preprocess_device.prepare_packed; in place for rotation 0) and detected from
        that buffer (MTCNNDetector.detect_packed); ``sources[i]`` is (PackedFrames, row), ``imgs[i]`` stays None, and a frame that
        overflowed is read back from its range of the prepared buffer and redone alone."""
        from . import preprocess_device
        from .mtcnn import empty_detection, plan_mixed_passes, plan_passes
        from .mtcnn_ragged import PackedFrames
        torch = _lib.require_gpu()
        raw = []
        for d in draws:
            d = np.asarray(d)
            if d.ndim != 3 or d.shape[2] != 3 or d.dtype != np.uint8:
                raise ValueError("device_frames takes uint8 BGR frames [H, W, 3]")
            raw.append(d)
        shapes = [(d.shape[1], d.shape[0]) if rotation else (d.shape[0], d.shape[1]) for d in raw]
        imgs, detections, sources = [None] * len(raw), [None] * len(raw), [None] * len(raw)
        det = self.detector

        def alone(i, img):                         # the single-frame call, through the path a lone frame takes without device_frames
            imgs[i] = img
            detections[i] = det.detect_batch([img], max_frames=max_frames)[0]

        def host_rgb(i):                           # frame i turned and converted on the host, as without device_frames
            return self._bgr_to_rgb(preprocess_device.turn_frame(raw[i], rotation))

        def run_pass(idx, host, prepare, detect, frame_of):
            """One pass on the device.  ``host``: its frames as ONE array, as decoded; ``prepare(buf, out)``: that array on the device
            turned and converted by one launch into ``out`` -> the pass's source; ``detect(source)``: the detector's entry for such a
            source; ``frame_of(source, row)``: one frame of it."""
            buf = torch.from_numpy(host).to(det.device)                    # one upload per pass, as decoded
            source = prepare(buf, buf if rotation == 0 else None)          # in place for rotation 0: never a second buffer
            del buf                                                        # (a quarter turn's raw buffer is released here)
            for row, (i, res) in enumerate(zip(idx, detect(source))):
                if res is not None:
                    detections[i], sources[i] = res, (source, row)
                else:                                                      # overflowed: read back from the prepared buffer and redone alone
                    alone(i, frame_of(source, row).cpu().numpy())
        lone: list = []                            # mixed_sizes: the frames alone in their size group, in list order
        for (h, w), idx in plan_passes(shapes, max_frames):
            if not det.pyramid_scales(h, w):                               # smaller than minsize: no level, no launch, no upload
                for i in idx:
                    detections[i] = empty_detection()
            elif len(idx) > 1:
                run_pass(idx, np.stack([raw[i] for i in idx]), lambda buf, out: preprocess_device.prepare_frames(buf, rotation, True, out=out),
                         det.detect_stack, lambda stack, row: stack[row])
            elif not mixed_sizes:
                alone(idx[0], host_rgb(idx[0]))
            else:
                lone.append(idx[0])
                if not mixed_device:
                    imgs[idx[0]] = host_rgb(idx[0])
        if lone and mixed_device:
            for hw, part in plan_mixed_passes([shapes[i] for i in lone], max_frames, minsize=det.minsize, factor=det.FACTOR):
                idx = [lone[k] for k in part]
                if hw is not None:                                         # a pass of one: the single-frame call, converted on the host
                    for i in idx:
                        alone(i, host_rgb(i))
                    continue
                det.ragged_passes += 1
                det.ragged_frames += len(idx)
                raw_shapes, turned = [raw[i].shape[:2] for i in idx], [shapes[i] for i in idx]
                run_pass(idx, np.concatenate([np.ascontiguousarray(raw[i]).reshape(-1) for i in idx]),
                         lambda buf, out: PackedFrames(preprocess_device.prepare_packed(buf, raw_shapes, rotation, True, out=out), turned),
                         det.detect_packed, PackedFrames.frame)
        elif lone:
            for i, res in zip(lone, det.detect_batch([imgs[i] for i in lone], max_frames=max_frames, mixed_sizes=True)):
                detections[i] = res
        return imgs, shapes, detections, sources

    def process_images(self, draws, max_frames: int = 32, device_crops: bool = False, return_crops: bool = False, rotation: int = 0,
                       device_frames: bool = False, mixed_sizes: bool = False, mixed_device: bool = False):
        """process_image for a list of BGR uint8 frames (the photos of an album, the frames of a video: process_photos.py:92-118,
        :238-247) -> a list of process_image's 5-tuples, in list order.  One detect_faces_batch call over all frames, then ONE
        age_gender_batch call over the crops of all frames on the bulk plan (it chunks by max_batch itself), split back per frame.
        With latency_plan=False process_image runs the same plan and the results are equal bit for bit; the small-batch plan of
        latency_plan=True differs from them in the last bits (see __init__).
        device_crops: the faces are cut and resized on the device from the frame stacks the detector's passes uploaded (_resized_faces)
        instead of cut on the host and uploaded again grouped by size; the same bytes reach the net in the same batches, so the results
        are those of device_crops=False bit for bit.  Needs device_preprocess=True and an engine that takes bytes (ValueError otherwise,
        before any device work).
        return_crops: -> (that list, crops) with crops[i] the frame's resized faces, RGB uint8 [n_i, h, w, 3] (process_photos.py:38's
        facial_images up to channel order), read back in one copy.
        rotation: 0, 90 or 270 -- every frame of the call is turned by that many degrees clockwise first (process_photos.py:102-107,
        :242-247: the retry passes of an album, a video stored turned); boxes and points refer to the turned frame.
        device_frames: the frames are uploaded as decoded and turned and converted to RGB on the device, a pass in one launch
        (_detect_device_frames), instead of copied twice on the host; the detector and the crop kernel read that stack.  Implies
        device_crops and has its rule: ValueError without device_preprocess=True, an engine that accepts bytes and a detector with
        ``detect_stack``.  Results are those of device_frames=False bit for bit.
        mixed_sizes: the frames whose (turned) size no other frame of the call shares -- today one single-frame detector call each --
        are detected together in mixed-size passes (MTCNNDetector.detect_batch(mixed_sizes=True)); with device_frames they are converted
        on the host as before, and their faces are cut on the host, as for any frame without a source stack (mixed_device, below,
        moves both onto the device).  Same-size groups keep
        the device frames and the device crops.  Results are those of mixed_sizes=False bit for bit.  Needs a detector whose
        detect_batch takes the keyword.
        mixed_device (with mixed_sizes and one of device_crops / device_frames; ValueError otherwise, before any device work): the
        mixed-size passes get what the same-size passes get.  Under device_crops the faces of such a pass are cut by one launch from
        the buffer the pass uploaded (preprocess_device.face_crops_packed) and no crop is uploaded; under device_frames, additionally,
        the pass's frames are uploaded as decoded and turned and converted by one launch (preprocess_device.prepare_packed), and the
        host never touches their pixels.  Results are those of mixed_device=False bit for bit.  Needs an MTCNNDetector with
        device_boxes (``detect_packed``)."""
        from . import preprocess_device
        from .mtcnn import split_by_counts
        rotation = preprocess_device.check_rotation(rotation)
        byte_path = self.device_preprocess and self.sess.accepts_u8
        if mixed_device and not mixed_sizes:
            raise ValueError("mixed_device needs mixed_sizes=True (it moves the mixed-size passes' frames and crops onto the device)")
        if mixed_device and not (device_crops or device_frames):
            raise ValueError("mixed_device needs device_crops=True or device_frames=True")
        if device_frames and not self.device_frames_supported():
            raise ValueError("device_frames needs device_preprocess=True, an engine that accepts bytes and a detector with detect_stack "
                             "(an MTCNNDetector with device_boxes)")
        if device_crops and not byte_path:
            raise ValueError("device_crops needs device_preprocess=True and an engine that accepts bytes")
        if mixed_device and not (getattr(self.detector, "detect_packed", None) is not None and getattr(self.detector, "device_boxes", False)):
            raise ValueError("mixed_device needs a detector with detect_packed (an MTCNNDetector with device_boxes)")
        device_crops = bool(device_crops or device_frames)
        if not device_frames:
            imgs = [self._bgr_to_rgb(preprocess_device.turn_frame(np.asarray(d), rotation) if rotation else d) for d in draws]
            shapes = [img.shape[:2] for img in imgs]
        t = time.time()
        if device_frames:
            imgs, shapes, detections, sources = self._detect_device_frames(draws, rotation, max_frames, mixed_sizes, mixed_device)
        elif device_crops and getattr(self.detector, "detect_batch", None) is not None:
            # (a detector whose detect_batch cannot hand its stacks back raises here: device_crops was asked for)
            detections, sources = self.detector.detect_batch(imgs, max_frames=max_frames, return_stacks=True, **self._mixed_kw(mixed_sizes),
                                                                 **self._packed_kw(mixed_device))
        else:                                      # no batched detector: every frame takes the single-frame call and the host crops
            detections, sources = self.detect_faces_batch(imgs, max_frames=max_frames, mixed_sizes=mixed_sizes), [None] * len(imgs)
        if self.print_stat:
            print('detection elapsed', time.time() - t)
        all_bboxes, crops = [], []
        for img, (img_h, img_w), (bounding_boxes, _) in zip(imgs, shapes, detections):
            bboxes = self.face_boxes(bounding_boxes, img_w, img_h)
            all_bboxes.append(bboxes)
            if not device_crops:
                crops += [img[y1:y2, x1:x2, :] for (x1, y1, x2, y2) in bboxes]
        counts = [len(b) for b in all_bboxes]
        t = time.time()
        resized = None
        if sum(counts) == 0:
            ages, genders, features = [], [], []
        elif device_crops or (return_crops and byte_path):
            x8 = self._resized_faces(imgs, all_bboxes, sources)
            ages, genders, features = self._forward_u8_batch(x8)
            if return_crops:
                resized = x8.cpu().numpy()
        else:
            ages, genders, features = self.age_gender_batch(crops, latency=False)
        if self.print_stat:
            print('age gender elapsed', time.time() - t)
        out = [(bboxes, points if points is not None else [], a, g, f)
               for bboxes, (_, points), a, g, f in zip(all_bboxes, detections, split_by_counts(ages, counts), split_by_counts(genders, counts),
                                                       split_by_counts(features, counts))]
        if not return_crops:
            return out
        if resized is None:       # no faces at all, or a host-preprocess configuration: OpenCV's resize restated on the host
            resized = np.stack([preprocess.resize_linear_u8(c, self.w, self.h) for c in crops]) if crops else \
                np.empty((0, self.h, self.w, 3), np.uint8)
        at = np.concatenate([[0], np.cumsum(counts)])
        return out, [resized[at[i]:at[i + 1]] for i in range(len(counts))]
