"""CPU suite: the bookkeeping of the batched detection entry points, without a GPU -- how MTCNNDetector.detect_batch groups frames by
size, cuts a group into passes and puts the results back in list order (plan_passes, and detect_batch itself over a detector whose
device pass is faked), and how FacialImageProcessing.process_images splits the one age/gender list back per frame (split_by_counts)."""
import numpy as np
import pytest

from hse_facerec_tf_amd.mtcnn import MTCNNDetector, empty_detection, plan_passes, split_by_counts


def test_plan_passes_groups_by_size_and_chunks_in_list_order():
    shapes = [(588, 784), (480, 600), (588, 784), (20, 500), (588, 784), (480, 600), (588, 784)]
    assert plan_passes(shapes, 32) == [((588, 784), [0, 2, 4, 6]), ((480, 600), [1, 5]), ((20, 500), [3])]
    assert plan_passes(shapes, 3) == [((588, 784), [0, 2, 4]), ((588, 784), [6]), ((480, 600), [1, 5]), ((20, 500), [3])]
    assert plan_passes(shapes, 1) == [((588, 784), [0]), ((588, 784), [2]), ((588, 784), [4]), ((588, 784), [6]), ((480, 600), [1]),
                                      ((480, 600), [5]), ((20, 500), [3])]
    assert plan_passes([], 8) == []
    # (h, w) and (w, h) are different sizes; NumPy integers are as good as ints
    assert plan_passes([(np.int64(10), 20), (20, 10), (10, np.int32(20))], 8) == [((10, 20), [0, 2]), ((20, 10), [1])]


@pytest.mark.parametrize("n, max_frames", [(1, 1), (7, 3), (8, 8), (9, 8), (65, 32), (5, 100)])
def test_plan_passes_covers_every_frame_once(n, max_frames):
    rs = np.random.RandomState(n * 100 + max_frames)
    shapes = [(int(rs.choice([90, 588])), int(rs.choice([200, 784]))) for _ in range(n)]
    passes = plan_passes(shapes, max_frames)
    seen = [i for _, idx in passes for i in idx]
    assert sorted(seen) == list(range(n))
    for hw, idx in passes:
        assert 1 <= len(idx) <= max_frames and idx == sorted(idx) and all(shapes[i] == hw for i in idx)


@pytest.mark.parametrize("bad", [0, -1])
def test_plan_passes_refuses_an_empty_pass(bad):
    with pytest.raises(ValueError):
        plan_passes([(10, 10)], bad)


def test_split_by_counts():
    assert split_by_counts(list("abcdef"), [2, 0, 3, 1]) == [["a", "b"], [], ["c", "d", "e"], ["f"]]
    assert split_by_counts([], [0, 0]) == [[], []]
    assert split_by_counts([], []) == []
    for items, counts in ((list("abc"), [1, 1]), (list("ab"), [3]), ([], [1])):
        with pytest.raises(ValueError):
            split_by_counts(items, counts)


class FakeDetector(MTCNNDetector):
    """detect_batch over a device pass that only records what it was given.  A frame's first byte is its identity: the 'detection' of
    frame v is v % 4 boxes whose scores are v; a frame whose second byte is 255 'overflows'."""

    def __init__(self, device_boxes=True):
        self.minsize, self.device_resize, self.device_boxes, self.host_fallbacks = 32, True, device_boxes, 0
        self.passes, self.alone = [], []

    @staticmethod
    def result(img):
        v = int(img[0, 0, 0])
        return np.full((v % 4, 5), float(v)), np.full((10, v % 4), np.float32(v)) if v % 4 else np.array([])

    def _detect_pass(self, imgs):
        assert len({f.shape for f in imgs}) == 1
        self.passes.append([int(f[0, 0, 0]) for f in imgs])
        return [None if f[0, 0, 1] == 255 else (self.result(f) if f[0, 0, 0] % 4 else empty_detection()) for f in imgs]

    def __call__(self, img):
        self.alone.append(int(img[0, 0, 0]))
        return self.result(img)


def frame(v, h=64, w=48, overflow=False):
    f = np.zeros((h, w, 3), np.uint8)
    f[0, 0, 0] = v
    f[0, 0, 1] = 255 if overflow else 0
    return f


def check(results, values):
    assert len(results) == len(values)
    for (boxes, points), v in zip(results, values):
        assert boxes.shape == (v % 4, 5) and points.shape == (10, v % 4) and boxes.dtype == np.float64 and points.dtype == np.float32
        assert np.all(boxes == v) and np.all(points == v)


def test_detect_batch_restores_list_order_over_sizes_and_passes():
    det = FakeDetector()
    values = [5, 6, 7, 8, 9, 10, 11, 13]
    sizes = [(64, 48), (40, 90), (64, 48), (64, 48), (40, 90), (64, 48), (20, 500), (64, 48)]       # 20 x 500: below minsize, no level
    frames = [frame(v, h, w) for v, (h, w) in zip(values, sizes)]
    got = det.detect_batch(frames, max_frames=2)
    assert det.passes == [[5, 7], [8, 10], [6, 9]] and det.alone == [13]                           # a pass of one frame: the single-frame call
    check(got[:6] + got[7:], values[:6] + values[7:])
    assert got[6][0].shape == (0, 5) and got[6][1].shape == (10, 0)                                # no launch for that one
    det = FakeDetector()
    check(det.detect_batch(frames[:6], max_frames=32), values[:6])
    assert det.passes == [[5, 7, 8, 10], [6, 9]] and det.alone == []
    det = FakeDetector()
    check(det.detect_batch(frames[:6], max_frames=1), values[:6])
    assert det.passes == [] and det.alone == [5, 7, 8, 10, 6, 9]


def test_an_overflowed_frame_alone_is_redone():
    det = FakeDetector()
    frames = [frame(1), frame(2, overflow=True), frame(3), frame(4, overflow=True)]
    check(det.detect_batch(frames), [1, 2, 3, 4])
    assert det.passes == [[1, 2, 3, 4]] and det.alone == [2, 4]      # frame 4 has no box: its redo's empty shapes are made the batch's


def test_a_detector_without_device_boxes_loops_over_call():
    det = FakeDetector(device_boxes=False)
    check(det.detect_batch([frame(3), frame(4), frame(1, 40, 90)]), [3, 4, 1])
    assert det.passes == [] and det.alone == [3, 4, 1]


def test_argument_errors_come_before_any_pass():
    det = FakeDetector()
    good = frame(1)
    for bad, kw in (([good, good.astype(np.float32)], {}), ([good, good[:, :, 0]], {}), ([good, good[:, :, :2]], {}), ([good], dict(max_frames=0))):
        with pytest.raises(ValueError):
            det.detect_batch(bad, **kw)
    assert det.passes == [] and det.alone == []
    assert det.detect_batch([]) == []


def test_an_overflowed_pass_of_one_falls_back_to_the_host_cascade():
    """The single-frame call is a pass of one frame: where that pass reports an overflow (None), __call__ counts a host fallback and
    runs the host cascade on the same upload.  Faked one level below FakeDetector: the pass body and the host stage 1."""
    import torch

    class Overflowing(MTCNNDetector):
        def __init__(self):
            self.minsize, self.device_resize, self.device_boxes, self.host_fallbacks = 32, True, True, 0
            self._torch, self.device = torch, torch.device("cpu")
            self.passes, self.host = [], []

        def _detect_stack_body(self, stack, counts=None):
            self.passes.append(tuple(stack.shape))
            return [None]

        def _stage1(self, img, frame=None):
            self.host.append((img.shape, tuple(frame.shape)))
            return np.empty((0, 9))                                        # the host cascade ends here: no candidates

    det = Overflowing()
    boxes, points = det(frame(7))
    assert det.passes == [(1, 64, 48, 3)] and det.host == [((64, 48, 3), (64, 48, 3))] and det.host_fallbacks == 1
    assert boxes.shape == (0, 9) and points.shape == (0,)
    det(frame(8, 40, 90))
    assert det.passes[1:] == [(1, 40, 90, 3)] and len(det.host) == 2 and det.host_fallbacks == 2
    with pytest.raises(ValueError):                                        # the frame check comes before the pass
        det(frame(1).astype(np.float32))
    assert len(det.passes) == 2
