"""Seeded inputs for MTCNN's box logic, one stage at a time: what tests/test_mtcnn_stages_cpu.py feeds the product's host functions
and tests/test_mtcnn_stages_gpu.py feeds the kernels of csrc/mtcnn_post.hip, each against oracle.mtcnn's stage functions.

Everything is a pure function of ``cap`` (the capacity of a device list: hsefr_mtcnn_post_capacity() on the GPU side, NOMINAL_CAP
where no library is loaded) and of the case's name, which seeds its RandomState: both suites see the same arrays.  The names do
not depend on ``cap``, so a test can be parametrised by name before the capacity is known.

Layouts are the device's: a P-Net face map is prob [W', H'] float32 with reg [W', H', 4]; an R-/O-Net list is boxes_in [n, 5]
float64 (integer-valued corners), prob [n, 2], reg [n, 4], pts [n, 10], all float32.

The generator promises, and test_mtcnn_stages_cpu.py asserts on the oracle's output: every firing count and boundary listed
there is present, and every box a stage hands on overlaps the frame (crop row x1 <= x2, y1 <= y2): what the cascade does with a
box wholly outside the frame is the reference's own failure and not a case here.

ragged_net_cases / ragged_edge_frames are the lists of a launch over frames of DIFFERENT sizes (tests/test_mtcnn_ragged_stages_cpu.py
asserts what they promise, tests/test_mtcnn_ragged_stages_gpu.py feeds them to libhsefr_ragged.so).
"""
import zlib

import numpy as np

NOMINAL_CAP = 2048                       # the capacity the CPU suite generates for; the GPU suite passes the library's own
THR = (0.6, 0.7, 0.9)                    # MTCNNDetector.THRESHOLDS
PYRAMID = [12.0 / 32 * 0.709 ** k for k in range(9)]       # minsize 32: 12/minsize * 0.709^k
SCALES = PYRAMID + [0.5, 1.0]            # ... and two scales at which (2x + 1) / scale lands on integers
F32 = np.float32


def _rs(name):
    return np.random.RandomState(zlib.crc32(name.encode()))


def thr32(t):
    return F32(t)


def below(t):
    """The largest float32 below float32(t)."""
    return np.nextafter(F32(t), F32(0))


# ---------------------------------------------------------------------------------------------------------------------------
# stage-1 levels
# ---------------------------------------------------------------------------------------------------------------------------
def _cells_block(w, h, k):
    """k adjacent cells: the first k, row-major, of a compact block (neighbours overlap heavily)."""
    by = min(h, max(1, int(np.ceil(np.sqrt(max(k, 1))))))
    bx = int(np.ceil(k / by)) if k else 0
    assert bx <= w
    x0, y0 = (w - bx) // 2, (h - by) // 2
    idx = np.arange(k)
    return np.stack([x0 + idx // by, y0 + idx % by], axis=1).reshape(-1, 2)


def _cells_scattered(rs, w, h, k):
    idx = rs.permutation(w * h)[:k]
    return np.stack([idx // h, idx % h], axis=1).reshape(-1, 2)


def _cells_spaced(w, h, ox=0, oy=0, step=6):
    """Cells `step` apart in both axes: their boxes do not reach IoU 0.5, so every one survives the level's NMS."""
    xs, ys = np.arange(ox, w, step), np.arange(oy, h, step)
    return np.stack(np.meshgrid(xs, ys, indexing="ij"), axis=-1).reshape(-1, 2)


def _scores(rs, k, mode, thr):
    t = thr32(thr)
    s = np.maximum(rs.uniform(float(t), 1.0, k).astype(F32), t)
    if mode == "ones":                   # runs of bit-equal 1.0f (softmax saturated)
        for a in range(0, k, 9):
            s[a:a + 4] = F32(1.0)
    elif mode == "equal":
        s[:] = F32(0.8)
    else:
        assert mode == "random"
    return s


def _level(name, w, h, cells, scores, scale, thr=THR[0], rs=None):
    rs = rs or _rs(name)
    prob = rs.uniform(0.0, 0.5, (w, h)).astype(F32)           # below the threshold everywhere ...
    cells = np.asarray(cells, np.int64).reshape(-1, 2)
    prob[cells[:, 0], cells[:, 1]] = scores                  # ... then the chosen cells
    reg = (0.1 * rs.randn(w, h, 4)).astype(F32)              # differs per cell
    n_fire = int(np.count_nonzero(np.asarray(scores, F32) >= thr32(thr)))
    return dict(name=name, prob=prob, reg=reg, scale=float(scale), thr=float(thr), n_fire=n_fire, cells=cells)


def level_counts(cap):
    return [("0", 0), ("1", 1), ("2", 2), ("17", 17), ("1023", 1023), ("1024", 1024), ("1025", 1025),
            ("cap-1", cap - 1), ("cap", cap), ("cap+1", cap + 1)]


def level_cases(cap=NOMINAL_CAP):
    """-> list of dict(name, prob, reg, scale, thr, n_fire, cells).  A level with n_fire > cap must raise the overflow flag."""
    out = []
    long_side = 64
    short_side = (cap + 1 + long_side - 1) // long_side + 8         # a map that holds cap + 1 firing cells and some more
    for i, (label, k) in enumerate(level_counts(cap)):
        for geometry, (w, h) in (("clustered", (long_side, short_side)), ("scattered", (short_side, long_side))):
            name = "level/%s/%s" % (geometry, label)
            rs = _rs(name)
            cells = _cells_block(w, h, k) if geometry == "clustered" else _cells_scattered(rs, w, h, k)
            mode = ("random", "ones", "random")[i % 3] if geometry == "clustered" else ("ones", "random", "random")[i % 3]
            scale = SCALES[(2 * i + (geometry == "scattered")) % len(SCALES)]
            out.append(_level(name, w, h, cells, _scores(rs, k, mode, THR[0]), scale, rs=rs))
    # exactly one firing cell, off the centre column, on maps whose regression differs per cell: a missing flip changes the row
    out.append(_level("level/single/7x5", 7, 5, [[1, 3]], [F32(0.93)], PYRAMID[3]))
    out.append(_level("level/single/9x1", 9, 1, [[2, 0]], [F32(0.71)], 0.5))
    out.append(_level("level/single/1x9", 1, 9, [[0, 6]], [F32(0.88)], PYRAMID[1]))
    # degenerate maps
    for label, (w, h), k in (("1x9-all", (1, 9), 9), ("1x9-three", (1, 9), 3), ("9x1-all", (9, 1), 9), ("9x1-two", (9, 1), 2),
                             ("1x1-fires", (1, 1), 1), ("1x1-silent", (1, 1), 0)):
        name = "level/degenerate/" + label
        rs = _rs(name)
        out.append(_level(name, w, h, _cells_scattered(rs, w, h, k), _scores(rs, k, "random", THR[0]), SCALES[len(out) % len(SCALES)], rs=rs))
    # the threshold's edge: stage 1 fires on >=.  Cells far apart, so each one that fires is a row of the result
    t = thr32(THR[0])
    out.append(_level("level/threshold-edge", 30, 20, [[0, 0], [6, 6], [12, 12], [18, 18]], [F32(0.9), t, below(THR[0]), F32(0.75)], 1.0))
    out.append(_level("level/threshold-edge-pyramid", 30, 20, [[1, 2], [9, 8], [17, 14], [25, 2]], [t, F32(0.65), t, below(THR[0])], PYRAMID[0]))
    # every score equal: the order is the tie rule alone
    for label, (w, h), k, geo in (("17-scattered", (23, 31), 17, "scattered"), ("300-clustered", (40, 33), 300, "clustered"),
                                  ("1100-scattered", (50, 45), 1100, "scattered")):
        name = "level/all-equal/" + label
        rs = _rs(name)
        cells = _cells_block(w, h, k) if geo == "clustered" else _cells_scattered(rs, w, h, k)
        out.append(_level(name, w, h, cells, _scores(rs, k, "equal", THR[0]), SCALES[len(out) % len(SCALES)], rs=rs))
    # cells 6 apart: all 400 survive
    cells = _cells_spaced(120, 120)
    out.append(_level("level/spaced/120x120", 120, 120, cells, _scores(_rs("spaced"), len(cells), "ones", THR[0]), PYRAMID[0]))
    return out


# ---------------------------------------------------------------------------------------------------------------------------
# level sequences sharing one `counters` / `found`, finished by stage1_finish on their frame
# ---------------------------------------------------------------------------------------------------------------------------
def _map_dims(img_w, img_h, scale):
    """A face map whose boxes stay inside the frame's extent, as P-Net's map of that level does."""
    ws, hs = int(np.ceil(img_w * scale)), int(np.ceil(img_h * scale))
    return (ws - 12) // 2 + 1, (hs - 12) // 2 + 1


def sequence_cases(cap=NOMINAL_CAP):
    """-> list of dict(name, levels, img_w, img_h, overflow_at).  overflow_at: index of the level at which the survivors' total
    crosses cap (that call must raise the flag and leave everything else alone), or None."""
    img_w, img_h = 784, 588
    out = []
    # below the capacity: every kind of level in one frame, with 1.0f runs in several levels (ties across levels at the finish)
    name = "sequence/below-cap"
    rs = _rs(name)
    levels = []
    for j, (scale, kind) in enumerate(((PYRAMID[0], "spaced"), (PYRAMID[1], "clustered"), (PYRAMID[2], "silent"), (PYRAMID[3], "single"),
                                       (PYRAMID[4], "scattered"), (PYRAMID[0], "spaced-shifted"), (PYRAMID[5], "scattered"))):
        w, h = _map_dims(img_w, img_h, scale)
        cells = {"spaced": lambda: _cells_spaced(w, h), "spaced-shifted": lambda: _cells_spaced(w, h, 1, 0)[:min(300, cap // 8)],
                 "clustered": lambda: _cells_block(w, h, min(1025, cap // 2 + 1)), "silent": lambda: np.empty((0, 2), np.int64),
                 "single": lambda: np.asarray([[w // 4, h // 3]]), "scattered": lambda: _cells_scattered(rs, w, h, 17)}[kind]()
        if kind == "spaced":
            cells = cells[:min(len(cells), cap // 4)]
        levels.append(_level("%s/%d-%s" % (name, j, kind), w, h, cells, _scores(rs, len(cells), "ones", THR[0]), scale, rs=rs))
    out.append(dict(name=name, levels=levels, img_w=img_w, img_h=img_h, overflow_at=None))
    # the survivors' total lands on cap exactly (no overflow) / crosses it (overflow at the crossing level)
    for label, exact in (("exactly-cap", True), ("crosses-cap", False)):
        name = "sequence/" + label
        rs = _rs(name)
        levels, total, j = [], 0, 0
        while total <= cap and not (exact and total == cap):
            scale = (PYRAMID[0], 0.5)[j % 2]
            w, h = _map_dims(img_w, img_h, scale)
            cells = _cells_spaced(w, h, j % 6, (j // 2) % 6)
            if exact:
                cells = cells[:cap - total]
            total += len(cells)
            levels.append(_level("%s/%d" % (name, j), w, h, cells, _scores(rs, len(cells), "ones" if j % 2 else "random", THR[0]), scale, rs=rs))
            j += 1
        out.append(dict(name=name, levels=levels, img_w=img_w, img_h=img_h, overflow_at=None if exact else len(levels) - 1))
    return out


# ---------------------------------------------------------------------------------------------------------------------------
# boxes that clip: one list per frame, squares (so squaring leaves them alone) to be fed with zero regressions
# ---------------------------------------------------------------------------------------------------------------------------
def _edge_corners(w, h):
    """The eight boxes of edge_boxes()'s first list, placed against the edges of a w x h frame (at least 90 x 70): left, top, right,
    bottom, three corners and one inside.  Every box overlaps the frame."""
    assert w >= 90 and h >= 70
    mx, my = w // 2 - 20, h // 2 - 20
    return np.asarray([[-10, my, 29, my + 39],                # left
                       [mx, -5, mx + 29, 24],                 # top
                       [w - 20, my, w + 19, my + 39],         # right
                       [mx, h - 20, mx + 39, h + 19],         # bottom
                       [-8, -8, 21, 21],                      # corner: left + top
                       [w - 15, h - 15, w + 24, h + 24],      # corner: right + bottom
                       [w - 50, -12, w + 39, 77],             # corner: right + top (the bottom too where h < 77)
                       [mx, my, mx + 29, my + 29]], np.float64)   # inside


def edge_boxes(size=None):
    """-> list of (label, img_w, img_h, corners [n, 4]): boxes over each edge, two opposite edges at once, and corners.
    ``size`` = (img_w, img_h): one list of eight boxes placed against the edges of a frame of that size instead."""
    if size is not None:
        w, h = size
        return [("%dx%d" % (w, h), w, h, _edge_corners(w, h))]
    wide = [[-10, 60, 29, 99],           # left
            [80, -5, 109, 24],           # top
            [180, 60, 219, 99],          # right
            [80, 130, 119, 169],         # bottom
            [-8, -8, 21, 21],            # corner: left + top
            [185, 135, 224, 174],        # corner: right + bottom
            [150, -12, 239, 77],         # corner: right + top
            [60, 60, 89, 89]]            # inside
    return [("200x150", 200, 150, np.asarray(wide, np.float64)),
            ("40x200", 40, 200, np.asarray([[-10, 50, 69, 129], [5, 150, 34, 179]], np.float64)),        # left + right at once
            ("200x40", 200, 40, np.asarray([[50, -20, 129, 59], [150, 5, 179, 34]], np.float64)),        # top + bottom at once
            ("30x30", 30, 30, np.asarray([[-15, -15, 44, 44]], np.float64))]                            # larger than the frame


def clip_sides(boxes, img_w, img_h):
    """Per box: the frozenset of frame edges it crosses, from 'L', 'T', 'R', 'B'."""
    b = np.asarray(boxes, np.float64)
    flags = np.stack([b[:, 0] < 1, b[:, 1] < 1, b[:, 2] > img_w, b[:, 3] > img_h], axis=1)
    return [frozenset(s for s, f in zip("LTRB", row) if f) for row in flags]


REQUIRED_CLIPS = [frozenset("L"), frozenset("T"), frozenset("R"), frozenset("B"), frozenset("LR"), frozenset("TB"), frozenset("LT"),
                  frozenset("RB"), frozenset("LTRB")]


def _clustered_squares(rs, n, img_w, img_h, x_hi=None):
    """Integer-valued square boxes in clusters of near-duplicates, every fourth nested in its predecessor (same centre, a
    fraction of the side): intersection / smaller area ('Min') and IoU disagree on those."""
    x_hi = img_w - 20 if x_hi is None else x_hi
    n_clusters = max(1, n // 12)
    ccx, ccy = rs.uniform(20, x_hi, n_clusters), rs.uniform(20, img_h - 20, n_clusters)
    which = rs.randint(0, n_clusters, n)
    cx = ccx[which] + rs.uniform(-6, 6, n)
    cy = ccy[which] + rs.uniform(-6, 6, n)
    side = rs.choice([24, 31, 40, 56, 64, 90, 120], n).astype(np.float64)
    for i in range(3, n, 4):
        cx[i], cy[i], side[i] = cx[i - 1], cy[i - 1], np.floor(side[i - 1] * rs.choice([0.5, 0.8]))
    x1, y1 = np.fix(cx - side / 2), np.fix(cy - side / 2)
    return np.stack([x1, y1, x1 + side - 1, y1 + side - 1], axis=1)


# ---------------------------------------------------------------------------------------------------------------------------
# stage-1 finish on synthetic lists (the lists that come from levels are sequence_cases)
# ---------------------------------------------------------------------------------------------------------------------------
def finish_cases(cap=NOMINAL_CAP):
    """-> list of dict(name, found [n, 9] float64, img_w, img_h, crops).  crops: also cut crops from the device's table."""
    out = []
    for label, n in (("1", 1), ("2", 2), ("300", 300), ("cap", cap)):
        name = "finish/clustered/" + label
        rs = _rs(name)
        img_w, img_h = 320, 240
        score = _scores(rs, n, "ones" if n > 2 else "random", THR[0])
        if n > 20:
            score[5::11] = score[2]                                  # more ties, not at 1.0f
        reg = (0.1 * rs.randn(n, 4)).astype(F32)
        found = np.hstack([_clustered_squares(rs, n, img_w, img_h), score[:, None].astype(np.float64), reg.astype(np.float64)])
        out.append(dict(name=name, found=found, img_w=img_w, img_h=img_h, crops=n <= 2))
    for label, img_w, img_h, corners in edge_boxes():
        name = "finish/edges/" + label
        n = corners.shape[0]
        score = np.linspace(0.95, 0.65, n).astype(F32)
        found = np.hstack([corners, score[:, None].astype(np.float64), np.zeros((n, 4))])
        out.append(dict(name=name, found=found, img_w=img_w, img_h=img_h, crops=True))
    return out


# ---------------------------------------------------------------------------------------------------------------------------
# stages 2 and 3
# ---------------------------------------------------------------------------------------------------------------------------
ISOLATED = np.asarray([282.0, 202.0, 311.0, 231.0])     # a box no cluster reaches (cluster centres stay left of x = 200)


def _net_list(name, stage, n, mode, img_w=320, img_h=240, x_hi=200, isolated=ISOLATED):
    """``x_hi``: the cluster centres' right end (they start 20 px inside the frame on the other three sides); ``isolated``: the box of
    the at-threshold mode, which no cluster may reach.  The defaults are fitted to 320 x 240."""
    rs = _rs(name)
    thr = THR[stage - 1]
    t = thr32(thr)
    corners = _clustered_squares(rs, n, img_w, img_h, x_hi=x_hi)
    score = rs.uniform(float(t) - 0.25, 1.0, n).astype(F32)
    if n > 4:
        score[1::5] = F32(1.0)                                       # saturated softmax: ties
    at_thr = None
    if mode == "at-threshold":                                       # stages 2 and 3 pass on >: this one must not
        at_thr = 5
        corners[at_thr] = isolated
        score[at_thr] = t
    elif mode == "none-pass":
        score = np.minimum(score, t)
        score[0] = t
    elif mode == "all-tied":
        score[:] = F32(0.95)
    else:
        assert mode == "random"
    boxes_in = np.hstack([corners, rs.uniform(0.6, 1.0, (n, 1)).astype(F32).astype(np.float64)])   # column 4: the previous stage's score, unused
    prob = np.stack([F32(1) - score, score], axis=1).astype(F32)
    reg = (0.1 * rs.randn(n, 4)).astype(F32)
    pts = rs.uniform(0.0, 1.0, (n, 10)).astype(F32)
    return dict(name=name, stage=stage, boxes_in=boxes_in, prob=prob, reg=reg, pts=pts, thr=float(thr), img_w=img_w, img_h=img_h,
                at_thr=at_thr, crops=False)


def net_counts(cap):
    return [("0", 0), ("1", 1), ("5", 5), ("16", 16), ("17", 17), ("700", 700), ("cap", cap), ("cap+1", cap + 1)]


def net_cases(stage, cap=NOMINAL_CAP):
    """-> list of dict(name, stage, boxes_in, prob, reg, pts, thr, img_w, img_h, at_thr, crops).  A list longer than cap must
    raise the overflow flag and write count 0."""
    assert stage in (2, 3)
    out = []
    for label, n in net_counts(cap):
        c = _net_list("stage%d/random/%s" % (stage, label), stage, n, "random")
        c["crops"] = stage == 2 and 5 <= n <= 17
        out.append(c)
    out.append(_net_list("stage%d/at-threshold/17" % stage, stage, 17, "at-threshold"))
    out.append(_net_list("stage%d/none-pass/16" % stage, stage, 16, "none-pass"))
    out.append(_net_list("stage%d/all-tied/300" % stage, stage, 300, "all-tied"))
    out.append(_net_list("stage%d/all-tied/1500" % stage, stage, min(1500, cap), "all-tied"))
    if stage == 2:
        for label, img_w, img_h, corners in edge_boxes():
            n = corners.shape[0]
            c = _net_list("stage2/edges/" + label, 2, n, "random", img_w, img_h)
            c["boxes_in"][:, 0:4] = corners
            c["prob"][:, 1] = np.linspace(0.99, 0.75, n).astype(F32)
            c["prob"][:, 0] = F32(1) - c["prob"][:, 1]
            c["reg"][:] = 0
            c["crops"] = True
            out.append(c)
    return out


# frames of different sizes in one launch (tests/test_mtcnn_ragged_stages_*.py): (img_w, img_h) per frame, the counts of
# test_mtcnn_batch_stages_gpu.NET_LABELS.  Small frames hold the long lists, so that boxes leave them over every edge and pair of
# edges; 160 x 100 and 100 x 160 have one area; 251 * 187 * 3 is odd; 784 x 588 holds the at-threshold list with its isolated box.
RAGGED_SIZES = [(100, 160), (200, 150), (90, 70), (640, 480), (251, 187), (160, 100), (784, 588)]
RAGGED_LABELS = ["700", "0", "5", "cap+1", "1", "cap", "17"]


def ragged_net_cases(stage, cap=NOMINAL_CAP):
    """-> seven cases as net_cases gives them, one per frame of a mixed-size launch, every frame of another size.  Cluster centres lie
    at least 20 px inside their frame, so every box overlaps it."""
    assert stage in (2, 3)
    counts = dict(net_counts(cap))
    out = []
    for b, ((img_w, img_h), label) in enumerate(zip(RAGGED_SIZES, RAGGED_LABELS)):
        name = "stage%d/ragged/%d-%dx%d/%s" % (stage, b, img_w, img_h, label)
        if label == "17":           # clusters in the left 60 % of the frame, the isolated box in its bottom right corner
            c = _net_list(name, stage, 17, "at-threshold", img_w, img_h, x_hi=int(0.6 * img_w),
                          isolated=np.asarray([img_w - 38.0, img_h - 38.0, img_w - 9.0, img_h - 9.0]))
        else:
            c = _net_list(name, stage, counts[label], "random", img_w, img_h, x_hi=img_w - 20)
        out.append(c)
    return out


def ragged_edge_frames():
    """-> three lists of edge boxes on frames of three sizes: edge_boxes()'s 200 x 150, 251 x 187 (an odd number of bytes: the next
    frame of a packed buffer starts on an odd address) and the portrait 120 x 160."""
    return [edge_boxes()[0], edge_boxes((251, 187))[0], edge_boxes((120, 160))[0]]


def names(cases):
    return [c["name"] for c in cases]


def by_name(cases):
    d = {c["name"]: c for c in cases}
    assert len(d) == len(cases)
    return d
