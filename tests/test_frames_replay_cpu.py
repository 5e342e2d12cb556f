"""CPU suite: the index arithmetic of csrc/frames.hip replayed thread by thread on the host, on a flat byte array per stack -- every
12-byte access starts on a dword, no access leaves its stack, every destination byte is written exactly once, the result is NumPy's,
and the load phase's transposed LDS writes fall on 32 banks per half wave.  The replay restates the two kernels' loops (swap_kernel,
turn_kernel) and the launcher's choice of the vector and byte forms; its tile constants are read from the source, so a change there
must be made here too."""
import itertools
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SOURCE = open(os.path.join(ROOT, "hse_facerec_tf_amd", "csrc", "frames.hip")).read()
TILE = int(re.search(r"constexpr int TILE = (\d+);", SOURCE).group(1))
STRIDE = TILE + int(re.search(r"constexpr int TILE_STRIDE = TILE \+ (\d+);", SOURCE).group(1))
THREADS = int(re.search(r"constexpr int THREADS = (\d+);", SOURCE).group(1))
M24 = 0xffffff


class Mem:
    """A stack as flat bytes whose first byte stands at address ``base`` (mod 4)."""

    def __init__(self, arr, base):
        self.a, self.base = arr, base
        self.written = np.zeros(arr.size, np.int32)

    def load12(self, off):
        assert (self.base + off) % 4 == 0, "12-byte load off a dword"
        assert 0 <= off and off + 12 <= self.a.size, ("load outside the stack", off)
        b = [int(v) for v in self.a[off:off + 12]]
        return [b[4 * i] | b[4 * i + 1] << 8 | b[4 * i + 2] << 16 | b[4 * i + 3] << 24 for i in range(3)]

    def store12(self, off, words):
        assert (self.base + off) % 4 == 0, "12-byte store off a dword"
        assert 0 <= off and off + 12 <= self.a.size, ("store outside the stack", off)
        for i in range(3):
            for k in range(4):
                self.a[off + 4 * i + k] = (words[i] >> (8 * k)) & 255
        self.written[off:off + 12] += 1

    def load1(self, off):
        assert 0 <= off < self.a.size, ("load outside the stack", off)
        return int(self.a[off])

    def store1(self, off, v):
        assert 0 <= off < self.a.size, ("store outside the stack", off)
        self.a[off] = v
        self.written[off] += 1


def swap_02(p):
    return ((p & 0xff) << 16) | (p & 0xff00) | ((p >> 16) & 0xff)


def unpack4(v, swap):
    a, b, c = v
    p = [a & M24, ((a >> 24) | (b << 8)) & M24, ((b >> 16) | (c << 16)) & M24, c >> 8]
    return [swap_02(x) for x in p] if swap else p


def pack4(p0, p1, p2, p3):
    return [(p0 | (p1 << 24)) & 0xffffffff, ((p1 >> 8) | (p2 << 16)) & 0xffffffff, ((p2 >> 16) | (p3 << 8)) & 0xffffffff]


def load_pixel(m, off, swap):
    c0, c1, c2 = m.load1(off), m.load1(off + 1), m.load1(off + 2)
    return (c2 | c1 << 8 | c0 << 16) if swap else (c0 | c1 << 8 | c2 << 16)


def store_pixel(m, off, p):
    m.store1(off, p & 255)
    m.store1(off + 1, (p >> 8) & 255)
    m.store1(off + 2, (p >> 16) & 255)


def replay(x, rotation, swap, src_base=0, dst_base=0, grid_x_cap=3, grid_y_cap=65535, in_place=False):
    """hsefr_frames_prepare on the host -> the destination Mem.  ``grid_x_cap`` / ``grid_y_cap`` shrink the grid so that the strided
    loops over units and frames run more than once."""
    n, h, w, _ = x.shape
    fb = h * w * 3
    s = Mem(x.reshape(-1).copy(), src_base)
    d = s if in_place else Mem(np.full(n * fb, 0xEE, np.uint8), dst_base)
    src4, dst4 = src_base % 4 == 0, dst_base % 4 == 0
    gy = min(n, grid_y_cap)
    if rotation == 0:
        vec = src4 and dst4 and (h * w) % 4 == 0
        units = h * w // 4 if vec else h * w
        gx = min(-(-units // THREADS), grid_x_cap)
        for by, bx, t in itertools.product(range(gy), range(gx), range(THREADS)):
            for frame in range(by, n, gy):
                for u in range(bx * THREADS + t, units, gx * THREADS):
                    if vec:
                        at = frame * fb + u * 12
                        d.store12(at, pack4(*unpack4(s.load12(at), swap)))
                    else:
                        at = frame * fb + u * 3
                        store_pixel(d, at, load_pixel(s, at, swap))
        return d
    tiles_x, tiles_y = -(-w // TILE), -(-h // TILE)
    loadv, storev = src4 and w % 4 == 0, dst4 and h % 4 == 0
    ccw = rotation == 270
    for by, b in itertools.product(range(gy), range(tiles_x * tiles_y)):
        ty, tx = divmod(b, tiles_x)
        x0, y0 = tx * TILE, ty * TILE
        tw, th = min(TILE, w - x0), min(TILE, h - y0)
        for frame in range(by, n, gy):
            fo = frame * fb
            tile = [None] * (TILE * STRIDE)
            for t in range(THREADS):
                lane, wave = t & 63, t >> 6
                if loadv:
                    r = wave * 16 + (lane & 15)
                    for i in range(4):
                        c = (i * 4 + (lane >> 4)) * 4
                        if r < th and c < tw:
                            off = ((y0 + r) * w + x0 + c) * 3
                            assert off + 12 <= fb
                            p = unpack4(s.load12(fo + off), swap)
                            for k in range(4):
                                assert tile[(c + k) * STRIDE + r] is None
                                tile[(c + k) * STRIDE + r] = p[k]
                else:
                    for i in range(t, TILE * TILE, THREADS):
                        c, r = i & (TILE - 1), i // TILE
                        if r < th and c < tw:
                            off = ((y0 + r) * w + x0 + c) * 3
                            assert off + 3 <= fb
                            tile[c * STRIDE + r] = load_pixel(s, fo + off, swap)
            for t in range(THREADS):
                lane, wave = t & 63, t >> 6
                if storev:
                    q = (lane & 15) * 4
                    for i in range(4):
                        c = i * 16 + wave * 4 + (lane >> 4)
                        if c < tw and q < th:
                            assert (c * STRIDE + q) % 4 == 0                          # the ds_read_b128 is 16-byte aligned
                            v = tile[c * STRIDE + q:c * STRIDE + q + 4]
                            assert None not in v
                            if ccw:
                                off, words = ((w - 1 - x0 - c) * h + y0 + q) * 3, pack4(*v)
                            else:
                                off, words = ((x0 + c) * h + (h - 4 - y0 - q)) * 3, pack4(v[3], v[2], v[1], v[0])
                            assert 0 <= off and off + 12 <= fb
                            d.store12(fo + off, words)
                else:
                    for i in range(t, TILE * TILE, THREADS):
                        r, c = i & (TILE - 1), i // TILE
                        if c < tw and r < th:
                            row = (w - 1 - x0 - c) if ccw else x0 + c
                            col = (y0 + r) if ccw else h - 1 - y0 - r
                            off = (row * h + col) * 3
                            assert 0 <= off and off + 3 <= fb
                            store_pixel(d, fo + off, tile[c * STRIDE + r])
    return d


def expected(x, rotation, swap):
    want = np.rot90(x, {0: 0, 90: -1, 270: 1}[rotation], axes=(1, 2))
    return want[..., ::-1] if swap else want


def check(x, rotation, swap, src_base, dst_base, **kw):
    d = replay(x, rotation, swap, src_base, dst_base, **kw)
    case = (x.shape, rotation, swap, src_base, dst_base, kw)
    assert (d.written == 1).all(), ("a destination byte written %s times" % sorted(set(d.written.tolist())), case)
    want = expected(x, rotation, swap)
    assert np.array_equal(d.a.reshape(want.shape), want), case


def test_the_replay_reads_the_kernels_constants():
    assert (TILE, STRIDE, THREADS) == (64, 68, 256)
    for text in ("tile[(c + k) * TILE_STRIDE + r] = p[k]", "((y0 + r) * w + x0 + c) * 3", "((w - 1 - x0 - c) * h + y0 + q) * 3",
                 "((x0 + c) * h + (h - 4 - y0 - q)) * 3", "(row * h + col) * 3", "const int r = wave * 16 + (lane & 15);",
                 "const int c = (i * 4 + (lane >> 4)) * 4;", "const int c = i * 16 + wave * 4 + (lane >> 4);"):
        assert text in SOURCE, "csrc/frames.hip no longer holds `%s`: bring the replay in line with it" % text


def test_load_phase_lds_writes_fall_on_32_banks_per_half_wave():
    for i, k, half in itertools.product(range(4), range(4), range(2)):
        banks = set()
        for lane in range(32 * half, 32 * half + 32):
            r, c = lane & 15, (i * 4 + (lane >> 4)) * 4
            banks.add(((c + k) * STRIDE + r) % 32)
        assert len(banks) == 32, (i, k, half, sorted(banks))


# small shapes at every combination; the shapes with several tiles once per form (both vector, byte load, byte store, both byte)
SMALL = [(1, 1), (3, 5), (4, 8), (2, 70)]
LARGE = [(65, 63), (67, 130), (68, 132)]
ALIGNMENTS = [(0, 0), (0, 1), (1, 0), (2, 3)]


@pytest.mark.parametrize("hw", SMALL, ids=lambda hw: "%dx%d" % hw)
def test_replay_of_small_frames_at_every_rotation_alignment_and_grid(hw):
    rng = np.random.RandomState(hw[0] * 100 + hw[1])
    for n, rotation, swap, (sb, db) in itertools.product((1, 3), (0, 90, 270), (0, 1), ALIGNMENTS):
        x = rng.randint(0, 256, (n,) + hw + (3,)).astype(np.uint8)
        check(x, rotation, swap, sb, db)
        if n == 3:
            check(x, rotation, swap, sb, db, grid_y_cap=2)                             # a workgroup takes frames 0 and 2
        if rotation == 0 and sb == db:
            d = replay(x, 0, swap, sb, db, in_place=True)
            assert np.array_equal(d.a.reshape(x.shape), expected(x, 0, swap)), ("in place", hw, n, swap, sb)


@pytest.mark.parametrize("hw", LARGE, ids=lambda hw: "%dx%d" % hw)
def test_replay_of_frames_of_several_tiles(hw):
    rng = np.random.RandomState(hw[0] * 100 + hw[1])
    x = rng.randint(0, 256, (1,) + hw + (3,)).astype(np.uint8)
    for rotation, (sb, db) in itertools.product((90, 270), ALIGNMENTS):
        check(x, rotation, 1, sb, db)
    check(x, 0, 1, 0, 0, grid_x_cap=2)
    check(x, 0, 0, 1, 0, grid_x_cap=2)
