"""CPU suite: what makes tests/test_mtcnn_ragged_stages_gpu.py discriminating, asserted from the oracle alone (oracle.mtcnn) on the cases
of mtcnn_stage_cases.ragged_net_cases / ragged_edge_frames: a kernel that took another frame's size, or another frame's table row,
would give other bytes on these inputs.  Also that the generator's new parameters left the 320 x 240 lists as they were."""
import zlib

import numpy as np
import pytest

from oracle import mtcnn as om

import mtcnn_stage_cases as gen

CAP = gen.NOMINAL_CAP
RAGGED = {2: gen.ragged_net_cases(2, CAP), 3: gen.ragged_net_cases(3, CAP)}


def overlaps_frame(tab):
    return bool(np.all(tab[:, 0] <= tab[:, 2]) and np.all(tab[:, 1] <= tab[:, 3]))


def stage2(c, size=None):
    w, h = size or (c["img_w"], c["img_h"])
    return om.stage2_finish(c["boxes_in"], c["prob"], c["reg"], c["thr"], w, h)


def test_seven_frames_of_seven_sizes_with_the_batch_tests_counts():
    sizes = gen.RAGGED_SIZES
    assert len(sizes) == 7 and len(set(sizes)) == 7
    assert any(w > h and (h, w) in sizes for w, h in sizes)                              # a landscape and a portrait frame of one area
    assert any(w < 100 and h < 100 for w, h in sizes) and (784, 588) in sizes
    for stage in (2, 3):
        cs = RAGGED[stage]
        assert [c["boxes_in"].shape[0] for c in cs] == [700, 0, 5, CAP + 1, 1, CAP, 17]
        assert [(c["img_w"], c["img_h"]) for c in cs] == sizes and len(set(gen.names(cs))) == 7
        for c in cs:
            assert np.array_equal(c["boxes_in"][:, 0:4], np.fix(c["boxes_in"][:, 0:4]))
            assert c["prob"].dtype == c["reg"].dtype == c["pts"].dtype == np.float32
            # every box at least partly inside its frame: what the oracle's pad() is defined for
            b = c["boxes_in"]
            assert np.all(b[:, 2] >= 1) and np.all(b[:, 3] >= 1) and np.all(b[:, 0] <= c["img_w"]) and np.all(b[:, 1] <= c["img_h"]), c["name"]
        for cap in (1500, 4096):
            other = gen.ragged_net_cases(stage, cap)
            assert gen.names(other) == gen.names(cs) and [c["boxes_in"].shape[0] for c in other] == [700, 0, 5, cap + 1, 1, cap, 17]


def test_the_new_parameters_leave_the_320_x_240_lists_as_they_were():
    """crc32 of the arrays of four lists, taken before the generator got its parameters."""
    got = {}
    for stage in (2, 3):
        for c in gen.net_cases(stage, CAP):
            if c["name"] in PINNED:
                crc = 0
                for k in ("boxes_in", "prob", "reg", "pts"):
                    crc = zlib.crc32(np.ascontiguousarray(c[k]).tobytes(), crc)
                got[c["name"]] = crc
    assert got == PINNED, got
    # the default of edge_boxes is its four lists; a size gives one list of eight boxes, each overlapping the frame
    assert [l for l, _, _, _ in gen.edge_boxes()] == ["200x150", "40x200", "200x40", "30x30"]
    assert zlib.crc32(np.concatenate([c.reshape(-1) for _, _, _, c in gen.edge_boxes()]).tobytes()) == EDGE_CRC


PINNED = {"stage2/random/17": 3273490354, "stage2/at-threshold/17": 417303161, "stage3/random/700": 2588393927, "stage3/all-tied/300": 2993030344}
EDGE_CRC = 1308352697


def test_stage2_with_another_frames_size_gives_another_crop_table():
    """What a wrong frame_tab row would produce.  For at least three of the frames with a result, EVERY other size of the launch
    changes the crop table -- frame 0's among them, which a kernel reading row 0 for every frame would use."""
    cs = RAGGED[2]
    live = [b for b, c in enumerate(cs) if 0 < c["boxes_in"].shape[0] <= CAP]
    assert live == [0, 2, 4, 5, 6]
    own = {b: stage2(cs[b]) for b in live}
    for b in live:
        assert overlaps_frame(own[b][1]), cs[b]["name"]
    print({b: own[b][0].shape[0] for b in live})
    assert sum(own[b][0].shape[0] > 0 for b in live) >= 4                                 # (the list of one box may lose it to the threshold)
    differs = {b: [not np.array_equal(stage2(cs[b], gen.RAGGED_SIZES[o])[1], own[b][1]) for o in range(7) if o != b] for b in live}
    print({b: sum(v) for b, v in differs.items()})
    assert sum(all(v) for v in differs.values()) >= 3, differs
    with_frame_0 = [b for b in live if b != 0 and not np.array_equal(stage2(cs[b], gen.RAGGED_SIZES[0])[1], own[b][1])]
    assert len(with_frame_0) >= 3, with_frame_0
    # the boxes themselves do not depend on the size: only the table shows it
    for b in live:
        assert np.array_equal(stage2(cs[b], gen.RAGGED_SIZES[(b + 1) % 7])[0], own[b][0])


def test_the_seven_frames_results_cross_every_edge_and_pair_of_edges():
    seen = set()
    for c in RAGGED[2]:
        if 0 < c["boxes_in"].shape[0] <= CAP:
            boxes, tab = stage2(c)
            seen |= set(gen.clip_sides(boxes, c["img_w"], c["img_h"]))
    assert set(gen.REQUIRED_CLIPS) <= seen, set(gen.REQUIRED_CLIPS) - seen


def test_the_at_threshold_list_keeps_its_meaning_on_its_own_frame():
    for stage in (2, 3):
        c = RAGGED[stage][6]
        k, thr = c["at_thr"], gen.thr32(c["thr"])
        assert k is not None and c["prob"][k, 1] == thr and c["boxes_in"][k, 2] <= c["img_w"] and c["boxes_in"][k, 3] <= c["img_h"]
        up = c["prob"].copy()
        up[k, 1] = np.nextafter(thr, np.float32(1))
        if stage == 2:
            at, above = stage2(c)[0], om.stage2_finish(c["boxes_in"], up, c["reg"], c["thr"], c["img_w"], c["img_h"])[0]
        else:
            at = om.stage3_finish(c["boxes_in"], c["prob"], c["reg"], c["pts"], c["thr"])[0]
            above = om.stage3_finish(c["boxes_in"], up, c["reg"], c["pts"], c["thr"])[0]
        assert above.shape[0] == at.shape[0] + 1 and at.shape[0] > 0


def test_edge_lists_exist_for_three_sizes_one_of_an_odd_number_of_bytes():
    frames = gen.ragged_edge_frames()
    assert len({(w, h) for _, w, h, _ in frames}) >= 3
    assert any((w * h * 3) % 2 == 1 for _, w, h, _ in frames)
    assert frames[0][1:3] == (200, 150) and np.array_equal(frames[0][3], gen.edge_boxes()[0][3])
    for label, w, h, corners in frames:
        assert corners.shape == (8, 4) and np.array_equal(corners, np.fix(corners))
        tab = om.crop_table(corners, w, h)
        assert overlaps_frame(tab), label
        assert {frozenset("L"), frozenset("T"), frozenset("R"), frozenset("B"), frozenset("LT"), frozenset("RB"), frozenset()} \
            <= set(gen.clip_sides(corners, w, h)), label
        # the windows differ from frame to frame: a crop cut with another frame's table, or from another frame, is another crop
    tabs = [om.crop_table(c, w, h) for _, w, h, c in frames]
    assert not np.array_equal(tabs[0], tabs[1]) and not np.array_equal(tabs[1], tabs[2]) and not np.array_equal(tabs[0], tabs[2])
    with pytest.raises(AssertionError):
        gen.edge_boxes((60, 60))
