"""CPU suite: MTCNN's box logic one stage at a time.  The product's four host functions (hse_facerec_tf_amd.mtcnn.stage1_level /
stage1_finish / stage2_finish / stage3_finish: the detector's host path and its overflow fallback) against the oracle's four
(oracle.mtcnn, the reference's generateBoundingBox / nms / bbreg / rerec / pad with the stable argsort) on every case of
tests/mtcnn_stage_cases.py, value for value; and the generator's own promises, which the GPU suite relies on."""
import numpy as np
import pytest

from hse_facerec_tf_amd import mtcnn as pm
from oracle import mtcnn as om

import mtcnn_stage_cases as gen

CAP = gen.NOMINAL_CAP
LEVELS = gen.level_cases(CAP)
SEQUENCES = gen.sequence_cases(CAP)
FINISHES = gen.finish_cases(CAP)
NETS = {2: gen.net_cases(2, CAP), 3: gen.net_cases(3, CAP)}


def same_values(got, want):
    """Equal shapes and values; dtypes may differ (stage 2's reference list is int32, the product's too, the device's float64)."""
    got, want = np.asarray(got), np.asarray(want)
    return got.shape == want.shape and np.array_equal(got, want)


def same_bits(got, want):
    got, want = np.asarray(got), np.asarray(want)
    return got.dtype == want.dtype == np.float32 and got.shape == want.shape and np.array_equal(got.view(np.uint32), want.view(np.uint32))


def overlaps_frame(tab):
    return bool(np.all(tab[:, 0] <= tab[:, 2]) and np.all(tab[:, 1] <= tab[:, 3]))


# ---- product host function == oracle function, on every case ----------------------------------------------------------------------
@pytest.mark.parametrize("name", gen.names(LEVELS))
def test_host_stage1_level_is_the_oracles(name):
    c = gen.by_name(LEVELS)[name]
    want = om.stage1_level(c["prob"], c["reg"], c["scale"], c["thr"])
    got = pm.stage1_level(c["prob"], c["reg"], c["scale"], c["thr"])
    assert want.shape[1] == 9 and same_values(got, want), name
    assert (want.shape[0] == 0) == (c["n_fire"] == 0)


@pytest.mark.parametrize("name", gen.names(SEQUENCES))
def test_host_level_sequence_and_finish_are_the_oracles(name):
    c = gen.by_name(SEQUENCES)[name]
    want = np.concatenate([om.stage1_level(l["prob"], l["reg"], l["scale"], l["thr"]) for l in c["levels"]], axis=0)
    got = np.concatenate([pm.stage1_level(l["prob"], l["reg"], l["scale"], l["thr"]) for l in c["levels"]], axis=0)
    assert same_values(got, want), name
    wb, wt = om.stage1_finish(want, c["img_w"], c["img_h"])
    gb, gt = pm.stage1_finish(got, c["img_w"], c["img_h"])
    assert wb.shape[0] > 0 and same_values(gb, wb) and same_values(gt, wt), name
    assert overlaps_frame(wt), name


@pytest.mark.parametrize("name", gen.names(FINISHES))
def test_host_stage1_finish_is_the_oracles(name):
    c = gen.by_name(FINISHES)[name]
    wb, wt = om.stage1_finish(c["found"], c["img_w"], c["img_h"])
    gb, gt = pm.stage1_finish(c["found"], c["img_w"], c["img_h"])
    assert wb.shape == (wt.shape[0], 5) and wt.shape[1] == 8 and wb.shape[0] > 0
    assert same_values(gb, wb) and same_values(gt, wt), name
    assert overlaps_frame(wt), name


@pytest.mark.parametrize("name", gen.names(NETS[2]))
def test_host_stage2_finish_is_the_oracles(name):
    c = gen.by_name(NETS[2])[name]
    args = (c["boxes_in"], c["prob"], c["reg"], c["thr"], c["img_w"], c["img_h"])
    wb, wt = om.stage2_finish(*args)
    gb, gt = pm.stage2_finish(*args)
    assert wb.shape == (wt.shape[0], 5) and wt.shape[1] == 8
    assert same_values(gb, wb) and same_values(gt, wt), name
    assert overlaps_frame(wt), name


@pytest.mark.parametrize("name", gen.names(NETS[3]))
def test_host_stage3_finish_is_the_oracles(name):
    c = gen.by_name(NETS[3])[name]
    args = (c["boxes_in"], c["prob"], c["reg"], c["pts"], c["thr"])
    wb, wp = om.stage3_finish(*args)
    gb, gp = pm.stage3_finish(*args)
    assert wb.shape == (wp.shape[0], 5) and wp.shape[1] == 10
    assert same_values(gb, wb) and same_bits(gp, wp), name


def test_stage_functions_do_not_touch_their_inputs():
    for mod in (om, pm):
        c = gen.by_name(NETS[3])["stage3/random/17"]
        before = [np.array(c[k], copy=True) for k in ("boxes_in", "prob", "reg", "pts")]
        mod.stage3_finish(c["boxes_in"], c["prob"], c["reg"], c["pts"], c["thr"])
        mod.stage2_finish(c["boxes_in"], c["prob"], c["reg"], c["thr"], c["img_w"], c["img_h"])
        f = gen.by_name(FINISHES)["finish/clustered/300"]
        found = f["found"].copy()
        mod.stage1_finish(f["found"], f["img_w"], f["img_h"])
        l = gen.by_name(LEVELS)["level/clustered/17"]
        pr, rg = l["prob"].copy(), l["reg"].copy()
        mod.stage1_level(l["prob"], l["reg"], l["scale"], l["thr"])
        assert all(np.array_equal(a, c[k]) for a, k in zip(before, ("boxes_in", "prob", "reg", "pts")))
        assert np.array_equal(found, f["found"]) and np.array_equal(pr, l["prob"]) and np.array_equal(rg, l["reg"])


# ---- what the generator promises --------------------------------------------------------------------------------------------------
def test_generator_is_seeded_and_takes_the_capacity():
    again = gen.level_cases(CAP)
    assert gen.names(again) == gen.names(LEVELS)
    assert all(np.array_equal(a["prob"], b["prob"]) and np.array_equal(a["reg"], b["reg"]) for a, b in zip(again, LEVELS))
    for cap in (1500, 4096):                        # another capacity: the same names, the counts follow it
        lv = gen.level_cases(cap)
        assert gen.names(lv) == gen.names(LEVELS)
        assert {cap - 1, cap, cap + 1} <= {c["n_fire"] for c in lv}
        assert gen.names(gen.sequence_cases(cap)) == gen.names(SEQUENCES)
        for stage in (2, 3):
            nc = gen.net_cases(stage, cap)
            assert gen.names(nc) == gen.names(NETS[stage])
            assert {cap, cap + 1} <= {c["boxes_in"].shape[0] for c in nc}
        assert cap in {c["found"].shape[0] for c in gen.finish_cases(cap)}


def test_generated_levels_hold_every_count_shape_and_edge():
    t = gen.thr32(gen.THR[0])
    for c in LEVELS:
        assert c["prob"].dtype == c["reg"].dtype == np.float32 and c["reg"].shape == c["prob"].shape + (4,)
        assert int(np.count_nonzero(c["prob"] >= t)) == c["n_fire"]
    fire = {c["n_fire"] for c in LEVELS}
    assert {0, 1, 2, 17, 1023, 1024, 1025, CAP - 1, CAP, CAP + 1} <= fire
    shapes = {c["prob"].shape for c in LEVELS}
    assert any(w > h > 1 for w, h in shapes) and any(h > w > 1 for w, h in shapes)
    assert any(w == 1 and h > 1 for w, h in shapes) and any(h == 1 and w > 1 for w, h in shapes) and (1, 1) in shapes
    scales = {c["scale"] for c in LEVELS}
    assert 0.5 in scales and 1.0 in scales and len(scales & set(gen.PYRAMID)) >= 4
    # runs of bit-equal 1.0f, a map with all scores equal, and lists on the second trip of a 1024-thread loop with ties
    assert any(np.count_nonzero(c["prob"] == np.float32(1)) >= 4 and c["n_fire"] > 1024 for c in LEVELS)
    assert any(c["n_fire"] > 1024 and np.unique(c["prob"][c["prob"] >= t]).size == 1 for c in LEVELS)
    # the single firing cell sits off the centre column and the flipped regression row differs from the unflipped one
    singles = [c for c in LEVELS if c["n_fire"] == 1 and c["prob"].shape[0] > 1]
    assert singles
    for c in singles:
        (xi, yi), = np.argwhere(c["prob"] >= t)
        w = c["prob"].shape[0]
        assert w - 1 - xi != xi and not np.array_equal(c["reg"][xi, yi], c["reg"][w - 1 - xi, yi])
        assert np.array_equal(om.stage1_level(c["prob"], c["reg"], c["scale"], c["thr"])[0, 5:9], c["reg"][w - 1 - xi, yi].astype(np.float64))
    # clustered lists lose most of their boxes to the NMS, spaced ones none
    lv = gen.by_name(LEVELS)
    assert om.stage1_level(*[lv["level/spaced/120x120"][k] for k in ("prob", "reg", "scale", "thr")]).shape[0] == 400
    assert om.stage1_level(*[lv["level/clustered/cap"][k] for k in ("prob", "reg", "scale", "thr")]).shape[0] < CAP // 4


def test_generated_threshold_edges_fire_as_the_reference_compares():
    t, b = gen.thr32(gen.THR[0]), gen.below(gen.THR[0])
    assert b < t and np.nextafter(b, np.float32(1)) == t
    for name in ("level/threshold-edge", "level/threshold-edge-pyramid"):
        c = gen.by_name(LEVELS)[name]
        scores = c["prob"][tuple(c["cells"].T)]
        assert np.count_nonzero(scores == t) >= 1 and np.count_nonzero(scores == b) >= 1
        rows = om.stage1_level(c["prob"], c["reg"], c["scale"], c["thr"])
        got = np.sort(rows[:, 4].astype(np.float32))
        assert np.array_equal(got, np.sort(scores[scores >= t]))                # the cell at float32(thr) fires, the one below does not
    for stage in (2, 3):                                                         # stages 2 and 3: a score AT the threshold does not pass
        c = gen.by_name(NETS[stage])["stage%d/at-threshold/17" % stage]
        k, thr = c["at_thr"], gen.thr32(c["thr"])
        assert c["prob"][k, 1] == thr
        up = c["prob"].copy()
        up[k, 1] = np.nextafter(thr, np.float32(1))
        if stage == 2:
            at = om.stage2_finish(c["boxes_in"], c["prob"], c["reg"], c["thr"], c["img_w"], c["img_h"])[0]
            above = om.stage2_finish(c["boxes_in"], up, c["reg"], c["thr"], c["img_w"], c["img_h"])[0]
        else:
            at = om.stage3_finish(c["boxes_in"], c["prob"], c["reg"], c["pts"], c["thr"])[0]
            above = om.stage3_finish(c["boxes_in"], up, c["reg"], c["pts"], c["thr"])[0]
        assert above.shape[0] == at.shape[0] + 1 and at.shape[0] > 0


def test_generated_sequences_fill_and_cross_the_capacity():
    seq = gen.by_name(SEQUENCES)
    counts = {}
    for name, c in seq.items():
        counts[name] = [om.stage1_level(l["prob"], l["reg"], l["scale"], l["thr"]).shape[0] for l in c["levels"]]
    below, exact, cross = counts["sequence/below-cap"], counts["sequence/exactly-cap"], counts["sequence/crosses-cap"]
    assert seq["sequence/below-cap"]["overflow_at"] is None and 0 < sum(below) < CAP
    assert 0 in below and 1 in below and sum(1 for k in below if k > 0) >= 4
    assert any(l["n_fire"] > 1024 for l in seq["sequence/below-cap"]["levels"])
    assert seq["sequence/exactly-cap"]["overflow_at"] is None and sum(exact) == CAP
    assert exact == [l["n_fire"] for l in seq["sequence/exactly-cap"]["levels"]]              # cells 6 apart: all survive
    at = seq["sequence/crosses-cap"]["overflow_at"]
    assert at == len(cross) - 1 and sum(cross[:at]) <= CAP < sum(cross) and cross == [l["n_fire"] for l in seq["sequence/crosses-cap"]["levels"]]
    assert all(k <= CAP for k in cross)                                                        # no single level overflows: the total does
    # ties across levels reach the finish
    rows = np.concatenate([om.stage1_level(l["prob"], l["reg"], l["scale"], l["thr"]) for l in seq["sequence/below-cap"]["levels"]], axis=0)
    assert np.count_nonzero(rows[:, 4] == 1.0) > 8


def test_generated_lists_hold_every_size_tie_and_boundary():
    assert {1, 2, 300, CAP} <= {c["found"].shape[0] for c in FINISHES}
    for c in FINISHES:
        assert np.array_equal(c["found"][:, 0:4], np.fix(c["found"][:, 0:4]))
        assert np.array_equal(c["found"][:, 4:9], c["found"][:, 4:9].astype(np.float32).astype(np.float64))
    big = gen.by_name(FINISHES)["finish/clustered/cap"]["found"]
    assert CAP - np.unique(big[:, 4]).size >= CAP // 4                          # ties, at 1.0f and elsewhere
    for stage in (2, 3):
        sizes = {c["boxes_in"].shape[0] for c in NETS[stage]}
        assert {0, 1, 5, 16, 17, 700, CAP, CAP + 1} <= sizes
        for c in NETS[stage]:
            assert np.array_equal(c["boxes_in"][:, 0:4], np.fix(c["boxes_in"][:, 0:4]))
            assert c["prob"].dtype == c["reg"].dtype == c["pts"].dtype == np.float32
        none = gen.by_name(NETS[stage])["stage%d/none-pass/16" % stage]
        assert not np.any(none["prob"][:, 1] > gen.thr32(none["thr"])) and np.any(none["prob"][:, 1] == gen.thr32(none["thr"]))
        tied = gen.by_name(NETS[stage])["stage%d/all-tied/1500" % stage]
        assert np.unique(tied["prob"][:, 1]).size == 1 and tied["prob"][0, 1] > gen.thr32(tied["thr"])
    # nested boxes: the 'Min' overlap and IoU give different lists
    c = gen.by_name(NETS[3])["stage3/random/700"]
    b = om.bbreg(np.hstack([c["boxes_in"][:, 0:4], c["prob"][:, 1:2].astype(np.float64)]), c["reg"])
    b = b[c["prob"][:, 1] > c["thr"]]
    assert list(om.nms(b.copy(), 0.7, 'Min', om.stable_argsort)) != list(om.nms(b.copy(), 0.7, 'Union', om.stable_argsort))
    # boundaries: among the cases whose crops the GPU suite cuts, boxes over each edge, two opposite edges at once, corners
    seen = {1: set(), 2: set()}
    for c in FINISHES:
        if c["crops"]:
            boxes, tab = om.stage1_finish(c["found"], c["img_w"], c["img_h"])
            seen[1] |= set(gen.clip_sides(boxes, c["img_w"], c["img_h"]))
            assert overlaps_frame(tab) and 0 < boxes.shape[0] <= 40, c["name"]         # a list the per-box host crops can afford
    for c in NETS[2]:
        if c["crops"]:
            boxes, tab = om.stage2_finish(c["boxes_in"], c["prob"], c["reg"], c["thr"], c["img_w"], c["img_h"])
            seen[2] |= set(gen.clip_sides(boxes, c["img_w"], c["img_h"]))
            assert overlaps_frame(tab) and 0 < boxes.shape[0] <= 40, c["name"]
    for stage in (1, 2):
        assert set(gen.REQUIRED_CLIPS) <= seen[stage], (stage, set(gen.REQUIRED_CLIPS) - seen[stage])
