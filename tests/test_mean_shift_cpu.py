"""CPU suite: mean-shift clustering without a GPU -- the NumPy restatement the GPU suite compares with is scikit-learn on every recorded
case (tests/golden/mean_shift.npz, recorded by tools/record_mean_shift_golden.py) and on a live fit of the small ones, the margins in
the file are the restatement's, and what is libhsefr_shift.so's own: its functions' argument counts, the header's limits, bound and info
words against ops, its row of csrc/build.sh, what its source promises, every refused argument before any device work.  What holds for
every library of the package -- header, exports and binding agree, version, loaded once, gfx950 only, the ISA lint, no other library's
names -- tests/test_libraries_cpu.py asserts for this one too."""
import ctypes
import os
import re

import numpy as np
import pytest

import build_table
import mean_shift_cases as cases
import mean_shift_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "hsefr_shift.h")
NAMES = ["hsefr_shift_assign", "hsefr_shift_fit", "hsefr_shift_last_error", "hsefr_shift_version", "hsefr_shift_workspace_bytes"]
KERNELS = 14        # prep, norms x 2, member x 2, means, step, compact, rank, gather, suppress, centers, assign, info
GOLDEN = cases.load_golden()
IDS = [cases.case_id(case) for case, _ in GOLDEN]


_RESULTS = {}


def restated(case):
    """the restatement of a case, computed once"""
    if case not in _RESULTS:
        _RESULTS[case] = ref.mean_shift(cases.case_features(case), case[3])
    return _RESULTS[case]


# ---- the restatement is scikit-learn -------------------------------------------------------------------------------------------------
def test_the_file_holds_the_cases_of_the_module():
    assert [case for case, _ in GOLDEN] == [tuple(c) for c in cases.CASES] and len(GOLDEN) == 13
    assert [want["n"] for _, want in GOLDEN[:12]] == [142, 167, 112, 279, 328, 327, 484, 414, 428, 167, 162, 182]
    assert 1000 <= GOLDEN[12][1]["n"] <= 1300
    assert os.path.getsize(cases.GOLDEN) < 64 * 1024


@pytest.mark.parametrize("case,want", GOLDEN, ids=IDS)
def test_the_restatement_gives_the_recorded_answer(case, want):
    X = cases.case_features(case)
    assert len(X) == want["n"] and X.dtype == np.float32
    r = restated(case)
    assert np.array_equal(r.labels, want["labels"])
    assert r.n_iter == want["n_iter"]
    assert len(r.centers) == want["centers"] == len(r.intensity)
    assert r.stopped_by_max_iter == 0 and r.completed.max() == r.n_iter
    assert tuple(r.margins) == want["margins"]                          # the margins in the file are those the restatement reports now


@pytest.mark.parametrize("case,want", [g for g in GOLDEN if g[0][2] == 64 and g[1]["n"] < 200], ids=[i for i, g in zip(IDS, GOLDEN) if g[0][2] == 64 and g[1]["n"] < 200])
def test_the_restatement_is_a_live_fit(case, want):
    from sklearn.cluster import MeanShift
    X = cases.case_features(case)
    ms = MeanShift(bandwidth=case[3]).fit(X)
    r = restated(case)
    assert np.array_equal(ms.labels_, r.labels) and np.array_equal(ms.labels_, want["labels"])
    assert ms.n_iter_ == r.n_iter
    assert np.abs(ms.cluster_centers_ - r.centers).max() < 1e-6         # scikit-learn keeps float32 inputs in float32
    assert np.array_equal(ms.predict(X), ref.nearest_center(X, r.centers)[0])


def test_the_recorded_cases_are_decidable():
    """every recorded case's margins are far above what another fp64 arithmetic can move: the GPU suite asserts the member margin
    against the header's bound case by case; here the floors the cases were chosen by"""
    margins = np.array([want["margins"] for _, want in GOLDEN])
    assert margins[:, 0].min() >= 7e-7 and margins[:12, 0].min() >= 2.8e-6
    assert margins[:, 1].min() >= 1e-4 and margins[:, 2].min() >= 5e-4 and margins[:, 3].min() >= 6e-3


def test_the_restatement_on_small_inputs():
    one = ref.mean_shift(np.ones((1, 4), np.float32), 0.7)
    assert one.labels.tolist() == [0] and one.n_iter == 0 and one.intensity.tolist() == [1] and np.array_equal(one.centers, np.ones((1, 4)))
    same = ref.mean_shift(np.ones((5, 4), np.float32), 0.7)
    assert same.labels.tolist() == [0] * 5 and same.intensity.tolist() == [5] and same.distinct == 1
    X = np.array([[0, 0, 0, 0], [0.1, 0, 0, 0], [5, 0, 0, 0]], np.float32)
    r = ref.mean_shift(X, 0.7, cluster_all=False)
    assert r.labels.tolist() == [0, 0, 1] and r.intensity.tolist() == [2, 1]
    for m in (0, 1):
        r = ref.mean_shift(cases.case_features(cases.CASES[9]), 0.7, max_iter=m)
        assert r.n_iter == m and r.stopped_by_max_iter > 0 and r.completed.max() == m
    assert ref.cluster_lists([1, 0, 1, -1, 2, 1]) == [[0, 2, 5], [1], [4]]


# ---- names -----------------------------------------------------------------------------------------------------------------------------
def no_device(monkeypatch):
    from hse_facerec_tf_amd import _lib

    def refuse(*a, **k):
        raise AssertionError("device work")
    for name in ("require_gpu", "lib", "shift_lib", "split_lib", "cuda_device"):
        monkeypatch.setattr(_lib, name, refuse)


def test_the_python_entry_points_check_their_arguments_before_any_device_work(monkeypatch):
    from hse_facerec_tf_amd import clustering
    no_device(monkeypatch)
    X = np.ones((5, 8), np.float32)
    assert clustering.MEAN_SHIFT_BANDWIDTH == 0.7
    for bad in (0, -1.0, float("nan"), float("inf"), None, "0.7", True):
        for call in (lambda: clustering.mean_shift(X, bad), lambda: clustering.cluster_faces_mean_shift(X, bad),
                     lambda: clustering.mean_shift_scores(X, [0] * 5, [0.7, bad] if not isinstance(bad, (str, type(None))) else [bad])):
            with pytest.raises((ValueError, TypeError)):
                call()
        with pytest.raises(ValueError, match="bandwidth"):
            clustering.mean_shift(X, bad)
    for bad in (-1, 1.5, None, True):
        with pytest.raises(ValueError, match="max_iter"):
            clustering.mean_shift(X, 0.7, max_iter=bad)
    with pytest.raises(ValueError, match="split"):
        clustering.cluster_faces_mean_shift(X, 0.7, all_indices=[0, 0, 1, 2, 3], split="bogus")
    Xn = X.copy()
    Xn[2, 3] = np.nan
    for call in (lambda: clustering.mean_shift(Xn), lambda: clustering.cluster_faces_mean_shift(Xn),
                 lambda: clustering.mean_shift_predict(Xn, np.ones((2, 8))), lambda: clustering.mean_shift_scores(Xn, [0] * 5, [0.7])):
        with pytest.raises(ValueError, match="non-finite"):
            call()
    with pytest.raises(ValueError):
        clustering.mean_shift(np.ones(8, np.float32))
    with pytest.raises(ValueError, match="as the centres"):
        clustering.mean_shift_predict(X, np.ones((2, 4)))
    with pytest.raises(ValueError, match="cluster_centers"):
        clustering.mean_shift_predict(X, np.ones((0, 8)))


@pytest.mark.parametrize("name", ["meanshift", "mean_shift", "MeanShift"])
def test_the_older_entry_points_still_refuse_the_name(monkeypatch, name):
    from hse_facerec_tf_amd import clustering
    no_device(monkeypatch)
    X = np.ones((5, 8), np.float32)
    assert name not in clustering.CLUSTER_METHODS + clustering.GEOMETRIC_METHODS
    for call in (lambda: clustering.cluster_faces(X, 0.5, method=name), lambda: clustering.get_facial_clusters(np.ones((5, 5)), 0.5, method=name),
                 lambda: clustering.threshold_sweep(X, [0, 0, 1, 1, 2], name, [0.5]),
                 lambda: clustering.select_threshold([(X, [0, 0, 1, 1, 2])], name)):
        with pytest.raises(ValueError):
            call()


# ---- the library: what is libhsefr_shift.so's own (what every library shares is asserted for it in tests/test_libraries_cpu.py) ---------
def test_the_arguments_limits_bound_and_info_words_are_the_headers():
    from hse_facerec_tf_amd import _lib, ops
    assert sorted(_lib.SHIFT_SIGNATURES) == NAMES
    header = open(HEADER).read()
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    for name in ("hsefr_shift_fit", "hsefr_shift_assign", "hsefr_shift_workspace_bytes"):
        args = re.search(r"\b%s\((.*?)\);" % name, code, flags=re.S).group(1)
        assert len(args.split(",")) == len(_lib.SHIFT_SIGNATURES[name][1]) == {"hsefr_shift_fit": 13, "hsefr_shift_assign": 8}.get(name, 2)
    for macro, value in (("MAX_N", ops.SHIFT_MAX_N), ("MAX_D", ops.SHIFT_MAX_D), ("D_MULTIPLE", ops.SHIFT_D_MULTIPLE),
                         ("MAX_ITER", ops.SHIFT_MAX_ITER)):
        assert int(re.search(r"#define HSEFR_SHIFT_%s (\d+)" % macro, header).group(1)) == value
    assert (ops.SHIFT_MAX_N, ops.SHIFT_MAX_D, ops.SHIFT_D_MULTIPLE, ops.SHIFT_MAX_ITER) == (65535, 4096, 4, 10000)
    plus = int(re.search(r"#define HSEFR_SHIFT_DIST2_ULPS\(d\) \(\(d\) \+ (\d+)\)", header).group(1))
    assert plus == ops.SHIFT_DIST2_ULPS_PLUS
    assert ops.mean_shift_distance_bound(256, 0.7) == (256 + plus) * 2.0 ** -53 * (4 + 0.49) / 0.7 < 2e-13
    words = re.search(r"enum \{(.*?)\};", code, flags=re.S).group(1)
    assert [int(v) for v in re.findall(r"HSEFR_SHIFT_INFO_[A-Z_]+ = (\d+)", words)] == [0, 1, 2, 3, 4, 5, 6, 8] and len(ops.SHIFT_INFO) == 8


def test_the_librarys_row_of_the_build_table():
    row = build_table.rows()["shift"]
    assert (row["out"], row["srcs"]) == ("../libhsefr_shift.so", ["mean_shift.hip"])
    assert build_table.stale_against("shift", "common.h", "include/hsefr.h", "include/hsefr_shift.h")
    assert row["flags"] == build_table.rows()["frames"]["flags"]                       # $COMMON, the flags of the other later libraries


def test_the_source_keeps_its_promises():
    src = open(os.path.join(ROOT, "hse_facerec_tf_amd", "csrc", "mean_shift.hip")).read().split('#include <math.h>')[1]
    assert src.count("__builtin_amdgcn_mfma_f64_16x16x4f64") == 4                      # the product tile and the member sums, two tiles each
    for word in ("cooperative", "__threadfence", "while (atomic", "volatile", " printf(", "assert(", "atomicAdd(double", "float atomic"):
        assert word not in src, word
    assert len(re.findall(r"__global__", src)) == KERNELS - 2                          # two of the fourteen are second instances of a template


# ---- refused arguments: a status and a message, no device call ---------------------------------------------------------------------------
def test_fit_and_assign_check_their_arguments_without_a_gpu():
    from hse_facerec_tf_amd import _lib
    L = _lib.shift_lib()
    need = L.hsefr_shift_workspace_bytes(4, 8)
    assert need > 2 * 4 * 8 * 8 and L.hsefr_shift_workspace_bytes(65535, 4096) > 2 * 65535 * 4096 * 8
    for n, d in ((0, 8), (-1, 8), (65536, 8), (4, 0), (4, 6), (4, 4100), (4, -4)):
        assert L.hsefr_shift_workspace_bytes(n, d) == 0
    buf = ctypes.create_string_buffer(need + 8192 + 64)
    p = (ctypes.cast(buf, ctypes.c_void_p).value + 63) // 64 * 64
    ok = dict(x=p, n=4, d=8, h=0.7, m=300, centers=p + 512, intensity=p + 1024, labels=p + 1536, dist=p + 2048, info=p + 2560, ws=p + 4096,
              bytes=need)

    def fit(**kw):
        a = dict(ok, **kw)
        return L.hsefr_shift_fit(a["x"], a["n"], a["d"], a["h"], a["m"], a["centers"], a["intensity"], a["labels"], a["dist"], a["info"],
                                 a["ws"], a["bytes"], None)

    def refused(call, kw, status, word):
        rc, msg = call(**kw), _lib.shift_last_error()
        assert rc == status and msg.startswith("shift_") and word in msg, (kw, rc, msg)
    for out in ("x", "centers", "intensity", "labels", "dist", "info", "ws"):
        refused(fit, {out: None}, _lib.ERR_INVALID, "null pointer")
    for n in (0, -3):
        refused(fit, dict(n=n), _lib.ERR_INVALID, "n=")
    for h in (0.0, -0.7, float("nan"), float("inf")):
        refused(fit, dict(h=h), _lib.ERR_INVALID, "bandwidth")
    refused(fit, dict(n=65536), _lib.ERR_UNSUPPORTED, "n=65536")
    for d in (0, 6, 10, -4, 4100):
        refused(fit, dict(d=d), _lib.ERR_UNSUPPORTED, "d=%d" % d)
    for m in (-1, 10001):
        refused(fit, dict(m=m), _lib.ERR_UNSUPPORTED, "max_iter=%d" % m)
    refused(fit, dict(bytes=need - 1), _lib.ERR_INVALID, "%d needed" % need)           # one byte short
    refused(fit, dict(bytes=0), _lib.ERR_INVALID, "workspace")
    refused(fit, dict(ws=p + 4096 + 8), _lib.ERR_INVALID, "misaligned")

    oka = dict(q=p, nq=4, d=8, centers=p + 512, k=2, labels=p + 1024, dist=p + 1536)

    def assign(**kw):
        a = dict(oka, **kw)
        return L.hsefr_shift_assign(a["q"], a["nq"], a["d"], a["centers"], a["k"], a["labels"], a["dist"], None)
    for out in ("q", "centers", "labels", "dist"):
        refused(assign, {out: None}, _lib.ERR_INVALID, "null pointer")
    for kw in (dict(nq=0), dict(k=0), dict(k=-2)):
        refused(assign, kw, _lib.ERR_INVALID, "nq=")
    for kw in (dict(nq=65536), dict(k=65536), dict(d=6), dict(d=0), dict(d=4100)):
        refused(assign, kw, _lib.ERR_UNSUPPORTED, "d=")
    with pytest.raises(ValueError, match="bandwidth"):
        _lib.shift_check(fit(h=0.0), "hsefr_shift_fit")
    with pytest.raises(NotImplementedError, match="max_iter=-1"):
        _lib.shift_check(fit(m=-1), "hsefr_shift_fit")
