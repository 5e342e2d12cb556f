"""CPU suite: affinity-propagation clustering without a GPU -- the NumPy restatement the GPU suite compares with is scikit-learn (on fp64
input) on every recorded case (tests/golden/affinity.npz, recorded by tools/record_affinity_golden.py), without noise and with the
header's hash noise; the hash restated in NumPy is the header's; and what is libhsefr_affinity.so's own: its functions' argument counts,
the header's limits, bounds and info words against ops, its row of csrc/build.sh, what its source promises, every refused argument before
any device work.  What holds for every library of the package -- header, exports and binding agree, version, loaded once, gfx950 only,
the ISA lint, no other library's names -- tests/test_libraries_cpu.py asserts for this one too."""
import ctypes
import os
import re
import warnings

import numpy as np
import pytest

import affinity_cases as cases
import affinity_ref as ref
import build_table

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "hsefr_affinity.h")
NAMES = ["hsefr_affinity_fit", "hsefr_affinity_fit_dense", "hsefr_affinity_last_error", "hsefr_affinity_version",
         "hsefr_affinity_workspace_bytes"]
KERNELS = 19        # norms, sim, copy, minmax, hist, digit, prepare, sweep x 2, colsum, stop, select, assign, member_sum, winner, relist, labels, trivial, info
GOLDEN, STEPS = cases.load_golden()
IDS = [cases.case_id(case) for case, _ in GOLDEN]
LIVE_N = 1300                                            # above it a host fit takes seconds: the recorded answer stands for scikit-learn's live one


# ---- the restatement is scikit-learn -------------------------------------------------------------------------------------------------
def test_the_file_holds_the_cases_of_the_module():
    assert [case for case, _ in GOLDEN] == [tuple(c) for c in cases.CASES]
    sizes = [want["n"] for _, want in GOLDEN]
    assert {63, 64, 65, 257, 1212} <= set(sizes) and any(1850 <= n <= 1950 for n in sizes)
    assert os.path.getsize(cases.GOLDEN) < 64 * 1024
    for case, want in GOLDEN:
        assert len(want["partition"]) == want["n"] and want["partition"].max() + 1 == want["clusters"] == len(want["exemplars"])
        assert np.array_equal(want["partition"], ref.first_occurrence(want["partition"]))
        assert len(want["refinement_decidable"]) == want["clusters"] and want["refinement_decidable"].sum() >= want["clusters"] - 3
        assert 15 < want["n_iter"] < 200
    assert sorted(STEPS) == [1, 5, 16]
    assert STEPS[1]["n_iter"] == 1 and len(STEPS[1]["exemplars"]) == 0 and (STEPS[1]["labels"] == -1).all()      # no exemplar yet
    assert [STEPS[m]["n_iter"] for m in (1, 5, 16)] == [1, 5, 16] and not any(STEPS[m]["converged"] for m in STEPS)
    assert len(STEPS[5]["exemplars"]) > len(STEPS[16]["exemplars"]) >= 1


def test_the_recorded_cases_are_decidable():
    """every recorded margin is far above what another fp64 arithmetic can move: the GPU suite asserts them against 100 x the header's
    bound case by case; here the floors the cases were chosen by"""
    from hse_facerec_tf_amd import ops
    for case, want in GOLDEN:
        bound = ops.affinity_message_bound(want["n"], case[2], 5.0)
        assert want["margin_diag"] >= 1e-6 and want["margin_assign"] >= 5e-4
        assert min(want["margin_diag"], want["margin_assign"]) > 100 * bound


@pytest.mark.parametrize("case,want", GOLDEN, ids=IDS)
def test_the_restatement_is_scikit_learn(case, want):
    from sklearn.cluster import AffinityPropagation
    X = cases.case_features(case)
    assert len(X) == want["n"] and X.dtype == np.float32
    if len(X) <= LIVE_N:
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            fit = AffinityPropagation(random_state=0).fit(X.astype(np.float64))
        live = (ref.first_occurrence(fit.labels_), fit.n_iter_, len(fit.cluster_centers_indices_))
        assert np.array_equal(live[0], want["partition"]) and live[1:] == (want["n_iter"], want["clusters"])
        assert np.array_equal(fit.cluster_centers_indices_, want["exemplars"])
    S = ref.similarities(X)
    for seed in (None, 0) if len(X) <= LIVE_N else (0,):
        r = ref.affinity_propagation(S, seed=seed)
        assert np.array_equal(ref.first_occurrence(r.labels), want["partition"]), seed
        assert (r.n_iter, len(r.exemplars), r.converged, r.equal) == (want["n_iter"], want["clusters"], True, False), seed
        assert r.margins.diag >= want["margin_diag"] and r.margins.assign >= want["margin_assign"]
        assert np.array_equal(r.exemplars, np.sort(r.exemplars)) and np.array_equal(r.labels[r.exemplars], np.arange(len(r.exemplars)))
        for k, e in enumerate(want["exemplars"]):
            if want["refinement_decidable"][k]:
                assert r.exemplars[r.labels[e]] == e


def test_the_recorded_steps_are_the_restatements():
    S = ref.similarities(cases.case_features(cases.CASES[cases.STEPS_CASE]))
    for m, want in STEPS.items():
        r = ref.affinity_propagation(S, max_iter=m)
        assert np.array_equal(r.labels, want["labels"]) and np.array_equal(r.exemplars, want["exemplars"])
        assert (r.n_iter, int(r.converged)) == (want["n_iter"], want["converged"])


def test_the_restatement_on_small_inputs():
    one = ref.fit_features(np.ones((1, 4), np.float32))
    assert one.labels.tolist() == [0] and one.exemplars.tolist() == [0] and one.n_iter == 0 and one.equal
    two = ref.fit_features(np.array([[0, 0, 0, 0], [1, 0, 0, 0]], np.float32))
    assert two.preference == -0.5 and two.labels.tolist() == [0, 1] and two.equal                   # the median exceeds S: n clusters
    below = ref.fit_features(np.array([[0, 0, 0, 0], [1, 0, 0, 0]], np.float32), preference=-2.0)
    assert below.labels.tolist() == [0, 0] and below.exemplars.tolist() == [0]
    same = ref.fit_features(np.ones((3, 4), np.float32))
    assert same.labels.tolist() == [0, 0, 0] and same.preference == 0.0
    from sklearn.cluster import AffinityPropagation
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        for X, pref in ((np.ones((3, 4)), None), (np.array([[0.0, 0, 0, 0], [1, 0, 0, 0]]), None), (np.array([[0.0, 0, 0, 0], [1, 0, 0, 0]]), -2.0)):
            fit = AffinityPropagation(preference=pref, random_state=0).fit(X)
            r = ref.fit_features(X.astype(np.float32), preference=pref)
            assert fit.labels_.tolist() == r.labels.tolist() and list(fit.cluster_centers_indices_) == r.exemplars.tolist() and fit.n_iter_ == 0
    assert ref.first_occurrence([5, 5, 2, 5, 9, 2]).tolist() == [0, 0, 1, 0, 2, 1]
    assert ref.cluster_lists([1, 0, 1, -1, 2, 1]) == [[0, 2, 5], [1], [4]]


def test_an_asymmetric_precomputed_matrix_is_scikit_learns():
    from sklearn.cluster import AffinityPropagation
    rs = np.random.RandomState(5)
    X = cases.case_features(cases.CASES[7])
    S = ref.similarities(X) * (1.0 + 0.05 * rs.uniform(size=(len(X), len(X))))
    assert not np.array_equal(S, S.T)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        fit = AffinityPropagation(affinity="precomputed", random_state=0).fit(S.copy())
    for seed in (None, 0):
        r = ref.affinity_propagation(S, seed=seed)
        assert np.array_equal(ref.first_occurrence(r.labels), ref.first_occurrence(fit.labels_)) and r.n_iter == fit.n_iter_
    assert r.preference == np.median(S)


# ---- the hash --------------------------------------------------------------------------------------------------------------------------
def test_the_hash_restated_in_numpy_is_the_headers():
    header = open(HEADER).read()
    for macro, value in (("HASH_SEED_MUL", ref.SEED_MUL), ("HASH_GAMMA", ref.GAMMA), ("HASH_MUL1", ref.MUL1), ("HASH_MUL2", ref.MUL2)):
        assert int(re.search(r"#define HSEFR_AFFINITY_%s (0x[0-9A-Fa-f]+)ull" % macro, header).group(1), 16) == value
    assert float(re.search(r"#define HSEFR_AFFINITY_SQRT3 ([0-9.]+)", header).group(1)) == ref.SQRT3 == np.sqrt(3.0)
    for line in ("z = (uint64) e + (uint64) seed * HSEFR_AFFINITY_HASH_SEED_MUL + HSEFR_AFFINITY_HASH_GAMMA",
                 "z = (z ^ (z >> 30)) * HSEFR_AFFINITY_HASH_MUL1;  z = (z ^ (z >> 27)) * HSEFR_AFFINITY_HASH_MUL2;  z = z ^ (z >> 31)",
                 "g = (((double)(z >> 12) + 0.5) * 2^-52 * 2.0 - 1.0) * HSEFR_AFFINITY_SQRT3",
                 "S[e] = S[e] + (2^-52 * S[e] + 100.0 * DBL_MIN) * g"):
        assert line in header, line

    def scalar(seed, e):                                                                # the header's lines in Python integers
        z = (e + seed * ref.SEED_MUL + ref.GAMMA) & ref.MASK
        z = ((z ^ (z >> 30)) * ref.MUL1) & ref.MASK
        z = ((z ^ (z >> 27)) * ref.MUL2) & ref.MASK
        z ^= z >> 31
        return (((z >> 12) + 0.5) * 2.0 ** -52 * 2.0 - 1.0) * ref.SQRT3
    for seed in (0, 1, 2 ** 40 + 3):
        g = ref.noise_factor(seed, 37)
        assert g.shape == (37, 37) and all(g.flat[e] == scalar(seed, e) for e in (0, 1, 36, 37, 700, 37 * 37 - 1))
    g = ref.noise_factor(0, 300)
    assert np.abs(g).max() < np.sqrt(3.0) and abs(g.mean()) < 0.01 and abs(g.var() - 1.0) < 0.01
    assert not np.array_equal(ref.noise_factor(0, 8), ref.noise_factor(1, 8))
    src = open(os.path.join(ROOT, "hse_facerec_tf_amd", "csrc", "affinity.hip")).read()
    assert "#pragma clang fp contract(off)" in src                                       # every operation rounded on its own


# ---- names -----------------------------------------------------------------------------------------------------------------------------
def no_device(monkeypatch):
    from hse_facerec_tf_amd import _lib

    def refuse(*a, **k):
        raise AssertionError("device work")
    for name in ("require_gpu", "lib", "shift_lib", "affinity_lib", "split_lib", "cuda_device"):
        monkeypatch.setattr(_lib, name, refuse)


def test_the_python_entry_points_check_their_arguments_before_any_device_work(monkeypatch):
    from hse_facerec_tf_amd import clustering
    no_device(monkeypatch)
    X = np.ones((5, 8), np.float32)
    S = -np.ones((5, 5))
    assert (clustering.AFFINITY_DAMPING, clustering.AFFINITY_MAX_ITER, clustering.AFFINITY_CONVERGENCE_ITER) == (0.5, 200, 15)
    assert issubclass(clustering.ConvergenceWarning, UserWarning)
    calls = (lambda **kw: clustering.affinity_propagation(X, **kw), lambda **kw: clustering.affinity_propagation_dense(S, **kw),
             lambda **kw: clustering.cluster_faces_affinity_propagation(X, **kw))
    for call in calls:
        for bad in (0.49, 1.0, -1, float("nan"), None, "0.5", True):
            with pytest.raises(ValueError, match="damping"):
                call(damping=bad)
        for bad in (0, -1, 1.5, None, True):
            with pytest.raises(ValueError, match="max_iter"):
                call(max_iter=bad)
        for bad in (0, 65, 1.5, None, True):
            with pytest.raises(ValueError, match="convergence_iter"):
                call(convergence_iter=bad)
        for bad in (float("nan"), float("inf"), "x", True):
            with pytest.raises(ValueError, match="preference"):
                call(preference=bad)
        for bad in (-1, 1.5, "0", True):
            with pytest.raises(ValueError, match="seed"):
                call(seed=bad)
    with pytest.raises(ValueError, match="preference"):
        clustering.affinity_propagation_scores(X, [0] * 5, [-1.0, float("inf")])
    with pytest.raises(ValueError, match="split"):
        clustering.cluster_faces_affinity_propagation(X, all_indices=[0, 0, 1, 2, 3], split="bogus")
    Xn = X.copy()
    Xn[2, 3] = np.nan
    for call in (lambda: clustering.affinity_propagation(Xn), lambda: clustering.cluster_faces_affinity_propagation(Xn),
                 lambda: clustering.affinity_propagation_predict(Xn, np.ones((2, 8))),
                 lambda: clustering.affinity_propagation_scores(Xn, [0] * 5, [None])):
        with pytest.raises(ValueError, match="non-finite"):
            call()
    Sn = S.copy()
    Sn[1, 2] = np.inf
    with pytest.raises(ValueError, match="non-finite"):
        clustering.affinity_propagation_dense(Sn)
    with pytest.raises(ValueError, match="square"):
        clustering.affinity_propagation_dense(np.ones((3, 4)))
    with pytest.raises(ValueError):
        clustering.affinity_propagation(np.ones(8, np.float32))
    with pytest.raises(ValueError, match="as the centres"):
        clustering.affinity_propagation_predict(X, np.ones((2, 4)))
    assert clustering.affinity_propagation_predict(X, np.ones((0, 8))).tolist() == [-1] * 5          # a fit without a centre


@pytest.mark.parametrize("name", ["affinity", "affinity_propagation", "AffinityPropagation", "ap"])
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


# ---- the library: what is libhsefr_affinity.so's own (what every library shares is asserted for it in tests/test_libraries_cpu.py) ------
def test_the_arguments_limits_bounds_and_info_words_are_the_headers():
    from hse_facerec_tf_amd import _lib, ops
    assert sorted(_lib.AFFINITY_SIGNATURES) == NAMES
    header = open(HEADER).read()
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    for name, count in (("hsefr_affinity_fit", 16), ("hsefr_affinity_fit_dense", 15), ("hsefr_affinity_workspace_bytes", 2)):
        args = re.search(r"\b%s\((.*?)\);" % name, code, flags=re.S).group(1)
        assert len(args.split(",")) == len(_lib.AFFINITY_SIGNATURES[name][1]) == count
    for macro, value in (("MAX_N", ops.AFFINITY_MAX_N), ("MAX_D", ops.AFFINITY_MAX_D), ("D_MULTIPLE", ops.AFFINITY_D_MULTIPLE),
                         ("MAX_ITER", ops.AFFINITY_MAX_ITER), ("MAX_CONVERGENCE_ITER", ops.AFFINITY_MAX_CONVERGENCE_ITER)):
        assert int(re.search(r"#define HSEFR_AFFINITY_%s (\d+)" % macro, header).group(1)) == value
    assert (ops.AFFINITY_MAX_N, ops.AFFINITY_MAX_D, ops.AFFINITY_D_MULTIPLE, ops.AFFINITY_MAX_ITER) == (16384, 4096, 4, 10000)
    assert ops.AFFINITY_MAX_N * 8 + 32 * 1024 <= 160 * 1024                              # a row of doubles beside the scratch in a CU's LDS
    assert int(re.search(r"#define HSEFR_AFFINITY_SIM_ULPS\(d\) \(\(d\) \+ (\d+)\)", header).group(1)) == ops.AFFINITY_SIM_ULPS_PLUS
    plus = int(re.search(r"#define HSEFR_AFFINITY_MSG_ULPS\(n, d\) \(\(n\) \* \(\(d\) \+ (\d+)\)\)", header).group(1))
    assert plus == ops.AFFINITY_MSG_ULPS_PLUS
    assert ops.affinity_message_bound(1926, 64, 4.0) == 1926 * (64 + plus) * 2.0 ** -53 * 4.0 < 8e-11
    words = re.search(r"enum \{(.*?)\};", code, flags=re.S).group(1)
    assert [int(v) for v in re.findall(r"HSEFR_AFFINITY_INFO_[A-Z_]+ = (\d+)", words)] == [0, 1, 2, 3, 4, 5, 8] and len(ops.AFFINITY_INFO) == 8


def test_the_librarys_row_of_the_build_table():
    row = build_table.rows()["affinity"]
    assert (row["out"], row["srcs"]) == ("../libhsefr_affinity.so", ["affinity.hip"])
    assert build_table.stale_against("affinity", "common.h", "include/hsefr.h", "include/hsefr_affinity.h")
    assert row["flags"] == build_table.rows()["frames"]["flags"]                       # $COMMON, the flags of the other later libraries


def test_the_source_keeps_its_promises():
    src = open(os.path.join(ROOT, "hse_facerec_tf_amd", "csrc", "affinity.hip")).read().split('#include <algorithm>')[1]
    assert src.count("__builtin_amdgcn_mfma_f64_16x16x4f64") == 2                      # the similarities' product, two tiles
    for word in ("cooperative", "__threadfence", "while (atomic", "volatile", " printf(", "assert(", "atomicAdd(double", "float atomic"):
        assert word not in src, word
    assert len(re.findall(r"__global__", src)) == KERNELS - 1                          # one of the nineteen is a second instance of a template
    for name in re.findall(r"atomic[A-Z][a-z]+\(&(\w+)", src):                         # every atomic is an integer's
        assert name in ("sel", "s_hist", "out", "s_un", "s_k", "best", "winner"), name


# ---- refused arguments: a status and a message, no device call ---------------------------------------------------------------------------
def test_the_fits_check_their_arguments_without_a_gpu():
    from hse_facerec_tf_amd import _lib
    L = _lib.affinity_lib()
    need = L.hsefr_affinity_workspace_bytes(4, 8)
    assert need > 3 * 4 * 4 * 8 and L.hsefr_affinity_workspace_bytes(16384, 4096) > 3 * 16384 * 16384 * 8
    assert L.hsefr_affinity_workspace_bytes(4, 4) == need                              # the matrices do not depend on d
    for n, d in ((0, 8), (-1, 8), (16385, 8), (4, 0), (4, 6), (4, 4100), (4, -4)):
        assert L.hsefr_affinity_workspace_bytes(n, d) == 0
    buf = ctypes.create_string_buffer(need + 8192 + 64)
    p = (ctypes.cast(buf, ctypes.c_void_p).value + 63) // 64 * 64
    ok = dict(x=p, n=4, d=8, damping=0.5, m=200, c=15, pref=float("nan"), seed=0, exemplars=p + 512, labels=p + 1024, diag=p + 1536,
              preference=p + 2048, info=p + 2560, ws=p + 4096, bytes=need)

    def tail(a):
        return (a["damping"], a["m"], a["c"], a["pref"], a["seed"], a["exemplars"], a["labels"], a["diag"], a["preference"], a["info"], a["ws"],
                a["bytes"], None)

    def fit(**kw):
        a = dict(ok, **kw)
        return L.hsefr_affinity_fit(a["x"], a["n"], a["d"], *tail(a))

    def dense(**kw):
        a = dict(ok, **kw)
        return L.hsefr_affinity_fit_dense(a["x"], a["n"], *tail(a))

    def refused(call, kw, status, word):
        rc, msg = call(**kw), _lib.affinity_last_error()
        assert rc == status and msg.startswith("affinity_") and word in msg, (kw, rc, msg)
    for call, who in ((fit, "affinity_fit:"), (dense, "affinity_fit_dense:")):
        for out in ("x", "exemplars", "labels", "diag", "preference", "info", "ws"):
            refused(call, {out: None}, _lib.ERR_INVALID, "null pointer")
        for n in (0, -3):
            refused(call, dict(n=n), _lib.ERR_INVALID, "n=")
        for damping in (0.49, 1.0, 1.5, -0.5, float("nan")):
            refused(call, dict(damping=damping), _lib.ERR_INVALID, "damping")
        for c in (0, 65, -1):
            refused(call, dict(c=c), _lib.ERR_INVALID, "convergence_iter=%d" % c)
        for pref in (float("inf"), float("-inf")):
            refused(call, dict(pref=pref), _lib.ERR_INVALID, "preference")
        refused(call, dict(seed=-2), _lib.ERR_INVALID, "noise_seed=-2")
        refused(call, dict(n=16385), _lib.ERR_UNSUPPORTED, "n=16385")
        for m in (0, -1, 10001):
            refused(call, dict(m=m), _lib.ERR_UNSUPPORTED, "max_iter=%d" % m)
        refused(call, dict(bytes=need - 1), _lib.ERR_INVALID, "%d needed" % need)       # one byte short
        refused(call, dict(bytes=0), _lib.ERR_INVALID, "workspace")
        refused(call, dict(ws=p + 4096 + 8), _lib.ERR_INVALID, "misaligned")
        assert _lib.affinity_last_error().startswith(who)
    for d in (0, 6, 10, -4, 4100):
        refused(fit, dict(d=d), _lib.ERR_UNSUPPORTED, "d=%d" % d)
    with pytest.raises(ValueError, match="damping"):
        _lib.affinity_check(fit(damping=0.2), "hsefr_affinity_fit")
    with pytest.raises(NotImplementedError, match="max_iter=0"):
        _lib.affinity_check(fit(m=0), "hsefr_affinity_fit")
