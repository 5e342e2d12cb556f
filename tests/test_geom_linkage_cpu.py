"""CPU suite: centroid, median and Ward linkage without a GPU -- the NumPy restatements the GPU suite compares with are scipy's trees on
every dense input that suite uses (so the GPU suite stands on inputs the reference alone passes), clustering.linkage_from_sequence,
flat cuts of a tree with inversions, the names the entry points take and refuse, the names libhsefr_geom.so exports with its header's
limit and enum (what holds for every library is in tests/test_libraries_cpu.py) and every refused argument of hsefr_geom_linkage
before any device work."""
import ctypes
import os
import re

import numpy as np
import pytest
from scipy.cluster import hierarchy as hac
from scipy.spatial.distance import squareform

import build_table
import geom_linkage_ref as gref
import linkage_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "hse_facerec_tf_amd", "csrc")
HEADER = os.path.join(ROOT, "include", "hsefr_geom.h")
NAMES = ["hsefr_geom_last_error", "hsefr_geom_linkage", "hsefr_geom_version"]


# ---- the restatement is scipy ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", gref.DENSE_DS)
@pytest.mark.parametrize("n", gref.DENSE_NS)
def test_the_closest_pair_restatement_is_scipy_bit_for_bit(n, d):
    """A guard on the GPU suite's REFERENCE (it passes without the library): on every dense input of that suite the primitive algorithm
    with the tie order (distance, lower slot, higher slot) gives scipy's Z bit for bit, inversions included."""
    from hse_facerec_tf_amd import clustering
    D = gref.euclidean(n, d, gref.case_seed(n, d))
    for method in ("centroid", "median"):
        a, b, h, clamps = gref.closest_pair_sequence(D, method, return_clamps=True)
        assert np.array_equal(clustering.linkage_from_sequence(a, b, h, n), hac.linkage(squareform(D, checks=False), method)), method
        assert clamps == 0                               # the merged pair is the least entry: no radicand of a real matrix is negative


@pytest.mark.parametrize("d", gref.DENSE_DS)
@pytest.mark.parametrize("n", gref.DENSE_NS + gref.WARD_EXTRA_NS)
def test_the_ward_rounds_restatement_is_scipys_tree(n, d):
    """The same guard for Ward: reciprocal-nearest-neighbour rounds with the three-term rule, two pairs of a round applied one after
    the other, give scipy's ids and sizes, and its heights at the bar test_means_dense_match_scipy sets for the two means."""
    from hse_facerec_tf_amd import clustering
    D = gref.euclidean(n, d, gref.case_seed(n, d))
    a, b, h, r, clamps = gref.ward_rounds(D, return_clamps=True)
    Z = clustering.linkage_from_merges(a, b, h, r, n)
    Zs = hac.linkage(squareform(D, checks=False), "ward")
    assert np.array_equal(Z[:, [0, 1, 3]], Zs[:, [0, 1, 3]])
    assert np.allclose(Z[:, 2], Zs[:, 2], rtol=1e-12, atol=0)
    assert clamps == 0
    if n >= 64:
        assert r.max() + 1 < n // 2                      # rounds, not steps: many pairs merge at once


def test_centroid_trees_of_the_suite_have_inversions():
    D = gref.euclidean(129, 16, gref.case_seed(129, 16))
    for method in ("centroid", "median"):
        h = gref.closest_pair_sequence(D, method)[2]
        assert (np.diff(h) < 0).sum() >= 10, method


def test_the_clamp_case_is_one_scipy_does_not_survive():
    """The GPU suite's clamp input: what the seeded search finds first, a matrix on which the restatement clamps a radicand.  scipy's
    sqrt gives NaN there; scipy 1.15's centroid search then refuses the matrix (find_min_dist) where older ones returned the NaN."""
    assert gref.clamp_search(gref.CLAMP_CASE[0])[0] == gref.CLAMP_CASE[1]
    D = gref.clamp_case()
    assert D.shape[0] <= 8 and np.array_equal(D, D.T) and (D < 0).any()
    a, b, h, clamps = gref.closest_pair_sequence(D, "centroid", return_clamps=True)
    assert clamps > 0 and np.isfinite(h).all()
    try:
        Zs = hac.linkage(squareform(D, checks=False), "centroid")
    except ValueError as e:
        assert "NaN" in str(e)
    else:
        assert np.isnan(Zs).any()


# ---- linkage_from_sequence ---------------------------------------------------------------------------------------------------------
def test_linkage_from_sequence_keeps_the_order_and_a_falling_height():
    from hse_facerec_tf_amd import clustering
    # the second merge is lower than the first (an inversion) and stays second; ids are union-find's, the lower first
    Z = clustering.linkage_from_sequence([2, 0, 1], [3, 3, 3], [2.0, 1.5, 3.0], 4)
    assert Z.tolist() == [[2, 3, 2.0, 2], [0, 4, 1.5, 3], [1, 5, 3.0, 4]]
    # the same records in another order are another tree: nothing is sorted
    Z2 = clustering.linkage_from_sequence([0, 2, 1], [3, 3, 3], [1.5, 2.0, 3.0], 4)
    assert Z2.tolist() == [[0, 3, 1.5, 2], [2, 4, 2.0, 3], [1, 5, 3.0, 4]]
    assert clustering.linkage_from_sequence([], [], [], 1).shape == (0, 4)
    # either endpoint may be given first
    assert np.array_equal(clustering.linkage_from_sequence([3, 3, 3], [2, 0, 1], [2.0, 1.5, 3.0], 4), Z)


def test_sequence_records_are_checked():
    from hse_facerec_tf_amd import clustering
    with pytest.raises(ValueError):
        clustering.linkage_from_sequence([0], [1], [1.0], 4)                                    # too few records
    with pytest.raises(RuntimeError):
        clustering.linkage_from_sequence([0, 0, 1], [1, 2, 2], [1.0, 2.0, 3.0], 4)              # a cycle: point 3 never joins
    with pytest.raises(RuntimeError):
        clustering.linkage_from_sequence([0, 1, -1], [1, 2, 3], [1.0, 2.0, 3.0], 4)             # a record the device did not write
    with pytest.raises(RuntimeError):
        clustering.linkage_from_sequence([0, 1, 2], [1, 2, 4], [1.0, 2.0, 3.0], 4)


@pytest.mark.parametrize("method", ["centroid", "median"])
def test_flat_cuts_of_a_tree_with_inversions_are_scipys(method):
    from hse_facerec_tf_amd import clustering
    D = gref.euclidean(129, 16, gref.case_seed(129, 16))
    Z = clustering.linkage_from_sequence(*gref.closest_pair_sequence(D, method), 129)
    assert (np.diff(Z[:, 2]) < 0).any()
    ts = ref.gap_thresholds(Z[:, 2], np.quantile(Z[:, 2], [0.05, 0.2, 0.4, 0.6, 0.8, 0.95]), 1e-9) + [Z[:, 2].min() - 1, Z[:, 2].max() + 1]
    got = clustering.fcluster_distance(Z, ts)
    for t, lab in zip(ts, got):
        assert np.array_equal(ref.canonical(lab), ref.canonical(hac.fcluster(Z, t, "distance"))), t


# ---- names and pins ----------------------------------------------------------------------------------------------------------------
def no_device(monkeypatch):
    from hse_facerec_tf_amd import _lib

    def refuse(*a, **k):
        raise AssertionError("device work")
    for name in ("require_gpu", "lib", "geom_lib", "split_lib", "cuda_device"):
        monkeypatch.setattr(_lib, name, refuse)


def test_the_names_are_as_specified():
    from hse_facerec_tf_amd import clustering, ops
    assert clustering.GEOMETRIC_METHODS == ("centroid", "median", "ward")
    assert clustering.LINKAGE_METHODS == ("single", "average", "complete", "weighted")
    assert clustering.CLUSTER_METHODS == clustering.LINKAGE_METHODS + ("dbscan", "rankorder")
    assert ops.GEOM_METHODS == {"centroid": 0, "median": 1, "ward": 2}
    assert ops.LINK_METHODS == {"average": 0, "complete": 1, "weighted": 2}


@pytest.mark.parametrize("name", ["centroid", "median", "ward"])
def test_the_older_entry_points_still_refuse_the_three_names(monkeypatch, name):
    from hse_facerec_tf_amd import clustering
    no_device(monkeypatch)
    D = gref.euclidean(5, 2, 1)
    X = np.ones((5, 8), np.float32)
    for call in (lambda: clustering.linkage_dense(D, name), lambda: clustering.linkage(X, name),
                 lambda: clustering.get_facial_clusters(D, 0.5, method=name), lambda: clustering.cluster_faces(X, 0.5, method=name),
                 lambda: clustering.select_threshold([(X, [0, 0, 1, 1, 2])], name)):
        with pytest.raises(ValueError) as e:
            call()
        assert "average" in str(e.value) and "complete" in str(e.value) and "weighted" in str(e.value)


@pytest.mark.parametrize("bad", ["average", "single", "complete", "dbscan", "Ward", "", None])
def test_bad_names_raise_from_the_new_functions_before_any_device_work(monkeypatch, bad):
    from hse_facerec_tf_amd import clustering
    no_device(monkeypatch)
    D = gref.euclidean(5, 2, 1)
    X = np.ones((5, 8), np.float32)
    for call in (lambda: clustering.linkage_geometric_dense(D, bad), lambda: clustering.linkage_geometric(X, bad),
                 lambda: clustering.get_facial_clusters_geometric(D, 0.5, bad), lambda: clustering.cluster_faces_geometric(X, 0.5, bad),
                 lambda: clustering.get_facial_clusters_geometric(D[:1, :1], 0.5, bad)):
        with pytest.raises(ValueError) as e:
            call()
        assert "centroid" in str(e.value) and "median" in str(e.value) and "ward" in str(e.value)
    for good in clustering.GEOMETRIC_METHODS:
        for split in ("bogus", None):
            with pytest.raises(ValueError, match="split"):
                clustering.get_facial_clusters_geometric(D, 0.5, good, [0, 0, 1, 2, 3], split=split)
            with pytest.raises(ValueError, match="split"):
                clustering.cluster_faces_geometric(X, 0.5, good, all_indices=[0, 0, 1, 2, 3], split=split)
        bad_matrix = D.copy()
        bad_matrix[1, 2] = np.inf
        with pytest.raises(ValueError, match="non-finite"):
            clustering.linkage_geometric_dense(bad_matrix, good)
        with pytest.raises(ValueError, match="square"):
            clustering.linkage_geometric_dense(np.ones((3, 4)), good)
    with pytest.raises(ValueError) as e:
        clustering.threshold_sweep(X, [0, 0, 1, 1, 2], "bogus", [0.5])
    for name in clustering.CLUSTER_METHODS + clustering.GEOMETRIC_METHODS:                      # the error names every method
        assert name in str(e.value)


# ---- the library -------------------------------------------------------------------------------------------------------------------
def test_header_library_and_binding_agree():
    from hse_facerec_tf_amd import _lib, ops
    header = open(HEADER).read()
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    assert sorted(_lib.GEOM_SIGNATURES) == NAMES
    args = re.search(r"int hsefr_geom_linkage\((.*?)\);", code, flags=re.S).group(1)
    assert len(args.split(",")) == len(_lib.GEOM_SIGNATURES["hsefr_geom_linkage"][1]) == 14
    assert int(re.search(r"#define HSEFR_GEOM_LDS_MAX (\d+)", header).group(1)) == ops.GEOM_LDS_MAX == 128
    assert {ops.GEOM_LDS_MAX - 1, ops.GEOM_LDS_MAX, ops.GEOM_LDS_MAX + 1} <= set(gref.DENSE_NS)      # the GPU suite stands on both sides
    enum = re.search(r"enum \{ HSEFR_GEOM_CENTROID = (\d), HSEFR_GEOM_MEDIAN = (\d), HSEFR_GEOM_WARD = (\d) \};", header).groups()
    assert [int(v) for v in enum] == [ops.GEOM_METHODS[m] for m in ("centroid", "median", "ward")]


def test_the_rounds_and_the_matrix_are_compiled_twice_not_written_twice():
    """Ward's rounds, the matrix build and the row rescan are hier_linkage.hip's, compiled into this library under one macro; without the
    macro that file is what libhsefr.so has always compiled."""
    table = build_table.rows()
    assert table["geom"]["srcs"] == ["geom_linkage.hip", "hier_linkage.hip"] and "hier_linkage.hip" in table["hsefr"]["srcs"]
    assert "-DHSEFR_GEOM_LIB" in table["geom"]["flags"] and "-DHSEFR_GEOM_LIB" not in table["hsefr"]["flags"]
    assert [f for f in table["geom"]["flags"] if f != "-DHSEFR_GEOM_LIB"] == table["hsefr"]["flags"]
    assert build_table.stale_against("geom", "linkage_scan.h", "mfma_dot.h", "common.h", "hier_build.h", "geom_rules.h", "include/hsefr.h",
                                     "include/hsefr_geom.h")
    assert table["geom"]["lint"] == "1"
    geom = open(os.path.join(CSRC, "geom_linkage.hip")).read()
    assert '#include "hier_build.h"' in geom and "build_working_matrix(" in geom and "rescan_rows(" in geom and "launch_ward_linkage(" in geom
    assert "feat_tile" not in geom and "hl_rescan_kernel" not in geom and "HSEFR_KNOB" not in geom
    for word in ("cooperative", "__threadfence", "while (atomic", "volatile"):
        assert word not in geom.split('#include <math.h>')[1], word          # no grid barrier, no spin-wait between workgroups
    # every line the macro adds to the shared sources stands between #ifdef HSEFR_GEOM_LIB (or the #else of an #ifndef) and its #endif
    src = open(os.path.join(CSRC, "hier_linkage.hip")).read()
    assert src.count("#ifdef HSEFR_GEOM_LIB") + src.count("#ifndef HSEFR_GEOM_LIB") == src.count("#endif") >= 8
    assert "geom::ward(" in src and "geom::" not in re.sub(r"#ifdef HSEFR_GEOM_LIB.*?#endif", "", re.sub(
        r"#ifndef HSEFR_GEOM_LIB(.*?)#else.*?#endif", r"\1", src, flags=re.S), flags=re.S)
    rules = open(os.path.join(CSRC, "geom_rules.h")).read()
    assert rules.count("#pragma clang fp contract(off)") == 3


def test_geom_linkage_checks_its_arguments_without_a_gpu():
    from hse_facerec_tf_amd import _lib
    L = _lib.geom_lib()
    buf = ctypes.create_string_buffer(4096)
    p = ctypes.cast(buf, ctypes.c_void_p).value
    ok = dict(x=p, n=4, d=8, born=None, year=None, dense=None, method=0, ma=p + 512, mb=p + 1024, mh=p + 1536, mr=p + 2048)

    def call(**kw):
        a = dict(ok, **kw)
        return L.hsefr_geom_linkage(a["x"], a["n"], a["d"], a["born"], a["year"], a["dense"], a["method"], a["ma"], a["mb"], a["mh"], a["mr"],
                                    None, None, None)

    def refused(kw, word):
        rc, msg = call(**kw), _lib.geom_last_error()
        assert rc == _lib.ERR_INVALID and "geom_linkage" in msg and word in msg, (kw, rc, msg)
    for n in (0, -3):
        refused(dict(n=n), "n=")
    refused(dict(dense=p + 2560), "exactly one")                                        # both sources
    refused(dict(x=None), "exactly one")                                                # neither
    for d in (0, 4, 12, -8):
        refused(dict(d=d), "multiple of 8")
    refused(dict(born=p + 2560), "come together")
    refused(dict(year=p + 2560), "come together")
    refused(dict(x=None, dense=p + 2560, born=p + 3072, year=p + 3584), "features path")
    for method in (3, -1, 100):
        refused(dict(method=method), "method=%d" % method)
    for out in ("ma", "mb", "mh", "mr"):
        for method in (0, 1, 2):
            refused({out: None, "method": method}, "null pointer")
    with pytest.raises(ValueError, match="method=3"):
        _lib.geom_check(call(method=3), "hsefr_geom_linkage")
