"""GPU suite: mean-shift clustering on the device (libhsefr_shift.so through ops.mean_shift_fit / mean_shift_assign and clustering's
entry points) against scikit-learn's recorded answers (tests/golden/mean_shift.npz) and the fp64 NumPy restatement
(tests/mean_shift_ref.py), which tests/test_mean_shift_cpu.py holds to scikit-learn.  A case is compared only after its margins prove
it decidable: the restatement's member margin against 100 x the bound the header states for the device's distance."""
import numpy as np
import pytest

import mean_shift_cases as cases
import mean_shift_ref as ref

pytestmark = pytest.mark.gpu

GOLDEN = cases.load_golden()
IDS = [cases.case_id(case) for case, _ in GOLDEN]
SHIFTING = [g for g in GOLDEN if g[0][2] == 32]          # the group whose seeds stop at different times: 8-9 iterations
# the device's fp64 arithmetic moves a shift, a centre distance or a label distance by parts in 1e-13 of values of order 1: a comparison
# the restatement decides by 1e-9 or more is the device's too
DECIDED = 1e-9
_RESULTS = {}


def restated(key, X, h, max_iter=300):
    """the restatement of an input, computed once per module run and never changed"""
    if key not in _RESULTS:
        _RESULTS[key] = ref.mean_shift(X, h, max_iter)
    return _RESULTS[key]


def shape_features(n, d):
    X = cases.features(16, 30, d, 0.5, 1000 * n + d)
    assert len(X) >= n
    return np.ascontiguousarray(X[:n])


def fit(X, h, max_iter=300, **kw):
    import torch
    from hse_facerec_tf_amd import ops
    centers, intensity, labels, dist, info = ops.mean_shift_fit(torch.from_numpy(X).cuda(), h, max_iter, **kw)
    return centers.cpu().numpy(), intensity.cpu().numpy(), labels.cpu().numpy().astype(np.int64), dist.cpu().numpy(), info


def decidable(r, X, h):
    from hse_facerec_tf_amd import ops
    norm = float(np.linalg.norm(X.astype(np.float64), axis=1).max())                # a mean is no longer than the longest row
    bound = ops.mean_shift_distance_bound(X.shape[1] + (-X.shape[1]) % 4, h, norm, norm)
    assert r.margins.member > 100 * bound, (r.margins.member, bound)
    assert min(r.margins.shift, r.margins.centre, r.margins.label) > DECIDED, r.margins
    return bound


def check(X, h, r, got, max_iter=300):
    centers, intensity, labels, dist, info = got
    print("n=%d d=%d: centres %d (distinct means %d), n_iter %d, work %d, |centres - ref| %.2e, |dist - ref| %.2e"
          % (X.shape[0], X.shape[1], info["centers"], info["distinct"], info["n_iter"], info["work"],
             np.abs(centers - r.centers).max() if centers.shape == r.centers.shape else np.nan, np.abs(dist - r.label_dist).max()))
    assert info["nonfinite"] == 0 and info["internal"] == 0
    assert info["n_iter"] == r.n_iter
    assert info["centers"] == len(r.centers) == len(centers) and info["distinct"] == r.distinct
    assert np.array_equal(intensity, r.intensity)
    assert np.array_equal(labels, r.labels)
    assert np.abs(centers - r.centers).max() <= 1e-12
    assert np.abs(dist - r.label_dist).max() <= 1e-12
    assert info["max_iter"] == r.stopped_by_max_iter
    assert info["work"] == int((r.completed + 1).sum())                             # a seed is launched once more than it completes


# ---- the recorded cases ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case,want", GOLDEN, ids=IDS)
def test_recorded_cases_are_scikit_learns(case, want):
    X, h = cases.case_features(case), case[3]
    r = restated(case, X, h)
    assert tuple(r.margins) == want["margins"]
    decidable(r, X, h)
    got = fit(X, h)
    assert np.array_equal(got[2], want["labels"]) and got[4]["n_iter"] == want["n_iter"] and got[4]["centers"] == want["centers"]
    check(X, h, r, got)
    assert got[4]["max_iter"] == 0


@pytest.mark.parametrize("case,want", SHIFTING, ids=[cases.case_id(c) for c, _ in SHIFTING])
def test_the_active_list_shrinks(case, want):
    """seeds stop at different times: the iterations launch over fewer and fewer, and the work done is the sum of what each completed"""
    X, h = cases.case_features(case), case[3]
    r = restated(case, X, h)
    info = fit(X, h)[4]
    assert info["n_iter"] == r.n_iter >= 8 and info["max_iter"] == 0
    assert len(np.unique(r.completed)) >= 4
    assert info["work"] == int(r.completed.sum()) + len(X) < (r.n_iter + 1) * len(X) * 0.6


# ---- shapes where the bit rows and the tiles can go wrong --------------------------------------------------------------------------------
@pytest.mark.parametrize("d", [4, 8, 36])
@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 129])
def test_shapes_at_the_edges_of_words_and_tiles(n, d):
    X = shape_features(n, d)
    r = restated(("shape", n, d), X, 0.7)
    decidable(r, X, 0.7)
    check(X, 0.7, r, fit(X, 0.7))


def test_a_width_that_is_no_multiple_of_four_is_padded():
    X = np.ascontiguousarray(shape_features(65, 8)[:, :6])
    X /= np.linalg.norm(X, axis=1, keepdims=True)
    r = restated(("shape6",), X, 0.7)
    decidable(r, X, 0.7)
    got = fit(X, 0.7)
    assert got[0].shape[1] == 6
    check(X, 0.7, r, got)


# ---- special inputs ----------------------------------------------------------------------------------------------------------------------
def test_an_isolated_face_stops_at_once():
    X = shape_features(64, 8).copy()
    X[17] = 0
    X[17, 3] = 25.0                                                                  # farther than the bandwidth from every other face
    r = restated(("isolated",), X, 0.7)
    decidable(r, X, 0.7)
    assert r.completed[17] == 0
    got = fit(X, 0.7)
    check(X, 0.7, r, got)
    c = int(got[2][17])
    assert got[1][c] == 1 and np.array_equal(got[0][c], X[17].astype(np.float64)) and got[3][17] == 0.0
    assert (got[2] == c).sum() == 1


@pytest.mark.parametrize("n", [1, 5, 64, 130])
def test_identical_rows_are_one_centre(n):
    row = shape_features(2, 36)[1]
    X = np.ascontiguousarray(np.tile(row, (n, 1)))
    centers, intensity, labels, dist, info = fit(X, 0.7)
    assert info["centers"] == 1 == info["distinct"] and info["n_iter"] == 0 and info["work"] == n and info["max_iter"] == 0
    assert intensity.tolist() == [n] and labels.tolist() == [0] * n
    assert np.array_equal(centers[0], row.astype(np.float64)) and (dist == 0).all()  # n equal fp32 values sum exactly in fp64


def test_two_identical_rows_inside_a_group_collapse():
    X = shape_features(65, 8).copy()
    X[40] = X[3]
    r = restated(("twins",), X, 0.7)
    decidable(r, X, 0.7)
    got = fit(X, 0.7)
    check(X, 0.7, r, got)
    assert r.distinct < len(X) and got[2][40] == got[2][3] and got[3][40] == got[3][3]


@pytest.mark.parametrize("max_iter", [0, 1])
def test_max_iter_is_scikit_learns(max_iter):
    """completed iterations == max_iter stops a seed after its mean update: max_iter = 0 is one update of every seed"""
    case = SHIFTING[0][0]
    X, h = cases.case_features(case), case[3]
    r = restated((case, max_iter), X, h, max_iter)
    decidable(r, X, h)
    assert r.n_iter == max_iter and r.stopped_by_max_iter > 0
    got = fit(X, h, max_iter)
    check(X, h, r, got, max_iter)
    assert got[4]["work"] <= (max_iter + 1) * len(X)


def test_cluster_all_false_marks_the_faces_beyond_the_bandwidth():
    from hse_facerec_tf_amd import clustering
    case = SHIFTING[1][0]
    X, h = cases.case_features(case), case[3]
    want = ref.mean_shift(X, h, cluster_all=False)
    assert (want.labels < 0).sum() >= 1 and np.abs(want.label_dist - h).min() > DECIDED
    centers, labels, n_iter = clustering.mean_shift(X, h, cluster_all=False)
    assert np.array_equal(labels, want.labels) and labels.dtype == np.int64 and n_iter == want.n_iter
    assert centers.dtype == np.float64 and np.abs(centers - want.centers).max() <= 1e-12
    every = clustering.mean_shift(X, h)[1]
    assert (every >= 0).all() and np.array_equal(every[labels >= 0], labels[labels >= 0])


def test_an_exact_intensity_tie_is_ordered_by_the_coordinates():
    G = shape_features(63, 8)[:20].copy()
    G[:, 0] = np.abs(G[:, 0]) + 2.0                                                  # one group, far on one side
    X = np.ascontiguousarray(np.concatenate([G, -G]))                                # and its mirror image: equal counts
    r = restated(("mirror",), X, 0.7)
    decidable(r, X, 0.7)
    assert len(set(r.intensity.tolist())) < len(r.intensity)                         # a tie among the centres
    assert r.centers[0, 0] > 0 and r.intensity[0] == r.intensity[1] and r.centers[1, 0] < 0
    check(X, 0.7, r, fit(X, 0.7))


def test_two_runs_give_identical_bytes():
    case = GOLDEN[12][0]
    X, h = cases.case_features(case), case[3]
    a, b = fit(X, h), fit(X, h)
    for u, v in zip(a[:4], b[:4]):
        assert u.tobytes() == v.tobytes()
    assert a[4] == b[4]


# ---- inputs and guards -------------------------------------------------------------------------------------------------------------------
def test_inputs_and_guards():
    import torch
    from hse_facerec_tf_amd import _lib, ops
    X = shape_features(65, 8)
    x = torch.from_numpy(X).cuda()
    before = x.clone()
    ops.mean_shift_fit(x, 0.7)
    assert torch.equal(x, before)                                                    # x is not written
    bad = x.clone()
    bad[33, 5] = float("nan")
    info = torch.full((8,), -1, dtype=torch.int32, device="cuda")
    with pytest.raises(ValueError, match="non-finite"):
        ops.mean_shift_fit(bad, 0.7, info=info)
    assert info.cpu().tolist() == [0, 0, 0, 0, 1, 0, 0, 0]
    bad[33, 5] = float("inf")
    with pytest.raises(ValueError, match="non-finite"):
        ops.mean_shift_fit(bad, 0.7)
    need = _lib.shift_lib().hsefr_shift_workspace_bytes(65, 8)
    with pytest.raises(ValueError, match="%d needed" % need):
        ops.mean_shift_fit(x, 0.7, workspace=torch.empty((need - 1,), dtype=torch.uint8, device="cuda"))
    r = restated(("shape", 65, 8), X, 0.7)
    ws = torch.full((need,), 0xAB, dtype=torch.uint8, device="cuda")                # exactly enough, and full of rubbish
    got = ops.mean_shift_fit(x, 0.7, workspace=ws)
    assert np.array_equal(got[2].cpu().numpy(), r.labels)
    with pytest.raises(ValueError):
        ops.mean_shift_fit(x.double(), 0.7)
    with pytest.raises(NotImplementedError, match="max_iter"):
        ops.mean_shift_fit(x, 0.7, max_iter=10001)


# ---- predict -----------------------------------------------------------------------------------------------------------------------------
def test_predict_is_the_nearest_centre():
    from hse_facerec_tf_amd import clustering
    case = GOLDEN[1][0]
    X, h = cases.case_features(case), case[3]
    r = restated(case, X, h)
    centers, labels, _ = clustering.mean_shift(X, h)
    assert np.array_equal(clustering.mean_shift_predict(X, centers), labels)         # the training rows get their labels
    Q = cases.features(case[0], case[1], case[2], case[4], 77)                       # held-out rows: other identities, same recipe
    want, want_dist = ref.nearest_center(Q, r.centers)
    two = np.sort(ref._dist(Q.astype(np.float64), r.centers), axis=1)[:, :2]
    assert (two[:, 1] - two[:, 0]).min() > DECIDED
    assert np.array_equal(clustering.mean_shift_predict(Q, centers), want)
    import torch
    from hse_facerec_tf_amd import ops
    lab, dist = ops.mean_shift_assign(torch.from_numpy(Q).cuda(), torch.from_numpy(r.centers).cuda())
    assert np.array_equal(lab.cpu().numpy(), want) and np.abs(dist.cpu().numpy() - want_dist).max() <= 1e-12
    one = clustering.mean_shift_predict(Q[:1], r.centers[:1])                        # one row, one centre
    assert one.tolist() == [0]


# ---- the reference's result form -----------------------------------------------------------------------------------------------------------
def test_cluster_faces_mean_shift_is_the_references_list_form():
    from hse_facerec_tf_amd import clustering
    case, want = GOLDEN[0]
    X, h = cases.case_features(case), case[3]
    lists = ref.cluster_lists(want["labels"])                                        # from scikit-learn's labels
    assert clustering.cluster_faces_mean_shift(X, h) == lists
    assert clustering.cluster_faces_mean_shift(X, h, min_cluster_size=5) == [c for c in lists if len(c) >= 5]
    photo = np.arange(len(X)) % 9                                                    # nine photos: most clusters hold two faces of one
    D = ref._dist(X.astype(np.float64), X.astype(np.float64))
    by_label = [np.flatnonzero(want["labels"] == c) for c in range(int(want["labels"].max()) + 1)]
    parts = clustering._split_groups(by_label, photo, len(X), lambda g: D[np.ix_(g, g)])
    expected = [[int(i) for i in p] for p in parts]
    expected.sort(key=len, reverse=True)
    assert len(expected) > len(lists)
    assert clustering.cluster_faces_mean_shift(X, h, all_indices=photo) == expected
    assert clustering.cluster_faces_mean_shift(X, h, all_indices=photo, split="device") == expected


def test_mean_shift_scores_are_clustering_scores_of_the_labels():
    from hse_facerec_tf_amd import clustering
    case = GOLDEN[2][0]
    X = cases.case_features(case)
    y = np.arange(len(X)) // 9                                                       # any labelling: they are compared for equality only
    bandwidths = [0.5, 0.7, 1.1]
    rows = clustering.mean_shift_scores(X, y, bandwidths)
    assert rows.shape == (3, len(clustering.STATS_NAMES))
    for row, b in zip(rows, bandwidths):
        assert np.array_equal(row, clustering.clustering_scores(y, clustering.mean_shift(X, b)[1]))
    assert len({tuple(r) for r in rows}) > 1
