"""GPU suite: affinity-propagation clustering on the device (libhsefr_affinity.so through ops.affinity_propagation_fit and clustering's
entry points) against scikit-learn's recorded answers on fp64 input (tests/golden/affinity.npz) and the fp64 NumPy restatement
(tests/affinity_ref.py), which tests/test_affinity_cpu.py holds to scikit-learn.  A case is compared only after its margins prove it
decidable: the recorded least |A_kk + R_kk| and assignment gap against 100 x the bound the header states for the messages.  Label
numbers and exemplars of tied clusters depend on scikit-learn's unseeded noise: partitions are compared, not label numbers."""
import warnings

import numpy as np
import pytest

import affinity_cases as cases
import affinity_ref as ref

pytestmark = pytest.mark.gpu

GOLDEN, STEPS = cases.load_golden()
IDS = [cases.case_id(case) for case, _ in GOLDEN]
S_MAX = 4.0 * (1 + 1e-6)        # |S_ij| <= (|x_i| + |x_j|)^2 of rows normalised in float32, and the median preference lies among them
_RESULTS = {}


def restated(key, make):
    """a restatement computed once per module run and never changed"""
    if key not in _RESULTS:
        _RESULTS[key] = make()
    return _RESULTS[key]


def fit(X=None, S=None, **kw):
    import torch
    from hse_facerec_tf_amd import ops
    source = dict(x=torch.from_numpy(X).cuda()) if X is not None else dict(S=torch.from_numpy(np.ascontiguousarray(S, np.float64)).cuda())
    exemplars, labels, diag, pref, info = ops.affinity_propagation_fit(**source, **kw)
    return exemplars.cpu().numpy().astype(np.int64), labels.cpu().numpy().astype(np.int64), diag.cpu().numpy(), pref, info


def valid(got, n):
    """what every answer satisfies: the exemplars ascending, each a member of the cluster it names, labels their positions"""
    exemplars, labels, diag, pref, info = got
    K = info["clusters"]
    assert info["nonfinite"] == 0 and info["internal"] == 0 and len(exemplars) == K and len(labels) == n == len(diag)
    if K == 0:
        assert (labels == -1).all()
        return
    assert (np.diff(exemplars) > 0).all() and exemplars[0] >= 0 and exemplars[-1] < n
    assert labels.min() >= 0 and labels.max() < K
    assert np.array_equal(labels[exemplars], np.arange(K))
    assert np.isfinite(diag).all() and np.isfinite(pref)


def bound_for(X):
    from hse_facerec_tf_amd import ops
    assert float(np.linalg.norm(X.astype(np.float64), axis=1).max()) <= 1 + 2.5e-7
    return ops.affinity_message_bound(X.shape[0], X.shape[1] + (-X.shape[1]) % 4, S_MAX)


# ---- 1. the recorded cases ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", [0, None], ids=["seed0", "noiseless"])
@pytest.mark.parametrize("case,want", GOLDEN, ids=IDS)
def test_recorded_cases_are_scikit_learns(case, want, seed):
    X = cases.case_features(case)
    bound = bound_for(X)
    print("%s: margins diag %.2e assign %.2e, 100 x bound %.2e" % (cases.case_id(case), want["margin_diag"], want["margin_assign"], 100 * bound))
    assert want["margin_diag"] >= 100 * bound and want["margin_assign"] >= 100 * bound
    got = fit(X, seed=seed)
    valid(got, len(X))
    exemplars, labels, diag, pref, info = got
    print("    device: K %d, n_iter %d, converged %d, least |diag| %.2e" % (info["clusters"], info["n_iter"], info["converged"], np.abs(diag).min()))
    assert np.array_equal(ref.first_occurrence(labels), want["partition"])
    assert (info["n_iter"], info["clusters"], info["converged"], info["equal"]) == (want["n_iter"], want["clusters"], 1, 0)
    assert (diag > 0).sum() == want["clusters"] and np.abs(diag).min() >= want["margin_diag"] - bound


# ---- 2. the exemplars ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [0, 2, 4, 9], ids=[IDS[k] for k in (0, 2, 4, 9)])
def test_exemplars_are_scikit_learns_where_the_refinement_is_decidable(k):
    case, want = GOLDEN[k]
    X = cases.case_features(case)
    bound = bound_for(X)
    r = restated(("hashed", k), lambda: ref.fit_features(X, seed=0))
    got = fit(X, seed=0)
    valid(got, len(X))
    exemplars, labels = got[0], got[1]
    assert np.array_equal(ref.first_occurrence(labels), want["partition"])
    undecided = 0
    for c, e in enumerate(want["exemplars"]):
        mine = exemplars[labels[e]]                                       # the device's exemplar of the cluster scikit-learn's e lies in
        if want["refinement_decidable"][c]:
            assert mine == e
            continue
        undecided += 1
        members, sums = r.member_sums[r.first_labels[e]]                  # the restatement's member sums of that cluster
        assert mine in members
        assert sums.max() - sums[list(members).index(mine)] <= bound
    assert undecided == (~want["refinement_decidable"]).sum()


# ---- 3. exact arithmetic --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [70, 257, 2100])
def test_small_integers_give_the_restatements_bits(n):
    """every operation is exact in fp64 (small integers, damping 0.5, eight iterations: multiples of 2^-16 below 2^18), so the order of
    the column sums does not matter and the device must give NumPy's bits: what a wrong update rule cannot pass.  2100 points are past
    2048, where the sweep kernel's other instance (1024 threads, 16 columns a thread) takes over"""
    rs = np.random.RandomState(n)
    S = -rs.randint(1, 40, (n, n)).astype(np.float64)                     # asymmetric, heavily tied
    r = ref.affinity_propagation(S, damping=0.5, max_iter=8, convergence_iter=64)
    assert r.n_iter == 8 and not r.converged and len(r.exemplars) >= 1
    got = fit(S=S, damping=0.5, max_iter=8, convergence_iter=64, seed=None)
    valid(got, n)
    exemplars, labels, diag, pref, info = got
    assert pref == r.preference == np.median(S)
    assert (diag + 0.0).tobytes() == (r.diag + 0.0).tobytes()
    assert np.array_equal(exemplars, r.exemplars) and np.array_equal(labels, r.labels)
    assert (info["n_iter"], info["converged"], info["clusters"]) == (8, 0, len(r.exemplars))


# ---- 4. the median and the dense path -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [11, 12, 64])
def test_the_preference_is_numpys_median(n):
    S = np.random.RandomState(n).standard_normal((n, n)) * 3.0
    pref = fit(S=S, max_iter=1, seed=None)[3]
    assert np.float64(pref).tobytes() == np.float64(np.median(S)).tobytes()


def test_the_median_of_heavily_tied_integers_and_an_explicit_preference():
    rs = np.random.RandomState(3)
    S = -rs.randint(0, 4, (50, 50)).astype(np.float64)
    assert np.float64(fit(S=S, max_iter=1, seed=None)[3]).tobytes() == np.float64(np.median(S)).tobytes()
    S[:, :26] = -2.0
    S[:, 26:] = -1.0                                                       # 1300 and 1200 of 2500: both middle entries are -2
    assert fit(S=S, max_iter=1, seed=None)[3] == np.median(S) == -2.0
    S[:, :25] = -2.0
    S[:, 25:] = -1.0                                                       # 1250 each: the mean of the two middle entries
    assert fit(S=S, max_iter=1, seed=None)[3] == np.median(S) == -1.5
    before = S.copy()
    got = fit(S=S, max_iter=3, preference=-7.25, seed=None)
    assert got[3] == -7.25 and np.array_equal(S, before)


def test_an_asymmetric_dense_matrix_matches_the_restatement():
    from hse_facerec_tf_amd import clustering, ops
    rs = np.random.RandomState(5)
    X = cases.case_features(cases.CASES[7])
    S = ref.similarities(X) * (1.0 + 0.05 * rs.uniform(size=(len(X), len(X))))
    assert not np.array_equal(S, S.T)
    for seed in (None, 0):
        r = ref.affinity_propagation(S, seed=seed)
        assert min(r.margins.diag, r.margins.assign) >= 100 * ops.affinity_message_bound(len(X), 4, np.abs(S).max())
        got = fit(S=S, seed=seed)
        valid(got, len(X))
        assert np.array_equal(ref.first_occurrence(got[1]), ref.first_occurrence(r.labels))
        assert (got[4]["n_iter"], got[4]["clusters"], got[4]["converged"]) == (r.n_iter, len(r.exemplars), 1)
        assert got[3] == r.preference == np.median(S)
        assert np.abs(got[2] - r.diag).max() <= ops.affinity_message_bound(len(X), 4, np.abs(S).max())
    ex, labels, n_iter = clustering.affinity_propagation_dense(S)
    assert np.array_equal(labels, got[1]) and np.array_equal(ex, got[0]) and n_iter == r.n_iter and labels.dtype == np.int64


# ---- 5. the paths that do not converge ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("max_iter", cases.STEPS)
def test_the_recorded_steps(max_iter):
    from hse_facerec_tf_amd import clustering
    want = STEPS[max_iter]
    X = cases.case_features(cases.CASES[cases.STEPS_CASE])
    assert min(want["margin_diag"], want["margin_assign"]) >= 100 * bound_for(X)
    got = fit(X, max_iter=max_iter, seed=None)
    valid(got, len(X))
    assert (got[4]["n_iter"], got[4]["converged"], got[4]["clusters"], got[4]["equal"]) == (max_iter, 0, len(want["exemplars"]), 0)
    if len(want["exemplars"]) == 0:
        assert (got[1] == -1).all() and max_iter == 1
    else:
        assert np.array_equal(ref.first_occurrence(got[1]), ref.first_occurrence(want["labels"]))
    with pytest.warns(clustering.ConvergenceWarning, match="did not converge"):
        ex, labels, n_iter = clustering.affinity_propagation(X, max_iter=max_iter, seed=None)
    assert np.array_equal(labels, got[1]) and np.array_equal(ex, got[0]) and n_iter == max_iter


# ---- 6. degenerate inputs -------------------------------------------------------------------------------------------------------------------
def test_degenerate_inputs():
    import torch
    from hse_facerec_tf_amd import ops
    one = fit(np.ones((1, 4), np.float32))
    assert one[0].tolist() == [0] and one[1].tolist() == [0] and one[3] == 0.0
    assert (one[4]["clusters"], one[4]["n_iter"], one[4]["converged"], one[4]["equal"]) == (1, 0, 1, 1)
    pair = np.array([[0, 0, 0, 0], [1, 0, 0, 0]], np.float32)
    two = fit(pair)                                                        # the median of (0, 0, -1, -1) exceeds S: every point its own exemplar
    assert two[3] == -0.5 and two[0].tolist() == [0, 1] and two[1].tolist() == [0, 1] and two[4]["equal"] == 1 and two[4]["n_iter"] == 0
    below = fit(pair, preference=-2.0)
    assert below[3] == -2.0 and below[0].tolist() == [0] and below[1].tolist() == [0, 0] and below[4]["clusters"] == 1
    same = fit(np.ones((3, 8), np.float32))
    assert same[0].tolist() == [0] and same[1].tolist() == [0, 0, 0] and same[3] == 0.0 and same[4]["equal"] == 1
    for got in (one, two, below, same):
        assert (got[2] == 0).all()
    bad = torch.from_numpy(cases.case_features(cases.CASES[8])).cuda()
    before = bad.clone()
    ops.affinity_propagation_fit(x=bad)
    assert torch.equal(bad, before)                                        # x is not written
    bad[33, 5] = float("nan")
    info = torch.full((8,), -1, dtype=torch.int32, device="cuda")
    with pytest.raises(ValueError, match="non-finite"):
        ops.affinity_propagation_fit(x=bad, info=info)
    assert info.cpu().tolist() == [0, 0, 0, 0, 1, 0, 0, 0]
    Sbad = torch.zeros((5, 5), dtype=torch.float64, device="cuda")
    Sbad[1, 2] = float("inf")
    with pytest.raises(ValueError, match="non-finite"):
        ops.affinity_propagation_fit(S=Sbad)
    with pytest.raises(ValueError, match="exactly one"):
        ops.affinity_propagation_fit(x=before, S=Sbad)
    with pytest.raises(NotImplementedError, match="max_iter"):
        ops.affinity_propagation_fit(x=before, max_iter=10001)


# ---- 7. duplicated rows ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", [0, None], ids=["seed0", "noiseless"])
def test_duplicated_rows_terminate_with_a_valid_answer(seed):
    """a third of the rows twice: scikit-learn disagrees with itself from seed to seed here, so the device is held to termination,
    determinism and a valid answer"""
    X = cases.duplicated(cases.case_features(cases.CASES[8]))
    assert len(X) == 65 + 22
    a, b = fit(X, seed=seed), fit(X, seed=seed)
    valid(a, len(X))
    assert 1 <= a[4]["n_iter"] <= 200 and (a[4]["converged"] == 1 or a[4]["n_iter"] == 200)
    for u, v in zip(a[:3], b[:3]):
        assert u.tobytes() == v.tobytes()
    assert a[3] == b[3] and a[4] == b[4]


# ---- 8. determinism ---------------------------------------------------------------------------------------------------------------------------
def test_two_runs_and_a_dirty_workspace_give_identical_bytes():
    import torch
    from hse_facerec_tf_amd import _lib
    X = cases.case_features(cases.CASES[4])
    need = _lib.affinity_lib().hsefr_affinity_workspace_bytes(len(X), X.shape[1])
    ws = torch.full((need,), 0xFF, dtype=torch.uint8, device="cuda")       # exactly enough, and full of rubbish
    a, b, c = fit(X), fit(X), fit(X, workspace=ws)
    for other in (b, c):
        for u, v in zip(a[:3], other[:3]):
            assert u.tobytes() == v.tobytes()
        assert a[3] == other[3] and a[4] == other[4]
    with pytest.raises(ValueError, match="%d needed" % need):
        fit(X, workspace=torch.empty((need - 1,), dtype=torch.uint8, device="cuda"))


# ---- 9. predict and the reference's result form -----------------------------------------------------------------------------------------------
def test_predict_is_the_nearest_centre():
    from hse_facerec_tf_amd import clustering
    case, want = GOLDEN[1]
    X = cases.case_features(case)
    ex, labels, n_iter = clustering.affinity_propagation(X)
    assert n_iter == want["n_iter"] and labels.dtype == np.int64 and ex.dtype == np.int64
    centers = X[ex].astype(np.float64)
    Q = cases.mean_shift_cases.features(case[0], case[1], case[2], case[3], 77)       # held-out rows: other identities, same recipe
    brute, D = ref.nearest_center(Q, centers)
    two = np.sort(D, axis=1)[:, :2]
    assert (two[:, 1] - two[:, 0]).min() > 1e-9
    assert np.array_equal(clustering.affinity_propagation_predict(Q, centers), brute)
    own, _ = ref.nearest_center(X, centers)
    assert np.array_equal(clustering.affinity_propagation_predict(X, centers), own)
    assert np.array_equal(clustering.affinity_propagation_predict(X[ex], centers), np.arange(len(ex)))
    assert clustering.affinity_propagation_predict(Q, np.zeros((0, X.shape[1]))).tolist() == [-1] * len(Q)


def test_cluster_faces_affinity_propagation_is_the_references_list_form():
    from hse_facerec_tf_amd import clustering
    case, want = GOLDEN[0]
    X = cases.case_features(case)
    _, labels, _ = clustering.affinity_propagation(X)
    assert np.array_equal(ref.first_occurrence(labels), want["partition"])
    lists = ref.cluster_lists(labels)
    assert clustering.cluster_faces_affinity_propagation(X) == lists
    assert clustering.cluster_faces_affinity_propagation(X, min_cluster_size=5) == [c for c in lists if len(c) >= 5]
    photo = np.arange(len(X)) % 9                                                    # nine photos: most clusters hold two faces of one
    X64 = X.astype(np.float64)
    D = np.sqrt(np.maximum(-ref.similarities(X), 0.0))
    by_label = [np.flatnonzero(labels == c) for c in range(int(labels.max()) + 1)]
    parts = clustering._split_groups(by_label, photo, len(X), lambda g: D[np.ix_(g, g)])
    expected = [[int(i) for i in p] for p in parts]
    expected.sort(key=len, reverse=True)
    assert len(expected) > len(lists) and len(X64) == sum(len(c) for c in expected)
    assert clustering.cluster_faces_affinity_propagation(X, all_indices=photo) == expected
    assert clustering.cluster_faces_affinity_propagation(X, all_indices=photo, split="device") == expected


def test_affinity_propagation_scores_are_clustering_scores_of_the_labels():
    from hse_facerec_tf_amd import clustering
    X = cases.case_features(cases.CASES[1])
    y = np.arange(len(X)) // 9
    preferences = [None, -0.5, -3.0]
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", clustering.ConvergenceWarning)
        rows = clustering.affinity_propagation_scores(X, y, preferences)
        assert rows.shape == (3, len(clustering.STATS_NAMES))
        for row, p in zip(rows, preferences):
            assert np.array_equal(row, clustering.clustering_scores(y, clustering.affinity_propagation(X, preference=p)[1]))
    assert len({tuple(r) for r in rows}) > 1
