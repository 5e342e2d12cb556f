"""GPU suite: the same-photo split of every cluster in one device pass (libhsefr_split.so, ops.split_groups,
clustering.split_same_photo, the ``split`` keyword of get_facial_clusters / cluster_faces / perform_clustering).

Dense source: exact, ties included -- the sublabels are clustering.complete_linkage_labels of the matrix built on the host, for every
size class of the chain, and scipy's partition.  Features source: the matrix the device built is symmetric, within 1e-4 of the fp64
distances (the bound tests/test_hier_linkage_gpu.py uses for this arithmetic), bit for bit the working matrix of hsefr_hier_linkage,
and the sublabels are the host replay on that very matrix, exactly.  Entry points: the device split gives the host split's clusters.
The host expectations are computed once per module and never changed."""

import numpy as np
import pytest

import group_split_cases as cases
from group_split_cases import CUT, PENALTY
from test_linkage_gpu import ages, as_partition, features, fp64_distances, random_matrix, reference_get_facial_clusters

pytestmark = pytest.mark.gpu


def run(members, offsets, photo, **kw):
    """ops.split_groups on host arrays -> host results (sublabel, then what was asked for)"""
    import torch
    from hse_facerec_tf_amd import ops
    dev = (kw.get("x") if kw.get("x") is not None else kw["dense"]).device
    out = ops.split_groups(torch.from_numpy(np.asarray(members, np.int32)).to(dev), offsets, torch.from_numpy(np.asarray(photo, np.int32)).to(dev),
                           **kw)
    out = out if isinstance(out, tuple) else (out,)
    return tuple(o.cpu().numpy() if hasattr(o, "cpu") else o for o in out)


def check_against_scipy(sub, P_of_group, offsets, cut=CUT):
    for g in range(len(offsets) - 1):
        got = sub[offsets[g]:offsets[g + 1]]
        assert np.array_equal(got, cases.scipy_partition(P_of_group(g), cut)), (g, int(offsets[g + 1] - offsets[g]))


# ---- dense source ----------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def dense_cases():
    """(D, members, offsets, photo, expected sublabels, chained) for the natural order over all points, and for shuffled groups over a
    non-contiguous subset"""
    out = {}
    for name, n, shuffled in (("natural", None, False), ("shuffled subset", sum(cases.SIZES) + 77, True)):
        members, offsets, n = cases.grouping(cases.SIZES, 5, n, shuffled)
        D = cases.integer_matrix(n, 6)
        photo = cases.photos_with_shared(members, offsets, n, 7)
        P_of = lambda g, D=D, members=members, offsets=offsets, photo=photo: cases.host_P(D, members[offsets[g]:offsets[g + 1]], photo)  # noqa: E731
        want, chained = cases.expected_sublabels(P_of, offsets)
        out[name] = (D, members, offsets, photo, P_of, want, chained)
    return out


@pytest.mark.parametrize("name", ["natural", "shuffled subset"])
def test_dense_sublabels_are_the_host_chain_in_every_size_class(dense_cases, name):
    import torch
    D, members, offsets, photo, P_of, want, chained = dense_cases[name]
    if name == "shuffled subset":
        assert any((np.diff(members[offsets[g]:offsets[g + 1]]) < 0).any() for g in range(len(offsets) - 1))
        assert len(np.unique(members)) == len(members) < D.shape[0]
    Dd = torch.from_numpy(D).cuda()
    sub, dist, stats = run(members, offsets, photo, dense=Dd, return_distances=True, return_stats=True)
    assert np.array_equal(sub, want)
    check_against_scipy(sub, P_of, offsets)
    # one wave, one workgroup in LDS, one workgroup on the slab: every class ran, and the groups that needed no chain did not
    k = np.diff(offsets)
    assert chained[(k > 2) & (k <= cases.WAVE_MAX)].any() and chained[(k > cases.WAVE_MAX) & (k <= cases.LDS_MAX)].all() and \
        chained[k > cases.LDS_MAX].all() and not chained[k == 1].any()
    assert stats.tolist() == cases.expected_stats(offsets, chained)
    at = 0
    for g in range(len(offsets) - 1):                                                  # the matrices as first built
        got, P = dist[at:at + k[g] ** 2].reshape(k[g], k[g]), P_of(g)
        off = ~np.eye(k[g], dtype=bool)
        assert np.array_equal(got[off], P[off]), g
        at += k[g] ** 2
    assert np.array_equal(Dd.cpu().numpy().view(np.uint64), D.view(np.uint64))           # the caller's matrix is read only
    again = run(members, offsets, photo, dense=Dd, return_distances=True, return_stats=True)
    assert sub.tobytes() == again[0].tobytes() and dist[np.isfinite(dist)].tobytes() == again[1][np.isfinite(again[1])].tobytes()
    assert np.array_equal(np.isfinite(dist), np.isfinite(again[1])) and again[2].tolist() == stats.tolist()


def test_dense_reads_the_upper_triangle_only():
    import torch
    members, offsets, n = cases.grouping([40, 7], 3)
    D = cases.integer_matrix(n, 4)
    photo = cases.photos_with_shared(members, offsets, n, 5)
    want, _ = cases.expected_sublabels(lambda g: cases.host_P(D, members[offsets[g]:offsets[g + 1]], photo), offsets)
    lower_is_garbage = np.triu(D) + np.tril(np.full_like(D, 1e9), -1)
    assert np.array_equal(run(members, offsets, photo, dense=torch.from_numpy(lower_is_garbage).cuda())[0], want)


def test_the_early_answer_the_plain_chain_and_the_all_in_one_photo_group():
    import torch
    sizes = [20, 20, 20, 70, 70, 200, 200]
    members, offsets, n = cases.grouping(sizes, 8)
    D = cases.integer_matrix(n, 9)
    photo = np.arange(n, dtype=np.int32)                                               # nobody shares a photo ...
    D[offsets[1] + 3, offsets[1] + 11] = 77.0                                          # ... group 1 has ONE distance above the cut,
    D[offsets[4] + 2, offsets[4] + 60] = 51.0                                          # and so have groups 4
    D[offsets[6] + 150, offsets[6] + 199] = 50.5                                       # and 6 (each in its chain class)
    photo[offsets[2]:offsets[3]] = 7                                                   # group 2 is ONE photo
    P_of = lambda g: cases.host_P(D, members[offsets[g]:offsets[g + 1]], photo)      # noqa: E731
    want, chained = cases.expected_sublabels(P_of, offsets)
    assert chained.tolist() == [False, True, True, False, True, False, True]
    sub, stats = run(members, offsets, photo, dense=torch.from_numpy(D).cuda(), return_stats=True)
    assert np.array_equal(sub, want)
    check_against_scipy(sub, P_of, offsets)
    assert stats.tolist() == cases.expected_stats(offsets, chained) and stats[0] == 3
    for g in (0, 3, 5):                                                                # no entry above the cut: one cluster, no chain
        assert not sub[offsets[g]:offsets[g + 1]].any()
    for g in (1, 4, 6):                                                                # one distance above it: the chain splits the two
        part = sub[offsets[g]:offsets[g + 1]]
        assert part.max() == 1
    assert sub[offsets[1] + 3] != sub[offsets[1] + 11] and sub[offsets[4] + 2] != sub[offsets[4] + 60]
    assert sub[offsets[6] + 150] != sub[offsets[6] + 199]
    assert np.array_equal(sub[offsets[2]:offsets[3]], np.arange(20))                   # one photo: k singletons


def test_negative_dense_entries():
    import torch
    members, offsets, n = cases.grouping([5, 33, 140], 10, shuffled=True)
    D = cases.integer_matrix(n, 11, lo=-9, hi=-1)
    photo = cases.photos_with_shared(members, offsets, n, 12, share=0.1)
    for penalty, cut in ((100.0, 50.0), (2.0, -4.0), (0.0, -2.5), (0.0, -0.5)):
        P_of = lambda g: cases.host_P(D, members[offsets[g]:offsets[g + 1]], photo, penalty)      # noqa: E731
        want, chained = cases.expected_sublabels(P_of, offsets, cut)
        sub, stats = run(members, offsets, photo, dense=torch.from_numpy(D).cuda(), penalty=penalty, cut=cut, return_stats=True)
        assert np.array_equal(sub, want), (penalty, cut)                               # (scipy refuses negative distances)
        assert stats.tolist() == cases.expected_stats(offsets, chained), (penalty, cut)
    assert not chained.any()                                                           # all entries below -0.5: every group answered early


def test_a_member_outside_the_points_is_answered_not_followed():
    """A member index of -1 and one of n, both in the second group: a bounds check answers that group with -1; the others are right."""
    import torch
    from hse_facerec_tf_amd import _lib, ops
    sizes = [6, 40, 3, 150]
    members, offsets, n = cases.grouping(sizes, 13)
    D = cases.integer_matrix(n, 14)
    photo = cases.photos_with_shared(members, offsets, n, 15)
    want, chained = cases.expected_sublabels(lambda g: cases.host_P(D, members[offsets[g]:offsets[g + 1]], photo), offsets)
    bad = members.copy()
    bad[offsets[1] + 5], bad[offsets[1] + 30] = -1, n
    want[offsets[1]:offsets[2]] = -1
    chained[1] = False
    Dd, mt, pt = torch.from_numpy(D).cuda(), torch.from_numpy(bad).cuda(), torch.from_numpy(photo).cuda()
    sub = torch.full((len(bad),), -7, dtype=torch.int32, device="cuda")
    stats = torch.full((5,), -7, dtype=torch.int64, device="cuda")
    rc = _lib.split_lib().hsefr_split_groups(None, n, 0, None, None, Dd.data_ptr(), mt.data_ptr(), offsets.ctypes.data, len(sizes), pt.data_ptr(),
                                             PENALTY, CUT, sub.data_ptr(), None, stats.data_ptr(), _lib.current_stream_ptr())
    assert rc == 0, _lib.split_last_error()
    assert np.array_equal(sub.cpu().numpy(), want)
    got = stats.cpu().numpy().tolist()
    assert got[4] == 2
    expect = cases.expected_stats(offsets, chained, bad=2)
    expect[0] -= 1                                                                     # the refused group is no early answer
    assert got == expect
    with pytest.raises(ValueError, match="outside"):
        ops.split_groups(mt, offsets, pt, dense=Dd, return_stats=True)
    assert np.array_equal(ops.split_groups(mt, offsets, pt, dense=Dd).cpu().numpy(), want)       # without stats: -1, no exception


# ---- features source -------------------------------------------------------------------------------------------------------------------
N_FEAT = 600
FEAT_SIZES = [150, 70, 40, 33, 32, 31] + [8] * 26 + [5] * 7 + [1]                      # 40 groups of 600 points


@pytest.mark.parametrize("age", [False, True])
@pytest.mark.parametrize("d", [8, 128, 1024])
def test_features_matrix_and_sublabels(d, age):
    import torch
    from hse_facerec_tf_amd import clustering, ops
    assert len(FEAT_SIZES) == 40 and sum(FEAT_SIZES) == N_FEAT
    X = features(N_FEAT, d, 21 + d)
    born, year = ages(N_FEAT, 22) if age else (None, None)
    members, offsets, _ = cases.grouping(FEAT_SIZES, 23, shuffled=True)
    photo = np.random.RandomState(24).randint(0, 200, N_FEAT).astype(np.int32)
    want64 = fp64_distances(X, born, year)
    x = torch.from_numpy(X).cuda()
    src = dict(x=x)
    if age:
        src.update(born=torch.from_numpy(born.astype(np.float32)).cuda(), year=torch.from_numpy(year.astype(np.float32)).cuda())
    k = np.diff(offsets)
    # the reference's penalty and cut (chains where photos are shared), and a cut inside the distances (chains everywhere)
    inside = float(np.median(want64[np.triu_indices(N_FEAT, 1)]))
    for penalty, cut in ((PENALTY, CUT), (0.25, inside)):
        sub, dist, stats = run(members, offsets, photo, penalty=penalty, cut=cut, return_distances=True, return_stats=True, **src)
        at, Ps = 0, []
        for g in range(len(k)):
            m = members[offsets[g]:offsets[g + 1]]
            P = dist[at:at + k[g] ** 2].reshape(k[g], k[g]).copy()
            at += k[g] ** 2
            np.fill_diagonal(P, 0.0)                                                   # (unspecified)
            assert np.array_equal(P, P.T), g
            want = cases.host_P(want64, m, photo, penalty)
            err = float(np.abs(P - want).max())
            print("d=%d age=%s group %d (k=%d): max |P - fp64| = %.3e" % (d, age, g, k[g], err))
            assert err < 1e-4, (g, err)
            Ps.append(P)
        want_sub, chained = cases.expected_sublabels(lambda g: Ps[g], offsets, cut)    # the same replay as on the dense source: exact
        assert np.array_equal(sub, want_sub), (penalty, cut)
        assert stats.tolist() == cases.expected_stats(offsets, chained)
    assert chained[k >= 31].all()
    # one group of all points in natural order, no penalty: the matrix is hsefr_hier_linkage's working matrix, bit for bit -- every
    # round-0 merge of complete linkage has its height there
    everyone, table = np.arange(N_FEAT, dtype=np.int32), np.array([0, N_FEAT], dtype=np.int64)
    _, whole = run(everyone, table, photo, penalty=0.0, cut=CUT, return_distances=True, **src)
    whole = whole.reshape(N_FEAT, N_FEAT)
    ma, mb, mh, mr = (t.cpu().numpy() for t in ops.hier_linkage_merges(method="complete", **src))
    first = mr == 0
    assert first.sum() >= 1
    assert np.array_equal(whole[ma[first], mb[first]].view(np.uint64), mh[first].view(np.uint64))
    assert np.array_equal(whole[mb[first], ma[first]].view(np.uint64), mh[first].view(np.uint64))
    assert clustering.SAME_PHOTO_PENALTY == PENALTY


# ---- entry points ----------------------------------------------------------------------------------------------------------------------
N_ENTRY = 301


@pytest.mark.parametrize("method", ["single", "average", "complete", "weighted"])
@pytest.mark.parametrize("ties", [True, False])
def test_get_facial_clusters_device_split_equals_the_host_split(ties, method):
    from hse_facerec_tf_amd import clustering
    D = random_matrix(N_ENTRY, 31, ties)
    photos = np.random.RandomState(32).randint(0, 100, N_ENTRY)
    # thresholds from one giant cluster (single linkage on a tied matrix at 0: a chain over 301 faces) to many small ones
    multi = 0
    for t in ([0, 1, 3] if ties else [0.02, 0.1, 0.4]):
        host = clustering.get_facial_clusters(D, t, photos, method=method, split="host")
        assert clustering.get_facial_clusters(D, t, photos, method=method) == host
        assert clustering.get_facial_clusters(D, t, photos, method=method, split="device") == host, t
        multi += sum(len(c) > 1 for c in host)
        for c in host:
            assert len(set(photos[c])) == len(c)
    assert multi > 0
    assert clustering.get_facial_clusters(D, 1, None, method=method, split="device") == clustering.get_facial_clusters(D, 1, None, method=method)


# chosen on the CPU so that the reference alone satisfies the precondition below.  At 1.0 single linkage leaves 28 clusters, which the
# photo rule splits into 36; at 1.5 it leaves ONE cluster of all 301 faces, split into 11: a chain outside LDS on real distances
FACES_SEED, FACES_THRESHOLDS = 0, (1.0, 1.5)


def faces_case():
    X = features(N_ENTRY, 128, FACES_SEED, classes=15)
    born, year = ages(N_ENTRY, FACES_SEED + 1)
    photos = np.random.RandomState(FACES_SEED + 2).randint(0, 120, N_ENTRY)
    return X, born, year, photos


def reference_is_stable(D, photos, t):
    """The reference's partition (scipy on the fp64 distances) is the same under five random perturbations of +-2e-4, twice the
    accuracy bound of the device distances: no merge of the case is decided within the two arithmetics' difference."""
    want = as_partition(reference_get_facial_clusters(D, t, photos))
    rs = np.random.RandomState(99)
    for _ in range(5):
        E = np.triu(rs.uniform(-2e-4, 2e-4, D.shape), 1)
        if as_partition(reference_get_facial_clusters(D + E + E.T, t, photos)) != want:
            return None
    return want


def test_cluster_faces_device_split_equals_the_host_split():
    from hse_facerec_tf_amd import clustering
    X, born, year, photos = faces_case()
    D = fp64_distances(X, born, year)
    for t in FACES_THRESHOLDS:
        want = reference_is_stable(D, photos, t)
        assert want is not None, "the case's reference partition moves under a perturbation of 2e-4: choose another seed"
        assert len(want) > len(reference_get_facial_clusters(D, t, None))                # the photo rule does split clusters here
        host = clustering.cluster_faces(X, t, born, year, photos, split="host")
        device = clustering.cluster_faces(X, t, born, year, photos, split="device")
        assert as_partition(device) == as_partition(host) == want, t
        assert device == host == clustering.cluster_faces(X, t, born, year, photos)
        assert clustering.cluster_faces(X, t, born, year, photos, min_cluster_size=2, split="device") == [c for c in host if len(c) >= 2]
    for method in ("complete", "dbscan"):                                              # nothing to split: the keyword changes nothing
        assert clustering.cluster_faces(X, 1.0, born, year, None, method=method, split="device") == \
            clustering.cluster_faces(X, 1.0, born, year, None, method=method)


def test_split_same_photo_takes_either_source_and_any_labels():
    from hse_facerec_tf_amd import clustering
    X, born, year, photos = faces_case()
    D = fp64_distances(X, born, year)
    labels = np.random.RandomState(41).randint(0, 9, N_ENTRY) * 5 - 7                   # not dense, not from a linkage
    groups = clustering._groups(labels)
    want = clustering._split_groups(groups, photos, N_ENTRY, lambda g: D[np.ix_(g, g)])
    got = clustering.split_same_photo(labels, photos, dist_matrix=D)
    assert len(got) == len(want) and all(np.array_equal(a, b) for a, b in zip(got, want))
    got = clustering.split_same_photo(labels, [str(p) for p in photos], features=X, born_years=born, photo_years=year)
    assert as_partition(got) == as_partition(want)
    with pytest.raises(ValueError):
        clustering.split_same_photo(labels, photos, features=X, dist_matrix=D)
    with pytest.raises(ValueError):
        clustering.split_same_photo(labels, photos[:-1], dist_matrix=D)


def test_perform_clustering_device_split_equals_the_default_on_the_album():
    from hse_facerec_tf_amd import album
    from test_album_gpu import planted
    feats, born, _, all_indices, mdates = planted()
    config = album.AlbumConfig()
    for method in ("single", "complete"):
        for min_size, dates in ((3, False), (3, True), (4, True)):
            cfg = config._replace(method=method)
            default = album.perform_clustering(feats, born, mdates, all_indices, min_size, dates, cfg)
            assert album.perform_clustering(feats, born, mdates, all_indices, min_size, dates, cfg, split="device") == default
            assert album.perform_clustering(feats, born, mdates, all_indices, min_size, dates, cfg, split="host") == default
    assert [0, 2, 4] in album.perform_clustering(feats, born, mdates, all_indices, 3, False, config, split="device")      # the planted split
