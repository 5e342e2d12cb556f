"""Face clustering (the album tool and the clustering study of age_gender_identity/) with single, average, complete or weighted linkage
on the GPU.

The reference groups faces with ``hac.linkage(squareform(D), 'single')`` + ``fcluster(z, t, 'distance')`` on a dense host matrix
(facial_clustering.py:214-285, process_photos.py:45-77, facial_clustering_test.py:362-414).  Single linkage is the minimum spanning
tree of the distance graph, which libhsefr builds by Boruvka rounds without an N x N matrix (ops.single_linkage_edges,
csrc/linkage.hip).  Here the tree becomes scipy's linkage matrix Z, flat cuts of Z cost O(n) each (a threshold sweep pays for one
tree), and the reference's same-photo split (complete linkage on small per-cluster matrices) runs on the host in NumPy or, with
``split="device"``, for all clusters in one device pass (split_same_photo, ops.split_groups, csrc/group_split.hip).
The study's other methods (facial_clustering_test.py:513-514: 'average', 'complete', 'weighted') need the whole matrix: libhsefr
merges reciprocal nearest neighbours round by round on an fp64 n x n device matrix (ops.hier_linkage_merges, csrc/hier_linkage.hip).
The reference's third branch, scikit-learn's DBSCAN on the precomputed matrix (facial_clustering.py:260-265), runs on the device with
scikit-learn's labels from either source, without an N x N matrix from features (ops.dbscan_labels, csrc/dbscan.hip).
Its last branch, rank-order clustering (find_clusters, facial_clustering_test.py:23-239), runs on an fp64 n x n device matrix with the
reference's clusters (ops.rank_order_labels, csrc/rank_order.hip).
The study's statistics and its threshold selection (get_clustering_statistics, test_avg_clustering_with_model_selection,
facial_clustering_test.py:416-499) score a whole sweep on the device: one clustering per album, every threshold's labels cut there
(ops.flat_cuts), every row scored by one call and read back once (ops.partition_scores, csrc/partition_scores.hip): clustering_scores,
threshold_sweep, select_threshold.
The last three of the study's seven scipy methods ('centroid', 'median', 'ward', facial_clustering_test.py:514) have entry points of
their own -- linkage_geometric, linkage_geometric_dense, cluster_faces_geometric, get_facial_clusters_geometric -- over
ops.geom_linkage_merges (libhsefr_geom.so): Ward by the same rounds with its three-term update (csrc/hier_linkage.hip compiled a second
time), centroid and median, whose trees have inversions, by a closest-pair engine that merges the least pair step by step
(csrc/geom_linkage.hip).  threshold_sweep scores them as it scores the other linkages.
No CPU fallback: the functions that compute distances raise without the library or a GPU.
"""
from __future__ import annotations

import hashlib
import math
import numbers
from typing import List, NamedTuple, Optional, Sequence

import numpy as np

SAME_PHOTO_PENALTY = 100.0      # facial_clustering.py:254 (inf_dist)
# scipy's reducible methods with a two-term per-round Lance-Williams update (csrc/hier_linkage.hip as libhsefr.so compiles it).
# 'centroid' and 'median' are not reducible (their trees can have inversions) and 'ward''s update has a third term: GEOMETRIC_METHODS
LINKAGE_METHODS = ("single", "average", "complete", "weighted")
# get_facial_clusters and cluster_faces also take the reference's DBSCAN and rank-order branches
CLUSTER_METHODS = LINKAGE_METHODS + ("dbscan", "rankorder")
# the other three of scipy's seven: squared-Euclidean ("geometric") updates.  Entry points of their own: linkage_geometric and its kin
GEOMETRIC_METHODS = ("centroid", "median", "ward")
RANK_ORDER_NORM_THRESHOLD = 0.9     # find_clusters' defaults (facial_clustering_test.py:193)
RANK_ORDER_RANK_THRESHOLD = 14


def _check_method(method, supported=LINKAGE_METHODS):
    if method not in supported:
        raise ValueError("linkage method %r is not supported; the supported methods are %s" % (method, ", ".join(supported)))


# ---- linkage matrices ----------------------------------------------------------------------------------------------
def linkage_from_edges(edge_a, edge_b, edge_h, n: int) -> np.ndarray:
    """scipy-format Z [n-1, 4] float64 from the n - 1 edges of a minimum spanning tree: the edges sorted by (height, lower endpoint,
    higher endpoint), then merged by union-find.  Row k = [id_a, id_b, height, size] with id_a < id_b; the cluster made by row k is
    n + k."""
    a = np.asarray(edge_a, dtype=np.int64)
    b = np.asarray(edge_b, dtype=np.int64)
    h = np.asarray(edge_h, dtype=np.float64)
    if not (len(a) == len(b) == len(h) == n - 1):
        raise ValueError("a spanning tree of %d points has %d edges, got %d" % (n, n - 1, len(a)))
    lo, hi = np.minimum(a, b), np.maximum(a, b)
    return _join(lo, hi, h, np.lexsort((hi, lo, h)), n, "single linkage")


def linkage_from_merges(merge_a, merge_b, merge_h, merge_round, n: int) -> np.ndarray:
    """scipy-format Z from the n - 1 merge records of ops.hier_linkage_merges: record k joined the clusters of points merge_a[k] and
    merge_b[k] at merge_h[k] in round merge_round[k].  Records are taken in (height, round, surviving point) order -- a merge in an
    earlier round precedes one of a later round at the same height, so a child never follows its parent -- and joined by union-find
    as in linkage_from_edges."""
    a = np.asarray(merge_a, dtype=np.int64)
    b = np.asarray(merge_b, dtype=np.int64)
    h = np.asarray(merge_h, dtype=np.float64)
    r = np.asarray(merge_round, dtype=np.int64)
    if not (len(a) == len(b) == len(h) == len(r) == n - 1):
        raise ValueError("a hierarchy of %d points has %d merges, got %d" % (n, n - 1, len(a)))
    lo, hi = np.minimum(a, b), np.maximum(a, b)
    return _join(lo, hi, h, np.lexsort((lo, r, h)), n, "linkage")


def linkage_from_sequence(merge_a, merge_b, merge_h, n: int) -> np.ndarray:
    """scipy-format Z from the n - 1 merge records of a sequential algorithm (ops.geom_linkage_merges, 'centroid' / 'median'): record k
    joined the clusters of points merge_a[k] and merge_b[k] at merge_h[k], and the records are taken in the order given -- they are
    not sorted, since the heights of these trees may fall (inversions).  Joined by union-find as in linkage_from_edges: row k =
    [lower id, higher id, height, size]."""
    a = np.asarray(merge_a, dtype=np.int64)
    b = np.asarray(merge_b, dtype=np.int64)
    h = np.asarray(merge_h, dtype=np.float64)
    if not (len(a) == len(b) == len(h) == n - 1):
        raise ValueError("a hierarchy of %d points has %d merges, got %d" % (n, n - 1, len(a)))
    return _join(np.minimum(a, b), np.maximum(a, b), h, np.arange(n - 1), n, "linkage")


def _join(lo, hi, h, order, n, what) -> np.ndarray:
    if n > 1 and (lo.min() < 0 or hi.max() >= n):
        raise RuntimeError("%s: edge endpoints out of range (the tree is incomplete)" % what)
    parent = list(range(2 * n - 1))
    size = [1] * n + [0] * (n - 1)
    Z = np.empty((n - 1, 4), dtype=np.float64)

    def find(v):
        r = v
        while parent[r] != r:
            r = parent[r]
        while parent[v] != r:
            parent[v], v = r, parent[v]
        return r
    for k, e in enumerate(order.tolist()):
        ra, rb = find(int(lo[e])), find(int(hi[e]))
        if ra == rb:
            raise RuntimeError("%s: the edges close a cycle (not a spanning tree)" % what)
        if ra > rb:
            ra, rb = rb, ra
        parent[ra] = parent[rb] = n + k
        size[n + k] = size[ra] + size[rb]
        Z[k] = (ra, rb, h[e], size[n + k])
    return Z


def _device_tensor(a, dtype, device=None):
    from . import _lib
    torch = _lib.require_gpu()
    if isinstance(a, torch.Tensor):
        return a.to(device=_lib.cuda_device(device) if not a.is_cuda else a.device, dtype=dtype).contiguous()
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32 if dtype == torch.float32 else np.float64)) \
        .to(_lib.cuda_device(device)).contiguous()


def _age_arrays(born_years, photo_years, n):
    if born_years is None and photo_years is None:
        return None, None
    if born_years is None or photo_years is None:
        raise ValueError("born_years and photo_years come together")
    by = np.asarray(born_years, dtype=np.float64).reshape(-1)
    yr = np.asarray(photo_years, dtype=np.float64).reshape(-1)
    if len(by) != n or len(yr) != n:
        raise ValueError("%d faces, %d born years, %d photo years" % (n, len(by), len(yr)))
    if not (np.isfinite(by).all() and np.isfinite(yr).all()):
        raise ValueError("born_years / photo_years must be finite")
    if not (yr - by > 0).all():
        raise ValueError("every face needs photo_year - born_year > 0 (the age term divides by the sum of two ages)")
    return by, yr


def _age_tensors(by, yr, dev):
    import torch
    if by is None:
        return None, None
    return torch.from_numpy(by.astype(np.float32)).to(dev), torch.from_numpy(yr.astype(np.float32)).to(dev)


# ---- the two distance sources of every entry point: checked on the host (for host inputs) before any device work ------
def _check_dist_matrix(dist_matrix, negative=None):
    """A distance-matrix argument, host or CUDA -> the float64 array (or the caller's tensor): square, non-empty and finite, and with
    ``negative`` = the caller's message for it, free of negative entries (DBSCAN and rank-order demand that, linkage does not)."""
    D = dist_matrix if hasattr(dist_matrix, "is_cuda") else np.asarray(dist_matrix, dtype=np.float64)
    if D.ndim != 2 or D.shape[0] != D.shape[1] or D.shape[0] < 1:
        raise ValueError("dist_matrix must be a non-empty square matrix, got shape %r" % (tuple(D.shape),))
    if not bool(np.isfinite(D).all() if isinstance(D, np.ndarray) else D.isfinite().all()):
        raise ValueError("dist_matrix holds non-finite values")
    if negative is not None and bool((D < 0).any()):
        raise ValueError(negative)
    return D


def _dist_matrix(dist_matrix, device, negative=None):
    """_check_dist_matrix -> the float64 device tensor ops' ``dense`` takes."""
    from . import _lib
    D = _check_dist_matrix(dist_matrix, negative)
    return _device_tensor(D, _lib.require_gpu().float64, device)


def _features(features, born_years, photo_years, device, finite):
    """A features argument, host or CUDA, with its optional age arrays -> (x, born, year) as ops takes them: the float32 [n, d] device
    tensor with n >= 1 and the float32 born / year device tensors (None without an age term).  ``finite``: non-finite features raise
    (linkage, dbscan and rank_order check; linkage_single and cluster_faces' own pass do not)."""
    from . import _lib
    if not hasattr(features, "is_cuda"):
        features = np.asarray(features, dtype=np.float32)
    if features.ndim != 2 or features.shape[0] < 1:
        raise ValueError("features must be [n, d] with n >= 1")
    if finite and isinstance(features, np.ndarray) and not np.isfinite(features).all():
        raise ValueError("features hold non-finite values")
    by, yr = _age_arrays(born_years, photo_years, features.shape[0])
    torch = _lib.require_gpu()
    x = _device_tensor(features, torch.float32, device)
    if finite and not bool(torch.isfinite(x).all()):
        raise ValueError("features hold non-finite values")
    return (x,) + _age_tensors(by, yr, x.device)


def _linkage(method, n, **source):
    """Z of ``method`` for n points from ops' source arguments (x, born, year or dense)."""
    from . import ops
    if method == "single":
        return linkage_from_edges(*(t.cpu().numpy() for t in ops.single_linkage_edges(**source)), n)
    if method in GEOMETRIC_METHODS:
        records = [t.cpu().numpy() for t in ops.geom_linkage_merges(method=method, **source)]
        return linkage_from_merges(*records, n) if method == "ward" else linkage_from_sequence(*records[:3], n)
    return linkage_from_merges(*(t.cpu().numpy() for t in ops.hier_linkage_merges(method=method, **source)), n)


def linkage_single(features, born_years=None, photo_years=None, device=None) -> np.ndarray:
    """hac.linkage(squareform(D), 'single') for D = the feature distance of perform_clustering (process_photos.py:45-56):
    |x_i - x_j| (+ the age term with born / photo years), from the features [n, d] on the GPU, with no N x N matrix anywhere."""
    x, born, year = _features(features, born_years, photo_years, device, finite=False)
    return _linkage("single", x.shape[0], x=x, born=born, year=year)


def linkage_single_dense(dist_matrix, device=None) -> np.ndarray:
    """hac.linkage(squareform(dist_matrix, checks=False), 'single') with the spanning tree built on the GPU from the fp64 matrix's
    upper triangle: the heights are scipy's, bit for bit."""
    return linkage_dense(dist_matrix, "single", device)


def linkage(features, method, born_years=None, photo_years=None, device=None) -> np.ndarray:
    """hac.linkage(squareform(D), method) for D = the feature distance of perform_clustering (process_photos.py:45-56) from the
    features [n, d] on the GPU.  'single' is linkage_single (no N x N matrix); 'average', 'complete' and 'weighted' build D as an fp64
    device matrix (fp32 distances widened, 8 n^2 bytes) and merge reciprocal nearest neighbours there.  Non-finite features raise
    ValueError; so does any other method."""
    _check_method(method)
    x, born, year = _features(features, born_years, photo_years, device, finite=True)
    return _linkage(method, x.shape[0], x=x, born=born, year=year)


def linkage_dense(dist_matrix, method, device=None) -> np.ndarray:
    """hac.linkage(squareform(dist_matrix, checks=False), method), the matrix read as its upper triangle: 'single' is
    linkage_single_dense, 'average' / 'complete' / 'weighted' run on an fp64 device copy with scipy's Lance-Williams updates (complete
    linkage's heights are scipy's bit for bit; the two means agree to rounding)."""
    _check_method(method)
    D = _dist_matrix(dist_matrix, device)
    return _linkage(method, D.shape[0], dense=D)


def linkage_geometric(features, method, born_years=None, photo_years=None, device=None) -> np.ndarray:
    """hac.linkage(squareform(D), method) for ``method`` 'centroid', 'median' or 'ward' and D = the feature distance of
    perform_clustering (process_photos.py:45-56) from the features [n, d] on the GPU: D is built as an fp64 device matrix (fp32
    distances widened, 8 n^2 bytes), the matrix linkage builds.  Ward merges reciprocal nearest neighbours round by round; centroid
    and median merge the closest pair step by step, and their Z may have inversions (heights that fall).  scipy's update rules
    operation by operation, except that a negative radicand -- rounding, or the age term, which is not Euclidean -- gives 0 where
    scipy gives NaN.  Non-finite features raise ValueError; so does any other method, before any device work.  One point gives a
    (0, 4) array."""
    _check_method(method, GEOMETRIC_METHODS)
    x, born, year = _features(features, born_years, photo_years, device, finite=True)
    return _linkage(method, x.shape[0], x=x, born=born, year=year)


def linkage_geometric_dense(dist_matrix, method, device=None) -> np.ndarray:
    """hac.linkage(squareform(dist_matrix, checks=False), method) for ``method`` 'centroid', 'median' or 'ward', the matrix read as its
    upper triangle, on an fp64 device copy: centroid's and median's Z are scipy's bit for bit where the distances have no ties, Ward's
    has scipy's clusters and its heights to rounding.  A negative radicand gives 0 where scipy gives NaN (see linkage_geometric)."""
    _check_method(method, GEOMETRIC_METHODS)
    D = _dist_matrix(dist_matrix, device)
    return _linkage(method, D.shape[0], dense=D)


# ---- DBSCAN ---------------------------------------------------------------------------------------------------------
def _check_dbscan_args(eps, min_samples):
    if isinstance(eps, bool) or not isinstance(eps, numbers.Real) or not math.isfinite(eps) or not eps > 0:
        raise ValueError("dbscan: eps must be a finite real > 0, got %r" % (eps,))
    if isinstance(min_samples, bool) or not isinstance(min_samples, numbers.Integral) or min_samples < 1:
        raise ValueError("dbscan: min_samples must be an int >= 1, got %r" % (min_samples,))


def _dbscan_result(labels, core):
    labels = labels.cpu().numpy().astype(np.int64)
    return np.flatnonzero(core.cpu().numpy()).astype(np.int64), labels


def dbscan(features, eps=0.5, min_samples=5, born_years=None, photo_years=None, device=None):
    """sklearn.cluster.dbscan(D, eps, min_samples=min_samples, metric="precomputed") for D = the feature distance of
    perform_clustering (process_photos.py:45-56) from the features [n, d] on the GPU, with no N x N matrix anywhere ->
    (core_sample_indices, labels) int64, scikit-learn's.  Distances are the fp32 ones of linkage_single, compared as (double)w <= eps.
    Bad eps, min_samples, features or age arrays raise ValueError before any device work (for host inputs)."""
    from . import ops
    _check_dbscan_args(eps, min_samples)
    x, born, year = _features(features, born_years, photo_years, device, finite=True)
    return _dbscan_result(*ops.dbscan_labels(x=x, born=born, year=year, eps=eps, min_samples=min_samples))


def dbscan_dense(dist_matrix, eps=0.5, min_samples=5, device=None):
    """sklearn.cluster.dbscan(dist_matrix, eps, min_samples=min_samples, metric="precomputed") on the GPU -> (core_sample_indices,
    labels) int64.  The matrix is read as its upper triangle D[min(i,j), max(i,j)] (scikit-learn reads whole rows: the results agree
    on every symmetric matrix).  A non-square, empty, non-finite or negative matrix raises ValueError, as do bad eps / min_samples."""
    from . import ops
    _check_dbscan_args(eps, min_samples)
    D = _dist_matrix(dist_matrix, device, "dist_matrix holds negative values (scikit-learn rejects them in a precomputed matrix)")
    return _dbscan_result(*ops.dbscan_labels(dense=D, eps=eps, min_samples=min_samples))


def _clusters(labels) -> List[np.ndarray]:
    """Members of each non-negative label (noise dropped)."""
    labels = np.asarray(labels)
    keep = np.flatnonzero(labels >= 0)
    return [keep[g] for g in _groups(labels[keep])] if len(keep) else []


# ---- rank-order clustering -------------------------------------------------------------------------------------------
def _check_rank_order_pair(norm_threshold, rank_threshold):
    for name, v in (("norm_threshold", norm_threshold), ("rank_threshold", rank_threshold)):
        if isinstance(v, bool) or not isinstance(v, numbers.Real) or not math.isfinite(v) or not v > 0:
            raise ValueError("rank_order: %s must be a finite real > 0, got %r" % (name, v))
    return float(norm_threshold), float(rank_threshold)


def _rank_order_pairs(norm_threshold, rank_threshold, thresholds):
    """-> (list of checked (norm, rank) pairs, whether the caller passed a sequence)"""
    if thresholds is None:
        return [_check_rank_order_pair(norm_threshold, rank_threshold)], False
    pairs = []
    try:
        for pair in thresholds:
            norm, rank = pair
            pairs.append(_check_rank_order_pair(norm, rank))
    except TypeError:
        raise ValueError("rank_order: thresholds must be a sequence of (norm_threshold, rank_threshold) pairs, got %r" % (thresholds,))
    if not pairs:
        raise ValueError("rank_order: thresholds is empty")
    return pairs, True


def _rank_order_threshold_pair(threshold):
    """The study passes distanceThreshold = (norm, rank); a scalar is (scalar, the reference's default rank threshold)."""
    if isinstance(threshold, numbers.Real):
        return _check_rank_order_pair(threshold, RANK_ORDER_RANK_THRESHOLD)
    try:
        norm, rank = threshold
    except (TypeError, ValueError):
        raise ValueError("rank_order: the threshold must be a number or a (norm_threshold, rank_threshold) pair, got %r" % (threshold,))
    return _check_rank_order_pair(norm, rank)


def _rank_order_clusters(labels) -> List[List[int]]:
    """labels[i] = the smallest face of i's cluster -> the reference's matched_clusters: clusters of at least two faces, longest first,
    equal lengths by smallest face."""
    return _finish(_groups(np.asarray(labels)), 2)


def _rank_order(pairs, sweep, **source):
    """ops.rank_order_labels on its source arguments (x, born, year or dense) -> what rank_order returns."""
    from . import ops
    if not sweep:
        labels, iters = ops.rank_order_labels(norm_threshold=pairs[0][0], rank_threshold=pairs[0][1], **source)
        return _rank_order_clusters(labels.cpu().numpy()), iters
    labels, iters = ops.rank_order_labels(thresholds=pairs, **source)
    return [(_rank_order_clusters(row), it) for row, it in zip(labels.cpu().numpy(), iters)]


def rank_order(features, norm_threshold=RANK_ORDER_NORM_THRESHOLD, rank_threshold=RANK_ORDER_RANK_THRESHOLD, born_years=None,
               photo_years=None, device=None, thresholds=None):
    """The reference's rank-order clustering (find_clusters, facial_clustering_test.py:23-239; the rule is written out at
    hsefr_rank_order in include/hsefr.h) for D = the feature distance of perform_clustering (process_photos.py:45-56) from the features
    [n, d] on the GPU -> (clusters, iterations): clusters of at least two faces as sorted lists of face indices, longest first, equal
    lengths by their smallest face (the reference's order); iterations as the reference counts them.  Distances are the fp32 ones of
    linkage, widened to an fp64 n x n device matrix.  ``thresholds`` = a sequence of (norm, rank) pairs returns one (clusters,
    iterations) per pair from one matrix build.  Bad thresholds, features or age arrays raise ValueError before any device work (for
    host inputs).  One face gives []."""
    pairs, sweep = _rank_order_pairs(norm_threshold, rank_threshold, thresholds)
    x, born, year = _features(features, born_years, photo_years, device, finite=True)
    return _rank_order(pairs, sweep, x=x, born=born, year=year)


def rank_order_dense(dist_matrix, norm_threshold=RANK_ORDER_NORM_THRESHOLD, rank_threshold=RANK_ORDER_RANK_THRESHOLD, device=None,
                     thresholds=None):
    """rank_order on a distance matrix: the rank-order branch of get_facial_clusters(dist_matrix, (norm_threshold, rank_threshold)) on
    the GPU -> (clusters, iterations).  The matrix is read as its upper triangle D[min(i,j), max(i,j)] and its diagonal counts as 0 (the
    reference reads whole rows: the results agree on every symmetric matrix with a zero diagonal).  A non-square, empty, non-finite or
    negative matrix raises ValueError, as do bad thresholds.  ``thresholds`` as in rank_order."""
    pairs, sweep = _rank_order_pairs(norm_threshold, rank_threshold, thresholds)
    return _rank_order(pairs, sweep, dense=_dist_matrix(dist_matrix, device, "dist_matrix holds negative values"))


# ---- flat cuts ------------------------------------------------------------------------------------------------------
_CUT_CACHE = {}


def _cut_order(Z: np.ndarray):
    """Leaves in dendrogram order, and for each of the n - 1 gaps between neighbours in that order the largest height inside the
    smallest cluster that holds both (scipy's max-dist monocrit).  Every flat cluster of every cut is a run of that order."""
    Z = np.ascontiguousarray(Z, dtype=np.float64)
    key = hashlib.blake2b(Z.tobytes(), digest_size=16).digest()
    hit = _CUT_CACHE.get(key)
    if hit is not None:
        return hit
    n = Z.shape[0] + 1
    head = list(range(n)) + [0] * (n - 1)
    tail = list(range(n)) + [0] * (n - 1)
    maxh = [-np.inf] * n + [0.0] * (n - 1)
    nxt = [-1] * n
    gap_h = [0.0] * n
    ids = Z[:, :2].astype(np.int64).tolist()
    hs = Z[:, 2].tolist()
    for k in range(n - 1):
        a, b = ids[k]
        c = n + k
        m = max(hs[k], maxh[a], maxh[b])
        maxh[c] = m
        nxt[tail[a]] = head[b]
        gap_h[tail[a]] = m
        head[c], tail[c] = head[a], tail[b]
    order = np.empty(n, dtype=np.int64)
    v = head[2 * n - 2] if n > 1 else 0
    for p in range(n):
        order[p] = v
        v = nxt[v]
    gaps = np.asarray(gap_h, dtype=np.float64)[order[:-1]]
    if len(_CUT_CACHE) >= 8:
        _CUT_CACHE.clear()
    _CUT_CACHE[key] = (order, gaps)
    return order, gaps


def fcluster_distance(Z, t):
    """fcluster(Z, t, 'distance'): flat clusters whose members are joined at heights <= t, labelled 1..k (the partition is scipy's,
    label numbers are in dendrogram order).  ``t`` may be a sequence: one row of labels per threshold.  Z's leaf order is computed once
    and cached, so a sweep costs O(n) vectorised work per threshold."""
    Z = np.asarray(Z, dtype=np.float64)
    order, gaps = _cut_order(Z)
    n = len(order)
    ts = np.atleast_1d(np.asarray(t, dtype=np.float64))
    out = np.empty((len(ts), n), dtype=np.int32)
    for r, tv in enumerate(ts):
        run = np.empty(n, dtype=np.int32)
        run[0] = 1
        run[1:] = 1 + np.cumsum(gaps > tv)
        out[r, order] = run
    return out[0] if np.ndim(t) == 0 else out


def _groups(labels: np.ndarray) -> List[np.ndarray]:
    """Members of each label, ascending, the groups ordered by their smallest member."""
    labels = np.asarray(labels)
    order = np.argsort(labels, kind="stable")
    cuts = np.flatnonzero(np.diff(labels[order])) + 1
    groups = np.split(order, cuts)
    groups.sort(key=lambda g: int(g[0]))
    return groups


# ---- the same-photo split: complete linkage on the host --------------------------------------------------------------
def complete_linkage_labels(D: np.ndarray, t: float) -> np.ndarray:
    """fcluster(linkage(squareform(D), 'complete'), t, 'distance') for a small symmetric matrix, as labels 0..k-1 by first
    occurrence: the nearest-neighbour chain with scipy's tie rules (the previous chain element wins a tie; otherwise the lowest index),
    Lance-Williams complete update max(d(x,k), d(y,k)), merged cluster kept in the larger slot.  O(k^2)."""
    D = np.array(D, dtype=np.float64)
    k = D.shape[0]
    if k == 1:
        return np.zeros(1, dtype=np.int64)
    np.fill_diagonal(D, np.inf)
    parent = list(range(k))
    chain: List[int] = []
    alive = np.ones(k, dtype=bool)
    merges = []
    for _ in range(k - 1):
        if not chain:
            chain.append(int(np.flatnonzero(alive)[0]))
        while True:
            x = chain[-1]
            if len(chain) > 1:
                y, cur = chain[-2], D[x, chain[-2]]
            else:
                y, cur = -1, np.inf
            j = int(np.argmin(D[x]))
            if D[x, j] < cur:
                y = j
            if len(chain) > 1 and y == chain[-2]:
                break
            chain.append(y)
        x, y = chain.pop(), chain.pop()
        if x > y:
            x, y = y, x
        merges.append((x, y, D[x, y]))
        row = np.maximum(D[x], D[y])
        D[y, :] = row
        D[:, y] = row
        D[y, y] = np.inf
        D[x, :] = np.inf
        D[:, x] = np.inf
        alive[x] = False

    def find(v):
        while parent[v] != v:
            parent[v] = parent[parent[v]]
            v = parent[v]
        return v
    for x, y, h in merges:          # complete linkage has no inversions: a merge at h <= t has all its sub-merges <= t as well
        if h <= t:
            parent[find(x)] = find(y)
    roots = np.array([find(v) for v in range(k)])
    _, first = np.unique(roots, return_index=True)
    relabel = {int(roots[f]): i for i, f in enumerate(sorted(first))}
    return np.array([relabel[int(r)] for r in roots], dtype=np.int64)


def _split_same_photo(D_sub: np.ndarray, photo: np.ndarray) -> List[np.ndarray]:
    """facial_clustering.py:250-261 inside one cluster: +100 for two faces of one photo, complete linkage, cut at 50."""
    P = np.triu(np.asarray(D_sub, dtype=np.float64), 1)
    P = P + P.T
    same = photo[:, None] == photo[None, :]
    np.fill_diagonal(same, False)
    P += SAME_PHOTO_PENALTY * same
    lab = complete_linkage_labels(P, SAME_PHOTO_PENALTY / 2)
    return [np.flatnonzero(lab == v) for v in range(int(lab.max()) + 1)]


def _split_groups(groups, all_indices, n, sub_dist) -> List[np.ndarray]:
    """The same-photo split of every cluster of at least two faces; all_indices = the photo of each of the n faces, sub_dist(g) = the
    distances among the faces g of one cluster."""
    photo = np.asarray(all_indices).reshape(-1)
    if len(photo) != n:
        raise ValueError("%d faces, %d photo indices" % (n, len(photo)))
    clusters = []
    for g in groups:
        if len(g) > 1:
            clusters.extend(g[part] for part in _split_same_photo(sub_dist(g), photo[g]))
        else:
            clusters.append(g)
    return clusters


# ---- the same-photo split of every cluster in one device pass ----------------------------------------------------------
SPLIT_CHOICES = ("host", "device")


def _check_split(split):
    if split not in SPLIT_CHOICES:
        raise ValueError("split %r is not supported; the choices are %s" % (split, ", ".join(SPLIT_CHOICES)))


def group_table(labels):
    """The clusters of a labelling as ops.split_groups takes them -> (members int32 [n], offsets int64 [groups + 1]): group g holds the
    items members[offsets[g]:offsets[g + 1]], ascending, and the groups are ordered by their smallest member (_groups' order).  Labels
    are compared for equality only; they need not be dense.  Pure NumPy."""
    labels = np.asarray(labels).reshape(-1)
    n = len(labels)
    if n == 0:
        return np.zeros(0, dtype=np.int32), np.zeros(1, dtype=np.int64)
    _, first, inverse = np.unique(labels, return_index=True, return_inverse=True)
    rank = np.empty(len(first), dtype=np.int64)
    rank[np.argsort(first, kind="stable")] = np.arange(len(first))      # a group's place = the place of its smallest member
    group = rank[inverse.reshape(-1)]
    members = np.argsort(group, kind="stable").astype(np.int32)
    offsets = np.zeros(len(first) + 1, dtype=np.int64)
    np.cumsum(np.bincount(group, minlength=len(first)), out=offsets[1:])
    return members, offsets


def split_same_photo(labels, all_indices, features=None, dist_matrix=None, born_years=None, photo_years=None,
                     device=None) -> List[np.ndarray]:
    """The same-photo split (facial_clustering.py:250-261) of every cluster of ``labels`` in one device pass (ops.split_groups) ->
    the clusters as _split_groups returns them: cluster by cluster in _groups' order, each one's parts in order of their first face.
    ``all_indices`` is the photo of every face.  Exactly one source: ``features`` [n, d] with optional born / photo years -- the
    distances are then w(i,j), the ones the linkage itself uses -- or ``dist_matrix`` [n, n].  SAME_PHOTO_PENALTY between two faces of
    one photo, cut at half of it.  No faces give []."""
    if (features is None) == (dist_matrix is None):
        raise ValueError("split_same_photo: pass exactly one of features and dist_matrix")
    if len(np.asarray(labels).reshape(-1)) == 0 and len(np.asarray(all_indices).reshape(-1)) == 0:
        return []
    if features is not None:
        x, born, year = _features(features, born_years, photo_years, device, finite=False)
        source = dict(x=x, born=born, year=year)
    else:
        if born_years is not None or photo_years is not None:
            raise ValueError("split_same_photo: the age term belongs to the features path")
        source = dict(dense=_dist_matrix(dist_matrix, device))
    return _split_on_device(labels, all_indices, **source)


def _split_on_device(labels, all_indices, **source) -> List[np.ndarray]:
    """split_same_photo on ops' source arguments (x, born, year or dense), already checked and on the device."""
    from . import ops
    import torch
    labels = np.asarray(labels).reshape(-1)
    n = len(labels)
    photo = np.asarray(all_indices).reshape(-1)
    if len(photo) != n:
        raise ValueError("%d faces, %d photo indices" % (n, len(photo)))
    data = source["x"] if source.get("x") is not None else source["dense"]
    if data.shape[0] != n:
        raise ValueError("%d labels for %d faces" % (n, data.shape[0]))
    dev = data.device
    members, offsets = group_table(labels)
    codes = np.unique(photo, return_inverse=True)[1].reshape(-1).astype(np.int32)      # photos are compared for equality only
    sub, _ = ops.split_groups(torch.from_numpy(members).to(dev), offsets, torch.from_numpy(codes).to(dev),
                              penalty=SAME_PHOTO_PENALTY, cut=SAME_PHOTO_PENALTY / 2, return_stats=True, **source)
    sub = sub.cpu().numpy().astype(np.int64)
    key = np.repeat(np.arange(len(offsets) - 1, dtype=np.int64), np.diff(offsets)) * (int(sub.max()) + 1) + sub
    order = np.argsort(key, kind="stable")
    return np.split(members[order].astype(np.int64), np.flatnonzero(np.diff(key[order])) + 1)


def _finish(clusters: List[np.ndarray], min_size: int = 1) -> List[List[int]]:
    out = [sorted(int(i) for i in c) for c in clusters if len(c) >= min_size]
    out.sort(key=lambda c: (-len(c), c[0]))
    return out


def get_facial_clusters(dist_matrix, distanceThreshold=1, all_indices=None, no_images_in_cluster=1, device=None,
                        method="single", split="host") -> List[List[int]]:
    """The scipy branch of facial_clustering.get_facial_clusters (:243-261) with the linkage on the GPU (dense fp64 path) -- single
    linkage by default, or ``method`` 'average' / 'complete' / 'weighted' (the module global clusteringMethod the study sets):
    clusters of faces joined at distances <= distanceThreshold; with ``all_indices`` (the photo of every face) each cluster is split so
    that no two faces of one photo stay together (complete linkage on the cluster's penalised distances, cut at 50, as the reference).
    ``no_images_in_cluster`` is accepted and ignored, as that branch does.  Returns lists of face indices, longest first; clusters of
    equal length are ordered by their smallest index (the reference leaves that order to scipy's label numbering).  One face gives
    [[0]] (the reference's linkage raises on it).  Non-finite distances raise ValueError.
    ``method`` 'dbscan' is the DBSCAN branch (:260-265): dbscan_dense with eps = distanceThreshold and min_samples =
    no_images_in_cluster, noise dropped, ``all_indices`` accepted and ignored, the same order; one face gives scikit-learn's answer.
    ``method`` 'rankorder' is the rank-order branch (:229-239): rank_order_dense with distanceThreshold = the study's pair (norm, rank),
    or a scalar norm threshold with the reference's default rank threshold 14; clusters of at least two faces in the reference's order;
    ``all_indices`` and ``no_images_in_cluster`` accepted and ignored, as that branch does; one face gives [].
    ``split`` 'host' (the default) runs the same-photo split cluster by cluster in NumPy; 'device' runs it for all clusters in one
    device pass (split_same_photo) on the same matrix, with the same clusters, ties included.  Any other value raises ValueError before
    any device work; where ``all_indices`` is ignored ('dbscan', 'rankorder'), so is ``split``."""
    _check_method(method, CLUSTER_METHODS)
    _check_split(split)
    if method == "dbscan":
        return _finish(_clusters(dbscan_dense(dist_matrix, distanceThreshold, no_images_in_cluster, device)[1]))
    if method == "rankorder":
        return rank_order_dense(dist_matrix, *_rank_order_threshold_pair(distanceThreshold), device=device)[0]
    return _matrix_clusters(dist_matrix, distanceThreshold, all_indices, device, method, split)


def _matrix_clusters(dist_matrix, distanceThreshold, all_indices, device, method, split) -> List[List[int]]:
    """get_facial_clusters behind its argument checks for a linkage ``method``: the tree cut at distanceThreshold, the same-photo
    split, the order.  get_facial_clusters_geometric ends here too."""
    D = _check_dist_matrix(np.asarray(dist_matrix, dtype=np.float64))
    n = D.shape[0]
    if n == 1:
        return [[0]]
    Dd = _dist_matrix(D, device)                     # one upload for the linkage and the split
    labels = fcluster_distance(_linkage(method, n, dense=Dd), distanceThreshold)
    if split == "device" and all_indices is not None:
        return _finish(_split_on_device(labels, all_indices, dense=Dd))
    groups = _groups(labels)
    if all_indices is None:
        return _finish(groups)
    return _finish(_split_groups(groups, all_indices, n, lambda g: D[np.ix_(g, g)]))


def get_facial_clusters_geometric(dist_matrix, distanceThreshold, method, all_indices=None, device=None, split="host") -> List[List[int]]:
    """get_facial_clusters behind a 'centroid', 'median' or 'ward' tree (linkage_geometric_dense): the clusters of faces joined at
    distances <= distanceThreshold -- fcluster(Z, t, 'distance'), which on a tree with inversions cuts by the largest height inside a
    cluster -- then the same-photo split with ``all_indices`` and get_facial_clusters' order.  Any other method or split raises
    ValueError before any device work.  One face gives [[0]]."""
    _check_method(method, GEOMETRIC_METHODS)
    _check_split(split)
    return _matrix_clusters(dist_matrix, distanceThreshold, all_indices, device, method, split)


def cluster_faces(features, distance_threshold: float, born_years=None, photo_years=None, all_indices=None,
                  min_cluster_size: int = 1, device=None, method: str = "single", split: str = "host") -> List[List[int]]:
    """perform_clustering (process_photos.py:45-77) without the date rule, from the features: single linkage on the GPU with no N x N
    matrix (or ``method`` 'average' / 'complete' / 'weighted' on an fp64 device matrix; see linkage), the age term when born / photo
    years are given, the same-photo split on each cluster's own distances (its rows through
    ops.pairwise_distances plus the host age term, clipped at 0, as feature_distance_matrix builds them), and clusters shorter than
    ``min_cluster_size`` dropped.  Same order as get_facial_clusters.  ``method`` 'dbscan' is perform_clustering's DBSCAN branch:
    dbscan with eps = distance_threshold and min_samples = min_cluster_size, noise dropped, then the clusters shorter than
    min_cluster_size (a border point claimed by an earlier cluster can leave one short); ``all_indices`` is ignored.  ``method``
    'rankorder' is rank_order with distance_threshold = (norm, rank) or a scalar norm threshold (rank threshold 14): clusters of at least
    two faces; ``all_indices`` and ``min_cluster_size`` are ignored, as the reference's branch ignores them.
    ``split`` 'host' (the default) is the same-photo split described above; 'device' runs it for all clusters in one device pass
    (split_same_photo) and splits on w(i,j), the distance the clusters were formed by (csrc/linkage_scan.h's feat_tile, age term
    included), where the host split recomputes its distances another way.  Both are fp32 distances of the same features: the two
    choices can differ only where two candidate merges of a cluster are within rounding of each other.  Any other value raises
    ValueError before any device work; where ``all_indices`` is ignored ('dbscan', 'rankorder'), so is ``split``."""
    from . import ops
    _check_method(method, CLUSTER_METHODS)
    _check_split(split)
    if method == "dbscan":
        _, labels = dbscan(features, distance_threshold, min_cluster_size, born_years, photo_years, device)
        return _finish(_clusters(labels), min_cluster_size)
    if method == "rankorder":
        return rank_order(features, *_rank_order_threshold_pair(distance_threshold), born_years=born_years, photo_years=photo_years,
                          device=device)[0]
    return _feature_clusters(features, distance_threshold, born_years, photo_years, all_indices, min_cluster_size, device, method, split)


def _feature_clusters(features, distance_threshold, born_years, photo_years, all_indices, min_cluster_size, device, method,
                      split) -> List[List[int]]:
    """cluster_faces behind its argument checks for a linkage ``method``: the tree cut at distance_threshold, the same-photo split,
    the minimum size, the order.  cluster_faces_geometric ends here too."""
    from . import ops
    x, born, year = _features(features, born_years, photo_years, device, finite=False)
    n = x.shape[0]
    by, yr = _age_arrays(born_years, photo_years, n)
    if n == 1:
        return _finish([np.zeros(1, dtype=np.int64)], min_cluster_size)
    if method == "single":
        Z = linkage_single(x, by, yr)
    else:
        Z = linkage_geometric(x, method, by, yr) if method in GEOMETRIC_METHODS else linkage(x, method, by, yr)
    labels = fcluster_distance(Z, distance_threshold)
    if split == "device" and all_indices is not None:
        return _finish(_split_on_device(labels, all_indices, x=x, born=born, year=year), min_cluster_size)
    groups = _groups(labels)
    if all_indices is None:
        return _finish(groups, min_cluster_size)
    import torch
    xp = x if x.shape[1] % 8 == 0 else torch.nn.functional.pad(x, (0, 8 - x.shape[1] % 8)).contiguous()

    def sub_dist(g):
        rows = xp[torch.from_numpy(g).to(x.device)].contiguous()
        D = ops.pairwise_distances(rows).cpu().numpy().astype(np.float64)
        if by is not None:
            b, y = by[g], yr[g]
            max_year = np.maximum(y[:, None], y[None, :])
            ai, aj = max_year - b[:, None], max_year - b[None, :]
            D = D + 0.1 * (ai - aj) ** 2 / (ai + aj)
        return np.clip(D, 0, None)
    return _finish(_split_groups(groups, all_indices, n, sub_dist), min_cluster_size)


def cluster_faces_geometric(features, distance_threshold: float, method: str, born_years=None, photo_years=None, all_indices=None,
                            min_cluster_size: int = 1, device=None, split: str = "host") -> List[List[int]]:
    """cluster_faces behind a 'centroid', 'median' or 'ward' tree (linkage_geometric): the tree cut at distance_threshold, the age term
    when born / photo years are given, the same-photo split, clusters shorter than ``min_cluster_size`` dropped, cluster_faces' order
    and its two ``split`` choices.  Any other method or split raises ValueError before any device work."""
    _check_method(method, GEOMETRIC_METHODS)
    _check_split(split)
    return _feature_clusters(features, distance_threshold, born_years, photo_years, all_indices, min_cluster_size, device, method, split)


# ---- mean shift -----------------------------------------------------------------------------------------------------
MEAN_SHIFT_BANDWIDTH = 0.7      # facial_clustering_test.py:264: MeanShift(bandwidth=0.7).fit(all_features)


def _check_mean_shift_args(bandwidth, max_iter):
    if isinstance(bandwidth, bool) or not isinstance(bandwidth, numbers.Real) or not math.isfinite(bandwidth) or not bandwidth > 0:
        raise ValueError("mean_shift: bandwidth must be a finite real > 0, got %r" % (bandwidth,))
    if isinstance(max_iter, bool) or not isinstance(max_iter, numbers.Integral) or max_iter < 0:
        raise ValueError("mean_shift: max_iter must be an int >= 0, got %r" % (max_iter,))


def _mean_shift(x, bandwidth, max_iter, cluster_all):
    """mean_shift on the checked device tensor x -> (centres, labels, n_iter), host arrays"""
    from . import ops
    centers, _, labels, dist, info = ops.mean_shift_fit(x, bandwidth, max_iter)
    labels = labels.cpu().numpy().astype(np.int64)
    if not cluster_all:
        labels[dist.cpu().numpy() > bandwidth] = -1
    return centers.cpu().numpy(), labels, info["n_iter"]


def mean_shift(features, bandwidth=MEAN_SHIFT_BANDWIDTH, max_iter=300, cluster_all=True, device=None):
    """sklearn.cluster.MeanShift(bandwidth=bandwidth, max_iter=max_iter, cluster_all=cluster_all).fit(features) on the GPU -- every face a
    seed, all seeds advanced together in fp64, no N x N matrix but one of bits -> (cluster_centers float64 [k, d], labels int64 [n],
    n_iter), scikit-learn's cluster_centers_ (to rounding), labels_ and n_iter_.  The default bandwidth is the clustering study's
    (facial_clustering_test.py:264).  With ``cluster_all=False`` a face farther than the bandwidth from its nearest centre gets -1.
    Bad bandwidth, max_iter or features raise ValueError before any device work (for host inputs)."""
    _check_mean_shift_args(bandwidth, max_iter)
    x, _, _ = _features(features, None, None, device, finite=True)
    return _mean_shift(x, float(bandwidth), int(max_iter), cluster_all)


def mean_shift_predict(features, cluster_centers, device=None) -> np.ndarray:
    """MeanShift.predict: the index of the nearest of ``cluster_centers`` [k, d] for every row of ``features`` [n, d], the lowest index
    among equal distances -> int64 [n]."""
    from . import _lib, ops
    centers = cluster_centers if hasattr(cluster_centers, "is_cuda") else np.asarray(cluster_centers, dtype=np.float64)
    if centers.ndim != 2 or centers.shape[0] < 1:
        raise ValueError("cluster_centers must be [k, d] with k >= 1")
    if isinstance(centers, np.ndarray) and not np.isfinite(centers).all():
        raise ValueError("cluster_centers hold non-finite values")
    if not hasattr(features, "is_cuda"):
        features = np.asarray(features, dtype=np.float32)
    if features.ndim != 2 or features.shape[1] != centers.shape[1]:
        raise ValueError("features must be [n, %d] as the centres" % centers.shape[1])
    x, _, _ = _features(features, None, None, device, finite=True)
    c = _device_tensor(centers, _lib.require_gpu().float64, x.device)
    return ops.mean_shift_assign(x, c)[0].cpu().numpy().astype(np.int64)


def cluster_faces_mean_shift(features, bandwidth=MEAN_SHIFT_BANDWIDTH, all_indices=None, min_cluster_size: int = 1, split: str = "host",
                             device=None) -> List[List[int]]:
    """The scikit-learn branch of the reference's get_facial_clusters with its mean-shift row (facial_clustering_test.py:264-266, 285):
    the members of every label >= 0 of mean_shift(features, bandwidth), the largest cluster first (a stable sort of the clusters in
    label order), as lists of ints.  With ``all_indices`` (the photo of every face) every cluster goes through the same-photo split
    (facial_clustering.py:250-261) -- ``split`` 'host': cluster by cluster on the host, 'device': split_same_photo's one pass -- its
    parts in order of their first face; clusters shorter than ``min_cluster_size`` are dropped."""
    _check_mean_shift_args(bandwidth, 300)
    _check_split(split)
    x, _, _ = _features(features, None, None, device, finite=True)
    labels = _mean_shift(x, float(bandwidth), 300, True)[1]
    return _label_clusters(x, labels, all_indices, min_cluster_size, split)


def _label_clusters(x, labels, all_indices, min_cluster_size, split) -> List[List[int]]:
    """the list form of a labelling of the device features x: every label >= 0, the same-photo split, the largest first"""
    from . import ops
    n = x.shape[0]
    groups = [np.flatnonzero(labels == c) for c in range(int(labels.max()) + 1)]
    groups = [g for g in groups if len(g)]
    if all_indices is not None:
        if split == "device":
            groups = [np.sort(g) for g in split_same_photo(labels, all_indices, features=x)]      # clusters in order of their first face:
            groups.sort(key=lambda g: int(labels[g[0]]))                   # back to label order (stable: a cluster's parts stay in theirs)
        else:
            import torch
            xp = x if x.shape[1] % 8 == 0 else torch.nn.functional.pad(x, (0, 8 - x.shape[1] % 8)).contiguous()

            def sub_dist(g):
                rows = xp[torch.from_numpy(g).to(x.device)].contiguous()
                return np.clip(ops.pairwise_distances(rows).cpu().numpy().astype(np.float64), 0, None)
            groups = _split_groups(groups, all_indices, n, sub_dist)
    out = [[int(i) for i in g] for g in groups if len(g) >= min_cluster_size]
    out.sort(key=len, reverse=True)
    return out


# ---- affinity propagation --------------------------------------------------------------------------------------------
# facial_clustering_test.py:263: AffinityPropagation().fit(all_features) -- scikit-learn's defaults
AFFINITY_DAMPING = 0.5
AFFINITY_MAX_ITER = 200
AFFINITY_CONVERGENCE_ITER = 15


class ConvergenceWarning(UserWarning):
    """affinity propagation ran max_iter iterations without its stop test holding (scikit-learn's warning of the same name)"""


def _check_affinity_args(damping, max_iter, convergence_iter, preference, seed):
    if isinstance(damping, bool) or not isinstance(damping, numbers.Real) or not 0.5 <= damping < 1:
        raise ValueError("affinity_propagation: damping must be a real in [0.5, 1), got %r" % (damping,))
    if isinstance(max_iter, bool) or not isinstance(max_iter, numbers.Integral) or max_iter < 1:
        raise ValueError("affinity_propagation: max_iter must be an int >= 1, got %r" % (max_iter,))
    if isinstance(convergence_iter, bool) or not isinstance(convergence_iter, numbers.Integral) or not 1 <= convergence_iter <= 64:
        raise ValueError("affinity_propagation: convergence_iter must be an int in 1 .. 64, got %r" % (convergence_iter,))
    if preference is not None and (isinstance(preference, bool) or not isinstance(preference, numbers.Real) or not math.isfinite(preference)):
        raise ValueError("affinity_propagation: preference must be None (the median) or a finite real, got %r" % (preference,))
    if seed is not None and (isinstance(seed, bool) or not isinstance(seed, numbers.Integral) or seed < 0):
        raise ValueError("affinity_propagation: seed must be None (no noise) or an int >= 0, got %r" % (seed,))


def _affinity(source, damping, max_iter, convergence_iter, preference, seed):
    """affinity propagation on a checked device tensor, source = dict(x=...) or dict(S=...) -> (exemplars, labels, n_iter), host arrays"""
    import warnings
    from . import ops
    exemplars, labels, _, _, info = ops.affinity_propagation_fit(damping=float(damping), max_iter=int(max_iter),
                                                                 convergence_iter=int(convergence_iter), preference=preference, seed=seed,
                                                                 **source)
    if not info["converged"]:
        warnings.warn("Affinity propagation did not converge%s." % (", this model may return degenerate cluster centers and labels"
                                                                    if info["clusters"] else " and this model will not have any cluster centers"),
                      ConvergenceWarning, stacklevel=3)
    return exemplars.cpu().numpy().astype(np.int64), labels.cpu().numpy().astype(np.int64), info["n_iter"]


def affinity_propagation(features, damping=AFFINITY_DAMPING, max_iter=AFFINITY_MAX_ITER, convergence_iter=AFFINITY_CONVERGENCE_ITER,
                         preference=None, seed=0, device=None):
    """sklearn.cluster.AffinityPropagation(damping=, max_iter=, convergence_iter=, preference=).fit(features.astype(float64)) on the GPU
    -> (cluster_centers_indices int64 [K] ascending, labels int64 [n], n_iter).  The float32 features are widened exactly and everything
    is fp64 (scikit-learn keeps float32 input's similarities in float32 and perturbs them at float32's eps).  ``preference`` None: the
    median of the similarities.  ``seed``: the seed of the tie-breaking noise (scikit-learn's is unseeded; which member of a two-point
    cluster is its exemplar depends on it), None for none.  A fit that does not converge raises a ConvergenceWarning and, without an
    exemplar, labels every face -1.  Bad arguments or features raise ValueError before any device work (for host inputs)."""
    _check_affinity_args(damping, max_iter, convergence_iter, preference, seed)
    x, _, _ = _features(features, None, None, device, finite=True)
    return _affinity(dict(x=x), damping, max_iter, convergence_iter, preference, seed)


def affinity_propagation_dense(S, damping=AFFINITY_DAMPING, max_iter=AFFINITY_MAX_ITER, convergence_iter=AFFINITY_CONVERGENCE_ITER,
                               preference=None, seed=0, device=None):
    """AffinityPropagation(affinity="precomputed", ...).fit(S): ``S`` [n, n] similarities (larger is more alike; they may be asymmetric),
    host or CUDA, read as float64 -> as affinity_propagation."""
    from . import _lib
    _check_affinity_args(damping, max_iter, convergence_iter, preference, seed)
    M = S if hasattr(S, "is_cuda") else np.asarray(S, dtype=np.float64)
    if M.ndim != 2 or M.shape[0] != M.shape[1] or M.shape[0] < 1:
        raise ValueError("S must be a non-empty square matrix, got shape %r" % (tuple(M.shape),))
    if not bool(np.isfinite(M).all() if isinstance(M, np.ndarray) else M.isfinite().all()):
        raise ValueError("S holds non-finite values")
    return _affinity(dict(S=_device_tensor(M, _lib.require_gpu().float64, device)), damping, max_iter, convergence_iter, preference, seed)


def affinity_propagation_predict(features, centers, device=None) -> np.ndarray:
    """AffinityPropagation.predict: the index of the nearest of ``centers`` [K, d] (the exemplars' rows, cluster_centers_) for every row of
    ``features`` [n, d], the lowest index among equal distances -> int64 [n]; all -1 when the fit had no centre (K = 0)."""
    centers = centers if hasattr(centers, "is_cuda") else np.asarray(centers, dtype=np.float64)
    if centers.ndim != 2:
        raise ValueError("centers must be [K, d]")
    if centers.shape[0] == 0:
        n = features.shape[0] if hasattr(features, "shape") else len(features)
        return np.full(n, -1, dtype=np.int64)
    return mean_shift_predict(features, centers, device=device)


def cluster_faces_affinity_propagation(features, all_indices=None, min_cluster_size: int = 1, split: str = "host",
                                       damping=AFFINITY_DAMPING, max_iter=AFFINITY_MAX_ITER, convergence_iter=AFFINITY_CONVERGENCE_ITER,
                                       preference=None, seed=0, device=None) -> List[List[int]]:
    """The scikit-learn branch of the reference's get_facial_clusters with its affinity-propagation row (facial_clustering_test.py:263,
    265-266, 285): the members of every label >= 0 of affinity_propagation(features, ...), the largest cluster first (a stable sort of
    the clusters in label order), as lists of ints.  ``all_indices``, ``split`` and ``min_cluster_size`` as in cluster_faces_mean_shift."""
    _check_affinity_args(damping, max_iter, convergence_iter, preference, seed)
    _check_split(split)
    x, _, _ = _features(features, None, None, device, finite=True)
    labels = _affinity(dict(x=x), damping, max_iter, convergence_iter, preference, seed)[1]
    return _label_clusters(x, labels, all_indices, min_cluster_size, split)


# ---- scoring --------------------------------------------------------------------------------------------------------
def bcubed(y_true: Sequence, y_pred: Sequence):
    """Extended B-cubed of the clustering study (facial_clustering_test.py:321-359, one label per item) -> (precision, recall, f).
    In the study's naming, precision averages over items the share of their TRUE class that shares their predicted cluster, recall
    the share of their predicted cluster that shares their true class; f is their harmonic mean.  From the contingency table."""
    y_true, y_pred = np.asarray(y_true).reshape(-1), np.asarray(y_pred).reshape(-1)
    if len(y_true) != len(y_pred) or len(y_true) == 0:
        raise ValueError("bcubed: %d true labels, %d predicted" % (len(y_true), len(y_pred)))
    _, t = np.unique(y_true, return_inverse=True)
    _, p = np.unique(y_pred, return_inverse=True)
    t, p = t.reshape(-1), p.reshape(-1)
    cells = t.astype(np.int64) * (int(p.max()) + 1) + p
    _, cell, both = np.unique(cells, return_inverse=True, return_counts=True)
    both = both[cell.reshape(-1)].astype(np.float64)
    prec = float(np.mean(both / np.bincount(t)[t]))
    rec = float(np.mean(both / np.bincount(p)[p]))
    return prec, rec, 2.0 * prec * rec / (prec + rec)


# ---- the study's statistics on the device: one sweep, one read-back ----------------------------------------------------
# get_clustering_statistics' ten numbers, in test_avg_clustering's order (facial_clustering_test.py:435)
STATS_NAMES = ("classes", "clusters", "ARI", "AMI", "homogeneity", "completeness", "v-measure", "BCubed_precision", "BCubed_recall",
               "BCubed_FMeasure")
# test_avg_clustering_with_model_selection's grids and bounds (:447-499)
SWEEP_THRESHOLDS = np.linspace(0.6, 1.3, 71)
SWEEP_DROP = 0.01
SWEEP_CEILING = 0.85
RANK_ORDER_SWEEP_NORMS = np.linspace(1.02, 1.1, 9)
RANK_ORDER_SWEEP_RANKS = tuple(range(12, 22, 2))
# which of ops.partition_scores' three cluster counts is the reference's len(clusters): every flat cluster of a linkage cut, the
# non-noise clusters of DBSCAN, rank-order's clusters of at least two faces
_CLUSTERS_COLUMN = {"dbscan": 3, "rankorder": 2}
_EPS = float(np.finfo(np.float64).eps)


def scores_from_counts(counts_row, stats_row, n):
    """One row of ops.partition_scores (8 counts, 6 sums) for n items -> (ARI, AMI, homogeneity, completeness, v-measure,
    BCubed_precision, BCubed_recall, BCubed_FMeasure) as Python floats, the last eight of STATS_NAMES: scikit-learn 1.7's
    adjusted_rand_score, adjusted_mutual_info_score(average_method='arithmetic') and homogeneity_completeness_v_measure with their
    special cases, and bcubed's three numbers.  ARI is exact integer arithmetic up to scikit-learn's own final expression."""
    R, C, _, _, _, s_nij2, s_a2, s_b2 = (int(v) for v in counts_row)
    h_true, h_pred, mi, emi, bc_p, bc_r = (float(v) for v in stats_row)
    N = int(n)
    tp = s_nij2 - N
    fp = s_a2 - s_nij2
    fn = s_b2 - s_nij2
    tn = N * N - fp - fn - s_nij2
    if fn == 0 and fp == 0:
        ari = 1.0
    else:
        ari = 2.0 * (tp * tn - fn * fp) / ((tp + fn) * (fn + tn) + (tp + fp) * (fp + tn))
    mi = 0.0 if R == 1 or C == 1 else max(mi, 0.0)
    homogeneity = mi / h_true if h_true else 1.0
    completeness = mi / h_pred if h_pred else 1.0
    if homogeneity + completeness == 0.0:
        v_measure = 0.0
    else:
        v_measure = 2.0 * homogeneity * completeness / (homogeneity + completeness)
    if R == 1 and C == 1:
        ami = 1.0
    elif R == 1 or C == 1:
        ami = 0.0
    else:
        denominator = 0.5 * (h_true + h_pred) - emi
        denominator = min(denominator, -_EPS) if denominator < 0 else max(denominator, _EPS)
        numerator = mi - emi
        numerator = min(numerator, -_EPS) if numerator < 0 else max(numerator, _EPS)
        ami = numerator / denominator
    return (float(ari), float(ami), float(homogeneity), float(completeness), float(v_measure), bc_p, bc_r,
            2.0 * bc_p * bc_r / (bc_p + bc_r))


def _dense_labels(y, what):
    y = np.asarray(y).reshape(-1)
    if len(y) == 0:
        raise ValueError("%s is empty" % what)
    return np.unique(y, return_inverse=True)[1].reshape(-1).astype(np.int32)


def _score_rows(y_true, labels, clusters_column=1):
    """y_true int32 [n] (host) and labels int32 [rows, n] (device) -> float64 [rows, 10] in STATS_NAMES order: one
    ops.partition_scores call and one read-back."""
    from . import ops
    import torch
    n = labels.shape[1]
    if len(y_true) != n:
        raise ValueError("%d true labels for %d faces" % (len(y_true), n))
    counts, stats = ops.partition_scores(torch.from_numpy(y_true).to(labels.device), labels)
    packed = torch.cat([counts, stats.view(torch.int64)], dim=1).cpu().numpy()
    counts, stats = packed[:, :8], np.ascontiguousarray(packed[:, 8:]).view(np.float64)
    out = np.empty((len(counts), len(STATS_NAMES)), dtype=np.float64)
    for r in range(len(counts)):
        out[r, 0] = counts[r, 0]
        out[r, 1] = counts[r, clusters_column]
        out[r, 2:] = scores_from_counts(counts[r], stats[r], n)
    return out


def clustering_scores(y_true, y_pred, device=None) -> np.ndarray:
    """get_clustering_statistics' ten numbers (STATS_NAMES) for one labelling, scored on the device: y_true and y_pred are sequences
    of n labels of any kind, compared for equality only; 'clusters' is the number of distinct predicted labels."""
    from . import _lib
    torch = _lib.require_gpu()
    t, p = _dense_labels(y_true, "y_true"), _dense_labels(y_pred, "y_pred")
    if len(t) != len(p):
        raise ValueError("%d true labels, %d predicted" % (len(t), len(p)))
    return _score_rows(t, torch.from_numpy(p).to(_lib.cuda_device(device))[None])[0]


def mean_shift_scores(features, y_true, bandwidths, device=None) -> np.ndarray:
    """get_clustering_statistics' ten numbers (STATS_NAMES) of mean_shift(features, bandwidth) for every bandwidth -> float64
    [len(bandwidths), 10]: the row of a bandwidth is clustering_scores(y_true, its labels)."""
    bandwidths = list(bandwidths) if isinstance(bandwidths, (list, tuple)) else list(np.asarray(bandwidths).reshape(-1))
    for b in bandwidths:
        _check_mean_shift_args(b, 300)
    bandwidths = [float(b) for b in bandwidths]
    x, _, _ = _features(features, None, None, device, finite=True)
    if len(np.asarray(y_true).reshape(-1)) != x.shape[0]:
        raise ValueError("%d true labels for %d faces" % (len(np.asarray(y_true).reshape(-1)), x.shape[0]))
    out = np.empty((len(bandwidths), len(STATS_NAMES)), dtype=np.float64)
    for r, b in enumerate(bandwidths):
        out[r] = clustering_scores(y_true, _mean_shift(x, b, 300, True)[1], device=x.device)
    return out


def affinity_propagation_scores(features, y_true, preferences, damping=AFFINITY_DAMPING, max_iter=AFFINITY_MAX_ITER,
                                convergence_iter=AFFINITY_CONVERGENCE_ITER, seed=0, device=None) -> np.ndarray:
    """get_clustering_statistics' ten numbers (STATS_NAMES) of affinity_propagation(features, preference=p) for every preference (None: the
    median) -> float64 [len(preferences), 10]: the row of a preference is clustering_scores(y_true, its labels)."""
    preferences = list(preferences) if isinstance(preferences, (list, tuple)) else list(np.asarray(preferences).reshape(-1))
    for p in preferences:
        _check_affinity_args(damping, max_iter, convergence_iter, p, seed)
    x, _, _ = _features(features, None, None, device, finite=True)
    if len(np.asarray(y_true).reshape(-1)) != x.shape[0]:
        raise ValueError("%d true labels for %d faces" % (len(np.asarray(y_true).reshape(-1)), x.shape[0]))
    out = np.empty((len(preferences), len(STATS_NAMES)), dtype=np.float64)
    for r, p in enumerate(preferences):
        labels = _affinity(dict(x=x), damping, max_iter, convergence_iter, None if p is None else float(p), seed)[1]
        out[r] = clustering_scores(y_true, labels, device=x.device)
    return out


def _sweep_labels(source, method, thresholds, born_years, photo_years, dense, min_samples, device):
    """One clustering of the album -> labels int32 [len(thresholds), n] on the device"""
    from . import ops
    import torch
    if method == "rankorder":
        pairs = _rank_order_pairs(None, None, thresholds)[0]
    else:
        ts = np.asarray(thresholds, dtype=np.float64).reshape(-1)
        if len(ts) == 0 or not np.isfinite(ts).all():
            raise ValueError("threshold_sweep: thresholds must be a non-empty sequence of finite numbers")
        if method == "dbscan":
            for eps in ts:
                _check_dbscan_args(float(eps), min_samples)
    negative = None if method in LINKAGE_METHODS + GEOMETRIC_METHODS else "dist_matrix holds negative values"
    if dense:
        src = dict(dense=_dist_matrix(source, device, negative))
        n, dev = src["dense"].shape[0], src["dense"].device
    else:
        x, born, year = _features(source, born_years, photo_years, device, finite=True)
        src = dict(x=x, born=born, year=year)
        n, dev = x.shape[0], x.device
    if method == "rankorder":
        return ops.rank_order_labels(thresholds=pairs, **src)[0]
    if method == "dbscan":
        return torch.stack([ops.dbscan_labels(eps=float(eps), min_samples=min_samples, **src)[0] for eps in ts])
    if n == 1:
        return torch.ones((len(ts), 1), dtype=torch.int32, device=dev)
    order, gaps = _cut_order(_linkage(method, n, **src))
    return ops.flat_cuts(torch.from_numpy(order.astype(np.int32)).to(dev), torch.from_numpy(gaps).to(dev), torch.from_numpy(ts).to(dev))


def threshold_sweep(source, y_true, method, thresholds, born_years=None, photo_years=None, dense=False, min_samples=1,
                    device=None) -> np.ndarray:
    """get_clustering_statistics (facial_clustering_test.py:416-423) for every threshold of a sweep over one album -> float64
    [len(thresholds), 10] in STATS_NAMES order.  ``source`` is the features [n, d] (with optional born / photo years) or, with
    ``dense=True``, the distance matrix, as linkage / linkage_dense take them.  The album is clustered once: a linkage method's
    dendrogram is cut at all thresholds on the device (ops.flat_cuts), 'dbscan' gives one labelling per eps (``min_samples`` as
    get_facial_clusters' no_images_in_cluster), 'rankorder' takes (norm, rank) pairs through one matrix build; every row is scored by
    one ops.partition_scores call and read back once.  Faces outside every cluster (DBSCAN's noise, rank-order's single faces) are
    clusters of their own, as the study's y_pred has them, and 'clusters' is the reference's len(clusters): every flat cluster of a
    linkage cut, DBSCAN's non-noise clusters, rank-order's clusters of at least two faces.  ``method`` may also be one of
    GEOMETRIC_METHODS ('centroid', 'median', 'ward': linkage_geometric's trees), cut and scored as the other linkages' are."""
    _check_method(method, CLUSTER_METHODS + GEOMETRIC_METHODS)
    t = _dense_labels(y_true, "y_true")
    labels = _sweep_labels(source, method, thresholds, born_years, photo_years, dense, min_samples, device)
    return _score_rows(t, labels, _CLUSTERS_COLUMN.get(method, 1))


def select_from_curve(thresholds, statistic, drop=SWEEP_DROP, ceiling=SWEEP_CEILING):
    """The scalar loop of test_avg_clustering_with_model_selection (:476-495) over a statistic known at every threshold ->
    (best threshold, best statistic, points evaluated): the best is replaced on '>' (it starts as threshold 0 with statistic 0), and
    the point after which the loop stops -- the statistic fell more than ``drop`` below the previous point's, or exceeds ``ceiling``
    -- is still evaluated and may be the best."""
    best, best_threshold, prev, evaluated = 0, 0, 0, 0
    for threshold, current in zip(thresholds, statistic):
        evaluated += 1
        if current > best:
            best, best_threshold = current, threshold
        if current < prev - drop:
            break
        if current > ceiling:
            break
        prev = current
    return best_threshold, best, evaluated


def select_from_grid(norm_thresholds, rank_thresholds, statistic):
    """The rank-order loops of test_avg_clustering_with_model_selection (:451-474) over a statistic [norms, ranks] known on the whole
    grid -> (best (norm, rank), best statistic, the (i, j) grid points evaluated, in order): the best is replaced on '>' (it starts as
    (0, 0) with statistic 0); a row of rank thresholds ends after a point that is not above the one before it (the first is compared
    with 0), and the norm thresholds end after a row that did not replace the best."""
    best, best_threshold, evaluated = 0, (0, 0), []
    for i, norm in enumerate(norm_thresholds):
        prev, changed = 0, False
        for j, rank in enumerate(rank_thresholds):
            current = statistic[i][j]
            evaluated.append((i, j))
            if current > best:
                best, best_threshold, changed = current, (norm, rank), True
            if current <= prev:
                break
            prev = current
        if not changed:
            break
    return best_threshold, best, evaluated


class Selection(NamedTuple):
    """select_threshold's result"""
    threshold: object           # the best threshold (a (norm, rank) pair for rank-order)
    statistic: float            # the selection statistic there, averaged over the albums
    evaluated: list             # [(threshold, statistic)] for the points the reference would have evaluated, in its order
    mean: np.ndarray            # test_avg_clustering's np.mean of STATS_NAMES over the albums at the best threshold
    std: np.ndarray             # and its np.std


def select_threshold(albums, method, thresholds=None, drop=SWEEP_DROP, ceiling=SWEEP_CEILING, norm_thresholds=None,
                     rank_thresholds=None, dense=False, min_samples=1, device=None) -> Selection:
    """test_avg_clustering_with_model_selection (facial_clustering_test.py:447-499) with val_dirs_count = len(albums) (the
    reference's own "hack"): ``albums`` is a list of (source, y_true), each source as threshold_sweep takes it.  Linkage methods and
    'dbscan' sweep ``thresholds`` (default np.linspace(0.6, 1.3, 71)) for the study's B-cubed "precision" averaged over the albums
    with select_from_curve's rules (``drop``, ``ceiling``); 'rankorder' sweeps ``norm_thresholds`` x ``rank_thresholds`` (defaults
    np.linspace(1.02, 1.1, 9) x range(12, 22, 2)) for the V-measure with select_from_grid's.  Every album is clustered and scored once
    on the whole grid (threshold_sweep) and the reference's stopping rules are applied to the resulting arrays, which gives the
    reference's answer.  Returns a Selection: the best threshold, its statistic, the (threshold, statistic) points the reference
    would have evaluated, and test_avg_clustering's mean and standard deviation of the ten statistics over the albums at the best
    threshold.  When no point scores above 0 the reference goes on with its initial threshold 0: a linkage method is cut there;
    'dbscan' and 'rankorder', which accept no zero threshold, raise ValueError.  For 'centroid', 'median' and 'ward' apply
    select_from_curve to a threshold_sweep, which takes those names."""
    _check_method(method, CLUSTER_METHODS)
    albums = list(albums)
    if not albums:
        raise ValueError("select_threshold: no albums")
    kw = dict(dense=dense, min_samples=min_samples, device=device)
    if method == "rankorder":
        norms = list(RANK_ORDER_SWEEP_NORMS if norm_thresholds is None else norm_thresholds)
        ranks = list(RANK_ORDER_SWEEP_RANKS if rank_thresholds is None else rank_thresholds)
        grid = [(norm, rank) for norm in norms for rank in ranks]
        column = STATS_NAMES.index("v-measure")
    else:
        grid = list(SWEEP_THRESHOLDS if thresholds is None else thresholds)
        column = STATS_NAMES.index("BCubed_precision")
    tables = [threshold_sweep(source, y_true, method, grid, **kw) for source, y_true in albums]
    statistic = np.zeros(len(grid))
    for table in tables:                         # the reference's running sum over the albums, then one division
        statistic = statistic + table[:, column]
    statistic = statistic / len(albums)
    if method == "rankorder":
        best_threshold, best, points = select_from_grid(norms, ranks, statistic.reshape(len(norms), len(ranks)))
        points = [i * len(ranks) + j for i, j in points]
    else:
        best_threshold, best, count = select_from_curve(grid, statistic, drop, ceiling)
        points = list(range(count))
    evaluated = [(grid[k], float(statistic[k])) for k in points]
    at_best = [k for k in points if grid[k] == best_threshold]
    if at_best:
        rows = np.stack([table[at_best[0]] for table in tables])
    elif method not in LINKAGE_METHODS:
        raise ValueError("select_threshold: no point of the %s sweep scored above 0, so nothing was selected (the reference would go on "
                         "with its initial threshold %r, which that clustering does not accept)" % (method, best_threshold))
    else:                                        # nothing scored above 0: the reference goes on with its initial threshold 0
        rows = np.stack([threshold_sweep(source, y_true, method, [best_threshold], **kw)[0] for source, y_true in albums])
    return Selection(best_threshold, float(best), evaluated, np.mean(rows, axis=0), np.std(rows, axis=0))
