"""Host restatements for the centroid / median / Ward linkage tests (libhsefr_geom.so): the three update rules of scipy's
_hierarchy_distance_update.pxi operation by operation with the library's clamp, the primitive closest-pair algorithm of
csrc/geom_linkage.hip (centroid, median) and the reciprocal-nearest-neighbour rounds of csrc/hier_linkage.hip with Ward's three-term
rule, both with merge records in the device's format, and the inputs the CPU and the GPU suite share.  fp64, NumPy only."""
import numpy as np

from hier_linkage_ref import upper_symmetric

METHODS = ("centroid", "median", "ward")
# the dense cases of the GPU suite: every n on both sides of the one-workgroup class (128) and of a 256-column workgroup
DENSE_NS = (2, 3, 5, 64, 127, 128, 129, 257, 600)
DENSE_DS = (2, 16)
WARD_EXTRA_NS = (1000,)
# a case whose restatement is not scipy's Z on the CPU is not tie-free: give it another seed here (none needed so far)
SEED_OVERRIDES = {}


def case_seed(n, d):
    return SEED_OVERRIDES.get((n, d), 1000 * d + n)


def euclidean(n, d, seed):
    """Euclidean distances of Gaussian points (the one input built with scipy: its pdist, so that the matrix is the one a user of
    hac.linkage would have)."""
    from scipy.spatial.distance import pdist, squareform
    return squareform(pdist(np.random.default_rng(seed).standard_normal((n, d))))


def _root(r):
    """-> (sqrt(max(r, 0)), the number of strictly negative radicands)"""
    r = np.asarray(r, dtype=np.float64)
    return np.sqrt(np.maximum(r, 0.0)), int(np.count_nonzero(r < 0))


def centroid(dxi, dyi, dxy, sx, sy):
    return _root(((sx * dxi * dxi + sy * dyi * dyi) - (sx * sy * dxy * dxy) / (sx + sy)) / (sx + sy))


def median(dxi, dyi, dxy):
    return _root(0.5 * (dxi * dxi + dyi * dyi) - 0.25 * dxy * dxy)


def ward(dxi, dyi, dxy, sx, sy, si):
    t = 1.0 / (sx + sy + si)
    return _root((si + sx) * t * dxi * dxi + (si + sy) * t * dyi * dyi - si * t * dxy * dxy)


def closest_pair_sequence(D, method, return_clamps=False):
    """The primitive algorithm: n - 1 steps, each merging the least pair under the total order (distance, lower slot, higher slot);
    with x < y the pair, the merged cluster is kept in slot y.  -> (a, b, h) arrays of the n - 1 records in merge order (and the
    number of radicands clamped at zero)."""
    W = upper_symmetric(D)                          # diagonal +inf; dead rows and columns become +inf too
    n = W.shape[0]
    alive = np.ones(n, dtype=bool)
    size = np.ones(n, dtype=np.int64)
    a, b, h, clamps = [], [], [], 0
    for _ in range(n - 1):
        x, y = divmod(int(np.argmin(W)), n)         # the first least entry in row-major order: least (value, row, column), row < column
        assert x < y and alive[x] and alive[y]
        dxy = W[x, y]
        a.append(x)
        b.append(y)
        h.append(dxy)
        others = alive.copy()
        others[[x, y]] = False
        idx = np.flatnonzero(others)
        if method == "centroid":
            v, c = centroid(W[x, idx], W[y, idx], dxy, int(size[x]), int(size[y]))
        elif method == "median":
            v, c = median(W[x, idx], W[y, idx], dxy)
        else:
            raise ValueError(method)
        clamps += c
        W[y, idx] = v
        W[idx, y] = v
        W[x, :] = np.inf
        W[:, x] = np.inf
        alive[x] = False
        size[y] += size[x]
    out = (np.array(a, dtype=np.int64), np.array(b, dtype=np.int64), np.array(h, dtype=np.float64))
    return out + (clamps,) if return_clamps else out


def ward_rounds(D, return_clamps=False):
    """hier_linkage_ref.rnn_rounds with Ward's three-term rule: every round merges all reciprocal nearest-neighbour pairs, the lower
    slot surviving; the pairs of a round are applied one after the other, the lower survivor's first, each as scipy's update of the
    clusters alive at that moment.  -> (a, b, h, round) arrays of the n - 1 records, in round order."""
    W = upper_symmetric(D)
    n = W.shape[0]
    alive = np.ones(n, dtype=bool)
    size = np.ones(n, dtype=np.int64)
    recs, clamps, rnd = [], 0, 0
    while alive.sum() > 1:
        M = np.where(alive[None, :], W, np.inf)
        nn = np.full(n, -1)
        for i in np.flatnonzero(alive):
            nn[i] = int(np.argmin(M[i]))            # argmin takes the lowest index among equal values
        pairs = [(i, int(nn[i])) for i in np.flatnonzero(alive) if nn[nn[i]] == i and i < nn[i]]
        assert pairs, "no reciprocal pair"
        for x, y in pairs:
            recs.append((x, y, W[x, y], rnd))
        for x, y in pairs:
            others = alive.copy()
            others[[x, y]] = False
            idx = np.flatnonzero(others)
            v, c = ward(W[x, idx], W[y, idx], W[x, y], int(size[x]), int(size[y]), size[idx])
            clamps += c
            W[x, idx] = v
            W[idx, x] = v
            alive[y] = False
            size[x] += size[y]
        rnd += 1
    if not recs:
        out = (np.zeros(0, np.int64), np.zeros(0, np.int64), np.zeros(0), np.zeros(0, np.int64))
    else:
        a, b, h, r = zip(*recs)
        out = (np.array(a), np.array(b), np.array(h, dtype=np.float64), np.array(r))
    return out + (clamps,) if return_clamps else out


def signed_symmetric(n, seed):
    """Gaussian entries: no ties, not Euclidean, and half of them negative.  The pair that merges is the least entry of the matrix, so
    on non-negative distances no radicand of the three rules can be negative (dxy <= dxi, dyi); a negative least entry has a large
    square, and that is where scipy's sqrt gives NaN."""
    U = np.triu(np.random.RandomState(seed).randn(n, n), 1)
    return U + U.T


CLAMP_CASE = (7, 0)     # (n, seed) of clamp_case(): what clamp_search(7) finds first


def clamp_search(n, seeds=range(100)):
    """The first seed whose signed_symmetric(n, seed) makes the centroid restatement clamp a radicand -> (seed, D)"""
    for seed in seeds:
        D = signed_symmetric(n, seed)
        if closest_pair_sequence(D, "centroid", return_clamps=True)[3] > 0:
            return seed, D
    raise AssertionError("no clamping matrix among the seeds")


def clamp_case():
    return signed_symmetric(*CLAMP_CASE)
