"""Host restatements for the average / complete / weighted linkage tests: the reciprocal-nearest-neighbour rounds of
csrc/hier_linkage.hip in NumPy (merge records in the device's format), and a replay of merge records that checks each merge against the
clusters alive in its round.  fp64, NumPy only."""
import numpy as np


def lw(method, dx, dy, sx, sy):
    """scipy's Lance-Williams updates (_hierarchy_distance_update.pxi)."""
    if method == "average":
        return (sx * dx + sy * dy) / (sx + sy)
    if method == "complete":
        return np.maximum(dx, dy)
    if method == "weighted":
        return 0.5 * (dx + dy)
    raise ValueError(method)


def upper_symmetric(D):
    D = np.asarray(D, dtype=np.float64)
    U = np.triu(D, 1)
    W = U + U.T
    np.fill_diagonal(W, np.inf)
    return W


def rnn_rounds(D, method):
    """The device scheme on the host: every round merges all reciprocal nearest-neighbour pairs (nearest = least (distance, index)),
    the lower slot surviving.  -> (a, b, h, round) arrays of the n - 1 records, in round order."""
    W = upper_symmetric(D)
    n = W.shape[0]
    alive = np.ones(n, dtype=bool)
    size = np.ones(n, dtype=np.int64)
    recs = []
    rnd = 0
    while alive.sum() > 1:
        M = np.where(alive[None, :], W, np.inf)
        nn = np.full(n, -1)
        for i in np.flatnonzero(alive):
            nn[i] = int(np.argmin(M[i]))            # argmin takes the lowest index among equal values
        pairs = [(i, int(nn[i])) for i in np.flatnonzero(alive) if nn[nn[i]] == i and i < nn[i]]
        assert pairs, "no reciprocal pair"
        for a, b in pairs:
            recs.append((a, b, W[a, b], rnd))
        for a, b in pairs:                          # sequential two-way updates (the same values as the device's four-way step)
            row = lw(method, W[a], W[b], size[a], size[b])
            W[a, :] = row
            W[:, a] = row
            W[a, a] = np.inf
            alive[b] = False
            size[a] += size[b]
        rnd += 1
    if not recs:
        return (np.zeros(0, np.int64), np.zeros(0, np.int64), np.zeros(0), np.zeros(0, np.int64))
    a, b, h, r = zip(*recs)
    return np.array(a), np.array(b), np.array(h, dtype=np.float64), np.array(r)


def check_records(D, method, a, b, h, r, rtol=1e-12):
    """Replays merge records round by round on the host from D's upper triangle: every merge's height is the method's fp64 distance
    between its two clusters, and the two were mutually nearest among the clusters alive when their round began."""
    W = upper_symmetric(D)
    n = W.shape[0]
    alive = np.ones(n, dtype=bool)
    size = np.ones(n, dtype=np.int64)
    members = {i: [i] for i in range(n)}
    U = upper_symmetric(D)
    np.fill_diagonal(U, 0)
    a, b, h, r = (np.asarray(v) for v in (a, b, h, r))
    assert len(a) == n - 1
    assert (a < b).all()
    for rnd in np.unique(r):
        idx = np.flatnonzero(r == rnd)
        M = np.where(alive[None, :], W, np.inf)
        for k in idx:
            x, y = int(a[k]), int(b[k])
            assert alive[x] and alive[y], (rnd, x, y)
            want = W[x, y]
            assert abs(h[k] - want) <= rtol * abs(want), (rnd, x, y, h[k], want)
            tol = rtol * abs(want)
            assert want <= M[x].min() + tol and want <= M[y].min() + tol, (rnd, x, y)
            blk = U[np.ix_(members[x], members[y])]
            if method == "complete":
                assert h[k] == blk.max()
            elif method == "average":
                assert abs(h[k] - blk.mean()) <= rtol * abs(blk.mean())
        for k in idx:
            x, y = int(a[k]), int(b[k])
            row = lw(method, W[x], W[y], size[x], size[y])
            W[x, :] = row
            W[:, x] = row
            W[x, x] = np.inf
            alive[y] = False
            size[x] += size[y]
            members[x] = members[x] + members.pop(y)
    assert alive.sum() == 1
