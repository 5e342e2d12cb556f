"""hsefr_rbf_svm_fit / _decision / _predict's contract restated in NumPy float64: libsvm's C-SVC with the RBF kernel, one-vs-one.  For the
pair (i, j), i < j, class i is +1 and the dual  min 1/2 a^T Q a - e^T a,  0 <= a <= C,  y^T a = 0,  Q_ab = y_a y_b exp(-gamma |x_a - x_b|^2)
is solved to m(a) - M(a) <= tol by SMO with libsvm's second-order working set selection (pairs of equal class sizes advance together,
one NumPy operation for all of them); rho by libsvm's rule.  Layouts are libsvm's: dual_coef [(K - 1), n] in the caller's row order (row r
of column a: the opponent class r if r < labels[a], else r + 1), rho and decisions in the pair order (0,1), (0,2), ..., (1,2), ..."""
import numpy as np


def gamma_scale(X):
    """SVC(gamma='scale'): 1 / (d Var(X)) over all elements of the float64 copy; 1.0 where the variance is 0."""
    X = np.asarray(X, dtype=np.float64)
    var = X.var()
    return 1.0 / (X.shape[1] * var) if var > 0 else 1.0


def kernel(A, B, gamma):
    """exp(-gamma max(0, |a|^2 + |b|^2 - 2 <a, b>)): libsvm's own formula, float64."""
    A, B = np.asarray(A, dtype=np.float64), np.asarray(B, dtype=np.float64)
    d2 = (A * A).sum(1)[:, None] + (B * B).sum(1)[None, :] - 2.0 * (A @ B.T)
    return np.exp(-gamma * np.maximum(d2, 0.0))


def gram(X, gamma):
    """The training kernel matrix as libsvm holds it: every entry rounded to float32 (its Qfloat cache type -- the objective SVC minimises
    has THIS Q; against the unrounded one its optimum sits about 1e-8 off in decision values), the diagonal exactly 1."""
    G = kernel(X, X, gamma).astype(np.float32).astype(np.float64)
    np.fill_diagonal(G, 1.0)
    return G


def pair_list(K):
    return [(i, j) for i in range(K) for j in range(i + 1, K)]


def pair_index(i, j, K):
    return i * K - i * (i + 1) // 2 + (j - i - 1)


def rho_of(alpha, grad, y, C):
    """libsvm's calculate_rho: the mean of y G over the free variables, without one the midpoint of the bounded ones' range."""
    yg = y * grad
    free = (alpha > 0) & (alpha < C)
    if free.any():
        return float(yg[free].mean())
    upper, lower = alpha >= C, alpha <= 0
    ub = np.min(yg[(upper & (y < 0)) | (lower & (y > 0))], initial=np.inf)
    lb = np.max(yg[(upper & (y > 0)) | (lower & (y < 0))], initial=-np.inf)
    return float((ub + lb) / 2.0)


def solve_pairs(Kb, y, C, tol, max_iter=10 ** 6):
    """Kb [B, m, m]: the kernel matrices of B pairs whose m rows carry the same signs y [m].  Returns (alpha [B, m], iterations [B])."""
    B, m = Kb.shape[0], Kb.shape[1]
    rows = np.arange(B)
    alpha, grad = np.zeros((B, m)), -np.ones((B, m))
    iters = np.zeros(B, dtype=np.int64)
    pos = (y > 0)[None, :]
    for _ in range(max_iter):
        up = np.where(pos, alpha < C, alpha > 0)
        low = np.where(pos, alpha > 0, alpha < C)
        yg = y * grad
        vi = np.where(up, -yg, -np.inf)
        i = vi.argmax(1)
        gmax = vi[rows, i]
        gmax2 = np.where(low, yg, -np.inf).max(1)
        active = gmax + gmax2 > tol
        if not active.any():
            break
        Ki = Kb[rows, i]
        diff = gmax[:, None] + yg
        quad = 2.0 - 2.0 * Ki
        quad[quad <= 0] = 1e-12
        with np.errstate(invalid="ignore"):
            gain = np.where(low & (diff > 0), diff * diff / quad, -np.inf)
        j = gain.argmax(1)
        Kj = Kb[rows, j]
        yi, yj = y[i], y[j]
        ai, aj = alpha[rows, i], alpha[rows, j]
        # along a_i += y_i t, a_j -= y_j t: the unconstrained step, cut where either variable meets a bound
        t = (gmax + yg[rows, j]) / quad[rows, j]
        t = np.minimum(t, np.where(yi > 0, C - ai, ai))
        t = np.minimum(t, np.where(yj > 0, aj, C - aj))
        t = np.where(active, np.maximum(t, 0.0), 0.0)
        alpha[rows, i] = np.clip(ai + yi * t, 0.0, C)
        alpha[rows, j] = np.clip(aj - yj * t, 0.0, C)
        grad += y[None, :] * t[:, None] * (Ki - Kj)
        iters += active
    return alpha, iters


def fit(X, labels, K, gamma, C=1.0, tol=1e-12):
    """Returns (dual_coef [(K - 1), n], rho [K (K - 1) / 2], alpha-per-pair dict {(i, j): (rows, y, alpha, fresh gradient)}, the most
    iterations of any pair)."""
    X, labels = np.asarray(X, dtype=np.float64), np.asarray(labels)
    n = len(labels)
    G = gram(X, gamma)
    members = [np.nonzero(labels == c)[0] for c in range(K)]
    dual_coef, rho, pairs = np.zeros((K - 1, n)), np.zeros(K * (K - 1) // 2), {}
    groups = {}
    for i, j in pair_list(K):
        groups.setdefault((len(members[i]), len(members[j])), []).append((i, j))
    most = 0
    for (ni, nj), members_of in groups.items():
        y = np.concatenate([np.ones(ni), -np.ones(nj)])
        idx = np.array([np.concatenate([members[i], members[j]]) for i, j in members_of])
        Kb = G[idx[:, :, None], idx[:, None, :]]
        alpha, iters = solve_pairs(Kb, y, C, tol)
        most = max(most, int(iters.max()))
        fresh = y[None, :] * np.einsum("bst,bt->bs", Kb, alpha * y[None, :]) - 1.0      # Q a - e from the final a
        for b, (i, j) in enumerate(members_of):
            r = rho_of(alpha[b], fresh[b], y, C)
            rho[pair_index(i, j, K)] = r
            dual_coef[j - 1, members[i]] = alpha[b, :ni]
            dual_coef[i, members[j]] = -alpha[b, ni:]
            pairs[(i, j)] = (idx[b], y, alpha[b], fresh[b], r)
    return dual_coef, rho, pairs, most


def decision(Q, X, labels, K, gamma, dual_coef, rho):
    """[nq, K (K - 1) / 2]: sum over the rows a of classes i and j of dual_coef[.][a] k(q, a) - rho_ij."""
    labels = np.asarray(labels)
    KQ = kernel(Q, X, gamma)
    out = np.zeros((KQ.shape[0], K * (K - 1) // 2))
    # S[c][q][r] = sum over the rows a of class c of dual_coef[r][a] k(q, a)
    S = [KQ[:, labels == c] @ dual_coef[:, labels == c].T for c in range(K)]
    for i in range(K - 1):
        js = np.arange(i + 1, K)
        first = S[i][:, js - 1]
        second = np.stack([S[j][:, i] for j in js], axis=1)
        p0 = pair_index(i, i + 1, K)
        out[:, p0:p0 + len(js)] = first + second - rho[None, p0:p0 + len(js)]
    return out


def votes_of(dec, K):
    """libsvm's vote: a decision > 0 for i, anything else (exactly 0 too) for j.  Returns (votes [nq, K], the FIRST class with the most)."""
    votes = np.zeros((dec.shape[0], K), dtype=np.int32)
    p = 0
    for i in range(K - 1):
        width = K - 1 - i
        win = dec[:, p:p + width] > 0
        votes[:, i] += win.sum(1)
        votes[:, i + 1:] += ~win
        p += width
    return votes, votes.argmax(1).astype(np.int32)


def kkt_violation(X, labels, dual_coef, gamma, C):
    """Per pair in libsvm's order, from a fresh Q a - e of the given dual_coef: (m - M [P], |y^T a| [P], all of 0 <= a <= C [P] bool)."""
    X, labels = np.asarray(X, dtype=np.float64), np.asarray(labels)
    K = dual_coef.shape[0] + 1
    G = gram(X, gamma)
    members = [np.nonzero(labels == c)[0] for c in range(K)]
    gap, balance, inside = [], [], []
    for i, j in pair_list(K):
        rows = np.concatenate([members[i], members[j]])
        y = np.concatenate([np.ones(len(members[i])), -np.ones(len(members[j]))])
        ya = np.concatenate([dual_coef[j - 1, members[i]], dual_coef[i, members[j]]])
        alpha = y * ya
        yg = y * (y * (G[np.ix_(rows, rows)] @ ya) - 1.0)
        up = np.where(y > 0, alpha < C, alpha > 0)
        low = np.where(y > 0, alpha > 0, alpha < C)
        m = np.max(-yg[up], initial=-np.inf)
        M = np.min(-yg[low], initial=np.inf)
        gap.append(m - M)
        balance.append(abs(ya.sum()))
        inside.append(bool(((alpha >= 0) & (alpha <= C)).all()))
    return np.array(gap), np.array(balance), np.array(inside)


def bounded_slack(pairs, C):
    """The smallest distance of a bounded variable from its KKT threshold over all pairs: |y f(x) - 1| = |G - y rho| at a = 0 or a = C."""
    least = np.inf
    for rows, y, alpha, grad, rho in pairs.values():
        bounded = (alpha <= 0) | (alpha >= C)
        if bounded.any():
            least = min(least, float(np.abs(grad - y * rho)[bounded].min()))
    return least


def decision_bound(X, labels, gamma, pairs, eps, C=1.0):
    """How far a pair's decision value can be from the optimum's when the stopping violation is <= eps and the bounded set is the
    reference's.  With F the free set of a pair: restricted to that face Q_FF da + db y_F = r with |r_a| <= eps / 2 and da orthogonal to
    y_F, so |da|_2 <= (eps / 2) sqrt(n_F) |Q_FF^-1|_2; the kernel part of a decision (kernel values are at most 1) moves by at most
    |da|_1 <= (eps / 2) n_F |Q_FF^-1|_2, and rho by at most |Q_FF|_2 |da|_2 + eps / 2.  Returns (the largest sum of both over the pairs,
    the largest move of rho alone)."""
    X = np.asarray(X, dtype=np.float64)
    total, rho_part = 0.0, 0.0
    for rows, y, alpha, grad, rho in pairs.values():
        free = (alpha > 0) & (alpha < C)
        nf = int(free.sum())
        kern, r = 0.0, eps / 2.0
        if nf:
            ev = np.linalg.eigvalsh(gram(X[rows[free]], gamma))        # Q_FF = diag(y) K_FF diag(y): the same eigenvalues
            kern = (eps / 2.0) * nf / ev[0]
            r += ev[-1] * (eps / 2.0) * np.sqrt(nf) / ev[0]
        total, rho_part = max(total, kern + r), max(rho_part, r)
    return total, rho_part
