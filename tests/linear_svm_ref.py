"""hsefr_linear_svm_fit / _decision / _predict's contract restated in NumPy float64: LinearSVC()'s objective, one-vs-rest with the L2
penalty, the squared hinge loss and a bias that is regularised like any weight (liblinear; intercept_scaling = 1).  For class k, with
x~ = (x, 1) and y_ik = +1 where labels[i] == k, else -1,

    f_k(w~) = 1/2 |w~|^2 + C sum_i max(0, 1 - y_ik <w~, x~_i>)^2

is 1-strongly convex, so |w~ - w~*| <= |grad f_k(w~)| for any w~: every bound of the suites follows from a gradient evaluated here.
W [K', d + 1] holds (coef | intercept) row by row; K' = n_classes, except K' = 1 for two classes (the row of class 1)."""
import numpy as np


def signs(labels, n_classes):
    """Y [K', n] of +-1."""
    labels = np.asarray(labels)
    classes = np.array([1]) if n_classes == 2 else np.arange(n_classes)
    return np.where(labels[None, :] == classes[:, None], 1.0, -1.0)


def augmented(X):
    X = np.asarray(X, dtype=np.float64)
    return np.concatenate([X, np.ones((len(X), 1))], axis=1)


def pack(coef, intercept):
    return np.concatenate([np.asarray(coef, dtype=np.float64), np.asarray(intercept, dtype=np.float64)[:, None]], axis=1)


def objective(W, X, labels, n_classes, C=1.0):
    """f_k(W_k) for every class: [K']."""
    Y = signs(labels, n_classes)
    slack = np.maximum(0.0, 1.0 - Y * (W @ augmented(X).T))
    return 0.5 * (W * W).sum(1) + C * (slack * slack).sum(1)


def gradient(W, X, labels, n_classes, C=1.0):
    """grad f_k(W_k) for every class: [K', d + 1]."""
    Xa = augmented(X)
    Y = signs(labels, n_classes)
    S = W @ Xa.T
    R = np.where(1.0 - Y * S > 0.0, Y - S, 0.0)
    return W - 2.0 * C * (R @ Xa)


def fit(X, labels, n_classes, C=1.0, rtol=1e-12, max_iter=200):
    """Newton-CG from W = 0, every class at once, until |grad f_k| <= rtol |grad f_k(0)| for every k or until its floor in float64: a
    class ends when no step length t = 2^-m lowers its objective any more (the objective falls at every step; the gradient's norm
    need not, so it is no sign of the floor).
    Returns (coef [K',d], intercept [K'], info) with info["gradient_ratio"] = max_k |grad f_k| / |grad f_k(0)|."""
    Xa = augmented(X)
    Y = signs(labels, n_classes)
    K, d1 = len(Y), Xa.shape[1]
    W = np.zeros((K, d1))

    def grad(W):
        S = W @ Xa.T
        R = np.where(1.0 - Y * S > 0.0, Y - S, 0.0)
        return S, R, W - 2.0 * C * (R @ Xa)
    S, R, G = grad(W)
    g0 = np.sqrt((G * G).sum(1))
    stuck = np.zeros(K, bool)
    it = 0
    for it in range(1, max_iter + 1):
        gn = np.sqrt((G * G).sum(1))
        open_ = (gn > rtol * g0) & ~stuck
        if not open_.any():
            it -= 1
            break
        mask = (R != 0.0)
        D = np.zeros_like(W)
        Rc = -G.copy()
        P = Rc.copy()
        rs = (Rc * Rc).sum(1)
        live = open_.copy()
        for _ in range(4 * d1):
            if not live.any():
                break
            HP = P + 2.0 * C * ((mask * (P @ Xa.T)) @ Xa)
            alpha = np.where(live, rs / np.where(live, (P * HP).sum(1), 1.0), 0.0)
            D += alpha[:, None] * P
            Rc -= alpha[:, None] * HP
            rsn = (Rc * Rc).sum(1)
            live &= rsn > (1e-14 * gn) ** 2
            P = np.where(live[:, None], Rc + np.where(live, rsn / np.where(rs > 0, rs, 1.0), 0.0)[:, None] * P, P)
            rs = rsn
        Q = D @ Xa.T
        wd, dd, gd = (W * D).sum(1), (D * D).sum(1), (G * D).sum(1)
        t = np.ones(K)
        todo = open_ & (gd < 0.0)
        moved = np.zeros(K, bool)
        for _ in range(60):
            if not todo.any():
                break
            m = 1.0 - Y * S
            b = t[:, None] * Y * Q
            m2 = m - b
            both = (m > 0.0) & (m2 > 0.0)
            terms = np.where(both, b * (b - 2.0 * m), np.maximum(m2, 0.0) ** 2 - np.maximum(m, 0.0) ** 2)
            delta = t * wd + 0.5 * t * t * dd + C * terms.sum(1)
            ok = todo & (delta <= 1e-4 * t * gd)
            moved |= ok
            todo &= ~ok
            t = np.where(todo, 0.5 * t, t)
        stuck |= open_ & ~moved
        W = W + np.where(moved, t, 0.0)[:, None] * D
        S, R, G = grad(W)
    gn = np.sqrt((G * G).sum(1))
    ratio = float(np.max(gn / np.where(g0 > 0, g0, 1.0)))
    return W[:, :-1].copy(), W[:, -1].copy(), {"iterations": it, "gradient_ratio": ratio}


def decision(X, coef, intercept):
    """[n, K'] float64."""
    return np.asarray(X, dtype=np.float64) @ np.asarray(coef).T + np.asarray(intercept)[None, :]


def predict(dec):
    """np.argmax (the first maximum); K' = 1: decision > 0."""
    dec = np.asarray(dec)
    if dec.shape[1] == 1:
        return (dec[:, 0] > 0.0).astype(np.int32)
    return np.argmax(dec, axis=1).astype(np.int32)


def top_two_gap(dec):
    """Per row, the distance between the two largest decision values; K' = 1: the distance from the threshold, |decision|."""
    dec = np.asarray(dec)
    if dec.shape[1] == 1:
        return np.abs(dec[:, 0])
    s = np.sort(dec, axis=1)
    return s[:, -1] - s[:, -2]
