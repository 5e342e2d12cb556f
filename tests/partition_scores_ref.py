"""hsefr_partition_scores' and hsefr_flat_cuts' contracts restated in NumPy, and the error bounds their tests use.

A labelling is scored against y_true through the class sizes a_i, the cluster sizes b_j and the non-zero cells n_ij of the contingency
table; a negative predicted label is a cluster of its own.  The bounds are derived, not tuned (eps = 2^-52, N = n):
  * H_true, H_pred, MI and the two B-cubed sums are sums of at most n terms with sum |term| <= 2 ln N, each term a few correctly
    rounded operations: absolute bound (n + 8) eps 2 ln N.
  * EMI's terms carry exp() of nine lnGamma values of size at most N ln N each, so a relative 40 eps N ln N; on top comes the
    summation bound of the same kind as above over the T terms that are added, (T + 8) eps 2 ln N (sum |term| <= ln N because
    |ln(N k / (a b))| <= ln N and the weights k / N p(k) add up to 1).  For scikit-learn T counts its whole triple loop (emi_terms);
    the device and emi_grouped add one inner sum per pair of distinct sizes (emi_terms_grouped, far fewer), and that is the T they
    are held to.
  * AMI, homogeneity and completeness follow by propagation through their quotients.
"""
import numpy as np
from scipy.special import gammaln
from sklearn import metrics

EPS = 2.0 ** -52


def cluster_keys(labels):
    """int64 keys under which equal non-negative labels meet and every negative label stands alone"""
    labels = np.asarray(labels).astype(np.int64)
    return np.where(labels >= 0, labels, (1 << 31) + np.arange(len(labels), dtype=np.int64))


def table(y_true, labels):
    """-> (a [R], b [C], nij [cells], ci [cells], cj [cells], non-negative clusters): the sizes and the non-zero cells with their class
    and cluster indices"""
    y_true = np.asarray(y_true).astype(np.int64)
    keys = cluster_keys(labels)
    _, t, a = np.unique(y_true, return_inverse=True, return_counts=True)
    uk, p, b = np.unique(keys, return_inverse=True, return_counts=True)
    t, p = t.reshape(-1).astype(np.int64), p.reshape(-1).astype(np.int64)
    cells, nij = np.unique(t * len(b) + p, return_counts=True)
    return a.astype(np.int64), b.astype(np.int64), nij.astype(np.int64), cells // len(b), cells % len(b), int((uk < (1 << 31)).sum())


def distinct(sizes):
    s, m = np.unique(sizes, return_counts=True)
    return s.astype(np.int64), m.astype(np.int64)


def emi_terms(a, b, n):
    """how many terms expected_mutual_information's triple loop adds"""
    sa, ma = distinct(a)
    sb, mb = distinct(b)
    lo = np.maximum(1, sa[:, None] + sb[None, :] - n)
    hi = np.minimum(sa[:, None], sb[None, :])
    return int(((hi - lo + 1) * ma[:, None] * mb[None, :]).sum())


def emi_terms_grouped(a, b, n):
    """how many terms the evaluation per pair of DISTINCT sizes adds (the device's, and emi_grouped's)"""
    sa, sb = distinct(a)[0], distinct(b)[0]
    lo = np.maximum(1, sa[:, None] + sb[None, :] - n)
    hi = np.minimum(sa[:, None], sb[None, :])
    return int((hi - lo + 1).sum())


def emi_grouped(a, b, n):
    """scikit-learn's expected_mutual_information with the inner sum taken once per pair of DISTINCT sizes"""
    sa, ma = distinct(a)
    sb, mb = distinct(b)
    lf = gammaln(np.arange(n + 1, dtype=np.float64) + 1.0)
    total = 0.0
    for ai, wa in zip(sa.tolist(), ma.tolist()):
        for bj, wb in zip(sb.tolist(), mb.tolist()):
            k = np.arange(max(1, ai + bj - n), min(ai, bj) + 1)
            g = lf[ai] + lf[bj] + lf[n - ai] + lf[n - bj] - lf[n] - lf[k] - lf[ai - k] - lf[bj - k] - lf[n - ai - bj + k]
            total += wa * wb * float(np.sum(k / n * np.log(n * k / (float(ai) * bj)) * np.exp(g)))
    return total


def counts_of(a, b, nij, nonneg):
    return np.array([len(a), len(b), int((b >= 2).sum()), nonneg, len(nij), int((nij * nij).sum()), int((a * a).sum()),
                     int((b * b).sum())], dtype=np.int64)


def counts(y_true, labels):
    """One row of hsefr_partition_scores' counts int64 [8]"""
    a, b, nij, _, _, nonneg = table(y_true, labels)
    return counts_of(a, b, nij, nonneg)


def counts_stats(y_true, labels):
    """One row of hsefr_partition_scores: (counts int64 [8], stats float64 [6])"""
    a, b, nij, ci, cj, nonneg = table(y_true, labels)
    n = int(a.sum())
    counts = counts_of(a, b, nij, nonneg)
    fa, fb, fn = a.astype(np.float64), b.astype(np.float64), nij.astype(np.float64)
    stats = np.array([-np.sum(fa / n * (np.log(fa) - np.log(n))), -np.sum(fb / n * (np.log(fb) - np.log(n))),
                      np.sum(fn / n * np.log(n * fn / (fa[ci] * fb[cj]))), emi_grouped(a, b, n),
                      np.sum(fn * fn / fa[ci] / n), np.sum(fn * fn / fb[cj] / n)], dtype=np.float64)
    return counts, stats


def study_y_pred(labels):
    """The study's y_pred (facial_clustering_test.py:402-409) as far as scoring goes: every negative label a fresh label"""
    return np.unique(cluster_keys(labels), return_inverse=True)[1].reshape(-1)


def flat_cuts(order, gaps, thresholds):
    """hsefr_flat_cuts: labels[r][order[p]] = 1 + #{q < p : gaps[q] > thresholds[r]}"""
    order, gaps = np.asarray(order), np.asarray(gaps, dtype=np.float64)
    out = np.zeros((len(thresholds), len(order)), dtype=np.int32)
    for r, t in enumerate(thresholds):
        out[r, order] = 1 + np.concatenate([[0], np.cumsum(gaps > t)])
    return out


# ---- bounds ---------------------------------------------------------------------------------------------------------
def bound_sum(n):
    return (n + 8) * EPS * 2.0 * np.log(n)


def bound_emi(n, emi, terms):
    return 40.0 * EPS * n * np.log(n) * abs(emi) + (terms + 8) * EPS * 2.0 * np.log(n)


def bound_ratio(n, mi, h):
    """|MI / H| with both within bound_sum"""
    return bound_sum(n) * (1.0 + abs(mi / h)) / abs(h)


def bound_ami(n, ami, emi, terms, denominator):
    return ((bound_sum(n) + bound_emi(n, emi, terms)) * (1.0 + abs(ami)) + bound_sum(n)) / abs(denominator)


def assert_scores(name, y, row, exact, got, conditioned):
    """got = (ARI .. BCubed_FMeasure) of labelling ``row`` against scikit-learn and clustering.bcubed on the study's y_pred: ARI equal,
    the special cases equal, the others within the propagated bounds.  exact = the six sums the bounds and AMI's conditioning are
    computed from; conditioned = this case must have |mean(H) - EMI| >= 0.1.  AMI is compared through its quotient only with that
    denominator >= 0.1 -- and then identical partitions must also give 1 and all-singleton clusters 0 within the bound; with one class
    or one cluster it is scikit-learn's special value.  Returns ("quotient", denominator), ("special", None) or, for a smaller
    denominator, ("skipped", denominator): the callers count and report those."""
    from hse_facerec_tf_amd import clustering
    n = len(y)
    y_pred = study_y_pred(row)
    R, C = len(np.unique(y)), len(np.unique(y_pred))
    h_true, h_pred, mi, emi = exact[:4]
    ari, ami, hom, com, v, bp, br, bf = got
    assert ari == metrics.adjusted_rand_score(y, y_pred), name
    sk_hom, sk_com, sk_v = metrics.homogeneity_completeness_v_measure(y, y_pred)
    sk_ami = metrics.adjusted_mutual_info_score(y, y_pred, average_method="arithmetic")
    b_hom = bound_ratio(n, mi, h_true) if R > 1 else 0.0
    b_com = bound_ratio(n, mi, h_pred) if C > 1 else 0.0
    if R == 1 or C == 1:                       # scikit-learn's special cases: MI = 0, a zero entropy gives 1.0, AMI 1.0 or 0.0
        assert (hom, com, v, ami) == (sk_hom, sk_com, sk_v, sk_ami), name
        assert ami == (1.0 if R == C == 1 else 0.0) and hom == (1.0 if R == 1 else 0.0) and com == (1.0 if C == 1 else 0.0)
    else:
        assert abs(hom - sk_hom) <= b_hom and abs(com - sk_com) <= b_com, (name, hom - sk_hom, com - sk_com)
        assert abs(v - sk_v) <= 2 * (b_hom + b_com), (name, v - sk_v)
    want_p, want_r, want_f = clustering.bcubed(y, y_pred)
    b = bound_sum(n)
    assert abs(bp - want_p) <= b and abs(br - want_r) <= b and abs(bf - want_f) <= 4 * b, (name, bp - want_p, br - want_r, bf - want_f)
    if R > 1 and C > 1:
        denominator = 0.5 * (h_true + h_pred) - emi
        if conditioned:                        # a condition of the comparison, from the exact values
            assert abs(denominator) >= 0.1, (name, denominator)
        if abs(denominator) >= 0.1:
            a, bsz = table(y, row)[:2]
            bound = bound_ami(n, sk_ami, emi, emi_terms(a, bsz, n), denominator)
            assert abs(ami - sk_ami) <= bound, (name, ami - sk_ami, bound)
            if ari == 1.0:                     # the same partition under other names: numerator and denominator are one number
                assert abs(ami - 1.0) <= bound, (name, ami)
            if C == n:                         # all singletons: EMI = MI = H_true, the numerator is 0 (pushed to +-eps)
                assert abs(ami) <= bound + EPS / abs(denominator), (name, ami)
            return "quotient", denominator
        return "skipped", denominator
    return "special", None
