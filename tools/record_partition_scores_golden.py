#!/usr/bin/env python3
"""Records tests/golden/partition_scores_exact.npz: the six sums of hsefr_partition_scores (H_true, H_pred, MI, EMI and the two
B-cubed sums) for every row of every case of tests/partition_cases.py, evaluated with mpmath at 60 digits and rounded once to
float64.  The EMI's inner sum depends only on the pair of sizes, so it is taken once per pair of distinct sizes and multiplied by the
multiplicities -- the same number as scikit-learn's triple sum, exactly.  CPU only; a few minutes."""
import os
import sys

import mpmath as mp
import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import partition_cases  # noqa: E402
import partition_scores_ref as ref  # noqa: E402

mp.mp.dps = 60


def exact_stats(y_true, labels, lf_cache={}):
    a, b, nij, ci, cj, _ = ref.table(y_true, labels)
    n = int(a.sum())
    N = mp.mpf(n)

    def lf(m):
        if m not in lf_cache:
            lf_cache[m] = mp.loggamma(m + 1)
        return lf_cache[m]

    def entropy(sizes):
        s, m = ref.distinct(sizes)
        return -mp.fsum(int(w) * (mp.mpf(int(v)) / N) * (mp.log(int(v)) - mp.log(N)) for v, w in zip(s, m))
    mi = mp.fsum((mp.mpf(int(v)) / N) * mp.log(N * int(v) / (mp.mpf(int(a[i])) * int(b[j]))) for v, i, j in zip(nij, ci, cj))
    sa, ma = ref.distinct(a)
    sb, mb = ref.distinct(b)
    emi = mp.mpf(0)
    for ai, wa in zip(sa.tolist(), ma.tolist()):
        for bj, wb in zip(sb.tolist(), mb.tolist()):
            fixed = lf(ai) + lf(bj) + lf(n - ai) + lf(n - bj) - lf(n)
            inner = mp.fsum((mp.mpf(k) / N) * mp.log(N * k / (mp.mpf(ai) * bj))
                            * mp.exp(fixed - lf(k) - lf(ai - k) - lf(bj - k) - lf(n - ai - bj + k))
                            for k in range(max(1, ai + bj - n), min(ai, bj) + 1))
            emi += wa * wb * inner
    s_a = mp.fsum(mp.mpf(int(v)) * int(v) / int(a[i]) / N for v, i in zip(nij, ci))
    s_b = mp.fsum(mp.mpf(int(v)) * int(v) / int(b[j]) / N for v, j in zip(nij, cj))
    return [float(v) for v in (entropy(a), entropy(b), mi, emi, s_a, s_b)]


def main():
    out = {}
    for name, (y, labels) in partition_cases.CASES.items():
        seen = {}
        rows = []
        for row in labels:
            key = row.tobytes()
            if key not in seen:
                seen[key] = exact_stats(y, row)
            rows.append(seen[key])
        out[name] = np.array(rows, dtype=np.float64)
        print(name, out[name].shape, flush=True)
    path = os.path.join(ROOT, "tests", "golden", "partition_scores_exact.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
