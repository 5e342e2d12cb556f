"""Records tests/golden/rank_order_reference.npz: the reference's rank-order clusters on seeded cases.  Development machine only.

    python tools/record_rank_order_golden.py /path/to/reference/age_gender_identity

The study's source (facial_clustering_test.py) is loaded from the reference tree given on the command line, use_clustering is switched
to the rank-order branch in memory, and the modules that branch never calls (cv2, facerec_test) are stubbed; networkx must be installed.
get_facial_clusters(D, (norm, rank)) then runs on every case and its cluster lists are stored exactly as returned.  The fixture holds
generator parameters, thresholds and results only -- no matrices and nothing of the reference's text: tests rebuild the cases from the
seeds with tests/rank_order_ref.py (integer features, so the distances are square roots of exact integers on every machine).
A case whose restatement margin |nd - norm_threshold| / norm_threshold is under 1e-9 is refused: the reference adds a cluster's
neighbour sums in Python set order, so a pair that close to the threshold is not decided by the rule."""
import os
import sys
import time
import types

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests"))
import rank_order_ref as ror  # noqa: E402

THRESHOLDS = ((0.9, 14), (1.06, 16), (1.1, 20))
MIN_MARGIN = 1e-9


def cases():
    """(kind, n, classes, seed, threshold pair)"""
    out = []
    for i, n in enumerate((1, 2, 12, 13, 19, 20, 21)):                        # the KN / NB edges
        for t in (i % 3, (i + 1) % 3):
            out.append(("integer", n, 2, 100 + n, THRESHOLDS[t]))
    for n, classes, seed in ((40, 5, 1), (60, 6, 2), (150, 12, 3), (200, 18, 4), (300, 25, 5), (500, 40, 6)):
        for thr in THRESHOLDS:
            out.append(("integer", n, classes, seed, thr))
    for thr in THRESHOLDS:
        out.append(("coincident", 80, 6, 7, thr))                             # the zero guard of the study's copy
    for thr in THRESHOLDS[:2]:
        out.append(("integer", 1000, 60, 8, thr))
    return out


def build(kind, n, classes, seed):
    if kind == "coincident":
        return ror.coincident_case(n, seed)[1]
    return ror.integer_case(n, classes, seed)[1]


def load_reference(ref_dir):
    for name in ("cv2",):
        sys.modules[name] = types.ModuleType(name)
    stub = types.ModuleType("facerec_test")
    stub.TensorFlowInference = object
    stub.is_image = lambda f: True
    sys.modules["facerec_test"] = stub
    src = open(os.path.join(ref_dir, "facial_clustering_test.py")).read()
    switched = src.replace("use_clustering=scipy_clustering", "use_clustering=rankorder_clustering", 1)
    if switched == src:
        raise SystemExit("the study's source does not select its clustering branch where expected")
    ns = {"__name__": "rank_order_reference"}
    exec(compile(switched, "rank_order_reference", "exec"), ns)
    return ns["get_facial_clusters"]


def main():
    if len(sys.argv) != 2:
        raise SystemExit(__doc__)
    get_facial_clusters = load_reference(sys.argv[1])
    rec = {k: [] for k in ("kind", "n", "classes", "seed", "norm", "rank", "clusters", "sizes", "members")}
    for kind, n, classes, seed, (norm, rank) in cases():
        D = build(kind, n, classes, seed)
        mine, iters, margin = ror.rank_order(D, norm, rank)
        if margin < MIN_MARGIN:
            raise SystemExit("case %r: restatement margin %.3g < %g -- pick another seed" % ((kind, n, classes, seed, norm, rank), margin,
                                                                                             MIN_MARGIN))
        t0 = time.time()
        got = get_facial_clusters(D.copy(), (norm, rank))
        got = [[int(i) for i in c] for c in got]
        same = [sorted(c) for c in got] == mine
        print("%-10s n=%4d classes=%2d seed=%3d thr=(%.2f, %2d): %3d clusters, %4d faces in them, restatement %s (%d iterations, margin "
              "%.2e), %.1f s" % (kind, n, classes, seed, norm, rank, len(got), sum(map(len, got)), "equal" if same else "DIFFERS", iters,
                                 margin, time.time() - t0), flush=True)
        for key, v in (("kind", kind), ("n", n), ("classes", classes), ("seed", seed), ("norm", norm), ("rank", rank),
                       ("clusters", len(got))):
            rec[key].append(v)
        rec["sizes"].extend(len(c) for c in got)
        rec["members"].extend(i for c in got for i in c)
    out = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests", "golden", "rank_order_reference.npz")
    np.savez_compressed(out, kind=np.array(rec["kind"]), n=np.array(rec["n"], np.int32), classes=np.array(rec["classes"], np.int32),
                        seed=np.array(rec["seed"], np.int32), norm=np.array(rec["norm"], np.float64),
                        rank=np.array(rec["rank"], np.float64), clusters=np.array(rec["clusters"], np.int32),
                        sizes=np.array(rec["sizes"], np.int32), members=np.array(rec["members"], np.int32))
    print("wrote %s: %d cases, %d bytes" % (os.path.normpath(out), len(rec["n"]), os.path.getsize(out)))


if __name__ == "__main__":
    main()
