"""Records tests/golden/album_reference.npz: the reference's Dempster-Shafer gender fusion on seeded inputs.  Development machine only.

    python tools/record_album_golden.py /path/to/reference/age_gender_identity

The four functions of the fusion (calculate_proximity, compute_b, final_decision, dempster_shafer_gender) are taken from
process_photos.py of the reference tree given on the command line -- their definitions alone, by name, because the module itself imports
cv2 and matplotlib -- and run on every case: lists of 1 to 50 male probabilities in (0, 1), and lists whose values all lie near 0.614,
where a single face's two beliefs cross.  The fixture holds the inputs, the two summed log beliefs and the decisions: data only, nothing
of the reference's text."""
import ast
import os
import sys

import numpy as np

NAMES = ("calculate_proximity", "compute_b", "final_decision", "dempster_shafer_gender")
CROSSING = 0.614          # a face with this male probability is as close to one decision template as to the other


def load_reference(ref_dir):
    path = os.path.join(ref_dir, "process_photos.py")
    tree = ast.parse(open(path).read(), path)
    defs = [node for node in tree.body if isinstance(node, ast.FunctionDef) and node.name in NAMES]
    if sorted(d.name for d in defs) != sorted(NAMES):
        raise SystemExit("%s does not define %s" % (path, ", ".join(NAMES)))
    ns = {"np": np, "LA": np.linalg}
    exec(compile(ast.Module(body=defs, type_ignores=[]), path, "exec"), ns)
    return ns


def cases():
    """Lists of male probabilities, each value a [1] array as the net returns them."""
    rng = np.random.RandomState(20240)
    out = []
    for n in list(range(1, 51)) + [1, 2, 3, 5, 8, 13, 21, 34] * 4:
        out.append(rng.uniform(1e-3, 1 - 1e-3, n))
    for k in range(60):                                                       # near the crossing: the decision hangs on the last digits
        n = 1 + k % 12
        out.append(CROSSING + rng.uniform(-1, 1, n) * 10.0 ** -(1 + k % 5))
    for p in (0.5, 0.6, CROSSING, 0.7, 0.999, 0.001):
        out.append(np.array([p]))
        out.append(np.full(7, p))
    return [np.float32(c).astype(np.float64) for c in out]                    # the net's outputs are float32


def main():
    if len(sys.argv) != 2:
        raise SystemExit(__doc__)
    ref = load_reference(sys.argv[1])
    probs, lengths, beliefs, decisions = [], [], [], []
    for c in cases():
        male_probs = [np.array([p]) for p in c]
        per_face = []
        for mp in male_probs:                                                  # dempster_shafer_gender's loop, to keep the sums it compares
            prox = ref["calculate_proximity"]([[0.875, 0.125], [0.353, 0.647]], [[mp[0], 1 - mp[0]]], 2)
            per_face.append(ref["compute_b"](prox, 2))
        log_m = np.sum(per_face, axis=0)
        d = int(ref["dempster_shafer_gender"](male_probs))
        assert d == int(ref["final_decision"](per_face))
        probs.extend(c)
        lengths.append(len(c))
        beliefs.append(log_m)
        decisions.append(d)
    out = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests", "golden", "album_reference.npz")
    np.savez_compressed(out, probs=np.array(probs, np.float64), lengths=np.array(lengths, np.int32),
                        beliefs=np.array(beliefs, np.float64).reshape(-1, 2), decisions=np.array(decisions, np.int32))
    print("wrote %s: %d cases (%d male, %d female), %d bytes" % (os.path.normpath(out), len(lengths), decisions.count(0), decisions.count(1),
                                                                 os.path.getsize(out)))


if __name__ == "__main__":
    main()
