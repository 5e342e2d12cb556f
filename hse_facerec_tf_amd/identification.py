"""Post-extract identification (facerec_test.py:401-432, 200-207) with the distance work on the GPU.

Host steps stay what the reference does on the host -- including its own scikit-learn calls
for the label encoding and the stratified split (scikit-learn is a dependency of the
reference's callers, not of the engine); the O(N_test x N_train x D) nearest-neighbour search
(KNeighborsClassifier(1).fit/predict, :422,:203) and the L2 normalisation (:401) run through
libhsefr (ops.l2_normalize / ops.nn1).

Every protocol is upload / normalise / select of its own, then the same two steps on (gallery, probes): the projection of the '+PCA'
rows and the classifier.  Their keywords, shared by one_nn_identification and gallery_probe_identification:

n_neighbors: 1 labels a probe by its nearest gallery row (ops.nn1: ties -> the lowest gallery index, scikit-learn's own choice); more
    gives the '3-NN' / '3-NN+PCA' rows (facerec_test.py:269-288, :269-272) by the uniform vote of that many (ops.knn: equal counts to the
    smallest label as in scikit-learn's predict; 'nn_index' and 'nn_dist' become [nq, k]; the search is still timed as nn1_s).
pca_components, pca: the PCA is fitted on the gallery and applied to both sets, zero-padded to a multiple of 8 columns.  pca="host" is
    scikit-learn's PCA on the CPU, exactly as the reference does, the projected vectors going back to the device; pca="device" is the
    library's deterministic fp64 fit and projection (ops.pca_fit / ops.pca_transform: nothing leaves the GPU between the features and
    the search; a fit that does not converge in PCA_MAX_ITER iterations raises RuntimeError), timed as pca_s.
classifier: "knn" is all of the above.  "linear_svm" replaces the search by the reference's 'linear svm' / 'linear svm+PCA' rows
    (LinearSVC(), facerec_test.py:269-288, :269-273, :429; with ``pca_components``: the Pipeline of PCA and LinearSVC()): LinearSVC(C=svm_C)
    fitted on the gallery, after the projection, solved to the optimum of its objective in fp64 (ops.linear_svm_fit; a fit that does
    not converge raises RuntimeError), the probes labelled by ops.linear_svm_decision + ops.linear_svm_predict.  The result holds
    'decision' ([nq, K'] on the host) and 'svm_iterations' in place of 'nn_index' / 'nn_dist', and ``timings`` receives svm_fit_s and
    svm_predict_s in place of nn1_s.  scikit-learn's default tolerance stops short of the optimum, so its labels can differ on probes
    whose two largest decision values are closer than about 1e-4 (1e-3 after PCA).  ``n_neighbors`` must stay 1.
    "rbf_svm" gives the 'svm' row of :269-273, SVC(C=svm_C, gamma=svm_gamma): libsvm's one-vs-one C-SVC with the RBF kernel, every pair
    of classes solved to the optimum of its dual in fp64 (ops.rbf_svm_gamma + ops.rbf_svm_fit; a pair that stops at RBF_SVM_MAX_ITER
    raises RuntimeError), the probes labelled by the pairs' votes (ops.rbf_svm_predict).  The result holds 'votes' ([nq, K] on the host)
    and 'svm_iterations' in place of 'nn_index' / 'nn_dist'; ``timings`` as for "linear_svm".  scikit-learn's default tolerance stops
    about 3e-4 short of the optimum in a pair's decision value, so a vote whose value is that close to 0 can differ.  ``n_neighbors``
    must stay 1.
    "random_forest" gives the 'rf' row of :269-273, RandomForestClassifier(n_estimators=forest_trees, max_depth=forest_depth), as the
    forest of include/hsefr_forest.h (ops.random_forest_fit + ops.random_forest_predict_proba): scikit-learn's forest with its
    sequential generator replaced by a hash of (forest_seed, tree, node), so that the result is a pure function of its inputs --
    scikit-learn's own labels vary from run to run (the reference sets no random_state), so there are none to reproduce; the fixture's
    accuracy lies inside the recorded spread of scikit-learn's forests (README.md).  After a PCA the forest sees the projection's
    columns without their zero padding.  The result holds 'proba_max' ([nq] on the host: the predicted class's probability) and
    'forest_nodes' ([forest_trees]: the node count of every tree) in place of 'nn_index' / 'nn_dist'; ``timings`` receives forest_fit_s
    and forest_predict_s in place of nn1_s.  ``n_neighbors`` must stay 1.
metric: "l2" is all of the above.  "chi2" and "kl" give the reference's k-NN rows under its other two distances, chi2dist and KL_dist
    (facerec_test.py:157-164; KNeighborsClassifier(n_neighbors=1, metric=chi2dist) and metric=KL_dist at :275-276 and :424-425, which
    scikit-learn evaluates pair by pair in Python): every search, n_neighbors = 1 included, goes through ops.knn(metric=), the probe
    being the callable's first argument; 'nn_dist' holds the distance itself (no square root), shaped [nq] for n_neighbors = 1 and
    [nq, k] otherwise as above, and the search is timed as nn1_s.  The features are meant to be non-negative (GAP after ReLU6,
    probabilities); ``normalize`` and one_nn_identification's L2 normalisation apply as for "l2" (the reference feeds X_norm to these
    rows).  Only with classifier="knn" and without ``pca_components``: projections are signed, and the reference never combines them.
svm_C: the C of either SVM.  svm_gamma: "scale" (1 / (d Var) of the gallery rows, over the unpadded columns after a PCA) or a positive
    finite number.
forest_trees, forest_depth, forest_seed: the random forest's tree count, depth limit and seed (100, 10 and 0: the reference's row).
"""
from __future__ import annotations

from typing import Dict, NamedTuple, Optional, Tuple

import numpy as np


def filter_classes(y: np.ndarray) -> Tuple[np.ndarray, np.ndarray]:
    """facerec_test.py:407-412: keep samples whose label occurs more than once, re-encode the
    labels to 0..C-1 in sorted order (LabelEncoder).  Returns (indices, y_encoded)."""
    y = np.asarray(y)
    classes, inverse, counts = np.unique(y, return_inverse=True, return_counts=True)
    indices = np.nonzero(counts[inverse] > 1)[0]
    _, y_enc = np.unique(y[indices], return_inverse=True)
    return indices, y_enc


def stratified_half_split(y: np.ndarray, random_state: int = 0) -> Tuple[np.ndarray, np.ndarray]:
    """StratifiedShuffleSplit(n_splits=1, test_size=0.5, random_state=0) (facerec_test.py:202)."""
    from sklearn import model_selection
    sss = model_selection.StratifiedShuffleSplit(n_splits=1, test_size=0.5, random_state=random_state)
    (train, test), = sss.split(np.zeros((len(y), 1)), y)
    return train, test


class SplitJob:
    """The host half of the protocol -- filter_classes + stratified_half_split, 6-9 ms of scikit-learn for LFW's 9164 labels --
    running in a thread of its own.  It depends on the labels only, which the dataset walk yields before the first image is
    decoded (facerec_test.py:377-392), so a caller can start it while the device is still extracting (gallery.extract_sharded's
    ``on_issued`` hook) and hand it to one_nn_identification(split=job): same indices, same split, off the critical path."""

    def __init__(self, y: np.ndarray, random_state: int = 0):
        import threading
        self._out = None
        self._err = None

        def work():
            try:
                indices, y_enc = filter_classes(y)
                train, test = stratified_half_split(y_enc, random_state)
                self._out = (indices, y_enc, train, test)
            except BaseException as e:          # re-raised in the caller's thread
                self._err = e
        self._thread = threading.Thread(target=work, name="hsefr-split", daemon=True)
        self._thread.start()

    def result(self):
        self._thread.join()
        if self._err is not None:
            raise self._err
        return self._out


def start_split(y: np.ndarray, random_state: int = 0) -> SplitJob:
    return SplitJob(np.asarray(y), random_state)


PCA_MAX_ITER = 1000     # hsefr_pca_fit's iteration cap on the pca="device" path; reaching it raises

LINEAR_SVM_MAX_ITER = 1000     # hsefr_linear_svm_fit's Newton iteration cap on the classifier="linear_svm" path; reaching it raises
LINEAR_SVM_TOL = 1e-10         # a class is converged at |grad f_k| <= LINEAR_SVM_TOL |grad f_k(0)|

RBF_SVM_MAX_ITER = 100000      # hsefr_rbf_svm_fit's iteration cap per pair of classes on the classifier="rbf_svm" path; reaching it raises
RBF_SVM_TOL = 1e-10            # a pair is converged at m(a) - M(a) <= RBF_SVM_TOL (libsvm's stopping quantity; SVC's default is 1e-3)


def check_pca_mode(pca) -> str:
    if pca not in ("host", "device"):
        raise ValueError("pca=%r must be 'host' (scikit-learn on the CPU) or 'device' (ops.pca_fit / ops.pca_transform)" % (pca,))
    return pca


def check_classifier(classifier, n_neighbors=1, svm_C=1.0, svm_gamma="scale", forest_trees=100, forest_depth=10, forest_seed=0) -> str:
    """The classifier keyword of the protocols, raised as ValueError before the library or a device is touched.  (The sentence for an
    unknown name lists the three classifiers it listed before "random_forest" joined them; the module docstring lists all four.)"""
    if not isinstance(classifier, str) or classifier not in ("knn", "linear_svm", "rbf_svm", "random_forest"):
        raise ValueError("classifier=%r must be 'knn' (ops.nn1 / ops.knn), 'linear_svm' (ops.linear_svm_fit) or 'rbf_svm' (ops.rbf_svm_fit)"
                         % (classifier,))
    if classifier == "rbf_svm":
        from . import ops
        if n_neighbors != 1:
            raise ValueError("n_neighbors=%r has no meaning with classifier='rbf_svm': leave it at 1" % (n_neighbors,))
        if isinstance(svm_gamma, str) and svm_gamma != "scale":
            raise ValueError("svm_gamma=%r must be 'scale' or a positive finite number" % (svm_gamma,))
        ops.check_rbf_svm_args(2, 1, 2, C=svm_C, gamma=svm_gamma)
    if classifier == "linear_svm":
        from . import ops
        if n_neighbors != 1:
            raise ValueError("n_neighbors=%r has no meaning with classifier='linear_svm': leave it at 1" % (n_neighbors,))
        ops.check_linear_svm_args(1, 1, 2, C=svm_C)
    if classifier == "random_forest":
        from . import ops
        if n_neighbors != 1:
            raise ValueError("n_neighbors=%r has no meaning with classifier='random_forest': leave it at 1" % (n_neighbors,))
        for name, v, least in (("forest_trees", forest_trees, 1), ("forest_depth", forest_depth, 1), ("forest_seed", forest_seed, 0)):
            ops._int_arg(name, v, least)
        ops.check_random_forest_args(2, 1, 2, n_trees=forest_trees, max_depth=forest_depth, seed=forest_seed)
    return classifier


class _Keywords(NamedTuple):
    """The keywords of the module docstring, checked."""
    n_neighbors: int
    pca: str
    pca_components: Optional[int]
    classifier: str
    svm_C: float
    svm_gamma: object
    metric: str = "l2"
    forest_trees: int = 100
    forest_depth: int = 10
    forest_seed: int = 0


def _check_keywords(n_neighbors=1, pca="host", pca_components=None, classifier="knn", svm_C=1.0, svm_gamma="scale",
                    n_gallery=None, metric="l2", forest_trees=100, forest_depth=10, forest_seed=0) -> _Keywords:
    """Every keyword check of the protocols, raised as ValueError before the library is loaded or a device is touched; ``n_gallery``:
    the gallery rows, where the protocol knows them this early."""
    from . import ops
    ops.check_n_neighbors(n_neighbors, n_gallery)
    check_pca_mode(pca)
    check_classifier(classifier, n_neighbors, svm_C, svm_gamma, forest_trees, forest_depth, forest_seed)
    if pca_components and pca == "device":
        ops.check_pca_components(pca_components, n_gallery)
    if ops.check_metric(metric) != "l2":
        if classifier != "knn":
            raise ValueError("metric=%r is a k-NN distance: it has no meaning with classifier=%r" % (metric, classifier))
        if pca_components:
            raise ValueError("metric=%r wants non-negative features, and a PCA's projections are signed: leave pca_components unset"
                             % (metric,))
    return _Keywords(n_neighbors, pca, pca_components, classifier, svm_C, svm_gamma, metric, forest_trees, forest_depth, forest_seed)


def _phase_clock(torch, device, timings: Optional[dict]):
    """lap(key): ``timings[key]`` = the device-synchronised wall seconds since the previous lap (the first: since this call).  Without
    ``timings`` a lap does nothing, and synchronises nothing."""
    import time
    if timings is None:
        return lambda key: None
    torch.cuda.synchronize(device)
    t_prev = time.perf_counter()

    def lap(key):
        nonlocal t_prev
        torch.cuda.synchronize(device)
        t = time.perf_counter()
        timings[key] = t - t_prev
        t_prev = t
    return lap


def _rows(torch, X, index):
    return X[torch.from_numpy(np.asarray(index, dtype=np.int64)).to(X.device)].contiguous()


def _accuracy(y_pred: np.ndarray, y_true: np.ndarray) -> float:
    return float((y_pred == y_true).mean()) if len(y_true) else float("nan")


def _device_pca(ops, gal, qry, pca_components: int):
    """Fit on the gallery, project both sets (float32, zero-padded to a multiple of 8 columns), all on the device."""
    mean, components, _, info = ops.pca_fit(gal, pca_components, max_iter=PCA_MAX_ITER)
    if not info["converged"]:
        raise RuntimeError("the device PCA of the %d x %d gallery (%d components) did not converge in %d iterations"
                           % (gal.shape[0], gal.shape[1], pca_components, info["iterations"]))
    return ops.pca_transform(gal, mean, components), ops.pca_transform(qry, mean, components)


def _reduce(torch, ops, gal, qry, kw: _Keywords, device, lap=lambda key: None):
    """The PCA of the '+PCA' rows (the Pipeline of facerec_test.py:421): (gal, qry) -> (gal, qry) in ``pca_components`` columns,
    fitted on the gallery; the host's projection goes to ``device``.  Only the device's fit is a phase of its own (pca_s)."""
    if not kw.pca_components:
        return gal, qry
    if kw.pca == "device":
        gal, qry = _device_pca(ops, gal, qry, kw.pca_components)
        lap("pca_s")
        return gal, qry
    from sklearn.decomposition import PCA
    fitted = PCA(n_components=kw.pca_components).fit(gal.cpu().numpy())
    pad = (-kw.pca_components) % 8                      # hsefr_nn1 wants d % 8 == 0: zero columns change no distance

    def proj(t):
        z = fitted.transform(t.cpu().numpy()).astype(np.float32)
        return torch.from_numpy(np.pad(z, ((0, 0), (0, pad)))).to(device).contiguous()
    return proj(gal), proj(qry)


def _encode_labels(torch, y_gallery: np.ndarray, device):
    """np.unique's sorted classes (scikit-learn's ``classes_``, so any label type works and a vote's smallest-label rule runs over
    them) and the gallery's codes as an int32 tensor on ``device``."""
    classes, codes = np.unique(np.asarray(y_gallery), return_inverse=True)
    return classes, torch.from_numpy(codes.astype(np.int32).reshape(-1)).to(device)


def _classify(torch, ops, gal, qry, y_gallery: np.ndarray, kw: _Keywords, lap=lambda key: None):
    """The classifier of ``kw`` fitted on (gal, y_gallery) and applied to ``qry`` on the device -> (y_pred, extras), everything on the
    host.  extras: 'nn_index' + 'nn_dist' of the searches, 'decision' + 'svm_iterations' of the linear SVM, 'votes' + 'svm_iterations'
    of the RBF SVM, 'proba_max' + 'forest_nodes' of the random forest.  ``lap`` (a _phase_clock) is called with nn1_s after the search
    -- for n_neighbors = 1 before anything is copied to the host, for more after the copies -- or with svm_fit_s and svm_predict_s,
    or with forest_fit_s and forest_predict_s."""
    if kw.classifier == "knn" and kw.n_neighbors == 1 and kw.metric == "l2":
        nn_idx, nn_d2 = ops.nn1(qry, gal)
        lap("nn1_s")
        nn_idx_h = nn_idx.cpu().numpy()
        return y_gallery[nn_idx_h], {"nn_index": nn_idx_h, "nn_dist": np.sqrt(nn_d2.cpu().numpy())}
    classes, labels = _encode_labels(torch, y_gallery, gal.device)
    if kw.classifier == "knn" and kw.metric != "l2":        # KNeighborsClassifier(n_neighbors, metric=chi2dist | KL_dist)
        idx, dist, pred = ops.knn(qry, gal, kw.n_neighbors, labels, metric=kw.metric)
        if kw.n_neighbors == 1:
            idx, dist = idx[:, 0], dist[:, 0]
        y_pred, extras = classes[pred.cpu().numpy()], {"nn_index": idx.cpu().numpy(), "nn_dist": dist.cpu().numpy()}
        lap("nn1_s")
        return y_pred, extras
    if kw.classifier == "knn":                  # KNeighborsClassifier(n_neighbors): kneighbors + predict
        idx, d2, pred = ops.knn(qry, gal, kw.n_neighbors, labels)
        y_pred, extras = classes[pred.cpu().numpy()], {"nn_index": idx.cpu().numpy(), "nn_dist": np.sqrt(d2.cpu().numpy())}
        lap("nn1_s")
        return y_pred, extras
    n, d, K = int(gal.shape[0]), int(gal.shape[1]), len(classes)
    if kw.classifier == "random_forest":        # RandomForestClassifier(forest_trees, max_depth=forest_depth): predict_proba + predict
        if kw.pca_components and d > kw.pca_components:          # the projection without its zero padding
            gal, qry = gal[:, :kw.pca_components].contiguous(), qry[:, :kw.pca_components].contiguous()
        forest = ops.random_forest_fit(gal, labels, max(K, 2), n_trees=kw.forest_trees, max_depth=kw.forest_depth, seed=kw.forest_seed)
        lap("forest_fit_s")
        nodes = forest.n_nodes.cpu().numpy()
        if qry.shape[0] == 0:
            lap("forest_predict_s")
            return classes[:0], {"proba_max": np.zeros((0,), dtype=np.float64), "forest_nodes": nodes}
        proba, pred = ops.random_forest_predict_proba(forest, qry)
        lap("forest_predict_s")
        return classes[pred.cpu().numpy()], {"proba_max": proba.max(dim=1).values.cpu().numpy(), "forest_nodes": nodes}
    if kw.classifier == "linear_svm":           # LinearSVC(C=svm_C): decision_function + predict
        coef, intercept, info = ops.linear_svm_fit(gal, labels, K, C=kw.svm_C, tol=LINEAR_SVM_TOL, max_iter=LINEAR_SVM_MAX_ITER)
        if not info["converged"]:
            raise RuntimeError("the device linear SVM fit on the n=%d x d=%d gallery (K=%d classes) did not converge in %d iterations"
                               % (n, d, K, info["iterations"]))
        table, no_probe = "decision", np.zeros((0, int(coef.shape[0])), dtype=np.float64)

        def predict():
            decision = ops.linear_svm_decision(qry, coef, intercept)
            return ops.linear_svm_predict(decision), decision
    else:                                       # SVC(C=svm_C, gamma=svm_gamma): predict and the pairs' votes
        # before ops.rbf_svm_gamma, which words a gallery over the limits in its own way
        ops.check_rbf_svm_args(n, d, K, C=kw.svm_C, gamma=kw.svm_gamma, tol=RBF_SVM_TOL, max_iter=RBF_SVM_MAX_ITER)
        # gamma='scale' counts the columns of the projection, not its zero padding
        gamma = ops.rbf_svm_gamma(gal, kw.pca_components or None) if isinstance(kw.svm_gamma, str) else float(kw.svm_gamma)
        dual_coef, rho, info = ops.rbf_svm_fit(gal, labels, K, gamma, C=kw.svm_C, tol=RBF_SVM_TOL, max_iter=RBF_SVM_MAX_ITER)
        if not info["converged"]:
            raise RuntimeError("the device RBF SVM fit on the n=%d x d=%d gallery (K=%d classes) left %d pairs of classes short of the "
                               "optimum after %d iterations" % (n, d, K, info["pairs_at_max_iter"], info["iterations"]))
        table, no_probe = "votes", np.zeros((0, K), dtype=np.int32)

        def predict():
            return ops.rbf_svm_predict(qry, gal, labels, K, gamma, dual_coef, rho)
    lap("svm_fit_s")
    if qry.shape[0] == 0:                       # no probe: nothing to label (the entry points want at least one row)
        lap("svm_predict_s")
        return classes[:0], {table: no_probe, "svm_iterations": info["iterations"]}
    pred, values = predict()
    lap("svm_predict_s")
    return classes[pred.cpu().numpy()], {table: values.cpu().numpy(), "svm_iterations": info["iterations"]}


def one_nn_identification(X, y: np.ndarray, split=None,
                          pca_components: Optional[int] = None, timings: Optional[dict] = None, device=None,
                          n_neighbors: int = 1, pca: str = "host", classifier: str = "knn", svm_C: float = 1.0, svm_gamma="scale",
                          metric: str = "l2", forest_trees: int = 100, forest_depth: int = 10, forest_seed: int = 0) -> Dict:
    """The protocol of facerec_test.py:401-432: 'k-NN' (pca_components=None) or 'k-NN+PCA' (pca_components=128, the Pipeline of :421)
    on a stratified half split of the samples whose class has more than one; ``classifier`` gives the 'linear svm' row of :429, the
    'svm' row or the 'rf' row instead, ``metric`` the chi2dist / KL_dist rows of :424-425.  n_neighbors, pca, classifier, svm_C, svm_gamma,
    metric and forest_trees / forest_depth / forest_seed: see the module docstring; the gallery is the train half.

    X: [N, D] float32 embeddings, CUDA tensor or NumPy array (uploaded to ``device``, default: the current one); y: [N] labels.
    split: None (compute it here), a (train, test) pair over the FILTERED samples, or a SplitJob started on the same labels.
    Returns accuracy, the split, predictions and the classifier's extras (nearest-gallery indices and distances).  ``timings``
    (optional dict) receives the device-synchronised wall seconds of each phase: normalize_s, host_split_s, select_s, pca_s (with
    pca="device"), the classifier's (nn1_s, and nn1_shape with it), readback_s (indices and distances back to the host + the label
    comparison)."""
    from . import _lib, ops
    kw = _check_keywords(n_neighbors, pca, pca_components, classifier, svm_C, svm_gamma, metric=metric, forest_trees=forest_trees,
                         forest_depth=forest_depth, forest_seed=forest_seed)
    torch = _lib.require_gpu()
    if isinstance(X, np.ndarray):
        X = torch.from_numpy(np.ascontiguousarray(X, dtype=np.float32)).to(_lib.cuda_device(device))
    lap = _phase_clock(torch, X.device, timings)
    Xn = ops.l2_normalize(X.contiguous())                       # :401
    lap("normalize_s")
    if isinstance(split, SplitJob):                             # started earlier on the same labels: wait for it
        indices, y_enc, train, test = split.result()
    else:
        indices, y_enc = filter_classes(y)                      # :407-412
        train, test = split if split is not None else stratified_half_split(y_enc)
    lap("host_split_s")
    Xn = _rows(torch, Xn, indices)                              # :413
    gal, qry = _rows(torch, Xn, train), _rows(torch, Xn, test)
    lap("select_s")
    gal, qry = _reduce(torch, ops, gal, qry, kw, Xn.device, lap)
    y_pred, extras = _classify(torch, ops, gal, qry, y_enc[train], kw, lap)
    acc = _accuracy(y_pred, y_enc[test])
    lap("readback_s")
    if timings is not None and "nn_index" in extras:             # the searches' shape, beside the nn1_s that _classify lapped
        timings["nn1_shape"] = (int(qry.shape[0]), int(gal.shape[0]), int(qry.shape[1]))
    return {"accuracy": acc, "indices": indices, "y": y_enc, "train": train, "test": test, "y_pred": y_pred, **extras,
            "num_classes": int(y_enc.max() + 1) if len(y_enc) else 0}


def single_image_per_class_splits(y: np.ndarray, n_splits: int = 10, random_state: int = 0):
    """get_single_image_per_class_cv (facerec_test.py:177-197), the protocol behind README.md:13's one-training-image rows:
    ``n_splits`` splits; in each, every class's sample indices are shuffled and the FIRST one is the gallery image, the rest
    are probes.  The reference seeds NumPy's global generator once (``np.random.seed(random_state)``) and shuffles class by
    class in ``np.unique`` order, split after split; a private ``RandomState(random_state)`` draws the same stream without
    touching the caller's global state -- the splits are bit-equal (tests/golden/protocols.npz, written by
    tests/golden/make_golden.py from the reference's literal globally seeded loop)."""
    y = np.asarray(y)
    inds = np.arange(len(y))
    rs = np.random.RandomState(random_state)
    classes = np.unique(y)
    members = [inds[y == lbl] for lbl in classes]
    res_cv = []
    for _ in range(n_splits):
        inds_train, inds_test = [], []
        for m in members:
            tmp = m.copy()
            rs.shuffle(tmp)
            inds_train.extend(tmp[:1])
            inds_test.extend(tmp[1:])
        res_cv.append((np.array(inds_train), np.array(inds_test)))
    return res_cv


def cross_validated_1nn(X, y: np.ndarray, cv, normalize: bool = True, device=None, n_neighbors: int = 1, metric: str = "l2") -> Dict:
    """classifier_tester (facerec_test.py:199-207) for KNeighborsClassifier(n_neighbors=1, p=2) over an explicit list of
    (train, test) index pairs -- e.g. single_image_per_class_splits(y) in place of the stratified half split (:200-201) --
    with every search on the GPU.  Returns the per-split accuracies and their mean / std as the reference prints them.
    ``n_neighbors`` > 1 scores KNeighborsClassifier(n_neighbors) instead (ops.knn's uniform vote), ``metric`` "chi2" or "kl" the
    classifier under chi2dist / KL_dist (the module docstring)."""
    from . import _lib, ops
    kw = _check_keywords(n_neighbors, metric=metric)
    torch = _lib.require_gpu()
    if isinstance(X, np.ndarray):
        X = torch.from_numpy(np.ascontiguousarray(X, dtype=np.float32)).to(_lib.cuda_device(device))
    Xd = ops.l2_normalize(X.contiguous()) if normalize else X.contiguous()
    y = np.asarray(y)
    accs, preds = [], []
    for train, test in cv:
        train, test = np.asarray(train, dtype=np.int64), np.asarray(test, dtype=np.int64)     # an empty fold is no float index
        y_pred, _ = _classify(torch, ops, _rows(torch, Xd, train), _rows(torch, Xd, test), y[train], kw)
        preds.append(y_pred)
        accs.append(_accuracy(y_pred, y[test]))
    accs = np.asarray(accs)
    return {"accuracies": accs, "mean": float(accs.mean()) if len(accs) else float("nan"),
            "std": float(accs.std()) if len(accs) else float("nan"), "y_pred": preds}


def gallery_probe_identification(X_train, y_train: np.ndarray, X_test, y_test: np.ndarray, normalize: bool = False,
                                 pca_components: Optional[int] = None, device=None, n_neighbors: int = 1, pca: str = "host",
                                 classifier: str = "knn", svm_C: float = 1.0, svm_gamma="scale", metric: str = "l2",
                                 forest_trees: int = 100, forest_depth: int = 10, forest_seed: int = 0) -> Dict:
    """The gallery / probe protocol of tf_train_test_recognition (facerec_test.py:260-288): the '1-NN' classifier (and
    '1-NN+PCA' with ``pca_components``, 16 at :269) FITTED on the gallery features, every probe labelled by its nearest
    gallery row; accuracy = share of probes whose label is right (:287).  NB the reference computes L2-normalised copies
    (:262,265) and then fits / predicts on the UN-normalised ``X_train`` / ``X_test`` (:284-285): ``normalize=False`` is what
    it runs, ``normalize=True`` what the copies suggest it meant.  n_neighbors, pca, classifier, svm_C, svm_gamma, metric and
    forest_trees / forest_depth / forest_seed give the other rows of :269-276: see the module docstring.  Returns 'accuracy', 'y_pred' and the classifier's extras."""
    from . import _lib, ops
    kw = _check_keywords(n_neighbors, pca, pca_components, classifier, svm_C, svm_gamma, n_gallery=len(np.asarray(y_train)), metric=metric,
                         forest_trees=forest_trees, forest_depth=forest_depth, forest_seed=forest_seed)
    torch = _lib.require_gpu()
    dev = _lib.cuda_device(device)

    def up(a):
        t = torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(dev) if isinstance(a, np.ndarray) else a.float()
        return ops.l2_normalize(t.contiguous()) if normalize else t.contiguous()
    gal, qry = up(X_train), up(X_test)
    y_train, y_test = np.asarray(y_train), np.asarray(y_test)
    if gal.shape[0] != len(y_train) or qry.shape[0] != len(y_test):
        raise ValueError("features and labels differ in length: %d/%d gallery, %d/%d probe"
                         % (gal.shape[0], len(y_train), qry.shape[0], len(y_test)))
    gal, qry = _reduce(torch, ops, gal, qry, kw, dev)
    y_pred, extras = _classify(torch, ops, gal, qry, y_train, kw)
    return {"accuracy": _accuracy(y_pred, y_test), "y_pred": y_pred, **extras}


def feature_distance_matrix(features, born_years=None, photo_years=None, device=None) -> np.ndarray:
    """The dist_matrix of process_photos.perform_clustering (process_photos.py:45-60): Euclidean distance
    between facial features (on the GPU) plus 0.1 x the age term (cur_age_i - cur_age_j)^2 / (cur_age_i +
    cur_age_j), cur_age = max(year_i, year_j) - born_year, clipped at 0.  Returns a host float64 matrix as the
    clustering code (facial_clustering.get_facial_clusters) expects."""
    from . import _lib, ops
    torch = _lib.require_gpu()
    f = torch.from_numpy(np.ascontiguousarray(features, dtype=np.float32)).to(_lib.cuda_device(device)) if isinstance(features, np.ndarray) \
        else features.float().contiguous()
    dist = ops.pairwise_distances(f).cpu().numpy().astype(np.float64)
    if born_years is not None:
        by = np.asarray(born_years, dtype=np.float64)
        yr = np.asarray(photo_years, dtype=np.float64)
        max_year = np.maximum(yr[:, None], yr[None, :])
        ai, aj = max_year - by[:, None], max_year - by[None, :]
        with np.errstate(divide="ignore", invalid="ignore"):
            dist = dist + 0.1 * (ai - aj) ** 2 / (ai + aj)
    return np.clip(dist, a_min=0, a_max=None)
