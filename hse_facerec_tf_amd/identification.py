"""Post-extract identification (facerec_test.py:401-432, 200-207) with the distance work on the GPU.

Host steps stay what the reference does on the host -- including its own scikit-learn calls
for the label encoding and the stratified split (scikit-learn is a dependency of the
reference's callers, not of the engine); the O(N_test x N_train x D) nearest-neighbour search
(KNeighborsClassifier(1).fit/predict, :422,:203) and the L2 normalisation (:401) run through
libhsefr (ops.l2_normalize / ops.nn1; ops.knn for the reference's '3-NN' rows, facerec_test.py:269-288).  The PCA of the '+PCA' rows
is scikit-learn's on the host by default (``pca="host"``) or the library's deterministic fp64 fit and projection on the device
(``pca="device"``: ops.pca_fit / ops.pca_transform, nothing leaves the GPU between the features and the search).
``classifier="linear_svm"`` replaces the search by the reference's 'linear svm' / 'linear svm+PCA' rows (LinearSVC(), facerec_test.py:269-288,
:429): ops.linear_svm_fit on the gallery, solved to the optimum of LinearSVC's objective in fp64, ops.linear_svm_decision and
ops.linear_svm_predict on the probes.  ``classifier="rbf_svm"`` gives the 'svm' row (SVC(): libsvm's one-vs-one C-SVC with the RBF kernel):
ops.rbf_svm_gamma + ops.rbf_svm_fit on the gallery, every pair's dual solved to its optimum in fp64, ops.rbf_svm_predict on the probes.
"""
from __future__ import annotations

from typing import Dict, Optional, Tuple

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


def check_pca_mode(pca) -> str:
    if pca not in ("host", "device"):
        raise ValueError("pca=%r must be 'host' (scikit-learn on the CPU) or 'device' (ops.pca_fit / ops.pca_transform)" % (pca,))
    return pca


def _device_pca(ops, gal, qry, pca_components: int):
    """Fit on the gallery, project both sets (float32, zero-padded to a multiple of 8 columns), all on the device."""
    mean, components, _, info = ops.pca_fit(gal, pca_components, max_iter=PCA_MAX_ITER)
    if not info["converged"]:
        raise RuntimeError("the device PCA of the %d x %d gallery (%d components) did not converge in %d iterations"
                           % (gal.shape[0], gal.shape[1], pca_components, info["iterations"]))
    return ops.pca_transform(gal, mean, components), ops.pca_transform(qry, mean, components)


LINEAR_SVM_MAX_ITER = 1000     # hsefr_linear_svm_fit's Newton iteration cap on the classifier="linear_svm" path; reaching it raises
LINEAR_SVM_TOL = 1e-10         # a class is converged at |grad f_k| <= LINEAR_SVM_TOL |grad f_k(0)|


RBF_SVM_MAX_ITER = 100000      # hsefr_rbf_svm_fit's iteration cap per pair of classes on the classifier="rbf_svm" path; reaching it raises
RBF_SVM_TOL = 1e-10            # a pair is converged at m(a) - M(a) <= RBF_SVM_TOL (libsvm's stopping quantity; SVC's default is 1e-3)


def check_classifier(classifier, n_neighbors=1, svm_C=1.0, svm_gamma="scale") -> str:
    """The classifier keyword of the protocols, raised as ValueError before the library or a device is touched."""
    if not isinstance(classifier, str) or classifier not in ("knn", "linear_svm", "rbf_svm"):
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
    return classifier


def _linear_svm_predict(ops, qry, gal, y_gallery: np.ndarray, svm_C: float, lap=None):
    """LinearSVC(C=svm_C).fit(gal, y_gallery) at the objective's optimum -> decision_function + predict of ``qry`` on the device.  The
    labels are encoded with np.unique (scikit-learn's ``classes_``), so any label type works.  Returns (y_pred, decision [nq,K'] on the
    host, Newton iterations)."""
    from . import _lib
    torch = _lib.require_gpu()
    classes, codes = np.unique(np.asarray(y_gallery), return_inverse=True)
    n, d = int(gal.shape[0]), int(gal.shape[1])
    ops.check_linear_svm_args(n, d, len(classes), C=svm_C, tol=LINEAR_SVM_TOL, max_iter=LINEAR_SVM_MAX_ITER)
    labels = torch.from_numpy(codes.astype(np.int32).reshape(-1)).to(gal.device)
    coef, intercept, info = ops.linear_svm_fit(gal, labels, len(classes), C=svm_C, tol=LINEAR_SVM_TOL, max_iter=LINEAR_SVM_MAX_ITER)
    if not info["converged"]:
        raise RuntimeError("the device linear SVM fit on the n=%d x d=%d gallery (K=%d classes) did not converge in %d iterations"
                           % (n, d, len(classes), info["iterations"]))
    if lap is not None:
        lap("svm_fit_s")
    if qry.shape[0] == 0:                                       # no probe: nothing to label (the entry points want at least one row)
        if lap is not None:
            lap("svm_predict_s")
        return classes[:0], np.zeros((0, int(coef.shape[0])), dtype=np.float64), info["iterations"]
    decision = ops.linear_svm_decision(qry, coef, intercept)
    pred = ops.linear_svm_predict(decision)
    if lap is not None:
        lap("svm_predict_s")
    return classes[pred.cpu().numpy()], decision.cpu().numpy(), info["iterations"]


def _rbf_svm_predict(ops, qry, gal, y_gallery: np.ndarray, svm_C: float, svm_gamma, d_used=None, lap=None):
    """SVC(C=svm_C, gamma=svm_gamma).fit(gal, y_gallery) at the optimum of every pair's dual -> predict of ``qry`` on the device.  The
    labels are encoded with np.unique (scikit-learn's ``classes_``); ``d_used``: the columns that count for gamma='scale' (the rest is
    zero padding).  Returns (y_pred, votes [nq,K] on the host, the most iterations of any pair)."""
    from . import _lib
    torch = _lib.require_gpu()
    classes, codes = np.unique(np.asarray(y_gallery), return_inverse=True)
    n, d = int(gal.shape[0]), int(gal.shape[1])
    ops.check_rbf_svm_args(n, d, len(classes), C=svm_C, gamma=svm_gamma, tol=RBF_SVM_TOL, max_iter=RBF_SVM_MAX_ITER)
    labels = torch.from_numpy(codes.astype(np.int32).reshape(-1)).to(gal.device)
    gamma = ops.rbf_svm_gamma(gal, d_used) if isinstance(svm_gamma, str) else float(svm_gamma)
    dual_coef, rho, info = ops.rbf_svm_fit(gal, labels, len(classes), gamma, C=svm_C, tol=RBF_SVM_TOL, max_iter=RBF_SVM_MAX_ITER)
    if not info["converged"]:
        raise RuntimeError("the device RBF SVM fit on the n=%d x d=%d gallery (K=%d classes) left %d pairs of classes short of the optimum "
                           "after %d iterations" % (n, d, len(classes), info["pairs_at_max_iter"], info["iterations"]))
    if lap is not None:
        lap("svm_fit_s")
    if qry.shape[0] == 0:                                       # no probe: nothing to label (the entry points want at least one row)
        if lap is not None:
            lap("svm_predict_s")
        return classes[:0], np.zeros((0, len(classes)), dtype=np.int32), info["iterations"]
    pred, votes = ops.rbf_svm_predict(qry, gal, labels, len(classes), gamma, dual_coef, rho)
    if lap is not None:
        lap("svm_predict_s")
    return classes[pred.cpu().numpy()], votes.cpu().numpy(), info["iterations"]


def _knn_predict(ops, qry, gal, y_gallery: np.ndarray, n_neighbors: int):
    """KNeighborsClassifier(n_neighbors).fit(gal, y_gallery) -> kneighbors + predict of ``qry`` on the device (ops.knn).  The labels are
    encoded with np.unique, so the vote's smallest-label rule runs over scikit-learn's sorted ``classes_`` and any label type works.
    Returns (y_pred, nn_index [nq,k], nn_dist [nq,k]) on the host."""
    from . import _lib
    torch = _lib.require_gpu()
    classes, codes = np.unique(np.asarray(y_gallery), return_inverse=True)
    labels = torch.from_numpy(codes.astype(np.int32).reshape(-1)).to(gal.device)
    idx, d2, pred = ops.knn(qry, gal, n_neighbors, labels)
    return classes[pred.cpu().numpy()], idx.cpu().numpy(), np.sqrt(d2.cpu().numpy())


def one_nn_identification(X, y: np.ndarray, split=None,
                          pca_components: Optional[int] = None, timings: Optional[dict] = None, device=None,
                          n_neighbors: int = 1, pca: str = "host", classifier: str = "knn", svm_C: float = 1.0, svm_gamma="scale") -> Dict:
    """The protocol of facerec_test.py:401-432: 'k-NN' (pca_components=None) or 'k-NN+PCA'
    (pca_components=128, the Pipeline of :421 -- PCA is fitted on the gallery half by scikit-learn on
    the host, exactly as the reference does, and the projected vectors go back to the device for the search).

    X: [N, D] float32 embeddings, CUDA tensor or NumPy array (uploaded to ``device``, default: the current one); y: [N] labels.
    split: None (compute it here), a (train, test) pair over the FILTERED samples, or a SplitJob started on the same labels.
    Returns accuracy, the split, predictions and nearest-gallery indices.  ``timings`` (optional dict) receives the
    device-synchronised wall seconds of each phase: normalize_s, host_split_s, select_s, nn1_s, readback_s (indices and
    distances back to the host + the label comparison).
    n_neighbors: 1 labels a probe by its nearest gallery row (ops.nn1); more by the uniform vote of that many (ops.knn: 'nn_index' and
    'nn_dist' become [nq, k]; the search is still timed as nn1_s).
    pca: "host" fits and applies scikit-learn's PCA on the CPU as above; "device" runs ops.pca_fit on the gallery and
    ops.pca_transform on both halves without leaving the GPU (deterministic fp64; a fit that does not converge raises RuntimeError)
    and records the phase in ``timings`` as pca_s.
    classifier: "knn" is all of the above; "linear_svm" is the 'linear svm' row of :429 (with ``pca_components``: the Pipeline of
    PCA and LinearSVC()) -- LinearSVC(C=svm_C) fitted on the gallery half at the optimum of its objective (ops.linear_svm_fit; a fit
    that does not converge raises RuntimeError), the probes labelled by ops.linear_svm_predict.  The result then holds 'decision'
    ([nq, K'] on the host) and 'svm_iterations' in place of 'nn_index' / 'nn_dist', and ``timings`` receives svm_fit_s and
    svm_predict_s in place of nn1_s.  ``n_neighbors`` must stay 1.  "rbf_svm" is the 'svm' row, SVC(C=svm_C, gamma=svm_gamma): every pair of
    classes solved to the optimum of its dual (ops.rbf_svm_fit; a pair that stops at RBF_SVM_MAX_ITER raises RuntimeError), the probes
    labelled by the pairs' votes (ops.rbf_svm_predict).  ``svm_gamma``: "scale" (from the gallery half, the unpadded columns after a PCA)
    or a positive finite number.  The result holds 'votes' ([nq, K] on the host) and 'svm_iterations' in place of 'nn_index' /
    'nn_dist'; ``timings`` as for "linear_svm"."""
    import time
    from . import _lib, ops
    ops.check_n_neighbors(n_neighbors)
    check_pca_mode(pca)
    check_classifier(classifier, n_neighbors, svm_C, svm_gamma)
    if pca_components and pca == "device":
        ops.check_pca_components(pca_components)
    torch = _lib.require_gpu()
    if isinstance(X, np.ndarray):
        X = torch.from_numpy(np.ascontiguousarray(X, dtype=np.float32)).to(_lib.cuda_device(device))

    def lap(key, t_prev):
        if timings is None:
            return 0.0
        torch.cuda.synchronize(X.device)
        t = time.perf_counter()
        timings[key] = t - t_prev
        return t

    t = lap("_start", 0.0)
    Xn = ops.l2_normalize(X.contiguous())                       # :401
    t = lap("normalize_s", t)
    if isinstance(split, SplitJob):                             # started earlier on the same labels: wait for it
        indices, y_enc, train, test = split.result()
    else:
        indices, y_enc = filter_classes(y)                      # :407-412
        train, test = split if split is not None else stratified_half_split(y_enc)
    t = lap("host_split_s", t)
    Xn = Xn[torch.from_numpy(indices).to(Xn.device)].contiguous()   # :413
    gal = Xn[torch.from_numpy(train).to(Xn.device)].contiguous()
    qry = Xn[torch.from_numpy(test).to(Xn.device)].contiguous()
    t = lap("select_s", t)
    if pca_components and pca == "device":
        gal, qry = _device_pca(ops, gal, qry, pca_components)
        t = lap("pca_s", t)
    elif pca_components:
        from sklearn.decomposition import PCA
        fitted = PCA(n_components=pca_components).fit(gal.cpu().numpy())
        pad = (-pca_components) % 8                      # hsefr_nn1 wants d % 8 == 0: zero columns change no distance

        def proj(t):
            z = fitted.transform(t.cpu().numpy()).astype(np.float32)
            return torch.from_numpy(np.pad(z, ((0, 0), (0, pad)))).to(Xn.device).contiguous()
        gal, qry = proj(gal), proj(qry)
    if classifier in ("linear_svm", "rbf_svm"):
        clock = [t]

        def svm_lap(key):
            clock[0] = lap(key, clock[0])
        if classifier == "linear_svm":
            y_pred, table, svm_iterations = _linear_svm_predict(ops, qry, gal, y_enc[train], svm_C, svm_lap)
        else:
            y_pred, table, svm_iterations = _rbf_svm_predict(ops, qry, gal, y_enc[train], svm_C, svm_gamma, pca_components or None, svm_lap)
        t = clock[0]
        acc = float((y_pred == y_enc[test]).mean()) if len(test) else float("nan")
        t = lap("readback_s", t)
        if timings is not None:
            timings.pop("_start", None)
        return {"accuracy": acc, "indices": indices, "y": y_enc, "train": train, "test": test, "y_pred": y_pred,
                "decision" if classifier == "linear_svm" else "votes": table,
                "svm_iterations": svm_iterations, "num_classes": int(y_enc.max() + 1) if len(y_enc) else 0}
    if n_neighbors == 1:
        nn_idx, nn_d2 = ops.nn1(qry, gal)
        t = lap("nn1_s", t)
        nn_idx_h = nn_idx.cpu().numpy()
        nn_dist_h = np.sqrt(nn_d2.cpu().numpy())
        y_pred = y_enc[train][nn_idx_h]
    else:
        y_pred, nn_idx_h, nn_dist_h = _knn_predict(ops, qry, gal, y_enc[train], n_neighbors)
        t = lap("nn1_s", t)
    acc = float((y_pred == y_enc[test]).mean()) if len(test) else float("nan")
    t = lap("readback_s", t)
    if timings is not None:
        timings.pop("_start", None)
        timings["nn1_shape"] = (int(qry.shape[0]), int(gal.shape[0]), int(qry.shape[1]))
    return {"accuracy": acc, "indices": indices, "y": y_enc, "train": train, "test": test, "y_pred": y_pred,
            "nn_index": nn_idx_h, "nn_dist": nn_dist_h, "num_classes": int(y_enc.max() + 1) if len(y_enc) else 0}


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


def _nn1_predict(torch, ops, Xd, train, test, y, n_neighbors: int = 1):
    gal = Xd[torch.from_numpy(np.asarray(train, dtype=np.int64)).to(Xd.device)].contiguous()
    qry = Xd[torch.from_numpy(np.asarray(test, dtype=np.int64)).to(Xd.device)].contiguous()
    if n_neighbors != 1:
        return _knn_predict(ops, qry, gal, y[np.asarray(train)], n_neighbors)
    nn_idx, nn_d2 = ops.nn1(qry, gal)
    nn_idx_h = nn_idx.cpu().numpy()
    return y[np.asarray(train)][nn_idx_h], nn_idx_h, np.sqrt(nn_d2.cpu().numpy())


def cross_validated_1nn(X, y: np.ndarray, cv, normalize: bool = True, device=None, n_neighbors: int = 1) -> Dict:
    """classifier_tester (facerec_test.py:199-207) for KNeighborsClassifier(n_neighbors=1, p=2) over an explicit list of
    (train, test) index pairs -- e.g. single_image_per_class_splits(y) in place of the stratified half split (:200-201) --
    with every search on the GPU.  Returns the per-split accuracies and their mean / std as the reference prints them.
    ``n_neighbors`` > 1 scores KNeighborsClassifier(n_neighbors) instead (ops.knn's uniform vote)."""
    from . import _lib, ops
    ops.check_n_neighbors(n_neighbors)
    torch = _lib.require_gpu()
    if isinstance(X, np.ndarray):
        X = torch.from_numpy(np.ascontiguousarray(X, dtype=np.float32)).to(_lib.cuda_device(device))
    Xd = ops.l2_normalize(X.contiguous()) if normalize else X.contiguous()
    y = np.asarray(y)
    accs, preds = [], []
    for train, test in cv:
        y_pred, _, _ = _nn1_predict(torch, ops, Xd, train, test, y, n_neighbors)
        preds.append(y_pred)
        accs.append(float((y_pred == y[np.asarray(test)]).mean()) if len(test) else float("nan"))
    accs = np.asarray(accs)
    return {"accuracies": accs, "mean": float(accs.mean()) if len(accs) else float("nan"),
            "std": float(accs.std()) if len(accs) else float("nan"), "y_pred": preds}


def gallery_probe_identification(X_train, y_train: np.ndarray, X_test, y_test: np.ndarray, normalize: bool = False,
                                 pca_components: Optional[int] = None, device=None, n_neighbors: int = 1, pca: str = "host",
                                 classifier: str = "knn", svm_C: float = 1.0, svm_gamma="scale") -> Dict:
    """The gallery / probe protocol of tf_train_test_recognition (facerec_test.py:260-288): the '1-NN' classifier (and
    '1-NN+PCA' with ``pca_components``, 16 at :269) FITTED on the gallery features, every probe labelled by its nearest
    gallery row; accuracy = share of probes whose label is right (:287).  NB the reference computes L2-normalised copies
    (:262,265) and then fits / predicts on the UN-normalised ``X_train`` / ``X_test`` (:284-285): ``normalize=False`` is what
    it runs, ``normalize=True`` what the copies suggest it meant.  The search runs on the GPU (hsefr_nn1: ties -> the lowest
    gallery index, scikit-learn's own choice).  ``n_neighbors`` > 1 gives the '3-NN' / '3-NN+PCA' rows of :269-272 (hsefr_knn: the
    uniform vote, equal counts to the smallest label as in scikit-learn's predict; 'nn_index' and 'nn_dist' become [nq, k]).
    ``pca``: "host" is scikit-learn's PCA on the CPU; "device" fits on the gallery and projects both sets with ops.pca_fit /
    ops.pca_transform on the GPU (deterministic fp64; a fit that does not converge raises RuntimeError).
    ``classifier``: "knn" is all of the above; "linear_svm" gives the 'linear svm' / 'linear svm+PCA' rows of :269-273 -- LinearSVC(C=svm_C)
    fitted on the gallery (after the projection, when ``pca_components`` is set) at the optimum of its objective (ops.linear_svm_fit; a fit
    that does not converge raises RuntimeError), the probes labelled by ops.linear_svm_predict: the result holds 'accuracy', 'y_pred',
    'decision' ([nq, K'] on the host) and 'svm_iterations'.  scikit-learn's default tolerance stops short of the optimum, so its labels
    can differ on probes whose two largest decision values are closer than about 1e-4 (1e-3 after PCA).  ``n_neighbors`` must stay 1.
    "rbf_svm" gives the 'svm' row of :269-273, SVC(C=svm_C, gamma=svm_gamma): libsvm's one-vs-one C-SVC with the RBF kernel, every pair of
    classes solved to the optimum of its dual (ops.rbf_svm_fit; a pair that stops at RBF_SVM_MAX_ITER raises RuntimeError), the probes
    labelled by the pairs' votes (ops.rbf_svm_predict): the result holds 'accuracy', 'y_pred', 'votes' ([nq, K] on the host) and
    'svm_iterations'.  ``svm_gamma``: "scale" (1 / (d Var) of the gallery rows, over the unpadded columns after a PCA) or a positive finite
    number.  scikit-learn's default tolerance stops about 3e-4 short of the optimum in a pair's decision value, so a vote whose value
    is that close to 0 can differ."""
    from . import _lib, ops
    ops.check_n_neighbors(n_neighbors, len(np.asarray(y_train)))
    check_pca_mode(pca)
    check_classifier(classifier, n_neighbors, svm_C, svm_gamma)
    if pca_components and pca == "device":
        ops.check_pca_components(pca_components, len(np.asarray(y_train)))
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
    if pca_components and pca == "device":
        gal, qry = _device_pca(ops, gal, qry, pca_components)
    elif pca_components:
        from sklearn.decomposition import PCA
        fitted = PCA(n_components=pca_components).fit(gal.cpu().numpy())
        pad = (-pca_components) % 8

        def proj(t):
            z = fitted.transform(t.cpu().numpy()).astype(np.float32)
            return torch.from_numpy(np.pad(z, ((0, 0), (0, pad)))).to(dev).contiguous()
        gal, qry = proj(gal), proj(qry)
    if classifier == "linear_svm":
        y_pred, decision, svm_iterations = _linear_svm_predict(ops, qry, gal, y_train, svm_C)
        acc = float((y_pred == y_test).mean()) if len(y_test) else float("nan")
        return {"accuracy": acc, "y_pred": y_pred, "decision": decision, "svm_iterations": svm_iterations}
    if classifier == "rbf_svm":
        y_pred, votes, svm_iterations = _rbf_svm_predict(ops, qry, gal, y_train, svm_C, svm_gamma, pca_components or None)
        acc = float((y_pred == y_test).mean()) if len(y_test) else float("nan")
        return {"accuracy": acc, "y_pred": y_pred, "votes": votes, "svm_iterations": svm_iterations}
    if n_neighbors == 1:
        nn_idx, nn_d2 = ops.nn1(qry, gal)
        nn_idx_h = nn_idx.cpu().numpy()
        y_pred, nn_dist_h = y_train[nn_idx_h], np.sqrt(nn_d2.cpu().numpy())
    else:
        y_pred, nn_idx_h, nn_dist_h = _knn_predict(ops, qry, gal, y_train, n_neighbors)
    acc = float((y_pred == y_test).mean()) if len(y_test) else float("nan")
    return {"accuracy": acc, "y_pred": y_pred, "nn_index": nn_idx_h, "nn_dist": nn_dist_h}


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
