"""Cross-validation of a C-SVC on a gkm kernel matrix that stays in HBM -- SURVEY.md §8(f4).

The reference trains `sklearn.svm.SVC(kernel="precomputed")` once per fold on host copies of the
matrix (`scripts/gkmsvm.py:104-125`, fancy-indexed sub-matrices, one process per fold).  Here the
matrix never leaves the GPU: every fold of every repeat is one workgroup of `k_smo`
(gkmqc_amd/csrc/gkm_svm.hip, include/gkm_svm.h) reading the resident matrix through index lists,
and the decision values come from `k_decision`.  Only the index lists go up and the per-fold
decision values (a few thousand doubles) come back; fold generation (StratifiedKFold) and the AUC
stay scikit-learn's so that the folds and the metric are the reference's own.

Parity (tests/test_svm_gpu.py): dual coefficients, intercept and decision values bit-identical to
scikit-learn's LIBSVM on the same matrix, hence identical AUC.
"""
import ctypes
import logging

import numpy as np

from . import device


SHAPE_REFUSED = 5        # GKMSVM_RC_SHAPE_REFUSED (include/gkm_svm.h)
FAST_FOLD_SAMPLES = 16384  # k_smo: one workgroup per fold, 1024 threads x 16 samples in registers (gkm_svm.hip)
MAX_FOLD_SAMPLES = 60000   # k_smo_general: state in global memory (scanned part in LDS up to 8 192 samples), also the solver with LIBSVM's shrinking


class SvmError(RuntimeError):
    pass


def _lib():
    L = device.load()
    if not hasattr(L, "_svm_bound"):
        vp, i32, i64, dbl = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64, ctypes.c_double
        L.gkmsvm_train_batch.restype = i32
        L.gkmsvm_train_batch.argtypes = (i32, vp, i64, i32, i32, vp, vp, vp, dbl, dbl, vp, vp, vp, vp, vp)
        L.gkmsvm_train_batch_general.restype = i32
        L.gkmsvm_train_batch_general.argtypes = (i32, vp, i64, i32, i32, vp, vp, vp, dbl, dbl, i32, vp, vp, vp, vp, vp)
        L.gkmsvm_train_batch_boxed.restype = i32
        L.gkmsvm_train_batch_boxed.argtypes = (i32, vp, i64, i32, i32, vp, vp, vp, vp, dbl, vp, vp, vp, vp, vp)
        L.gkmsvm_train_batch_general_boxed.restype = i32
        L.gkmsvm_train_batch_general_boxed.argtypes = (i32, vp, i64, i32, i32, vp, vp, vp, vp, dbl, i32, vp, vp, vp, vp, vp)
        L.gkmsvm_decision_batch.restype = i32
        L.gkmsvm_decision_batch.argtypes = (i32, vp, i64, i32, vp, vp, vp, vp, vp, vp, vp, vp, vp)
        L.gkmsvm_train_svr_batch.restype = i32
        L.gkmsvm_train_svr_batch.argtypes = (i32, vp, i64, i32, i32, vp, vp, vp, dbl, dbl, dbl, vp, vp, vp, vp)
        L.gkmsvm_train_svr_batch_general.restype = i32
        L.gkmsvm_train_svr_batch_general.argtypes = (i32, vp, i64, i32, i32, vp, vp, vp, dbl, dbl, dbl, i32, vp, vp, vp, vp)
        L.gkmsvm_decision_signed_batch.restype = i32
        L.gkmsvm_decision_signed_batch.argtypes = (i32, vp, i64, i32, vp, vp, vp, vp, vp, vp, vp, vp)
        L.gkmsvm_last_error.restype = ctypes.c_char_p
        L.gkmsvm_release_cache.restype = None
        L._svm_bound = True
    return L


def libsvm_order(train, y):
    """Training indices in LIBSVM's internal order (sklearn's svm_group_classes: classes sorted by
    label, the samples of a class in their original order) and the size of class 0."""
    train = np.asarray(train)
    return _class_order(train, np.asarray(y)[train])


def _class_order(train, lab):
    """libsvm_order with the labels of the training samples themselves: lab[j] belongs to train[j]."""
    train, lab = np.asarray(train), np.asarray(lab)
    if lab.shape != train.shape:
        raise SvmError("a problem needs one label per training sample")
    classes = np.unique(lab)
    if len(classes) != 2:
        raise SvmError("a fold needs samples of exactly two classes")
    first = train[lab == classes[0]]
    second = train[lab == classes[1]]
    return np.concatenate((first, second)).astype(np.int32), int(len(first))


class FoldSolutions:
    """Result of `train_folds`: per-fold alpha (LIBSVM order), rho, iteration count, and `box`: the (nprob, 2) upper
    bounds of alpha, of the class-0 positions and of the rest (`problem_boxes`; (C, C) for a plain C)."""

    def __init__(self, idx, n0, alpha, grad, rho, iters, box=None):
        self.idx, self.n0, self.alpha, self.grad, self.rho, self.iters = idx, n0, alpha, grad, rho, iters
        self.box = box

    def dual_coef(self, f):
        """sklearn's `dual_coef_[0]` and `support_` of fold f (positions in the fold's `train`)."""
        a = self.alpha[f]
        ysign = np.where(np.arange(len(a)) < self.n0[f], 1.0, -1.0)
        sv = np.nonzero(a > 0)[0]
        return -(a[sv] * ysign[sv]), self.idx[f][sv]


def train_folds(K, trains, y, C=1.0, tol=1e-3, shrinking=False, about_to_launch=None, class_weight=None):
    """Solve one C-SVC per entry of `trains` (index arrays into the symmetric torch CUDA fp64
    matrix K) concurrently.  Returns (FoldSolutions, device handles for `decision_values`).
    `shrinking`: LIBSVM's shrinking heuristic (scikit-learn `SVC(shrinking=True)`); it and folds of more
    than 16 384 samples run on the general solver (k_smo_general), everything else on k_smo.
    `C`, `class_weight`: one value, or one per problem (`problem_boxes`)."""
    y = np.asarray(y)
    return train_tasks(K, trains, [y[np.asarray(t)] for t in trains], C, tol, shrinking, about_to_launch, class_weight)


def _is_pair(w):
    return (isinstance(w, (tuple, list, np.ndarray)) and len(w) == 2
            and all(isinstance(x, (int, float, np.integer, np.floating)) and not isinstance(x, bool) for x in w))


def problem_weights(labels, class_weight=None):
    """The class weights of every problem as numbers -> (nprob, 2) float64: column 0 weighs the class that sorts first
    (label 0), column 1 the other (label 1).  `class_weight`: None (1, 1); "balanced", resolved per problem to
    l / (2 * count of the class) in float64 -- scikit-learn's n_samples / (n_classes * np.bincount(y)); a pair
    (w0, w1); or a sequence of one of those per problem.  Weights that are not finite or not > 0 raise SvmError."""
    nprob = len(labels)
    if class_weight is None or isinstance(class_weight, str) or _is_pair(class_weight):
        per = [class_weight] * nprob
    else:
        try:
            per = list(class_weight)
        except TypeError:
            raise SvmError("class_weight: None, 'balanced', a pair (w0, w1) or one of those per problem")
        if len(per) != nprob:
            raise SvmError("%d class weightings for %d problems" % (len(per), nprob))
    w = np.ones((nprob, 2), dtype=np.float64)
    for t, (cw, lab) in enumerate(zip(per, labels)):
        if cw is None:
            continue
        if isinstance(cw, str):
            if cw != "balanced":
                raise SvmError("class_weight: unknown setting %r" % (cw,))
            lab = np.asarray(lab)
            classes, counts = np.unique(lab, return_counts=True)
            if len(classes) != 2:
                raise SvmError("a fold needs samples of exactly two classes")
            w[t] = np.float64(lab.size) / (2 * counts).astype(np.float64)
        elif _is_pair(cw):
            w[t] = (float(cw[0]), float(cw[1]))
        else:
            raise SvmError("class_weight: None, 'balanced', a pair (w0, w1) or one of those per problem")
    if not (np.isfinite(w).all() and (w > 0).all()):
        raise SvmError("class weights must be finite and > 0")
    return w


def problem_boxes(labels, C=1.0, class_weight=None):
    """The bounds the boxed solver entries take (include/gkm_svm.h) -> (nprob, 2) float64:
    box[t] = (C_t * w_t[0], C_t * w_t[1]), each one rounded float64 product -- what LIBSVM computes from scikit-learn's
    `class_weight_` (Cp and Cn; class 0 is LIBSVM's y = +1).  `C`: one float or one per problem; `class_weight`: see
    `problem_weights`.  A C or a weight that is not finite or not > 0 raises SvmError."""
    nprob = len(labels)
    w = problem_weights(labels, class_weight)
    try:
        Cs = np.asarray(C, dtype=np.float64)
    except (TypeError, ValueError):
        raise SvmError("C: one float or one per problem")
    if Cs.ndim == 0:
        Cs = np.repeat(Cs, nprob)
    if Cs.shape != (nprob,):
        raise SvmError("%d values of C for %d problems" % (Cs.size, nprob))
    if not (np.isfinite(Cs).all() and (Cs > 0).all()):
        raise SvmError("C must be finite and > 0")
    with np.errstate(over="ignore", under="ignore"):
        box = Cs[:, None] * w
    if not (np.isfinite(box).all() and (box > 0).all()):
        raise SvmError("C times a class weight must be finite and > 0")
    return np.ascontiguousarray(box)


def task_orders(trains, labels):
    """What train_tasks hands the solver per problem -> [(indices in LIBSVM's order, size of class 0)]: libsvm_order for
    labels given per training sample (labels[t][j] belongs to trains[t][j])."""
    if len(labels) != len(trains):
        raise SvmError("%d label vectors for %d problems" % (len(labels), len(trains)))
    return [_class_order(t, lab) for t, lab in zip(trains, labels)]


def train_tasks(K, trains, labels, C=1.0, tol=1e-3, shrinking=False, about_to_launch=None, class_weight=None):
    """train_folds with a label vector of its own per problem: labels[t][j] is the label of sample trains[t][j].  A
    problem is its index list in LIBSVM's order and the size of class 0, so the tasks of one labelled pool (one label
    column each, over any subset of the pool) are solved concurrently from the pool's one matrix.
    With one scalar `C` and `class_weight=None` every problem shares the box C (the unboxed solver entries); with a `C`
    per problem or class weights (`problem_boxes`) each problem has a bound per class, so a grid of settings is one
    launch (the boxed entries: same solvers, same choice between them)."""
    import torch
    if not (K.is_cuda and K.dtype == torch.float64 and K.dim() == 2 and K.shape[0] == K.shape[1]
            and K.stride(1) == 1):
        raise SvmError("K must be a square fp64 CUDA tensor with unit column stride")
    L = _lib()
    dev = K.device
    orders = task_orders(trains, labels)
    idx = [o[0] for o in orders]
    n0 = np.array([o[1] for o in orders], dtype=np.int32)
    off = np.zeros(len(idx) + 1, dtype=np.int64)
    off[1:] = np.cumsum([len(i) for i in idx])
    boxed = not (np.ndim(C) == 0 and class_weight is None)
    if boxed:
        box = problem_boxes(labels, C, class_weight)
        return _train_boxed(K, L, idx, n0, off, box, tol, shrinking, about_to_launch)
    with torch.cuda.device(dev):
        stream = torch.cuda.current_stream().cuda_stream
        d_idx = torch.from_numpy(np.concatenate(idx)).to(dev)
        d_alpha = torch.empty(int(off[-1]), dtype=torch.float64, device=dev)
        d_grad = torch.empty_like(d_alpha)
        d_rho = torch.empty(len(idx), dtype=torch.float64, device=dev)
        d_it = torch.empty(len(idx), dtype=torch.int32, device=dev)
        if about_to_launch is not None:
            about_to_launch()     # everything on the host is done: the solver kernel goes out within microseconds
        if shrinking or max(len(i) for i in idx) > FAST_FOLD_SAMPLES:
            rc = L.gkmsvm_train_batch_general(dev.index or 0, K.data_ptr(), K.stride(0), K.shape[0], len(idx),
                                              d_idx.data_ptr(), off.ctypes.data, n0.ctypes.data, float(C), float(tol),
                                              1 if shrinking else 0, d_alpha.data_ptr(), d_grad.data_ptr(),
                                              d_rho.data_ptr(), d_it.data_ptr(), stream)
        else:
            rc = L.gkmsvm_train_batch(dev.index or 0, K.data_ptr(), K.stride(0), K.shape[0], len(idx), d_idx.data_ptr(),
                                      off.ctypes.data, n0.ctypes.data, float(C), float(tol), d_alpha.data_ptr(),
                                      d_grad.data_ptr(), d_rho.data_ptr(), d_it.data_ptr(), stream)
            if rc == SHAPE_REFUSED:
                # ONLY a launch shape the device refuses (the big shapes take up to 144 KB of LDS; include/gkm_svm.h):
                # the general solver needs none of that and returns the same bits without shrinking.  Bad arguments
                # or a device fault are not retried -- the retry would fail too and hide the cause.
                first = L.gkmsvm_last_error().decode()
                logging.warning("k_smo: %s: solving with the general GPU solver", first)
                rc = L.gkmsvm_train_batch_general(dev.index or 0, K.data_ptr(), K.stride(0), K.shape[0], len(idx),
                                                  d_idx.data_ptr(), off.ctypes.data, n0.ctypes.data, float(C), float(tol),
                                                  0, d_alpha.data_ptr(), d_grad.data_ptr(), d_rho.data_ptr(),
                                                  d_it.data_ptr(), stream)
                if rc:
                    raise SvmError("gkmsvm_train_batch: %s; then gkmsvm_train_batch_general: %s"
                                   % (first, L.gkmsvm_last_error().decode()))
        if rc:
            raise SvmError("gkmsvm_train_batch: %s" % L.gkmsvm_last_error().decode())
        alpha = d_alpha.cpu().numpy()
        grad = d_grad.cpu().numpy()
        rho = d_rho.cpu().numpy()
        iters = d_it.cpu().numpy()
    if (iters < 0).any():
        # scikit-learn (max_iter=-1) would have kept iterating: these folds are not the reference's solution
        logging.warning("SMO stopped at the iteration cap in %d fold(s)", int((iters < 0).sum()))
    sol = FoldSolutions(idx, n0, [alpha[off[f]:off[f + 1]] for f in range(len(idx))],
                        [grad[off[f]:off[f + 1]] for f in range(len(idx))], rho, iters,
                        np.full((len(idx), 2), float(C)))
    return sol, dict(idx=d_idx, off=off, n0=n0, alpha=d_alpha, rho=d_rho)


def _train_boxed(K, L, idx, n0, off, box, tol, shrinking, about_to_launch):
    """train_tasks' launch with a box per problem: gkmsvm_train_batch_boxed / gkmsvm_train_batch_general_boxed, chosen
    and retried as the unboxed pair."""
    import torch
    dev = K.device
    with torch.cuda.device(dev):
        stream = torch.cuda.current_stream().cuda_stream
        d_idx = torch.from_numpy(np.concatenate(idx)).to(dev)
        d_alpha = torch.empty(int(off[-1]), dtype=torch.float64, device=dev)
        d_grad = torch.empty_like(d_alpha)
        d_rho = torch.empty(len(idx), dtype=torch.float64, device=dev)
        d_it = torch.empty(len(idx), dtype=torch.int32, device=dev)
        head = (dev.index or 0, K.data_ptr(), K.stride(0), K.shape[0], len(idx), d_idx.data_ptr(), off.ctypes.data,
                n0.ctypes.data, box.ctypes.data, float(tol))
        outs = (d_alpha.data_ptr(), d_grad.data_ptr(), d_rho.data_ptr(), d_it.data_ptr(), stream)
        if about_to_launch is not None:
            about_to_launch()
        if shrinking or max(len(i) for i in idx) > FAST_FOLD_SAMPLES:
            rc = L.gkmsvm_train_batch_general_boxed(*head, 1 if shrinking else 0, *outs)
        else:
            rc = L.gkmsvm_train_batch_boxed(*head, *outs)
            if rc == SHAPE_REFUSED:   # as the unboxed pair: only a launch shape the device refuses is retried
                first = L.gkmsvm_last_error().decode()
                logging.warning("k_smo: %s: solving with the general GPU solver", first)
                rc = L.gkmsvm_train_batch_general_boxed(*head, 0, *outs)
                if rc:
                    raise SvmError("gkmsvm_train_batch_boxed: %s; then gkmsvm_train_batch_general_boxed: %s"
                                   % (first, L.gkmsvm_last_error().decode()))
        if rc:
            raise SvmError("gkmsvm_train_batch_boxed: %s" % L.gkmsvm_last_error().decode())
        alpha = d_alpha.cpu().numpy()
        grad = d_grad.cpu().numpy()
        rho = d_rho.cpu().numpy()
        iters = d_it.cpu().numpy()
    if (iters < 0).any():
        logging.warning("SMO stopped at the iteration cap in %d fold(s)", int((iters < 0).sum()))
    sol = FoldSolutions(idx, n0, [alpha[off[f]:off[f + 1]] for f in range(len(idx))],
                        [grad[off[f]:off[f + 1]] for f in range(len(idx))], rho, iters, box)
    return sol, dict(idx=d_idx, off=off, n0=n0, alpha=d_alpha, rho=d_rho)


def decision_values(K, handles, tests):
    """scikit-learn's `decision_function` of every fold on its test samples (list of arrays)."""
    import torch
    L = _lib()
    dev = K.device
    toff = np.zeros(len(tests) + 1, dtype=np.int64)
    toff[1:] = np.cumsum([len(t) for t in tests])
    with torch.cuda.device(dev):
        stream = torch.cuda.current_stream().cuda_stream
        d_test = torch.from_numpy(np.concatenate(tests).astype(np.int32)).to(dev)
        d_dec = torch.empty(int(toff[-1]), dtype=torch.float64, device=dev)
        rc = L.gkmsvm_decision_batch(dev.index or 0, K.data_ptr(), K.stride(0), len(tests), handles["idx"].data_ptr(),
                                     handles["off"].ctypes.data, handles["n0"].ctypes.data,
                                     handles["alpha"].data_ptr(), handles["rho"].data_ptr(), d_test.data_ptr(),
                                     toff.ctypes.data, d_dec.data_ptr(), stream)
        if rc:
            raise SvmError("gkmsvm_decision_batch: %s" % L.gkmsvm_last_error().decode())
        dec = d_dec.cpu().numpy()
    # sklearn flips the sign of LIBSVM's decision value for a two-class problem
    return [-dec[toff[f]:toff[f + 1]] for f in range(len(tests))]


class SvrSolutions:
    """Result of `train_svr_folds`, per problem: scikit-learn's `support_` (positions in the problem's `train`, ascending),
    `dual_coef_[0]` (alpha_k - alpha_{l+k}, nonzero), `intercept_[0]` (LIBSVM's rho negated) and the iteration count
    (negative: the GPU solver stopped at its cap and scikit-learn re-solved the problem)."""

    def __init__(self, trains, support, dual_coef, intercept, iters):
        self.trains, self.support, self.dual_coef = trains, support, dual_coef
        self.intercept, self.iters = intercept, iters


def _intercept(rho):
    """scikit-learn's intercept_ from LIBSVM's rho (its copy_intercept: -rho, and +0.0 for a zero rho)"""
    return -rho if rho != 0 else 0.0


def train_svr_folds(K, trains, z, C=1.0, epsilon=0.1, tol=1e-3, shrinking=False):
    """Solve one epsilon-SVR per entry of `trains` (index arrays into the symmetric torch CUDA fp64 matrix K) with
    targets z (indexed like the rows of K) concurrently -> SvrSolutions.  LIBSVM's solve_epsilon_svr: 2l solver
    positions per problem, so the solver choice counts 2l -- k_smo up to FAST_FOLD_SAMPLES without shrinking, the
    general solver (k_smo_general) up to MAX_FOLD_SAMPLES.  A problem that stops at the iteration cap is re-solved with
    scikit-learn's SVR."""
    import torch
    if not (K.is_cuda and K.dtype == torch.float64 and K.dim() == 2 and K.shape[0] == K.shape[1]
            and K.stride(1) == 1):
        raise SvmError("K must be a square fp64 CUDA tensor with unit column stride")
    trains = [np.asarray(t, dtype=np.int64) for t in trains]
    z = np.asarray(z, dtype=np.float64)
    if not trains or min(len(t) for t in trains) == 0:
        raise SvmError("a problem needs at least one sample")
    if max(2 * len(t) for t in trains) > MAX_FOLD_SAMPLES:
        raise SvmError("a problem has more than %d samples (2l solver positions > %d)"
                       % (MAX_FOLD_SAMPLES // 2, MAX_FOLD_SAMPLES))
    if not np.isfinite(z[np.concatenate(trains)]).all():
        raise SvmError("targets must be finite")
    L = _lib()
    dev = K.device
    off = np.zeros(len(trains) + 1, dtype=np.int64)
    off[1:] = np.cumsum([len(t) for t in trains])
    idx = np.concatenate(trains).astype(np.int32)
    with torch.cuda.device(dev):
        stream = torch.cuda.current_stream().cuda_stream
        d_idx = torch.from_numpy(idx).to(dev)
        d_z = torch.from_numpy(np.ascontiguousarray(z[idx])).to(dev)
        d_coef = torch.empty(int(off[-1]), dtype=torch.float64, device=dev)
        d_rho = torch.empty(len(trains), dtype=torch.float64, device=dev)
        d_it = torch.empty(len(trains), dtype=torch.int32, device=dev)
        args = (dev.index or 0, K.data_ptr(), K.stride(0), K.shape[0], len(trains), d_idx.data_ptr(), off.ctypes.data,
                d_z.data_ptr(), float(C), float(epsilon), float(tol))
        outs = (d_coef.data_ptr(), d_rho.data_ptr(), d_it.data_ptr(), stream)
        if shrinking or 2 * max(len(t) for t in trains) > FAST_FOLD_SAMPLES:
            rc = L.gkmsvm_train_svr_batch_general(*args, 1 if shrinking else 0, *outs)
        else:
            rc = L.gkmsvm_train_svr_batch(*args, *outs)
            if rc == SHAPE_REFUSED:   # as train_folds: only a launch shape the device refuses is retried
                first = L.gkmsvm_last_error().decode()
                logging.warning("k_smo: %s: solving with the general GPU solver", first)
                rc = L.gkmsvm_train_svr_batch_general(*args, 0, *outs)
                if rc:
                    raise SvmError("gkmsvm_train_svr_batch: %s; then gkmsvm_train_svr_batch_general: %s"
                                   % (first, L.gkmsvm_last_error().decode()))
        if rc:
            raise SvmError("gkmsvm_train_svr_batch: %s" % L.gkmsvm_last_error().decode())
        coef = d_coef.cpu().numpy()
        rho = d_rho.cpu().numpy()
        iters = d_it.cpu().numpy()
    support, dual, intercept = [], [], np.zeros(len(trains))
    for f in range(len(trains)):
        c = coef[off[f]:off[f + 1]]
        sv = np.nonzero(c != 0)[0]       # LIBSVM: fabs(alpha) > 0
        support.append(sv)
        dual.append(c[sv])
        intercept[f] = _intercept(float(rho[f]))
    capped = [f for f in range(len(trains)) if iters[f] < 0]
    if capped:   # scikit-learn (max_iter=-1) would have kept iterating: re-solve these problems with it
        from sklearn.svm import SVR
        logging.warning("%d SVR problem(s) re-solved with scikit-learn (iteration cap of the GPU solver)", len(capped))
        for f in capped:
            tr = trains[f]
            m = SVR(kernel="precomputed", C=C, epsilon=epsilon, tol=tol, shrinking=bool(shrinking))
            m.fit(device_block(K, tr, tr).cpu().numpy(), z[tr])
            support[f], dual[f], intercept[f] = m.support_.astype(np.int64), m.dual_coef_[0].copy(), m.intercept_[0]
    return SvrSolutions(trains, support, dual, intercept, iters)


def svr_predict(K, sol, tests):
    """scikit-learn's `SVR.predict` of every problem of `sol` (SvrSolutions) on its test samples (index arrays into K):
    the signed decision k_decision<true>, sum_k dual_coef_k K(t, sv_k) in support-vector order minus rho."""
    import torch
    L = _lib()
    dev = K.device
    off = np.zeros(len(tests) + 1, dtype=np.int64)
    off[1:] = np.cumsum([len(s) for s in sol.support])
    toff = np.zeros(len(tests) + 1, dtype=np.int64)
    toff[1:] = np.cumsum([len(t) for t in tests])
    # (one padding entry past the last problem: the arrays are never empty, even when no problem has a support vector)
    rows = np.concatenate([sol.trains[f][sol.support[f]] for f in range(len(tests))] + [[0]]).astype(np.int32)
    with torch.cuda.device(dev):
        stream = torch.cuda.current_stream().cuda_stream
        d_idx = torch.from_numpy(rows).to(dev)
        d_coef = torch.from_numpy(np.concatenate(list(sol.dual_coef) + [[0.0]]).astype(np.float64)).to(dev)
        d_rho = torch.from_numpy(-np.asarray(sol.intercept, dtype=np.float64)).to(dev)    # scikit-learn's rho = -intercept_
        d_test = torch.from_numpy(np.concatenate(tests).astype(np.int32)).to(dev)
        d_dec = torch.empty(int(toff[-1]), dtype=torch.float64, device=dev)
        rc = L.gkmsvm_decision_signed_batch(dev.index or 0, K.data_ptr(), K.stride(0), len(tests), d_idx.data_ptr(),
                                            off.ctypes.data, d_coef.data_ptr(), d_rho.data_ptr(), d_test.data_ptr(),
                                            toff.ctypes.data, d_dec.data_ptr(), stream)
        if rc:
            raise SvmError("gkmsvm_decision_signed_batch: %s" % L.gkmsvm_last_error().decode())
        dec = d_dec.cpu().numpy()
    return [dec[toff[f]:toff[f + 1]] for f in range(len(tests))]


def device_block(K, rows, cols):
    """K[rows][:, cols] of the device matrix (torch tensor), still on the device."""
    import torch
    r = torch.as_tensor(np.asarray(rows), device=K.device, dtype=torch.long)
    c = torch.as_tensor(np.asarray(cols), device=K.device, dtype=torch.long)
    return K.index_select(0, r).index_select(1, c)


def plan_folds(args_svm, n_pseqs, n_nseqs):
    """The host-side half of `crossValidate` that does not need the matrix: labels and the ncv x repeats stratified folds
    (the reference's splitter and seeding, scripts/gkmsvm.py:134-150), equal folds solved once.  ~10 ms of scikit-learn
    at 10 000 sequences -- a pipeline draws the next subset's folds while the GPU is still busy with this one's."""
    from sklearn.model_selection import StratifiedKFold
    ncv, repeats, random_seeds = args_svm[4], args_svm[5], args_svm[7]
    if random_seeds is not None and random_seeds < 0:
        random_seeds = None
    seqids = ["p%4d" % i for i in range(n_pseqs)] + ["n%4d" % i for i in range(n_nseqs)]
    y = np.concatenate((np.repeat(1, n_pseqs), np.repeat(0, n_nseqs)))
    trains, tests = [], []
    for _ in range(repeats):
        folds = StratifiedKFold(n_splits=ncv, shuffle=True, random_state=random_seeds)
        for train, test in folds.split(seqids, y):
            trains.append(train)
            tests.append(test)
    # With a fixed seed the reference builds every repeat from the same random_state
    # (scripts/gkmsvm.py:148), i.e. the same folds again: solve each distinct fold once.
    first, which = {}, []
    for f, train in enumerate(trains):
        which.append(first.setdefault(train.tobytes(), len(first)))
    uniq = sorted(set(which))
    u_of = {w: [f for f in range(len(trains)) if which[f] == w][0] for w in uniq}
    return dict(sizes=(n_pseqs, n_nseqs), y=y, n_folds=len(trains), which=which,
                u_trains=[trains[u_of[w]] for w in uniq], u_tests=[tests[u_of[w]] for w in uniq])


def crossValidate(args_svm, K, n_pseqs, n_nseqs, about_to_launch=None, plan=None):
    """Same arguments and result as the reference's `crossValidate` (scripts/gkmsvm.py:127-176)
    with `K` a symmetric torch CUDA matrix: (mean AUC, std AUC) over ncv x repeats folds.
    about_to_launch: called once, right before the solver kernel is enqueued (init_many holds the next subset's Gram
    kernel back until then, so that the solver's few big workgroups find the CUs they need).
    plan: the folds drawn ahead of time by `plan_folds` for these sizes (otherwise drawn here)."""
    from sklearn.metrics import roc_auc_score
    regularization, precision, shrinking, _cache, _ncv, _repeats, fast_estimation = args_svm[:7]
    if fast_estimation != 0:
        raise NotImplementedError("fast AUC estimation is dead code in the reference (its regressor is never loaded)")
    if plan is None or plan["sizes"] != (n_pseqs, n_nseqs):
        plan = plan_folds(args_svm, n_pseqs, n_nseqs)
    y, which, u_trains, u_tests = plan["y"], plan["which"], plan["u_trains"], plan["u_tests"]
    logging.info("cross-validation on the GPU: %d folds (%d distinct)", plan["n_folds"], len(u_trains))
    sol, handles = train_folds(K, u_trains, y, regularization, precision, bool(shrinking), about_to_launch)
    scores = decision_values(K, handles, u_tests)
    capped = [f for f in range(len(u_trains)) if sol.iters[f] < 0]
    if capped:   # not converged within 10^7 iterations: the reference's solver has no cap, so use it for these folds
        from sklearn.svm import SVC
        logging.warning("%d fold(s) re-solved with scikit-learn (iteration cap of the GPU solver)", len(capped))
        for f in capped:
            tr, te = u_trains[f], u_tests[f]
            ktr = device_block(K, tr, tr).cpu().numpy()
            kte = device_block(K, te, tr).cpu().numpy()
            sv = SVC(kernel="precomputed", C=regularization, tol=precision, shrinking=bool(shrinking), cache_size=_cache)
            scores[f] = sv.fit(ktr, y[tr]).decision_function(kte)
            sol.alpha[f] = np.abs(sv.dual_coef_[0])     # (only its sum is used below)
    u_auc = []
    for f, (test, score) in enumerate(zip(u_tests, scores)):
        auc = roc_auc_score(y[test], score)
        nu = np.sum(sol.alpha[f]) / len(u_trains[f])
        logging.info("fold %d solved on the GPU: nu %.3f, AUC %.3f, %d iterations", f, nu, auc, abs(int(sol.iters[f])))
        u_auc.append(auc)
    aucs = [u_auc[w] for w in which]
    logging.info("cross-validation finished")
    return (np.mean(aucs), np.std(aucs))


def cross_validate_grid(K, n_pseqs, n_nseqs, Cs, class_weights=(None,), ncv=5, repeats=1, seed=1, tol=1e-3,
                        shrinking=False):
    """`crossValidate` for every setting of a grid at once: `Cs` x `class_weights` (entries as `problem_weights` takes:
    None, "balanced" or a pair (w0, w1) for labels 0 = negative and 1 = positive) on the folds of `plan_folds` -- the same
    folds for every setting.  Every (setting, distinct fold) problem goes into ONE `train_tasks` launch and one
    `decision_values` call on the resident matrix K; the AUC is scikit-learn's.  A problem that stops at the iteration
    cap is re-solved with scikit-learn (that problem alone) and counted.
    -> one record per setting, C outermost: dict(C, class_weight (as given), auc_mean, auc_std, capped).  The record of
    (C, None) holds exactly the two floats `crossValidate` returns for that C with the same ncv, repeats and seed."""
    from sklearn.metrics import roc_auc_score
    Cs, class_weights = list(Cs), list(class_weights)
    if not Cs or not class_weights:
        raise SvmError("the grid needs at least one C and one class weighting")
    plan = plan_folds((None, tol, shrinking, None, ncv, repeats, 0, seed), n_pseqs, n_nseqs)
    y, which, u_trains, u_tests = plan["y"], plan["which"], plan["u_trains"], plan["u_tests"]
    settings = [(C, cw) for C in Cs for cw in class_weights]
    nf = len(u_trains)
    trains = [u_trains[f] for _ in settings for f in range(nf)]
    tests = [u_tests[f] for _ in settings for f in range(nf)]
    labels = [y[t] for t in trains]
    C_of = [float(C) for C, _ in settings for _f in range(nf)]
    cw_of = [cw for _, cw in settings for _f in range(nf)]
    weights = problem_weights(labels, cw_of)
    logging.info("grid cross-validation on the GPU: %d settings x %d distinct folds in one launch", len(settings), nf)
    sol, handles = train_tasks(K, trains, labels, C_of, tol, bool(shrinking), None, cw_of)
    scores = decision_values(K, handles, tests)
    capped = [t for t in range(len(trains)) if sol.iters[t] < 0]
    if capped:
        from sklearn.svm import SVC
        logging.warning("%d problem(s) re-solved with scikit-learn (iteration cap of the GPU solver)", len(capped))
        for t in capped:
            tr, te = trains[t], tests[t]
            sv = SVC(kernel="precomputed", C=C_of[t], tol=tol, shrinking=bool(shrinking),
                     class_weight={0: float(weights[t, 0]), 1: float(weights[t, 1])})
            sv.fit(device_block(K, tr, tr).cpu().numpy(), y[tr])
            scores[t] = sv.decision_function(device_block(K, te, tr).cpu().numpy())
    records = []
    for s, (C, cw) in enumerate(settings):
        u_auc = [roc_auc_score(y[tests[s * nf + f]], scores[s * nf + f]) for f in range(nf)]
        aucs = [u_auc[w] for w in which]
        records.append(dict(C=C, class_weight=cw, auc_mean=np.mean(aucs), auc_std=np.std(aucs),
                            capped=sum(1 for t in capped if t // nf == s)))
    return records


def best_record(records):
    """Index of the best record of `cross_validate_grid`: the highest mean AUC; on a tie the smaller C, then the
    earlier entry (the earlier class weighting of one C)."""
    best = 0
    for r in range(1, len(records)):
        a, b = records[r], records[best]
        if a["auc_mean"] > b["auc_mean"] or (a["auc_mean"] == b["auc_mean"] and a["C"] < b["C"]):
            best = r
    return best
