"""Kernel matrices on which the SVM solvers' handling of the matrix DIAGONAL and of `quad_coef <= 0` matters, shared by
tests/test_svm_kernels_host.py (the reference against scikit-learn, and the conditions the cases are there for) and
tests/test_svm_kernels_gpu.py (the GPU solvers against both).  Every matrix the older SVM tests train on has one constant
on its whole diagonal and no negative eigenvalue by construction.

Families, as functions of (n, seed); X = default_rng(seed).normal(size=(n, 6)), the first half (label 1) shifted by 0.6;
every matrix is symmetrised with np.maximum(K, K.T):

  vardiag    rbf * s s^T, s = 10 ** uniform(-1, 1): positive definite, diagonal over four decades
  krein      (X * [1, 1, 1, 1, -1, -1]) @ X.T: indefinite, diagonal of both signs -- strictly negative quad_coef
  lowrank    X[:, :3] @ X[:, :3].T: rank 3, every clipping outcome
  poly       (1 + X @ X.T / 6) ** 2, not normalised
  negshift   rbf - 0.5: constant diagonal, indefinite

and of vardiag: a duplicated-sample variant (quad_coef == 0 exactly), one with near copies beside the copies (a quad_coef
between 0 and TAU competing with the zero), and two rescalings (K * 1e-3 with C = 100, K * 1e4 with C = 1e-3).
"""
import functools
from collections import namedtuple

import numpy as np

DIM = 6
FAMILIES = ("vardiag", "krein", "lowrank", "poly", "negshift")
NDUP = 40


def _points(n, seed):
    rng = np.random.default_rng(seed)
    X = rng.normal(size=(n, DIM))
    X[: n // 2] += 0.6
    return X, rng


def _rbf(X):
    d2 = ((X[:, None, :] - X[None, :, :]) ** 2).sum(-1)
    return np.exp(-d2 / (2.0 * DIM))


def _scales(n, rng):
    return 10.0 ** rng.uniform(-1, 1, n)


def vardiag(n, seed):
    X, rng = _points(n, seed)
    s = _scales(n, rng)
    K = _rbf(X) * s[:, None] * s[None, :]
    return np.maximum(K, K.T)


def vardiag_dup(n, seed):
    """vardiag with the rows and columns of its first NDUP samples copied over its last NDUP (the other class): exact ties
    in both selections and quad_coef == 0 between a sample and its copy, beside unequal diagonals everywhere else.  The
    scales of the copied samples are rounded to 10 bits, so that their diagonal entries s^2 are exact in float: QD (double)
    and 2 Q_ij (Qfloat) then cancel to exactly zero, not to a rounding error of either sign."""
    X, rng = _points(n, seed)
    s = _scales(n, rng)
    m, e = np.frexp(s[:NDUP])
    s[:NDUP] = np.ldexp(np.round(m * 1024) / 1024, e)
    K = _rbf(X) * s[:, None] * s[None, :]
    K = np.maximum(K, K.T)
    src, dst = np.arange(NDUP), np.arange(n - NDUP, n)
    K[dst, :] = K[src, :]
    K[:, dst] = K[:, src]
    assert (K == K.T).all()
    return K


def vardiag_neardup(n, seed):
    """vardiag_dup with a second copy of the same NDUP samples, in their own class, whose DIAGONAL entry is larger by
    2^-50 of itself.  A sample of the other class that is a copy too then meets two candidates in the second selection,
    with equal gradients: the exact copy, quad_coef == 0, and the near copy, 0 < quad_coef < TAU.  LIBSVM divides by TAU
    for the first and by quad_coef itself for the second, so the near copy wins; dividing by the zero (-inf) or testing
    `quad_coef > TAU` would pick the other."""
    K = vardiag_dup(n, seed)
    src, near = np.arange(NDUP), np.arange(NDUP, 2 * NDUP)
    K[near, :] = K[src, :]
    K[:, near] = K[:, src]
    K[near, near] *= 1.0 + 2.0 ** -50
    assert (K == K.T).all()
    return K


def krein(n, seed):
    X, _ = _points(n, seed)
    K = (X * np.array([1.0, 1, 1, 1, -1, -1])) @ X.T
    return np.maximum(K, K.T)


def lowrank(n, seed):
    X, _ = _points(n, seed)
    K = X[:, :3] @ X[:, :3].T
    return np.maximum(K, K.T)


def poly(n, seed):
    X, _ = _points(n, seed)
    K = (1 + X @ X.T / DIM) ** 2
    return np.maximum(K, K.T)


def negshift(n, seed):
    X, _ = _points(n, seed)
    K = _rbf(X) - 0.5
    return np.maximum(K, K.T)


_MAKERS = dict(vardiag=vardiag, vardiag_dup=vardiag_dup, vardiag_neardup=vardiag_neardup, krein=krein, lowrank=lowrank, poly=poly, negshift=negshift)


@functools.lru_cache(maxsize=None)
def matrix(family, n, seed, scale=1.0):
    """the (read-only) matrix of a family, times `scale`"""
    K = _MAKERS[family](n, seed) * scale
    K.setflags(write=False)
    return K


def labels(n):
    return np.concatenate((np.repeat(1, n // 2), np.repeat(0, n - n // 2)))


def svr_targets(n):
    """two levels a unit apart plus unit noise"""
    return np.random.default_rng(3).normal(size=n) + np.concatenate((np.ones(n // 2), np.zeros(n - n // 2)))


# ------------------------------------------------------------------ the committed cases
# C-SVC.  vardiag: the ratio max / min |.| of the diagonal is asserted >= 100 among the training samples of every fold.
# whole: train on all samples instead of three stratified folds.
SvcCase = namedtuple("SvcCase", "name family n seed scale C tol vardiag whole")

SEED = 7
_SETTINGS = [(600, 1.0, 1e-3), (600, 0.05, 1e-3), (400, 10.0, 1e-4)]


def _svc_cases():
    out = []
    for fam in FAMILIES:
        for n, C, tol in _SETTINGS:
            out.append(SvcCase("%s-%d-C%g" % (fam, n, C), fam, n, SEED, 1.0, C, tol, fam == "vardiag", False))
    out.append(SvcCase("vardiag_dup-600-C1", "vardiag_dup", 600, SEED, 1.0, 1.0, 1e-3, True, False))
    out.append(SvcCase("vardiag_neardup-600-C1", "vardiag_neardup", 600, SEED, 1.0, 1.0, 1e-3, True, False))
    out.append(SvcCase("vardiag_x1e-3-600-C100", "vardiag", 600, SEED, 1e-3, 100.0, 1e-3, True, False))
    out.append(SvcCase("vardiag_x1e4-600-C1e-3", "vardiag", 600, SEED, 1e4, 1e-3, 1e-3, True, False))
    return out


SVC_CASES = _svc_cases()

# "Path differs": with LIBSVM's shrinking scikit-learn takes another number of iterations than without it on EVERY fold
# of these, so a solver that matches SVC(shrinking=True) there has followed the shrinking path itself (asserted in
# tests/test_svm_kernels_host.py).  krein converges before the first round of shrinking at every setting and is not
# here.  Of the three stratified folds of vardiag and negshift only one each differs: those two train on all samples.
SHRINK_CASES = [
    SvcCase("lowrank-400-C10", "lowrank", 400, SEED, 1.0, 10.0, 1e-4, False, False),
    SvcCase("poly-400-C10", "poly", 400, SEED, 1.0, 10.0, 1e-4, False, False),
    SvcCase("vardiag-400-C10-whole", "vardiag", 400, SEED, 1.0, 10.0, 1e-4, True, True),
    SvcCase("negshift-400-C10-whole", "negshift", 400, SEED, 1.0, 10.0, 1e-4, False, True),
]


def svc_case_id(c):
    return c.name


def svc_matrix(c):
    return matrix(c.family, c.n, c.seed, c.scale)


def svc_folds(c):
    """(trains, tests): three stratified folds as tests/test_svm_gpu.py's _folds makes them, or all samples"""
    if c.whole:
        return [np.arange(c.n)], [np.arange(0, c.n, 7)]
    from tests.test_svm_gpu import _folds
    return _folds(c.n, c.n // 2, 3, seed=1)


# epsilon-SVR, n = 300, three KFold problems as tests/test_svr_gpu.py's _folds makes them
SvrCase = namedtuple("SvrCase", "name family n seed C epsilon tol shrinking whole")

SVR_SEED = 9
SVR_CASES = [
    SvrCase("vardiag", "vardiag", 300, SVR_SEED, 10.0, 0.05, 1e-4, False, False),
    SvrCase("lowrank", "lowrank", 300, SVR_SEED, 10.0, 0.05, 1e-4, True, False),
    SvrCase("krein", "krein", 300, SVR_SEED, 10.0, 0.05, 1e-4, False, False),
    SvrCase("vardiag-eps0", "vardiag", 300, SVR_SEED, 1.0, 0.0, 1e-3, False, False),
]


def svr_folds(c):
    if c.whole:
        return [np.arange(c.n)], [np.arange(0, c.n, 7)]
    from tests.test_svr_gpu import _folds
    return _folds(c.n, 3, seed=1)


# mixed fold sizes in one launch: 2 (one sample of each class), 65 and all 600 samples of vardiag
MIXED_SVC = (1.0, 1e-3)             # C, tol
MIXED_SVR = (1.0, 0.1, 1e-3)        # C, epsilon, tol


def mixed_folds(n=600):
    rng = np.random.default_rng(11)
    mid = np.sort(np.concatenate((rng.choice(n // 2, 30, replace=False), n // 2 + rng.choice(n - n // 2, 35, replace=False))))
    assert n == 600      # samples 246 and 457: the smallest and the largest diagonal entry, one of each class
    return [np.array([246, 457]), mid, np.arange(n)]


# ------------------------------------------------------------------ the reference's solutions, computed once per process
@functools.lru_cache(maxsize=None)
def svc_reference(name):
    """smo_ref's solution of every fold of a C-SVC case (tuple of Solution), in svmcv.libsvm_order's order"""
    from gkmqc_amd import svmcv
    from tests import smo_ref
    c = [x for x in SVC_CASES + SHRINK_CASES if x.name == name][0]
    K, y = svc_matrix(c), labels(c.n)
    trains, _ = svc_folds(c)
    out = []
    for tr in trains:
        idx, n0 = svmcv.libsvm_order(tr, y)
        out.append(smo_ref.svc(K, idx, n0, c.C, c.tol))
    return tuple(out)


@functools.lru_cache(maxsize=None)
def svr_reference(name):
    from tests import smo_ref
    c = [x for x in SVR_CASES if x.name == name][0]
    K, z = matrix(c.family, c.n, c.seed), svr_targets(c.n)
    trains, _ = svr_folds(c)
    return tuple(smo_ref.svr(K, tr, z, c.C, c.epsilon, c.tol) for tr in trains)
