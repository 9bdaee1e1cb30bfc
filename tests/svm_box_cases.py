"""The problems of the class-weight tests, shared by tests/test_svm_box_host.py (smo_box_ref against
scikit-learn, and the conditions each problem is there for) and tests/test_svm_box_gpu.py (the boxed GPU solvers against
both).  All of them are sub-problems of tests/svm_cases.py's matrices with its labels: samples 0 .. n/2-1 carry label 1,
the rest label 0, so class 0 -- LIBSVM's y = +1, the first positions of a problem -- is the SECOND half of a matrix.
`weights` is what `class_weight` takes: a pair (weight of label 0, weight of label 1), "balanced" or None.
"""
import functools
from collections import namedtuple

import numpy as np

from tests import svm_cases as S

Problem = namedtuple("Problem", "name case fold train weights C tol")


def case(name):
    return [c for c in S.SVC_CASES + S.SHRINK_CASES if c.name == name][0]


def _fold_problem(case_name, fold, weights, C=None):
    c = case(case_name)
    train = S.svc_folds(c)[0][fold]
    wname = weights if isinstance(weights, str) or weights is None else "%g:%g" % weights
    return Problem("%s/f%d/%s/C%g" % (case_name, fold, wname, c.C if C is None else C), c, fold, train, weights,
                   c.C if C is None else C, c.tol)


def unbalanced(n0, n1, n=600):
    """the first n0 samples of class 0 (label 0: the second half) and the first n1 of class 1, ascending"""
    return np.concatenate((np.arange(n1), n // 2 + np.arange(n0)))


# support vectors at both bounds, and the two bounds differ (counts: tests/test_svm_box_host.py)
TABLE = [
    _fold_problem("vardiag-600-C1", 0, (0.25, 4.0)),
    _fold_problem("vardiag-600-C1", 0, (4.0, 0.25)),
    _fold_problem("vardiag-600-C1", 0, (1e-3, 1e3)),
    _fold_problem("krein-600-C1", 0, (0.25, 4.0)),
    _fold_problem("vardiag-400-C10", 0, (0.25, 4.0)),
]
TABLE_COUNTS = [(188, 4, 48), (2, 182, 50), (200, 0, 30), (191, 11, 3), (105, 0, 74)]   # at class 0's bound, class 1's, free

# "balanced" on 263 : 37 -- on svm_cases' own folds it resolves to (1, 1)
BALANCED = [Problem("vardiag-600-C1/263:37/balanced/C%g" % C, case("vardiag-600-C1"), None, unbalanced(263, 37), "balanced",
                    C, 1e-3) for C in (0.01, 1.0, 100.0)]

# no free vector: rho is the midpoint (ub + lb) / 2 of bounds taken per class
NO_FREE = [Problem("%s/200:100/1:2/C0.001" % name, case(name), None, unbalanced(200, 100), (1.0, 2.0), 1e-3, 1e-3)
           for name in ("vardiag-600-C1", "krein-600-C1", "negshift-600-C1")]

# tiny and degenerate: one sample per class (the smallest and the largest diagonal entry), l = 3, one against 50
TINY = [
    Problem("vardiag-600-C1/l2", case("vardiag-600-C1"), None, np.array([246, 457]), (0.25, 4.0), 1.0, 1e-3),
    Problem("vardiag-600-C1/l3", case("vardiag-600-C1"), None, np.array([246, 457, 458]), (0.25, 4.0), 1.0, 1e-3),
    Problem("vardiag-600-C1/l3b", case("vardiag-600-C1"), None, np.array([245, 246, 457]), (4.0, 0.25), 1.0, 1e-3),
    Problem("vardiag-600-C1/1:50", case("vardiag-600-C1"), None, np.concatenate(([5], 300 + np.arange(50))), (0.25, 4.0),
            1.0, 1e-3),
    Problem("vardiag-600-C1/50:1/balanced", case("vardiag-600-C1"), None, np.concatenate((np.arange(50), [457])),
            "balanced", 1.0, 1e-3),
]

KSMO_PROBLEMS = TABLE + BALANCED + NO_FREE + TINY

# shrinking changes n_iter_ on every fold under both weightings
SHRINK_NAMES = ("poly-400-C10", "vardiag-400-C10", "vardiag-400-C10-whole", "negshift-400-C10-whole")
SHRINK_WEIGHTS = ((0.25, 4.0), (4.0, 0.25))
SHRINK = [_fold_problem(name, f, w) for name in SHRINK_NAMES for w in SHRINK_WEIGHTS
          for f in range(len(S.svc_folds(case(name))[0]))]

# one launch, many settings: C x (None, a pair, "balanced" on 263 : 37) x 3 folds; folds of 400 and the problem of 300
GRID_CS = (0.01, 1.0, 100.0)
GRID = ([_fold_problem("vardiag-600-C1", f, w, C) for C in GRID_CS for w in (None, (0.25, 4.0)) for f in range(3)]
        + [p for p in BALANCED])

EQUAL_BOX_CASES = ("vardiag-600-C1", "krein-600-C0.05", "poly-400-C10")


def problem_id(p):
    return p.name


def labels_of(p):
    return S.labels(p.case.n)[p.train]


def sk_class_weight(weights):
    return weights if weights is None or isinstance(weights, str) else {0: weights[0], 1: weights[1]}


@functools.lru_cache(maxsize=None)
def _fit(name, shrinking):
    from sklearn.svm import SVC
    p = [q for q in KSMO_PROBLEMS + SHRINK + GRID if q.name == name][0]
    K, y = S.svc_matrix(p.case), S.labels(p.case.n)
    m = SVC(kernel="precomputed", C=p.C, tol=p.tol, shrinking=shrinking, cache_size=512,
            class_weight=sk_class_weight(p.weights))
    return m.fit(K[np.ix_(p.train, p.train)], y[p.train])


def sklearn_fit(p, shrinking=False):
    """scikit-learn's SVC of the problem, fitted once per process"""
    return _fit(p.name, bool(shrinking))


def box_of(p):
    """(bound of class 0, bound of class 1) as LIBSVM has them: scikit-learn's class_weight_ times C"""
    w = sklearn_fit(p).class_weight_
    return (float(w[0] * p.C), float(w[1] * p.C))


@functools.lru_cache(maxsize=None)
def _ref(name):
    from gkmqc_amd import svmcv
    from tests import smo_box_ref
    p = [q for q in KSMO_PROBLEMS + SHRINK + GRID if q.name == name][0]
    idx, n0 = svmcv.libsvm_order(p.train, S.labels(p.case.n))
    return smo_box_ref.svc(S.svc_matrix(p.case), idx, n0, box_of(p), p.tol)


def reference(p):
    """smo_box_ref's Solution of the problem (positions in svmcv.libsvm_order's order), computed once per process"""
    return _ref(p.name)


def iters_of(m):
    return int(np.ravel(m.n_iter_)[0])
