"""The boxed builds of the SMO solvers (gkmqc_amd/csrc/gkm_svm.hip: k_smo<..., BOX> in its LDS-table and its 1024x16
build, k_smo_general<..., BOX> in its three builds; include/gkm_svm.h gkmsvm_train_batch_boxed and
gkmsvm_train_batch_general_boxed): a bound per problem and per class wherever LIBSVM's solver reads C.

References: scikit-learn's SVC(class_weight=...) (support set, dual coefficients, intercept, decision values, n_iter_),
bit for bit; and tests/smo_box_ref.py for what scikit-learn does not return: alpha by position, the final gradient and
rho.  tests/test_svm_box_host.py holds smo_box_ref to scikit-learn on every problem here and asserts the conditions each
problem is there for.  No tolerance anywhere.  Every test asserts iters >= 0, so that the scikit-learn re-solve of a
capped problem can never stand in for the kernel."""
import functools

import numpy as np
import pytest

from tests import svm_box_cases as B
from tests import svm_cases as S

pytestmark = pytest.mark.gpu

GEN_BUILDS = ({}, {"GKM_SVM_GEN_LDS": "0"}, {"GKM_SVM_GEN_T": "1024"})
KNOBS = ("GKM_SVM_SHAPE", "GKM_SVM_GEN_LDS", "GKM_SVM_GEN_T")


@functools.lru_cache(maxsize=8)
def _on_device(family, n, seed, scale):
    import torch
    return torch.tensor(S.matrix(family, n, seed, scale)).cuda()


def _device_matrix(c):
    return _on_device(c.family, c.n, c.seed, c.scale)


def _set(monkeypatch, env):
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)


def _same(a, b):
    return np.asarray(a, dtype=np.float64).tobytes() == np.asarray(b, dtype=np.float64).tobytes()


def _tests_of(p):
    return np.arange(0, p.case.n, 7)


def _launch(problems, shrinking=False, decisions=True):
    """the problems (of ONE matrix and tolerance) in one boxed launch: a C per problem, a weighting per problem"""
    from gkmqc_amd import svmcv
    c = problems[0].case
    assert all(p.case is c and p.tol == problems[0].tol for p in problems)
    Kd = _device_matrix(c)
    sol, handles = svmcv.train_tasks(Kd, [p.train for p in problems], [B.labels_of(p) for p in problems],
                                     [p.C for p in problems], problems[0].tol, shrinking, None,
                                     [p.weights for p in problems])
    assert (np.asarray(sol.iters) >= 0).all(), list(sol.iters)
    scores = svmcv.decision_values(Kd, handles, [_tests_of(p) for p in problems]) if decisions else None
    return sol, scores


def _assert_sklearn(sol, scores, f, p, shrinking=False):
    """support set, dual coefficients, intercept, decision values and n_iter_ of scikit-learn's SVC on problem p"""
    m = B.sklearn_fit(p, shrinking)
    coef, support = sol.dual_coef(f)
    where = {g: k for k, g in enumerate(p.train)}
    assert int(sol.iters[f]) == B.iters_of(m), (p.name, int(sol.iters[f]), B.iters_of(m))
    assert np.array_equal(np.array([where[g] for g in support]), m.support_), p.name
    assert _same(coef, m.dual_coef_[0]), (p.name, np.abs(coef - m.dual_coef_[0]).max())
    assert _same(sol.rho[f], m.intercept_[0]), (p.name, sol.rho[f], m.intercept_[0])
    assert _same(sol.box[f], B.box_of(p)), (p.name, sol.box[f], B.box_of(p))
    if scores is not None:
        want = m.decision_function(S.svc_matrix(p.case)[np.ix_(_tests_of(p), p.train)])
        assert _same(scores[f], want), (p.name, np.abs(scores[f] - want).max())


def _assert_reference(sol, f, p):
    """alpha by position, final gradient, rho and iteration count of smo_box_ref"""
    ref = B.reference(p)
    assert int(sol.iters[f]) == ref.iters, (p.name, int(sol.iters[f]), ref.iters)
    assert _same(sol.alpha[f], ref.alpha), (p.name, np.abs(sol.alpha[f] - ref.alpha).max())
    assert _same(sol.grad[f], ref.grad), (p.name, np.abs(sol.grad[f] - ref.grad).max())
    assert _same(sol.rho[f], ref.rho), (p.name, sol.rho[f], ref.rho)


def _assert_same_solutions(a, b, what):
    assert list(a.iters) == list(b.iters), (what, list(a.iters), list(b.iters))
    for f in range(len(a.alpha)):
        assert _same(a.alpha[f], b.alpha[f]) and _same(a.grad[f], b.grad[f]) and _same(a.rho[f], b.rho[f]), (what, f)


# ------------------------------------------------------------------ 1. boxed k_smo
@pytest.mark.parametrize("shape", [None, "512x8", "1024x16"], ids=["default", "512x8", "1024x16"])
@pytest.mark.parametrize("p", B.KSMO_PROBLEMS, ids=B.problem_id)
def test_boxed_k_smo(built, monkeypatch, p, shape):
    """The default launch shape, 512x8 and 1024x16 (TABM = 2: alpha in LDS): vectors at both bounds with different bounds,
    "balanced" on 263 : 37, no free vector at all (rho from the per-class bounds), l = 2 and 3, one sample against 50."""
    _set(monkeypatch, {"GKM_SVM_SHAPE": shape} if shape else {})
    sol, scores = _launch([p])
    _assert_sklearn(sol, scores, 0, p)
    _assert_reference(sol, 0, p)


# ------------------------------------------------------------------ 2. boxed k_smo_general, no shrinking
@pytest.mark.parametrize("p", B.KSMO_PROBLEMS, ids=B.problem_id)
def test_boxed_general_solver_without_shrinking(built, monkeypatch, p):
    """The three builds of k_smo_general (FAST_FOLD_SAMPLES lowered): is_upper, the state byte, the update and rho with
    the bound of the position's label."""
    from gkmqc_amd import svmcv
    monkeypatch.setattr(svmcv, "FAST_FOLD_SAMPLES", 1)
    for env in GEN_BUILDS:
        _set(monkeypatch, env)
        sol, scores = _launch([p], decisions=not env)
        _assert_reference(sol, 0, p)
        if not env:
            _assert_sklearn(sol, scores, 0, p)


# ------------------------------------------------------------------ 3. boxed k_smo_general with shrinking
@pytest.mark.parametrize("weights", B.SHRINK_WEIGHTS, ids=lambda w: "%g:%g" % w)
@pytest.mark.parametrize("name", B.SHRINK_NAMES)
def test_boxed_general_solver_with_shrinking(built, monkeypatch, name, weights):
    """Problems on which scikit-learn's shrinking run takes another number of iterations than its plain run on every
    fold (asserted in tests/test_svm_box_host.py): be_shrunk, G_bar (C_i Q_i, C_j Q_j) and the gradient reconstruction with
    a bound per class -- SVC(shrinking=True, class_weight=...)'s outputs and n_iter_, the three builds equal."""
    problems = [p for p in B.SHRINK if p.case.name == name and p.weights == weights]
    assert problems
    _set(monkeypatch, {})
    first, scores = _launch(problems, shrinking=True)
    for f, p in enumerate(problems):
        _assert_sklearn(first, scores, f, p, shrinking=True)
    for env in GEN_BUILDS[1:]:
        _set(monkeypatch, env)
        sol, _ = _launch(problems, shrinking=True, decisions=False)
        _assert_same_solutions(first, sol, (name, weights, env))


# ------------------------------------------------------------------ 4. equal bounds are the unboxed entry's bits
@pytest.mark.parametrize("mode", ["k_smo", "1024x16", "general", "shrinking"])
@pytest.mark.parametrize("name", B.EQUAL_BOX_CASES)
def test_equal_bounds_are_the_unboxed_bits(built, monkeypatch, name, mode):
    from gkmqc_amd import svmcv
    c = B.case(name)
    _set(monkeypatch, {"GKM_SVM_SHAPE": "1024x16"} if mode == "1024x16" else {})
    if mode == "general":
        monkeypatch.setattr(svmcv, "FAST_FOLD_SAMPLES", 1)
    trains, _ = S.svc_folds(c)
    y = S.labels(c.n)
    Kd = _device_matrix(c)
    plain, _ = svmcv.train_folds(Kd, trains, y, c.C, c.tol, mode == "shrinking")
    boxed, _ = svmcv.train_folds(Kd, trains, y, [c.C] * len(trains), c.tol, mode == "shrinking")
    assert (np.asarray(plain.iters) > 0).all() and (np.asarray(boxed.iters) > 0).all()
    assert _same(boxed.box, np.full((len(trains), 2), c.C)) and _same(plain.box, boxed.box)
    _assert_same_solutions(plain, boxed, (name, mode))


def test_scalar_C_without_weights_calls_the_unboxed_entries(built, monkeypatch):
    """train_tasks with a scalar C and class_weight=None goes where it always went; anything else to the boxed entries"""
    from gkmqc_amd import svmcv
    c = B.case("vardiag-600-C1")
    trains, _ = S.svc_folds(c)
    y, Kd = S.labels(c.n), _device_matrix(c)
    lib = svmcv._lib()
    calls = []

    class Spy:
        def __init__(self, lib):
            self._lib = lib

        def __getattr__(self, name):
            f = getattr(self._lib, name)
            if not name.startswith("gkmsvm_train"):
                return f

            def wrapped(*a):
                calls.append(name)
                return f(*a)
            return wrapped

    monkeypatch.setattr(svmcv, "_lib", lambda: Spy(lib))
    _set(monkeypatch, {})
    svmcv.train_folds(Kd, trains[:1], y, c.C, c.tol)
    svmcv.train_folds(Kd, trains[:1], y, c.C, c.tol, True)
    svmcv.train_folds(Kd, trains[:1], y, c.C, c.tol, class_weight=(1.0, 2.0))
    svmcv.train_folds(Kd, trains[:1], y, [c.C], c.tol, True)
    assert calls == ["gkmsvm_train_batch", "gkmsvm_train_batch_general", "gkmsvm_train_batch_boxed",
                     "gkmsvm_train_batch_general_boxed"]


# ------------------------------------------------------------------ 5. one launch, many settings
@pytest.mark.parametrize("mode", ["k_smo", "general"])
def test_a_grid_of_settings_in_one_launch(built, monkeypatch, mode):
    """C in (0.01, 1, 100) x (no weights, (0.25, 4), "balanced" on the 263 : 37 problem) x folds: 21 problems of 400 and
    300 samples in ONE launch.  Every problem's solution is that of the problem launched alone, and scikit-learn's."""
    from gkmqc_amd import svmcv
    _set(monkeypatch, {})
    if mode == "general":
        monkeypatch.setattr(svmcv, "FAST_FOLD_SAMPLES", 1)
    assert sorted(set(len(p.train) for p in B.GRID)) == [300, 400]
    sol, scores = _launch(B.GRID)
    for f, p in enumerate(B.GRID):
        _assert_sklearn(sol, scores, f, p)
    for f in range(0, len(B.GRID), 1 if mode == "k_smo" else 3):      # (a launch each)
        p = B.GRID[f]
        alone, _ = _launch([p], decisions=False)
        assert int(alone.iters[0]) == int(sol.iters[f]), p.name
        assert _same(alone.alpha[0], sol.alpha[f]) and _same(alone.grad[0], sol.grad[f]) and _same(alone.rho[0], sol.rho[f]), p.name


# ------------------------------------------------------------------ 6. tiny and degenerate problems in one launch
@pytest.mark.parametrize("mode", ["k_smo", "1024x16", "general", "shrinking"])
def test_tiny_problems_beside_a_large_one(built, monkeypatch, mode):
    """l = 2, l = 3, one sample against 50, the no-free-vector problem and a fold of 400, one launch: the launch shape is
    the large fold's, most threads of the small problems own no sample."""
    from gkmqc_amd import svmcv
    _set(monkeypatch, {"GKM_SVM_SHAPE": "1024x16"} if mode == "1024x16" else {})
    if mode == "general":
        monkeypatch.setattr(svmcv, "FAST_FOLD_SAMPLES", 1)
    problems = B.TINY + [B.NO_FREE[0], B.TABLE[0]]
    sol, scores = _launch(problems, shrinking=mode == "shrinking")
    for f, p in enumerate(problems):
        _assert_sklearn(sol, scores, f, p, shrinking=mode == "shrinking")
        if mode != "shrinking":
            _assert_reference(sol, f, p)


# ------------------------------------------------------------------ 7. refusals
@pytest.mark.parametrize("entry", ["gkmsvm_train_batch_boxed", "gkmsvm_train_batch_general_boxed"])
@pytest.mark.parametrize("bad", [0.0, -1.0, float("nan"), float("inf"), float("-inf")], ids=str)
@pytest.mark.parametrize("where", [0, 3])
def test_bad_bounds_are_refused_and_nothing_is_written(built, entry, bad, where):
    import torch
    from gkmqc_amd import svmcv
    lib = svmcv._lib()
    c = B.case("vardiag-600-C1")
    Kd = _device_matrix(c)
    trains = [B.TINY[3].train, B.TINY[1].train]
    orders = svmcv.task_orders(trains, [S.labels(c.n)[t] for t in trains])
    idx = np.concatenate([o[0] for o in orders]).astype(np.int32)
    n0 = np.array([o[1] for o in orders], dtype=np.int32)
    off = np.array([0, len(trains[0]), len(idx)], dtype=np.int64)
    box = np.array([[1.0, 2.0], [0.5, 1.0]])
    box.ravel()[where] = bad
    d_idx = torch.from_numpy(idx).cuda()
    sentinel = -12345.0
    d_alpha = torch.full((len(idx),), sentinel, dtype=torch.float64, device="cuda")
    d_grad = torch.full((len(idx),), sentinel, dtype=torch.float64, device="cuda")
    d_rho = torch.full((2,), sentinel, dtype=torch.float64, device="cuda")
    d_it = torch.full((2,), -77, dtype=torch.int32, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream
    head = (0, Kd.data_ptr(), Kd.stride(0), Kd.shape[0], 2, d_idx.data_ptr(), off.ctypes.data, n0.ctypes.data,
            box.ctypes.data, 1e-3)
    outs = (d_alpha.data_ptr(), d_grad.data_ptr(), d_rho.data_ptr(), d_it.data_ptr(), stream)
    rc = getattr(lib, entry)(*head, *outs) if entry.endswith("batch_boxed") else getattr(lib, entry)(*head, 0, *outs)
    torch.cuda.synchronize()
    assert rc == 2, rc
    assert b"bound" in lib.gkmsvm_last_error()
    assert (d_alpha == sentinel).all() and (d_grad == sentinel).all() and (d_rho == sentinel).all() and (d_it == -77).all()
    # and the same call with good bounds solves both problems
    box[:] = [[1.0, 2.0], [0.5, 1.0]]
    rc = getattr(lib, entry)(*head, *outs) if entry.endswith("batch_boxed") else getattr(lib, entry)(*head, 0, *outs)
    torch.cuda.synchronize()
    assert rc == 0 and (d_it > 0).all() and not (d_alpha == sentinel).any() and not (d_rho == sentinel).any()


def test_python_refuses_bad_weights_before_any_launch(built):
    from gkmqc_amd import svmcv
    c = B.case("vardiag-600-C1")
    trains, _ = S.svc_folds(c)
    for kw in (dict(C=0.0, class_weight=(1.0, 1.0)), dict(C=[1.0, 2.0]), dict(C=1.0, class_weight=(1.0, float("nan"))),
               dict(C=1.0, class_weight=(0.0, 1.0)), dict(C=1.0, class_weight="balance")):
        with pytest.raises(svmcv.SvmError):
            svmcv.train_folds(_device_matrix(c), trains[:1], S.labels(c.n), tol=c.tol, **kw)
