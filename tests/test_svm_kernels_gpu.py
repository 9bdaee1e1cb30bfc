"""The SMO solvers (gkmqc_amd/csrc/gkm_svm.hip: k_smo in its LDS-table and its 1024x16 build, k_smo_general in its three
builds, k_diag) on kernel matrices whose DIAGONAL varies and which are not positive semi-definite -- tests/svm_cases.py;
every matrix of test_svm_gpu.py, test_svr_gpu.py and tools/fuzz_svm.py's first three kinds has one constant on its whole
diagonal and no negative eigenvalue by construction, so QD looked up by the wrong index, QD left behind by a swap of the
shrinking, and the strictly negative side of both `quad_coef` tests changed nothing there.

References: scikit-learn (support set, dual coefficients, intercept, decision values / predictions, n_iter_), bit for
bit; and tests/smo_ref.py, LIBSVM's solver without shrinking in numpy, for what scikit-learn does not return: alpha by
position, the final GRADIENT and rho.  tests/test_svm_kernels_host.py holds smo_ref to scikit-learn on every problem here
and asserts the conditions each case is there for.  No tolerance anywhere."""
import functools

import numpy as np
import pytest

from tests import svm_cases as S

pytestmark = pytest.mark.gpu

GEN_BUILDS = ({}, {"GKM_SVM_GEN_LDS": "0"}, {"GKM_SVM_GEN_T": "1024"})     # state in LDS, in global memory, 1 024 threads
KNOBS = ("GKM_SVM_SHAPE", "GKM_SVM_GEN_LDS", "GKM_SVM_GEN_T")


@functools.lru_cache(maxsize=8)
def _on_device(family, n, seed, scale):
    import torch
    return torch.tensor(S.matrix(family, n, seed, scale)).cuda()


def _device_matrix(c):
    return _on_device(c.family, c.n, c.seed, c.scale)


_FITTED = {}


def _fitted(*key):
    """scikit-learn's estimators of a case and setting, fitted by the first test that compares with them"""
    return _FITTED.setdefault(key, [])


def _set(monkeypatch, env):
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)


def _iters(m):
    return int(np.ravel(m.n_iter_)[0])


def _same(a, b):
    return np.asarray(a, dtype=np.float64).tobytes() == np.asarray(b, dtype=np.float64).tobytes()


def _assert_reference(sol, refs, what):
    """alpha, gradient, rho and iteration count of every fold against smo_ref's, bit for bit"""
    assert len(sol.alpha) == len(refs)
    for f, ref in enumerate(refs):
        assert int(sol.iters[f]) == ref.iters, (what, f, int(sol.iters[f]), ref.iters)
        assert _same(sol.alpha[f], ref.alpha), (what, f, np.abs(sol.alpha[f] - ref.alpha).max())
        assert _same(sol.grad[f], ref.grad), (what, f, np.abs(sol.grad[f] - ref.grad).max())
        assert _same(sol.rho[f], ref.rho), (what, f, sol.rho[f], ref.rho)


def _assert_same_solutions(a, b, what):
    assert list(a.iters) == list(b.iters), (what, list(a.iters), list(b.iters))
    for f in range(len(a.alpha)):
        assert _same(a.alpha[f], b.alpha[f]) and _same(a.grad[f], b.grad[f]) and _same(a.rho[f], b.rho[f]), (what, f)


# ------------------------------------------------------------------ C-SVC, k_smo
@pytest.mark.parametrize("shape", [None, "1024x16"], ids=["default", "1024x16"])
@pytest.mark.parametrize("case", S.SVC_CASES, ids=S.svc_case_id)
def test_k_smo(built, monkeypatch, case, shape):
    """The default launch shape (matrix index and diagonal in LDS, by position) and 1024x16 (TABM = 2: the diagonal
    re-read from global memory by matrix index wherever it is used): scikit-learn's support, dual coefficients, intercept,
    decision values and n_iter_; smo_ref's alpha and gradient."""
    from tests.test_svm_gpu import _compare_with_sklearn
    _set(monkeypatch, {"GKM_SVM_SHAPE": shape} if shape else {})
    trains, tests = S.svc_folds(case)
    fitted = _fitted("svc", case.name, False)
    sol = _compare_with_sklearn(S.svc_matrix(case), case.n // 2, trains, tests, case.C, case.tol, Kd=_device_matrix(case),
                                fitted=fitted)
    assert [int(i) for i in sol.iters] == [_iters(m) for m in fitted]
    _assert_reference(sol, S.svc_reference(case.name), case.name)


# ------------------------------------------------------------------ C-SVC, k_smo_general
@pytest.mark.parametrize("case", S.SVC_CASES, ids=S.svc_case_id)
def test_general_solver_without_shrinking(built, monkeypatch, case):
    """The three builds of k_smo_general (FAST_FOLD_SAMPLES lowered, as tests/test_svm_gpu.py does): QD[] by position, read
    ahead for the second selection and at i and j -- smo_ref's alpha, gradient, rho and iteration count from each."""
    from gkmqc_amd import svmcv
    monkeypatch.setattr(svmcv, "FAST_FOLD_SAMPLES", 10)
    trains, _ = S.svc_folds(case)
    refs = S.svc_reference(case.name)
    for env in GEN_BUILDS:
        _set(monkeypatch, env)
        sol, _ = svmcv.train_folds(_device_matrix(case), trains, S.labels(case.n), case.C, case.tol, False)
        _assert_reference(sol, refs, (case.name, env))


@pytest.mark.parametrize("case", S.SHRINK_CASES, ids=S.svc_case_id)
def test_general_solver_with_shrinking(built, monkeypatch, case):
    """Cases on which scikit-learn's shrinking run takes another number of iterations than its plain run on every fold
    (asserted in tests/test_svm_kernels_host.py), so the active set has been permuted -- QD with it (swap_index) --
    before the solution is reached: SVC(shrinking=True)'s outputs and n_iter_, and the three builds equal to one another."""
    from gkmqc_amd import svmcv
    from tests.test_svm_gpu import _compare_with_sklearn
    trains, tests = S.svc_folds(case)
    _set(monkeypatch, {})
    fitted = _fitted("svc", case.name, True)
    first = _compare_with_sklearn(S.svc_matrix(case), case.n // 2, trains, tests, case.C, case.tol, shrinking=True,
                                  Kd=_device_matrix(case), fitted=fitted)
    assert [int(i) for i in first.iters] == [_iters(m) for m in fitted]
    for env in GEN_BUILDS[1:]:
        _set(monkeypatch, env)
        sol, _ = svmcv.train_folds(_device_matrix(case), trains, S.labels(case.n), case.C, case.tol, True)
        _assert_same_solutions(first, sol, (case.name, env))


# ------------------------------------------------------------------ epsilon-SVR
def _svr_modes():
    out = []
    for c in S.SVR_CASES:
        out += [(c, "k_smo"), (c, "general")]
        if c.shrinking:
            out.append((c, "shrinking"))
    out.append((S.SVR_CASES[2], "1024x16"))
    return out


def _svr_setup(monkeypatch, mode):
    """-> shrinking"""
    from gkmqc_amd import svmcv
    _set(monkeypatch, {"GKM_SVM_SHAPE": "1024x16"} if mode == "1024x16" else {})
    if mode == "general":
        monkeypatch.setattr(svmcv, "FAST_FOLD_SAMPLES", 10)
    return mode == "shrinking"


@pytest.mark.parametrize("case,mode", _svr_modes(), ids=lambda x: x if isinstance(x, str) else x.name)
def test_svr(built, monkeypatch, case, mode):
    """LIBSVM's 2l-position problem on both solvers: the diagonal entry of sample k serves positions k and l + k.
    SVR(kernel="precomputed")'s support, dual coefficients, intercept, predictions and n_iter_."""
    from tests.test_svr_gpu import _compare_with_sklearn
    shrinking = _svr_setup(monkeypatch, mode)
    trains, tests = S.svr_folds(case)
    fitted = _fitted("svr", case.name, shrinking)
    sol = _compare_with_sklearn(S.matrix(case.family, case.n, case.seed), S.svr_targets(case.n), trains, tests, case.C,
                                case.epsilon, case.tol, shrinking, Kd=_on_device(case.family, case.n, case.seed, 1.0),
                                fitted=fitted)
    assert [int(i) for i in sol.iters] == [_iters(m) for m in fitted]


# ------------------------------------------------------------------ mixed fold sizes in one launch
MIXED_MODES = ["default", "1024x16", "general", "shrinking"]


@pytest.mark.parametrize("mode", MIXED_MODES)
def test_mixed_fold_sizes_svc(built, monkeypatch, mode):
    """Folds of 2 (one sample of each class: the smallest and the largest diagonal entry), 65 and 600 samples in ONE
    launch, whose shape the largest fold decides: every fold equals scikit-learn fitted on that fold alone."""
    from gkmqc_amd import svmcv
    from tests.test_svm_gpu import _compare_with_sklearn
    _set(monkeypatch, {"GKM_SVM_SHAPE": "1024x16"} if mode == "1024x16" else {})
    if mode == "general":
        monkeypatch.setattr(svmcv, "FAST_FOLD_SAMPLES", 0)
    K = S.matrix("vardiag", 600, S.SEED)
    trains = S.mixed_folds(600)
    tests = [np.arange(0, 600, 7), np.arange(3, 600, 11), np.array([1, 599])]
    C, tol = S.MIXED_SVC
    fitted = _fitted("mixed svc", mode == "shrinking")
    sol = _compare_with_sklearn(K, 300, trains, tests, C, tol, shrinking=mode == "shrinking",
                                Kd=_on_device("vardiag", 600, S.SEED, 1.0), fitted=fitted)
    assert [len(a) for a in sol.alpha] == [2, 65, 600]
    assert [int(i) for i in sol.iters] == [_iters(m) for m in fitted]


@pytest.mark.parametrize("mode", MIXED_MODES)
def test_mixed_fold_sizes_svr(built, monkeypatch, mode):
    from gkmqc_amd import svmcv
    from tests.test_svr_gpu import _compare_with_sklearn
    _set(monkeypatch, {"GKM_SVM_SHAPE": "1024x16"} if mode == "1024x16" else {})
    if mode == "general":
        monkeypatch.setattr(svmcv, "FAST_FOLD_SAMPLES", 0)
    K = S.matrix("vardiag", 600, S.SEED)
    trains = S.mixed_folds(600)
    tests = [np.arange(0, 600, 7), np.arange(3, 600, 11), np.array([1, 599])]
    C, eps, tol = S.MIXED_SVR
    fitted = _fitted("mixed svr", mode == "shrinking")
    sol = _compare_with_sklearn(K, S.svr_targets(600), trains, tests, C, eps, tol, mode == "shrinking",
                                Kd=_on_device("vardiag", 600, S.SEED, 1.0), fitted=fitted)
    assert [int(i) for i in sol.iters] == [_iters(m) for m in fitted]


# ------------------------------------------------------------------ padding
@pytest.mark.parametrize("shrinking", [False, True], ids=["k_smo", "general-shrinking"])
def test_padded_matrix_with_a_varied_diagonal(built, monkeypatch, shrinking):
    """K as a view with row stride n + 11 and NaN padding: k_diag reads K[i * ld + i] and the solvers K[g * ld + k], here on
    a matrix whose diagonal is not one constant (every diagonal entry of the older padded tests' matrices is 1)."""
    from tests.abi_cases import nan_padded
    from tests.test_svm_gpu import _compare_with_sklearn
    case = [c for c in S.SVC_CASES + S.SHRINK_CASES if c.name == ("vardiag-400-C10-whole" if shrinking else "vardiag-600-C1")][0]
    _set(monkeypatch, {})
    K = S.svc_matrix(case)
    trains, tests = S.svc_folds(case)
    Kd = nan_padded(np.array(K), case.n + 11)
    assert Kd.stride(0) == case.n + 11
    fitted = _fitted("svc", case.name, shrinking)
    sol = _compare_with_sklearn(K, case.n // 2, trains, tests, case.C, case.tol, shrinking, Kd=Kd, fitted=fitted)
    assert [int(i) for i in sol.iters] == [_iters(m) for m in fitted]
    if not shrinking:
        _assert_reference(sol, S.svc_reference(case.name), case.name)
