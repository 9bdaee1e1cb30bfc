"""epsilon-SVR on the GPU (gkm_svm.hip gkmsvm_train_svr_batch[_general], gkmsvm_decision_signed_batch;
gkmqc_amd/svmcv.py train_svr_folds / svr_predict; gkmqc_amd/gkmpredict.py train_svr): LIBSVM's solve_epsilon_svr on the
GPU solvers against scikit-learn's SVR(kernel="precomputed") -- support set, dual coefficients, intercept and
predictions bit for bit -- and the downstream consumers of a model on an SVR model."""
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import helpers

pytestmark = pytest.mark.gpu

POS = os.path.join(helpers.GOLDEN, "motif_pos.fa")
NEG = os.path.join(helpers.GOLDEN, "motif_neg.fa")


def _rbf_matrix(n, dim, seed, dup=0):
    """A positive-definite test kernel; `dup` duplicated points force exact ties in the working-set selection."""
    rng = np.random.default_rng(seed)
    X = rng.normal(size=(n, dim))
    if dup:
        X[n - dup:] = X[:dup]
    d2 = ((X[:, None, :] - X[None, :, :]) ** 2).sum(-1)
    K = np.exp(-d2 / (2.0 * dim))
    return np.maximum(K, K.T), X


def _targets(X, seed, dup=0):
    """continuous targets: a smooth function of the points plus noise (duplicated points keep their own noise)"""
    rng = np.random.default_rng(seed + 1)
    return np.sin(X[:, 0]) + 0.5 * X[:, 1] + 0.3 * rng.normal(size=len(X))


def _folds(n, ncv, seed):
    from sklearn.model_selection import KFold
    trains, tests = zip(*KFold(n_splits=ncv, shuffle=True, random_state=seed).split(np.zeros(n)))
    return list(trains), list(tests)


def _compare_with_sklearn(K, z, trains, tests, C, eps, tol, shrinking=False, capped=False, Kd=None, fitted=None):
    """Kd: the device matrix handed to the solvers (default: a contiguous copy of K); fitted: a list that receives
    scikit-learn's SVR of every problem -- or holds them already, from an earlier call with the same problems and
    settings, and then spares the fits"""
    import torch
    from sklearn.svm import SVR
    from gkmqc_amd import svmcv
    if Kd is None:
        Kd = torch.from_numpy(K).cuda()
    sol = svmcv.train_svr_folds(Kd, trains, z, C, eps, tol, shrinking)
    pred = svmcv.svr_predict(Kd, sol, tests)
    for f, (train, test) in enumerate(zip(trains, tests)):
        if fitted is not None and len(fitted) > f:
            m = fitted[f]
        else:
            m = SVR(kernel="precomputed", C=C, epsilon=eps, tol=tol, shrinking=shrinking, cache_size=512)
            m.fit(K[train][:, train], z[train])
            if fitted is not None:
                fitted.append(m)
        assert (sol.iters[f] < 0) if capped else (sol.iters[f] >= 0), sol.iters[f]   # (0: every target within epsilon)
        assert np.array_equal(sol.support[f], m.support_), "problem %d: support set differs" % f
        assert sol.dual_coef[f].tobytes() == m.dual_coef_[0].tobytes(), "problem %d: max |diff| %g" % (
            f, np.abs(sol.dual_coef[f] - m.dual_coef_[0]).max())
        assert np.float64(sol.intercept[f]).tobytes() == np.float64(m.intercept_[0]).tobytes()
        want = m.predict(K[test][:, train])
        assert pred[f].tobytes() == want.tobytes(), "problem %d: predictions differ by %g" % (
            f, np.abs(pred[f] - want).max() if len(want) else 0)
    return sol


@pytest.mark.parametrize("shrinking", [False, True])
@pytest.mark.parametrize("n,dim,C,eps,tol,dup", [
    (200, 6, 1.0, 0.1, 1e-3, 0),
    (600, 10, 0.05, 0.1, 1e-3, 0),     # most coefficients at the bound
    (400, 4, 100.0, 0.01, 1e-4, 0),    # few bounded, many iterations
    (300, 5, 1.0, 0.2, 1e-3, 40),      # duplicated samples: exact ties
    (2600, 12, 1.0, 0.05, 1e-3, 0),    # 2l beyond 1 000 (shrinking every 1 000 iterations), several per thread
    (120, 3, 1.0, 0.0, 1e-3, 0),       # epsilon = 0: p_k = -z_k and +z_k
])
def test_solver_is_bit_identical_to_sklearn(built, n, dim, C, eps, tol, dup, shrinking):
    """Three problems per launch (k_smo without shrinking, k_smo_general with it)."""
    K, X = _rbf_matrix(n, dim, seed=n + dim, dup=dup)
    z = _targets(X, n)
    trains, tests = _folds(n, 3, seed=1)
    _compare_with_sklearn(K, z, trains, tests, C, eps, tol, shrinking)


@pytest.mark.parametrize("n,dim,general,shrinking", [
    (600, 10, False, False),       # k_smo
    (700, 8, True, False),         # the general solver, shrinking off (FAST_FOLD_SAMPLES lowered)
    (600, 10, False, True),        # the general solver with shrinking
    (2600, 12, False, False),      # several samples per thread
])
def test_padded_kernel_matrix(built, monkeypatch, n, dim, general, shrinking):
    """K as a view of a wider matrix (row stride n + 11) whose padding is NaN: the SVR setup, the solvers and the
    prediction kernel must index rows by the stride svmcv passes through.  One read of the padding is a NaN and ends
    the bit-identity with scikit-learn."""
    from tests.abi_cases import nan_padded
    if general:
        from gkmqc_amd import svmcv
        monkeypatch.setattr(svmcv, "FAST_FOLD_SAMPLES", 10)
    K, X = _rbf_matrix(n, dim, seed=n + dim)
    z = _targets(X, n)
    trains, tests = _folds(n, 3, seed=1)
    Kd = nan_padded(K, n + 11)
    assert Kd.stride(0) == n + 11
    _compare_with_sklearn(K, z, trains, tests, 1.0, 0.1, 1e-3, shrinking, Kd=Kd)


@pytest.mark.parametrize("shrinking", [False, True])
def test_tiny_problems(built, shrinking):
    """l = 1, 2 and 3 (2, 4 and 6 solver positions) in one launch, and a problem whose rows are one point twice."""
    K, X = _rbf_matrix(40, 3, seed=2, dup=4)
    z = _targets(X, 2)
    trains = [np.array([5]), np.array([3, 17]), np.array([0, 36, 8])]
    tests = [np.array([1, 2, 3]), np.array([4]), np.arange(40)]
    _compare_with_sklearn(K, z, trains, tests, 1.0, 0.1, 1e-3, shrinking)


def test_general_solver_without_shrinking(built, monkeypatch):
    """The general solver with shrinking off (the path of problems beyond k_smo's 16 384 positions) forced on small
    problems."""
    from gkmqc_amd import svmcv
    monkeypatch.setattr(svmcv, "FAST_FOLD_SAMPLES", 10)
    K, X = _rbf_matrix(700, 8, seed=11, dup=10)
    z = _targets(X, 11)
    trains, tests = _folds(700, 2, seed=2)
    _compare_with_sklearn(K, z, trains, tests, 1.0, 0.1, 1e-3)
    _compare_with_sklearn(K, z, [np.array([3]), np.array([0, 699])], [np.array([1]), np.array([2, 3])], 1.0, 0.1, 1e-3)


@pytest.mark.parametrize("shape", ["256x4", "512x4", "256x8", "512x8", "1024x4", "1024x8", "1024x10", "1024x12",
                                   "512x16", "1024x16"])
def test_every_launch_shape(built, monkeypatch, shape):
    monkeypatch.setenv("GKM_SVM_SHAPE", shape)
    K, X = _rbf_matrix(750, 8, seed=12, dup=10)
    z = _targets(X, 12)
    trains, tests = _folds(750, 3, seed=3)        # 500 samples = 1 000 positions: every shape holds them
    _compare_with_sklearn(K, z, trains, tests, 1.0, 0.1, 1e-3)


@pytest.mark.parametrize("env", [{"GKM_SVM_GEN_LDS": "0"}, {"GKM_SVM_GEN_T": "1024"}])
@pytest.mark.parametrize("shrinking", [False, True])
def test_general_solver_variants(built, monkeypatch, env, shrinking):
    """The general solver with its state in global memory and with 1 024 threads."""
    from gkmqc_amd import svmcv
    monkeypatch.setattr(svmcv, "FAST_FOLD_SAMPLES", 0)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    K, X = _rbf_matrix(900, 3, seed=21, dup=30)
    z = _targets(X, 21)
    trains, tests = _folds(900, 2, seed=4)
    _compare_with_sklearn(K, z, trains, tests, 10.0, 0.05, 1e-4, shrinking)


def test_iteration_cap_falls_back_to_sklearn(built, monkeypatch):
    monkeypatch.setenv("GKM_SVM_MAX_ITER", "7")
    K, X = _rbf_matrix(300, 5, seed=7)
    z = _targets(X, 7)
    trains, tests = _folds(300, 3, seed=5)
    _compare_with_sklearn(K, z, trains, tests, 1.0, 0.1, 1e-3, capped=True)
    _compare_with_sklearn(K, z, trains, tests, 1.0, 0.1, 1e-3, shrinking=True, capped=True)


def test_large_problems_both_solvers_agree(built, monkeypatch):
    """8 192 samples = 16 384 positions, k_smo's largest (1024 x 16, alpha in LDS), against the general solver: same
    support, coefficients, intercept and iteration count, bit for bit; and 12 000 samples (24 000 positions, the general
    solver only) converge.  scikit-learn would take minutes here; both solvers are pinned to it above."""
    import torch
    from gkmqc_amd import svmcv
    n, dim = 12000, 6
    g = torch.Generator(device="cpu").manual_seed(8)
    X = torch.randn(n, dim, generator=g, dtype=torch.float64)
    z = (torch.sin(X[:, 0]) + 0.5 * X[:, 1] + 0.3 * torch.randn(n, generator=g, dtype=torch.float64)).numpy()
    X = X.cuda()
    sq = (X * X).sum(1)
    K = torch.exp(-(sq[:, None] + sq[None, :] - 2.0 * X @ X.T).clamp_min(0) / (2.0 * dim))
    K = torch.maximum(K, K.T).contiguous()
    idx = np.random.default_rng(3).permutation(n)
    train = np.sort(idx[:8192])
    a = svmcv.train_svr_folds(K, [train], z, 1.0, 0.1, 1e-3)
    monkeypatch.setattr(svmcv, "FAST_FOLD_SAMPLES", 0)
    b = svmcv.train_svr_folds(K, [train], z, 1.0, 0.1, 1e-3)
    assert a.iters[0] > 0 and a.iters[0] == b.iters[0]
    assert np.array_equal(a.support[0], b.support[0]) and a.dual_coef[0].tobytes() == b.dual_coef[0].tobytes()
    assert a.intercept[0] == b.intercept[0]
    test = np.sort(idx[8192:])
    pa, pb = svmcv.svr_predict(K, a, [test])[0], svmcv.svr_predict(K, b, [test])[0]
    assert pa.tobytes() == pb.tobytes()
    assert np.corrcoef(pa, z[test])[0, 1] > 0.5                   # (it learnt something)
    monkeypatch.setattr(svmcv, "FAST_FOLD_SAMPLES", 16384)
    c = svmcv.train_svr_folds(K, [np.arange(n)], z, 1.0, 0.1, 1e-3)
    assert c.iters[0] > 0
    assert np.abs(c.dual_coef[0]).max() <= 1.0 and abs(c.dual_coef[0].sum()) < 1e-9   # box and sum(alpha - alpha*) = 0


def test_signed_decision_edges(built):
    """gkmsvm_decision_signed_batch called directly: zeros skipped, signs kept, the sum sequential in support-vector order
    from +0.0, then minus rho -- equal bit for bit to that loop."""
    import torch
    from gkmqc_amd import svmcv
    lib = svmcv._lib()
    rng = np.random.default_rng(4)
    n = 500
    X = rng.uniform(-1, 1, (n, n)) * 10.0 ** rng.integers(-6, 7, (n, n))
    K = np.triu(X) + np.triu(X, 1).T
    Kd = torch.from_numpy(K).cuda()
    probs = []
    for l in (1, 16, 17, 300):
        idx = rng.choice(n, l, replace=False).astype(np.int32)
        coef = rng.uniform(-1, 1, l) * 10.0 ** rng.integers(-4, 3, l)
        coef[rng.random(l) < 0.25] = 0.0
        test = rng.choice(n, int(rng.integers(1, 200)), replace=False).astype(np.int32)
        probs.append((idx, coef, float(rng.normal()), test))
    off = np.zeros(len(probs) + 1, dtype=np.int64)
    off[1:] = np.cumsum([len(p[0]) for p in probs])
    toff = np.zeros(len(probs) + 1, dtype=np.int64)
    toff[1:] = np.cumsum([len(p[3]) for p in probs])
    d_idx = torch.from_numpy(np.concatenate([p[0] for p in probs])).cuda()
    d_coef = torch.from_numpy(np.concatenate([p[1] for p in probs])).cuda()
    d_rho = torch.tensor([p[2] for p in probs], dtype=torch.float64).cuda()
    d_test = torch.from_numpy(np.concatenate([p[3] for p in probs])).cuda()
    d_dec = torch.full((int(toff[-1]),), 123.5, dtype=torch.float64).cuda()
    rc = lib.gkmsvm_decision_signed_batch(0, Kd.data_ptr(), n, len(probs), d_idx.data_ptr(), off.ctypes.data,
                                          d_coef.data_ptr(), d_rho.data_ptr(), d_test.data_ptr(), toff.ctypes.data,
                                          d_dec.data_ptr(), torch.cuda.current_stream().cuda_stream)
    assert rc == 0, lib.gkmsvm_last_error().decode()
    dec = d_dec.cpu().numpy()
    for p, (idx, coef, rho, test) in enumerate(probs):
        s = np.zeros(len(test))
        for k in range(len(idx)):
            if coef[k] != 0:
                s = s + coef[k] * K[idx[k], test]
        assert dec[toff[p]:toff[p + 1]].tobytes() == (s - rho).tobytes(), p


# ------------------------------------------------------------------ gkm end to end
@pytest.fixture(scope="module")
def dv(built):
    from gkmqc_amd import device
    return device


@pytest.fixture(scope="module")
def files(tmp_path_factory, built):
    """pos + neg in one file with seeded targets (class, GC content and the count of one 4-mer, plus noise) and a ragged
    synthetic query set"""
    from gkmqc_amd import device, synth
    tmp = tmp_path_factory.mktemp("svr")
    train_fa, query_fa, targets = str(tmp / "train.fa"), str(tmp / "q.fa"), str(tmp / "targets.txt")
    with open(train_fa, "w") as f:
        f.write(open(POS).read().rstrip("\n") + "\n" + open(NEG).read())
    synth.write_fasta(query_fa, synth.make_sequences(21, 45, 300, (30, 700)), "q")
    seqs, names, _, _ = device.read_fasta(train_fa)
    npos = len(device.read_fasta(POS)[1])
    rng = np.random.default_rng(17)
    z = []
    for i in range(len(seqs)):
        s = np.asarray(seqs[i])
        text = "".join("ACGT"[b] for b in s)
        z.append((1.0 if i < npos else 0.0) + 2.0 * np.mean((s == 1) | (s == 2)) + 0.2 * text.count("GATA")
                 + 0.1 * rng.normal())
    with open(targets, "w") as f:
        f.write("".join("%s\t%r\n" % (nm, float(v)) for nm, v in zip(names, z)))
    return dict(train=train_fa, query=query_fa, targets=targets, z=np.array(z), names=names, models={})


def _oracle_kernels(O, t, train_fa, query_fa):
    r = O.gram(O.make_opt(t, 10, 6, 3, posfile=train_fa, negfile=query_fa, nthreads=8), want_profiles=False)
    K = np.tril(r["K"]) + np.tril(r["K"], -1).T
    nt = r["n_pos"]
    return K[:nt, :nt], K[nt:, :nt]


def _gpu_kernels(dv, t, train_fa, query_fa):
    """the device's own matrices (RBF types: its exp() is not the host's): the training Gram matrix and the query x
    training block of the scoring path"""
    import torch
    tr, _, _, _ = dv.read_problem(train_fa, query_fa)
    nt = len(dv.read_fasta(train_fa)[1])
    res = dv.gram_matrix(tr, t, 10, 6, 3, symmetric=True)
    K_train = res["K"][:nt, :nt].cpu().numpy()
    del res
    ctx = dv.GramContext(t, 10, 6, 3, 50, 50.0, 1.0, 0)
    try:
        stream = torch.cuda.current_stream().cuda_stream
        ctx.set_sequences(tr, stream)
        G = torch.zeros((nt, len(tr) - nt), dtype=torch.float64, device="cuda")
        rows = np.arange(nt, dtype=np.int32)
        ctx.gram_block(rows, nt, len(tr), G.data_ptr(), len(tr) - nt, stream)
        sq = torch.zeros(len(tr), dtype=torch.float64, device="cuda")
        ctx.self_norms(sq.data_ptr(), stream)
        ctx.normalize_block(rows, nt, len(tr), G.data_ptr(), len(tr) - nt, sq.data_ptr(), stream)
        torch.cuda.synchronize()
        K_query = G.cpu().numpy().T.copy()
    finally:
        ctx.close()
    torch.cuda.empty_cache()
    return K_train, K_query


def _model(files, t, shrinking=False):
    from gkmqc_amd import gkmpredict as gp
    key = (t, shrinking)
    if key not in files["models"]:
        files["models"][key] = gp.train_svr(files["train"], files["targets"], kernel_type=t, shrinking=shrinking)
    return files["models"][key]


@pytest.mark.parametrize("t", [0, 2, 4, 3, 5])
@pytest.mark.parametrize("shrinking", [False, True])
def test_train_svr_and_score_match_sklearn(dv, files, t, shrinking):
    from sklearn.svm import SVR
    from gkmqc_amd import gkmpredict as gp
    from oracle import oracle as O
    model = _model(files, t, shrinking)
    assert model.is_svr and model.epsilon == 0.1 and model.n_iter > 0
    names, scores = gp.score(model, files["query"])
    if t in (3, 5):
        K_train, K_query = _gpu_kernels(dv, t, files["train"], files["query"])
    else:
        K_train, K_query = _oracle_kernels(O, t, files["train"], files["query"])
    m = SVR(kernel="precomputed", C=1.0, epsilon=0.1, tol=1e-3, shrinking=shrinking).fit(K_train, files["z"])
    assert [files["names"][i] for i in m.support_] == model.names
    assert model.dual_coef().tobytes() == m.dual_coef_[0].tobytes()
    assert model.rho == m.intercept_[0]
    want = m.predict(K_query)
    assert scores.tobytes() == want.tobytes(), helpers.max_rel_err(scores, want)
    assert 0 < model.n_sv < len(files["names"])


def test_scores_do_not_depend_on_the_block_size(dv, files):
    from gkmqc_amd import gkmpredict as gp
    from gkmqc_amd import synth
    model = _model(files, 4)
    qs = [dv.encode(s) for s in synth.make_sequences(31, 23, 300, (20, 400))]
    ref = None
    for block in (1, 7, None):
        _, scores = gp.score(model, qs, block=block)
        ref = scores if ref is None else ref
        assert scores.tobytes() == ref.tobytes(), block


def test_no_support_vectors_is_refused(dv, files):
    from gkmqc_amd import gkmpredict as gp
    with pytest.raises(gp.ModelError) as e:
        gp.train_svr(files["train"], files["targets"], kernel_type=4, epsilon=100.0)
    assert "epsilon" in str(e.value)


# ------------------------------------------------------------------ downstream on an SVR model
def _queries(dv, L):
    pos, _, _, _ = dv.read_fasta(POS)
    neg, _, _, _ = dv.read_fasta(NEG)
    return [np.array(pos[0]), np.array(neg[3]), np.array(pos[11])[:L + 5]]


def test_explain_sums_to_score_minus_rho(dv, files):
    from gkmqc_amd import gkmpredict as gp
    for t in (0, 2, 4):
        model = _model(files, t)
        qs = _queries(dv, model.L)
        _, E = gp.explain(model, qs)
        _, sc = gp.score(model, qs)
        tol = 1e-10 * np.abs(model.dual_coef()).sum()
        for e, s in zip(E, sc):
            assert abs(e.sum() - (s - model.rho)) <= tol, (t, e.sum(), s - model.rho)


def _mutant(x, t, b):
    y = np.array(x, copy=True)
    y[t] = b
    return y


def test_ism_and_hypothetical_on_an_svr_model(dv, files):
    from gkmqc_amd import gkmpredict as gp
    model = _model(files, 4)
    qs = _queries(dv, model.L)
    _, ism = gp.ism(model, qs)
    _, hyp = gp.hypothetical(model, qs)
    _, own = gp.explain(model, qs)
    _, sx = gp.score(model, qs)
    mutants, index = [], []
    for qi, x in enumerate(qs):
        assert hyp[qi][np.arange(len(x)), x].tobytes() == own[qi].tobytes()
        for t in sorted({0, 1, len(x) // 2, len(x) - 2, len(x) - 1}):
            for b in range(4):
                if b != x[t]:
                    mutants.append(_mutant(x, t, b))
                    index.append((qi, t, b))
    _, sy = gp.score(model, mutants)
    _, ey = gp.explain(model, mutants)
    tol = 1e-12 * np.abs(model.dual_coef()).sum()
    for (qi, t, b), s, e in zip(index, sy, ey):
        assert abs(ism[qi][t, b] - (s - sx[qi])) <= tol, (qi, t, b)
        assert hyp[qi][t, b] == e[t], (qi, t, b)
    assert max(abs(s - sx[qi]) for (qi, _, _), s in zip(index, sy)) > 1e3 * tol


def test_weights_table_scores_match_score(dv, files):
    from gkmqc_amd import gkmpredict as gp
    model = _model(files, 4)
    tab = gp.lmer_weights(model)
    assert tab.rho == model.rho
    qs = _queries(dv, model.L)
    _, got = gp.score_with_table(tab, qs)
    _, want = gp.score(model, qs)
    tol = 1e-12 * np.abs(model.dual_coef()).sum()
    assert (np.abs(got - want) <= tol).all(), np.abs(got - want).max()


def _run(*args):
    r = subprocess.run([sys.executable, "-m", "gkmqc_amd.gkmpredict"] + [str(a) for a in args], cwd=helpers.ROOT,
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr
    return r


def test_cli_train_svr_then_predict_explain_ism_weights(dv, files, tmp_path):
    from gkmqc_amd import gkmpredict as gp
    mpath, out = tmp_path / "m.txt", tmp_path / "out.txt"
    r = _run("train-svr", "-t", 4, "-p", 0.1, files["train"], files["targets"], mpath)
    assert "support vectors" in r.stderr and "iterations" in r.stderr
    assert open(mpath).readline() == "format gkmqc-svr-1\n"
    model = gp.load(str(mpath))
    api = _model(files, 4)
    assert model.names == api.names and model.alpha.tobytes() == api.alpha.tobytes() and model.rho == api.rho
    _run("predict", files["query"], mpath, out)
    names, want = gp.score(api, files["query"])
    lines = open(out).read().split("\n")[:-1]
    assert [ln.rsplit("\t", 1)[0] for ln in lines] == names
    assert np.array([float(ln.rsplit("\t", 1)[1]) for ln in lines]).tobytes() == want.tobytes()
    _run("explain", files["query"], mpath, tmp_path / "e.txt")
    _, ex = gp.read_explanation(str(tmp_path / "e.txt"))
    _, ew = gp.explain(api, files["query"])
    assert all(a.tobytes() == b.tobytes() for a, b in zip(ex, ew))
    _run("ism", files["query"], mpath, tmp_path / "i.txt")
    _, iv = gp.read_ism(str(tmp_path / "i.txt"))
    assert len(iv) == len(names)
    _run("weights", mpath, tmp_path / "w.txt")
    tab = gp.load_lmer_table(str(tmp_path / "w.txt"))
    assert tab.rho == api.rho
