"""Training on all sequences and scoring new ones on the GPU (gkmqc_amd/gkmpredict.py): the column-range launch of the
Gram kernels (gkmhip_gram_block + gkmhip_normalize_block) against the reference's batch output and the CPU oracle, and
the trained model's scores against scikit-learn on the oracle's kernel matrices."""
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import helpers

pytestmark = pytest.mark.gpu

POS = os.path.join(helpers.GOLDEN, "motif_pos.fa")
NEG = os.path.join(helpers.GOLDEN, "motif_neg.fa")
KERNELS = ("bitslice", "direct")


@pytest.fixture(scope="module")
def dv(built):
    from gkmqc_amd import device
    return device


def _kern(dv, name):
    return dv.KERNEL_BITSLICE if name == "bitslice" else dv.KERNEL_DIRECT


def _block(dv, seqs, params, rows, c0, c1, kernel, normalize=True, ld=None, extra_rows=0, sentinel=None):
    """gram_block (+ normalize_block) on a fresh context -> host array [len(rows) + extra_rows, ld]."""
    import torch
    t, L, k, d, M, H, g = params
    ctx = dv.GramContext(t, L, k, d, M, H, g, 0)
    try:
        ctx.set_kernel(kernel)
        stream = torch.cuda.current_stream().cuda_stream
        ctx.set_sequences(seqs, stream)
        ld = ld or (c1 - c0)
        G = torch.full((len(rows) + extra_rows, ld), sentinel if sentinel is not None else 0.0, dtype=torch.float64,
                       device="cuda")
        rows = np.asarray(rows, dtype=np.int32)
        ctx.gram_block(rows, c0, c1, G.data_ptr(), ld, stream)
        if normalize:
            sq = torch.zeros(len(seqs), dtype=torch.float64, device="cuda")
            ctx.self_norms(sq.data_ptr(), stream)
            ctx.normalize_block(rows, c0, c1, G.data_ptr(), ld, sq.data_ptr(), stream)
        torch.cuda.synchronize()
        return G.cpu().numpy(), ctx.last_kernel_name()
    finally:
        ctx.close()


@pytest.mark.parametrize("kernel", KERNELS)
def test_block_matches_the_reference_batch_output(dv, kernel):
    """Support vectors as rows, the queries as the column range: the transpose of the reference's
    gkmkernel_kernelfunc_batch output (tests/golden/batch_rows_expected.npz) for its support columns."""
    for c in helpers.batch_rows_expected():
        seqs = helpers.synth_codes(c["n_support"], c["n_query"], c["length"], c["length_range"])
        ns, n = c["n_support"], c["n_support"] + c["n_query"]
        params = (c["kernel_type"], c["L"], c["k"], c["d"], c["M"], c["H"], c["gamma"])
        got, name = _block(dv, seqs, params, np.arange(ns), ns, n, _kern(dv, kernel))
        assert name.startswith("k_gram_" + kernel), name
        want = c["K"][:, :ns].T
        assert got.shape == want.shape, c["name"]
        if c["kernel_type"] in (3, 5):    # RBF: the device's exp() against the host's libm
            assert helpers.max_rel_err(got, want) < 1e-12, c["name"]
        else:
            assert np.array_equal(got, want), (c["name"], helpers.max_rel_err(got, want))


def _oracle_raw(O, t, L, k, d, pf, nf):
    """Raw G(a, j) = sum_m c_m P_m(a, j), ascending m from 0.0, for every pair of the problem (CPU oracle)."""
    r = O.gram(O.make_opt(t, L, k, d, posfile=pf, negfile=nf, nthreads=8), want_profiles=True)
    P = r["P"]
    i, j = np.triu_indices(r["n"], 1)
    P[i, j] = P[j, i]
    c = O.mismatch_weights(t, L, k)[: d + 1]
    G = np.zeros(P.shape[:2])
    for m in range(d + 1):
        G = G + c[m] * P[:, :, m].astype(np.float64)
    return G


@pytest.mark.parametrize("kernel", KERNELS)
def test_range_away_from_zero_with_rows_inside_and_outside(dv, kernel, tmp_path):
    """Raw values of a column range in the middle of a ragged set, rows before, inside and after it, against the oracle;
    cells past the range's width and rows past nrows keep their sentinel."""
    from gkmqc_amd import synth
    from oracle import oracle as O
    pf, nf = str(tmp_path / "p.fa"), str(tmp_path / "n.fa")
    synth.write_problem(pf, nf, 40, 37, 300, (40, 500))
    seqs, _, _, _ = dv.read_problem(pf, nf)
    t, L, k, d = 4, 10, 6, 3
    G_ref = _oracle_raw(O, t, L, k, d, pf, nf)
    rows = np.array([0, 3, 17, 30, 31, 44, 50, 76])
    c0, c1, ld, sentinel = 30, 51, 27, -7.25
    got, _ = _block(dv, seqs, (t, L, k, d, 50, 50.0, 1.0), rows, c0, c1, _kern(dv, kernel), normalize=False, ld=ld,
                    extra_rows=2, sentinel=sentinel)
    assert np.array_equal(got[:len(rows), :c1 - c0], G_ref[rows][:, c0:c1])
    assert (got[:len(rows), c1 - c0:] == sentinel).all()
    assert (got[len(rows):] == sentinel).all()


def _sklearn_scores(K_train, y, K_query, C, tol, shrinking):
    from sklearn.svm import SVC
    m = SVC(kernel="precomputed", C=C, tol=tol, shrinking=shrinking).fit(K_train, y)
    return m, m.decision_function(K_query)


def _oracle_kernels(O, t, L, k, d, train_fa, query_fa):
    """Oracle K over [train; queries]: the training block and the query x training block."""
    r = O.gram(O.make_opt(t, L, k, d, posfile=train_fa, negfile=query_fa, nthreads=8), want_profiles=False)
    K = np.tril(r["K"]) + np.tril(r["K"], -1).T
    nt = r["n_pos"]
    return K[:nt, :nt], K[nt:, :nt]


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    """pos + neg in one file (the oracle's first set) and a ragged synthetic query set"""
    from gkmqc_amd import synth
    tmp = tmp_path_factory.mktemp("predict")
    train_fa, query_fa = str(tmp / "train.fa"), str(tmp / "q.fa")
    with open(train_fa, "w") as f:
        f.write(open(POS).read().rstrip("\n") + "\n" + open(NEG).read())
    synth.write_fasta(query_fa, synth.make_sequences(21, 45, 300, (30, 700)), "q")
    return dict(train=train_fa, query=query_fa, oracle={})


def _oracle_cached(O, files, t, query_fa):
    key = (t, query_fa)
    if key not in files["oracle"]:
        files["oracle"][key] = _oracle_kernels(O, t, 10, 6, 3, files["train"], query_fa)
    return files["oracle"][key]


def _check_model_against(model, m, names_all):
    assert [names_all[i] for i in m.support_] == model.names
    assert np.array_equal(model.dual_coef(), m.dual_coef_[0])
    assert model.rho == m.intercept_[0]     # scikit-learn's intercept_ of a two-class SVC is LIBSVM's rho


@pytest.mark.parametrize("t", [0, 2, 4, 3, 5])
@pytest.mark.parametrize("shrinking", [False, True])
def test_train_and_score_match_sklearn(dv, files, t, shrinking):
    from gkmqc_amd import gkmpredict as gp
    from oracle import oracle as O
    L, k, d, C, tol = 10, 6, 3, 1.0, 1e-3
    train_fa, query_fa = files["train"], files["query"]
    model = gp.train(POS, NEG, kernel_type=t, L=L, k=k, d=d, C=C, tol=tol, shrinking=shrinking)
    names, scores = gp.score(model, query_fa)
    _, qnames, _, _ = dv.read_fasta(query_fa)
    assert names == qnames
    pos, pnames, _, _ = dv.read_fasta(POS)
    neg, nnames, _, _ = dv.read_fasta(NEG)
    y = np.concatenate((np.repeat(1, len(pos)), np.repeat(0, len(neg))))
    if t in (3, 5):
        # RBF types: the device's exp() is not the host's, so scikit-learn gets the GPU's own matrices
        import torch
        tr, _, _, _ = dv.read_problem(train_fa, query_fa)
        nt = len(y)
        res = dv.gram_matrix(tr, t, L, k, d, symmetric=True)
        K_train = res["K"][:nt, :nt].cpu().numpy()
        blk, _ = _block(dv, tr, (t, L, k, d, 50, 50.0, 1.0), np.arange(nt), nt, len(tr), dv.KERNEL_AUTO)
        K_query = blk.T.copy()
        del res
        torch.cuda.empty_cache()
    else:
        K_train, K_query = _oracle_cached(O, files, t, query_fa)
    m, want = _sklearn_scores(K_train, y, K_query, C, tol, shrinking)
    _check_model_against(model, m, pnames + nnames)
    assert np.array_equal(scores, want), helpers.max_rel_err(scores, want)


def test_iteration_cap_falls_back_to_sklearn(dv, monkeypatch):
    from gkmqc_amd import gkmpredict as gp
    ref = gp.train(POS, NEG, kernel_type=4)
    monkeypatch.setenv("GKM_SVM_MAX_ITER", "7")
    capped = gp.train(POS, NEG, kernel_type=4)
    assert capped.names == ref.names and np.array_equal(capped.alpha, ref.alpha) and capped.rho == ref.rho


@pytest.mark.parametrize("kernel", KERNELS)
def test_scores_do_not_depend_on_the_block_size(dv, kernel):
    """Block sizes 1, 7 (a ragged last block) and all at once; the longest query lies in one block only, so the
    positional-weight table uploaded with the blocks differs."""
    from gkmqc_amd import gkmpredict as gp
    from gkmqc_amd import synth
    model = gp.train(POS, NEG, kernel_type=4)
    qs = [dv.encode(s) for s in synth.make_sequences(31, 23, 300, (20, 400))]
    qs[9] = dv.encode(synth.make_sequences(32, 1, 1500)[0])
    ref = None
    for block in (1, 7, None):
        names, scores = gp.score(model, qs, block=block, kernel=_kern(dv, kernel))
        if ref is None:
            ref = scores
        assert np.array_equal(scores, ref), block
    other = "direct" if kernel == "bitslice" else "bitslice"
    _, scores = gp.score(model, qs, block=5, kernel=_kern(dv, other))
    assert np.array_equal(scores, ref)


def _run(*args):
    r = subprocess.run([sys.executable, "-m", "gkmqc_amd.gkmpredict"] + [str(a) for a in args], cwd=helpers.ROOT,
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr
    return r


def test_save_load_and_cli(dv, files, tmp_path):
    """CLI train -> model.txt -> CLI predict (fresh processes) = the in-memory model and scores; the quirks FASTA as
    queries scores as scikit-learn does on the oracle's kernels of the same reader's codes."""
    from gkmqc_amd import gkmpredict as gp
    from oracle import oracle as O
    model_txt, out = tmp_path / "model.txt", tmp_path / "out.txt"
    _run("train", "-t", "2", "-L", "10", "-k", "6", "-d", "3", "-C", "0.5", POS, NEG, model_txt)
    _run("predict", helpers.QUIRK_POS, model_txt, out)
    model = gp.train(POS, NEG, kernel_type=2, L=10, k=6, d=3, C=0.5)
    loaded = gp.load(str(model_txt))
    assert loaded.names == model.names and loaded.alpha.tobytes() == model.alpha.tobytes()
    assert loaded.rho == model.rho and loaded.n0 == model.n0 and loaded.C == 0.5
    assert all(np.array_equal(a, b) for a, b in zip(loaded.seqs, model.seqs))
    names, scores = gp.score(model, helpers.QUIRK_POS)
    rows = [ln.split("\t") for ln in open(out).read().splitlines()]
    assert [r[0] for r in rows] == names
    raw = open(helpers.QUIRK_POS).read()
    assert names == [ln[1:].strip("\r") for ln in raw.split("\n") if ln.startswith(">")]
    assert np.array_equal(np.array([float(r[1]) for r in rows]), scores)
    y = np.concatenate((np.repeat(1, 150), np.repeat(0, 160)))
    K_train, K_query = _oracle_cached(O, files, 2, helpers.QUIRK_POS)
    assert K_train.shape[0] == len(y)
    _, want = _sklearn_scores(K_train, y, K_query, 0.5, 1e-3, False)
    assert np.array_equal(scores, want)
