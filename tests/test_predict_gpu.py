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
    G_ref = helpers.oracle_raw(O, t, L, k, d, pf, nf)
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


# ------------------------------------------------------------------ the column-range launch, kernel by kernel
def _raw_and_norm(dv, seqs, params, rows, c0, c1, kernel, ld=None, extra_rows=0, sentinel=-5.5):
    """gram_block, then self_norms + normalize_block, on one fresh context -> (raw, normalised, kernel name); both
    [len(rows) + extra_rows, ld] host arrays of a buffer prefilled with `sentinel`."""
    import torch
    ctx = dv.GramContext(*params)
    try:
        ctx.set_kernel(kernel)
        stream = torch.cuda.current_stream().cuda_stream
        ctx.set_sequences(seqs, stream)
        ld = ld or (c1 - c0)
        G = torch.full((len(rows) + extra_rows, ld), sentinel, dtype=torch.float64, device="cuda")
        rows = np.asarray(rows, dtype=np.int32)
        ctx.gram_block(rows, c0, c1, G.data_ptr(), ld, stream)
        torch.cuda.synchronize()
        raw = G.cpu().numpy()
        sq = torch.zeros(len(seqs), dtype=torch.float64, device="cuda")
        ctx.self_norms(sq.data_ptr(), stream)
        ctx.normalize_block(rows, c0, c1, G.data_ptr(), ld, sq.data_ptr(), stream)
        torch.cuda.synchronize()
        return raw, G.cpu().numpy(), ctx.last_kernel_name()
    finally:
        ctx.close()


def _same(a, b):
    return a.shape == b.shape and a.tobytes() == b.tobytes()


@pytest.mark.parametrize("L,d", helpers.ALL_LD)
def test_every_bitslice_instantiation_in_a_range(dv, L, d):
    """Every (L, d) the bit-sliced kernel is instantiated for, in the column-range launch: mixed-length input, a row set
    with jumps, a range that starts off an 8-column boundary and holds some of the rows.  Bit for bit the general
    kernel's block, raw and normalised, and on 14 sampled sequences the oracle's raw values."""
    rng = np.random.default_rng(100 * L + d + 7)
    seqs = [rng.integers(0, 4, int(n)).astype(np.uint8) for n in rng.integers(L, 900, 70)]
    seqs[3] = seqs[7].copy()
    seqs[11] = (3 - seqs[20][::-1]).astype(np.uint8)      # reverse complement of another sequence
    rows = np.r_[0:9, 30:41, 60:64]
    c0, c1 = 13, 59
    for t in (2, 4):
        params = (t, L, L - d, d, 50, 50.0, 1.0)
        a_raw, a_k, a_name = _raw_and_norm(dv, seqs, params, rows, c0, c1, dv.KERNEL_BITSLICE)
        b_raw, b_k, b_name = _raw_and_norm(dv, seqs, params, rows, c0, c1, dv.KERNEL_DIRECT)
        assert a_name.startswith("k_gram_bitslice") and b_name == "k_gram_direct"
        assert _same(a_raw, b_raw), (t, helpers.max_rel_err(a_raw, b_raw))
        assert _same(a_k, b_k), t
        ri = np.array([0, 4, 8, 9, 12, 19, 22])              # (positions in `rows`: rows 30, 33 and 40 lie in the range)
        cj = np.array([13, 14, 20, 30, 33, 45, 50, 57, 58])
        G, _ = helpers.oracle_cells(seqs, rows[ri], cj, params)
        assert len(np.unique(np.concatenate((rows[ri], cj)))) == 14
        assert _same(a_raw[np.ix_(ri, cj - c0)], G), t


def _sampled_oracle_check(seqs, params, raw, rows, c0, ri, cj):
    """raw[ri, cj - c0] (row positions ri, sequence columns cj) against the oracle on just those sequences"""
    G, _ = helpers.oracle_cells(seqs, rows[ri], cj, params)
    got = raw[np.ix_(ri, cj - c0)]
    assert _same(got, G), helpers.max_rel_err(got, G)


@pytest.mark.parametrize("shape,want", [("same", "k_gram_bitslice<same length>"), ("ragged", "k_gram_bitslice<packed>"),
                                        ("short", "k_gram_bitslice<packed,128>")])
def test_each_bitslice_variant_in_a_range(dv, shape, want):
    """Same-length 300-bp rows take `<same length>`, ragged 150-600 bp rows `<packed>`, many 60-110 bp rows
    `<packed,128>` (test_gpu_parity.py has the same rule for the triangle).  In a range off an 8-column boundary: the
    general kernel's block bit for bit and the oracle's raw values on a sampled sub-problem."""
    seqs = {"same": lambda: helpers.synth_codes(100, 100, 300),
            "ragged": lambda: helpers.synth_codes(100, 100, 300, (150, 600)),
            "short": lambda: helpers.synth_codes(150, 150, 300, (60, 110))}[shape]()
    n = len(seqs)
    params = (4, 12, 8, 4, 50, 50.0, 1.0) if shape == "ragged" else (4, 10, 6, 3, 50, 50.0, 1.0)
    rows = np.arange(n, dtype=np.int32)
    c0, c1 = 45, n - 3
    raw, K, name = _raw_and_norm(dv, seqs, params, rows, c0, c1, dv.KERNEL_BITSLICE)
    assert name == want
    d_raw, d_K, _ = _raw_and_norm(dv, seqs, params, rows, c0, c1, dv.KERNEL_DIRECT)
    assert _same(raw, d_raw) and _same(K, d_K)
    rng = np.random.default_rng(3)
    ri = np.sort(rng.choice(n, 10, replace=False))
    cj = np.sort(np.concatenate(([c0, c1 - 1], rng.choice(np.arange(c0 + 1, c1 - 1), 10, replace=False))))
    _sampled_oracle_check(seqs, params, raw, rows, c0, ri, cj)


@pytest.mark.parametrize("chunk", ["8", "40", "64"])
def test_column_chunked_order_in_a_range(dv, monkeypatch, chunk):
    """The (column chunk, tile) work order in a column-range launch: chunks of 8, 40 and 64 columns against the plain
    order on ragged data, a range that starts off an 8-column boundary and whose width is no multiple of the chunk (so
    the entries start at col_begin, not at a multiple of 8, and carry padding items).  Raw and normalised blocks bit
    for bit."""
    ragged = helpers.synth_codes(150, 150, 300, (150, 700))
    rows = np.r_[0:300:3, 101:104]
    rows = np.unique(rows).astype(np.int32)
    c0, c1 = 37, 240
    assert c0 % 8 and (c1 - c0) % int(chunk)
    for params in ((4, 12, 8, 4, 50, 50.0, 1.0), (2, 11, 7, 3, 50, 50.0, 1.0)):
        monkeypatch.setenv("GKM_COL_CHUNK", "0")
        want_raw, want_K, name = _raw_and_norm(dv, ragged, params, rows, c0, c1, dv.KERNEL_BITSLICE, ld=211, extra_rows=1)
        assert name.startswith("k_gram_bitslice")
        monkeypatch.setenv("GKM_COL_CHUNK", chunk)
        raw, K, _ = _raw_and_norm(dv, ragged, params, rows, c0, c1, dv.KERNEL_BITSLICE, ld=211, extra_rows=1)
        assert _same(raw, want_raw) and _same(K, want_K), params
        assert (raw[len(rows):] == -5.5).all() and (raw[:, c1 - c0:] == -5.5).all()


def _default_chunk(lens, L, W=10):
    """Restates plan_bitslice's default column chunk (gkmqc_amd/csrc/gkm_gram.hip, "work-item order"): chunks of 4 096
    columns where a chunk's column tables fit 3 MiB per XCD, over the mean length of ALL uploaded sequences."""
    mean_len = float(np.sum(np.asarray(lens) - L + 1)) / len(lens) + (L - 1)
    col_bytes = (4.0 * (mean_len + W) + 2.0 * (mean_len / 16.0 + 1.0)) * 4
    return 4096 if col_bytes * 4096.0 / 8.0 <= 3.0 * 1048576.0 else 0


def test_default_column_chunks_in_a_range(dv, monkeypatch):
    """The work order scoring takes at default settings: ~100 support-vector-like rows and a range of 4 600 ~300-bp
    columns, so plan_bitslice cuts the range into chunks of 4 096 columns by its own rule.  The block equals the plain
    order's and the general kernel's bit for bit, and 40 sampled columns on both sides of the chunk boundary (the last
    column among them) equal the oracle's raw values."""
    monkeypatch.delenv("GKM_COL_CHUNK", raising=False)
    monkeypatch.delenv("GKM_FORCE_PACKED", raising=False)
    seqs = helpers.synth_codes(103, 4600, 300, (240, 360))
    S, n = 103, len(seqs)
    c0, c1 = S, n
    params = (4, 10, 6, 3, 50, 50.0, 1.0)
    # the shape must keep meeting the rule, or this test would quietly stop covering the chunked order
    assert _default_chunk([len(s) for s in seqs], 10) == 4096 and c1 - c0 > 4096 and c0 % 8
    rows = np.arange(S, dtype=np.int32)
    raw, K, name = _raw_and_norm(dv, seqs, params, rows, c0, c1, dv.KERNEL_BITSLICE)
    assert name.startswith("k_gram_bitslice")
    monkeypatch.setenv("GKM_COL_CHUNK", "0")
    p_raw, p_K, _ = _raw_and_norm(dv, seqs, params, rows, c0, c1, dv.KERNEL_BITSLICE)
    monkeypatch.delenv("GKM_COL_CHUNK")
    d_raw, d_K, d_name = _raw_and_norm(dv, seqs, params, rows, c0, c1, dv.KERNEL_DIRECT)
    assert d_name == "k_gram_direct"
    assert _same(raw, p_raw) and _same(K, p_K)
    assert _same(raw, d_raw) and _same(K, d_K)
    rng = np.random.default_rng(8)
    edge = c0 + 4096
    cj = np.unique(np.concatenate((np.arange(edge - 6, edge + 6), [c0, c1 - 1], rng.choice(np.arange(c0, c1), 26, replace=False))))
    ri = np.array([0, 1, 50, 101, 102])
    assert len(cj) >= 40 and (cj < edge).any() and (cj >= edge).any()
    _sampled_oracle_check(seqs, params, raw, rows, c0, ri, cj)


def test_scores_at_a_production_sized_block(dv, files):
    """Training on the motif sets (type 4) and scoring 4 500 synthetic 300-bp queries: the default block takes them in
    one launch, in the chunked work order; block=1000 and either kernel give the same scores bit for bit.  60 sampled
    queries score as scikit-learn's decision_function does on the oracle's kernel values."""
    from gkmqc_amd import gkmpredict as gp
    from gkmqc_amd import synth
    from oracle import oracle as O
    model = gp.train(POS, NEG, kernel_type=4)
    qs = [dv.encode(s) for s in synth.make_sequences(41, 4500, 300, (270, 330))]
    S = model.n_sv
    assert gp.default_block(S) >= len(qs)
    lens = [len(s) for s in model.seqs] + [len(q) for q in qs]
    assert _default_chunk(lens, 10) == 4096 and len(qs) > 4096
    ref = None
    for kern in ("bitslice", "direct"):
        for block in (None, 1000):
            _, scores = gp.score(model, qs, block=block, kernel=_kern(dv, kern))
            if ref is None:
                ref = scores
            assert _same(scores, ref), (kern, block)
    # scikit-learn on the oracle's training matrix, its decision values from the oracle's query x support-vector cells
    # (a two-class LIBSVM model reads only its support vectors' columns)
    pos, pnames, _, _ = dv.read_fasta(POS)
    neg, nnames, _, _ = dv.read_fasta(NEG)
    train = list(pos) + list(neg)
    y = np.concatenate((np.repeat(1, len(pos)), np.repeat(0, len(neg))))
    K_train, _ = _oracle_cached(O, files, 4, files["query"])
    m, _ = _sklearn_scores(K_train, y, K_train[:1], 1.0, 1e-3, False)
    _check_model_against(model, m, pnames + nnames)
    sv = np.asarray(m.support_)
    pick = np.sort(np.random.default_rng(4).choice(len(qs), 60, replace=False))
    K_query = np.zeros((len(pick), len(train)))
    step = 200 - len(sv) if len(sv) < 170 else 30
    for g in range(0, len(pick), step):
        part = pick[g:g + step]
        both = [train[i] for i in sv] + [qs[i] for i in part]
        _, Kc = helpers.oracle_cells(both, np.arange(len(sv), len(both)), np.arange(len(sv)), (4, 10, 6, 3, 50, 50.0, 1.0))
        K_query[g:g + len(part)][:, sv] = Kc
    want = m.decision_function(K_query)
    assert _same(ref[pick], want), helpers.max_rel_err(ref[pick], want)


@pytest.mark.parametrize("t", [0, 2, 4, 3, 5])
def test_normalize_block_on_given_raw_values(dv, t):
    """gkmhip_normalize_block alone, on raw values and norms the test chooses: G / (sq[a] * sq[j]) -- the product
    first, one division -- bit for bit, RBF types exp(gamma (v - 1)) within 2 ulp of numpy, exactly 1.0 where the
    column is the row's own sequence (whatever the raw value there), NaN where the raw value is NaN, and every cell
    past the range's width or past the last row left alone."""
    import torch
    rng = np.random.default_rng(40 + t)
    n = 40
    seqs = [rng.integers(0, 4, 50).astype(np.uint8) for _ in range(n)]
    rows = np.array([1, 5, 12, 13, 20, 28, 31, 39], dtype=np.int32)
    c0, c1, ld, sentinel = 11, 29, 23, -7.25
    w = c1 - c0
    gamma = 0.7
    sq = rng.uniform(0.5, 3.0, n) * 10.0 ** rng.integers(-3, 4, n)
    raw = rng.uniform(-1.0, 1.0, (len(rows), w)) * np.outer(sq[rows], sq[c0:c1]) * rng.uniform(0.2, 1.5, (len(rows), w))
    raw[0, 3] = np.nan
    raw[2, 5] = -abs(raw[2, 5]) - 1e9                      # a wrapped (negative) profile
    raw[3, 1] = 1e-300                                      # a subnormal quotient
    own = [(i, a - c0) for i, a in enumerate(rows) if c0 <= a < c1]
    assert len(own) == 4                                    # rows 12, 13, 20, 28 meet their own column
    for i, jl in own:
        raw[i, jl] = 0.5 * sq[rows[i]] ** 2                 # not 1.0 if divided
    want = raw / (sq[rows][:, None] * sq[c0:c1][None, :])
    # (the test has teeth: dividing by one norm at a time rounds some cells differently)
    assert (want != raw / sq[rows][:, None] / sq[c0:c1][None, :]).sum() > 5
    if t in (3, 5):
        want = np.exp(gamma * (want - 1))
    for i, jl in own:
        want[i, jl] = 1.0
    ctx = dv.GramContext(t, 10, 6, 3, 50, 50.0, gamma)
    try:
        stream = torch.cuda.current_stream().cuda_stream
        ctx.set_sequences(seqs, stream)
        G = torch.full((len(rows) + 2, ld), sentinel, dtype=torch.float64, device="cuda")
        G[:len(rows), :w] = torch.from_numpy(raw)
        d_sq = torch.from_numpy(sq).cuda()
        ctx.normalize_block(rows, c0, c1, G.data_ptr(), ld, d_sq.data_ptr(), stream)
        torch.cuda.synchronize()
        got = G.cpu().numpy()
    finally:
        ctx.close()
    assert (got[:len(rows), w:] == sentinel).all() and (got[len(rows):] == sentinel).all()
    blk = got[:len(rows), :w]
    assert np.array_equal(np.isnan(blk), np.isnan(want)) and np.isnan(blk).sum() == 1
    for i, jl in own:
        assert blk[i, jl] == 1.0
    fin = ~np.isnan(want)
    if t in (3, 5):
        ulp = np.abs(blk[fin] - want[fin]) / np.spacing(np.abs(want[fin]))
        assert ulp.max() <= 2, ulp.max()
    else:
        assert blk[fin].tobytes() == want[fin].tobytes()
