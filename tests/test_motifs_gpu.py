"""PWM motifs against an l-mer weight table or panel on the GPU (gkmqc_amd/gkmmotifs.py, gkm_contract.hip).
Every profile value equals tests/motif_ref.py bit for bit: below, at and above one tile of 4^6 codes, through the fold
launch, at 1, 63, 64 and 65 windows; the results do not depend on the block or on the order of the motifs; a panel's
column is the single table's result; the reverse complement and the marginals' symmetry hold within a derived bound; and
a planted motif ranks first against a trained model's table."""
import numpy as np
import pytest

from tests import motif_ref as R

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -52
BG = np.array([0.3, 0.2, 0.2, 0.3])


@pytest.fixture(scope="module")
def gm(built):
    from gkmqc_amd import gkmmotifs
    return gkmmotifs


@pytest.fixture(scope="module")
def gt(built):
    from gkmqc_amd import gkmtables
    return gkmtables


_TABLES = {}


def _table(gt, L, seed=0):
    """one random symmetric table per (L, seed), shared by the tests and left unchanged"""
    if (L, seed) not in _TABLES:
        W = R.symmetric_table(np.random.default_rng(1000 * L + seed), L)
        _TABLES[L, seed] = gt.LmerTable(W, 2, L, L - 1, 1, 50, 50.0, 0.0)
    return _TABLES[L, seed]


def _motifs(L, seed):
    rng = np.random.default_rng(seed)
    widths = sorted({1, max(1, L - 1), L, 2 * L + 3})
    return [("w%d" % m, R.dirichlet_motif(rng, m)) for m in widths]


def _same(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and a.tobytes() == b.tobytes()


@pytest.mark.parametrize("L", [2, 3, 5, 6, 7, 10])
def test_profiles_equal_the_reference_bit_for_bit(gm, gt, L):
    table = _table(gt, L)
    motifs = _motifs(L, L)
    bg = BG if L % 2 else None
    r = gm.motif_scores(table, motifs, background=bg, profiles=True)
    bgv = R.normalise([BG])[0] if L % 2 else np.full(4, 0.25)
    b0 = R.contract(table.W, np.tile(bgv, (L, 1)))
    assert np.float64(r["background"]).tobytes() == b0.tobytes()
    assert r["names"] == [n for n, _ in motifs] and r["width"].tolist() == [len(M) for _, M in motifs]
    for i, (name, M) in enumerate(motifs):
        m = len(M)
        want = R.contract_many(table.W, R.windows(R.normalise(M), L, bgv))
        assert r["profiles"][i].shape == (m + L - 1,)
        assert _same(r["profiles"][i], want), (name, np.abs(r["profiles"][i] - want).max())
        # affinity, enrichment, peak and peak_offset follow from the profile by the stated host arithmetic
        aff, enr, peak, off = R.summary(r["profiles"][i], m, L, r["background"])
        assert (r["affinity"][i].tobytes(), r["enrichment"][i].tobytes(), r["peak"][i].tobytes(), int(r["peak_offset"][i])) == \
            (aff.tobytes(), enr.tobytes(), peak.tobytes(), off), name


@pytest.mark.parametrize("L", [2, 3, 5, 6, 7, 10])
def test_window_counts_around_a_wave_and_one_hot_windows(gm, gt, L):
    table = _table(gt, L)
    rng = np.random.default_rng(50 + L)
    P = rng.dirichlet(np.ones(4), size=(65, L))
    P[3, L - 1] = [0.0, 1.0, 0.0, 0.0]
    P[40, 0] = [0.5, 0.0, 0.0, 0.5]
    want = R.contract_many(table.W, P)
    for n in (1, 63, 64, 65):
        got = gm.contract_windows(table, np.ascontiguousarray(P[:n]), 0, None, None)
        assert _same(got, want[:n]), (n, np.abs(got - want[:n]).max())
    # a one-hot window returns its code's weight exactly
    codes = np.unique(np.concatenate(([0, 4 ** L - 1, 4 ** L // 3], rng.integers(0, 4 ** L, size=20))))
    digits = (codes[:, None] >> (2 * (L - 1 - np.arange(L)))[None, :]) & 3
    got = gm.contract_windows(table, np.ascontiguousarray(np.eye(4)[digits]), 0, None, None)
    assert _same(got, table.W[codes])


def test_two_windows_at_l_12(gm, gt):
    L = 12
    rng = np.random.default_rng(12)
    table = gt.LmerTable(R.symmetric_table(rng, L), 2, L, L - 1, 1, 50, 50.0, 0.0)
    P = rng.dirichlet(np.ones(4), size=(2, L))
    P[1, 5] = [0.0, 0.0, 1.0, 0.0]
    got = gm.contract_windows(table, P, 0, None, None)
    assert _same(got, R.contract_many(table.W, P))


@pytest.mark.parametrize("L", [5, 7])
def test_results_do_not_depend_on_the_block_or_the_order_of_the_motifs(gm, gt, L):
    table = _table(gt, L)
    motifs = _motifs(L, 70 + L) + [("x%d" % i, R.dirichlet_motif(np.random.default_rng(i), 4 + i)) for i in range(5)]
    seen = []
    whole = gm.motif_scores(table, motifs, background=BG, profiles=True, on_block=seen.append)
    assert len(seen) == 1 and seen[0]["kernel"] == "k_lmer_contract" and seen[0]["kernel_ms"] > 0
    assert seen[0]["terms"] == float(seen[0]["windows"]) * 4 ** L
    for block in (1, 7):
        seen = []
        r = gm.motif_scores(table, motifs, background=BG, profiles=True, block=block, on_block=seen.append)
        assert len(seen) == -(-(sum(len(M) + L - 1 for _, M in motifs) + 1) // block)
        for key in ("affinity", "enrichment", "peak", "peak_offset", "width"):
            assert r[key].tobytes() == whole[key].tobytes(), (block, key)
        assert r["background"] == whole["background"]
        assert all(_same(a, b) for a, b in zip(r["profiles"], whole["profiles"]))
    order = np.random.default_rng(9).permutation(len(motifs))
    r = gm.motif_scores(table, [motifs[i] for i in order], background=BG, profiles=True)
    for at, i in enumerate(order):
        assert r["names"][at] == motifs[i][0] and _same(r["profiles"][at], whole["profiles"][i])
        for key in ("affinity", "enrichment", "peak", "peak_offset"):
            assert r[key][at].tobytes() == whole[key][i].tobytes()


@pytest.mark.parametrize("L", [5, 7])
@pytest.mark.parametrize("nm", [1, 3, 8, 9, 64])
def test_a_panel_column_is_the_single_table(gm, gt, L, nm):
    tables = [_table(gt, L, seed) for seed in range(nm)]
    panel = gt.LmerPanel(tables)
    motifs = _motifs(L, 30 + L)
    seen = []
    rp = gm.motif_scores_with_panel(panel, motifs, background=BG, profiles=True, block=11, on_block=seen.append)
    assert seen[0]["kernel"] == "k_panel_contract" and seen[0]["models"] == nm
    assert seen[0]["terms"] == float(seen[0]["windows"]) * nm * 4 ** L
    assert rp["affinity"].shape == (len(motifs), nm) and rp["background"].shape == (nm,)
    for m in range(nm):
        r = gm.motif_scores(panel.table(m), motifs, background=BG, profiles=True)
        assert np.float64(rp["background"][m]).tobytes() == np.float64(r["background"]).tobytes()
        for key in ("affinity", "enrichment", "peak", "peak_offset"):
            assert np.ascontiguousarray(rp[key][:, m]).tobytes() == r[key].tobytes(), (m, key)
        assert all(_same(a[:, m], b) for a, b in zip(rp["profiles"], r["profiles"])), m
    marg = gm.position_marginals_with_panel(panel)
    assert marg.shape == (L, 4, nm)
    assert _same(marg[:, :, nm - 1], gm.position_marginals(tables[nm - 1]))


@pytest.mark.parametrize("nm", [9, 64])
def test_a_panel_over_several_rows_of_tiles_and_runs_of_windows(gm, gt, nm):
    """L = 8: 16 tiles, so that 64 models take four workgroup rows of tiles and 9 models (four groups per wave) fill one
    row exactly (the panels at L = 7 leave groups without a tile); 70 windows: two runs of windows, the second one partial."""
    L = 8
    tables = [_table(gt, L, seed) for seed in range(nm)]
    panel = gt.LmerPanel(tables)
    P = np.random.default_rng(8 + nm).dirichlet(np.ones(4), size=(70, L))
    got = gm.contract_windows(panel, P)
    assert got.shape == (70, nm)
    for m in (0, nm // 2, nm - 1):
        assert _same(got[:, m], R.contract_many(tables[m].W, P)), m
    assert _same(got, np.stack([gm.contract_windows(t, P) for t in tables], axis=1))
    for n in (63, 64, 65):
        assert _same(gm.contract_windows(panel, P[:n]), got[:n]), n


def _abs_bound(W, windows, L):
    """8 L eps a_abs(P): four rounded operations per level, L levels, two evaluations; a_abs the same contraction of |W|"""
    return 8 * L * EPS * R.contract_many(np.abs(W), windows)


def test_reverse_complement_motif_has_the_reversed_profile(gm, gt):
    L = 7
    table = _table(gt, L)
    motifs = _motifs(L, 21)
    fwd = gm.motif_scores(table, motifs, profiles=True)
    rev = gm.motif_scores(table, [(n, gm.reverse_complement_motif(M)) for n, M in motifs], profiles=True)
    worst = 0.0
    for (name, M), a, b in zip(motifs, fwd["profiles"], rev["profiles"]):
        bound = _abs_bound(table.W, R.windows(R.normalise(M), L), L)
        diff = np.abs(a - b[::-1])
        worst = max(worst, float((diff / bound).max()))
        assert (diff <= bound).all(), (name, float((diff / bound).max()))
    print("largest difference: %.3g of the bound" % worst)


@pytest.mark.parametrize("L", [5, 7])
def test_position_marginals(gm, gt, L):
    table = _table(gt, L)
    marg = gm.position_marginals(table)
    wins = gm.marginal_windows(L).reshape(4 * L, L, 4)
    assert marg.shape == (L, 4) and _same(marg.reshape(-1), R.contract_many(table.W, wins))
    bound = _abs_bound(table.W, wins, L).reshape(L, 4)
    assert (np.abs(marg - marg[::-1, ::-1]) <= bound).all()
    assert np.abs(marg).max() > 0


def test_the_three_commands_on_saved_files_equal_the_api(gm, gt, tmp_path, capsys):
    L = 6
    tables = [_table(gt, L, s) for s in range(3)]
    panel = gt.LmerPanel(tables, names=["a", "b", "c"])
    wpath, ppath, mpath = str(tmp_path / "w.txt"), str(tmp_path / "p.npz"), str(tmp_path / "m.meme")
    tables[0].save(wpath)
    panel.save(ppath)
    motifs = _motifs(L, 5)
    with open(mpath, "w") as f:
        f.write("MEME version 4\n\nALPHABET= ACGT\n\n")
        for name, M in motifs:
            f.write("MOTIF %s\nletter-probability matrix: alength= 4 w= %d\n" % (name, len(M)))
            f.write("".join("%.6f %.6f %.6f %.6f\n" % tuple(row) for row in M) + "\n")
    read = gm.read_motifs(mpath)
    out, prof = str(tmp_path / "o.tsv"), str(tmp_path / "prof.tsv")
    assert gm.main(["score", "--background", "0.3,0.2,0.2,0.3", "--profiles", prof, "--block", "5", wpath, mpath, out]) == 0
    want = gm.motif_scores(gt.load_lmer_table(wpath), read, background=BG, profiles=True)
    got = gm.read_motif_scores(out)
    assert got["names"] == want["names"] and got["background"] == want["background"]
    for key in ("width", "affinity", "enrichment", "peak", "peak_offset"):
        assert got[key].tobytes() == want[key].tobytes(), key
    names, offs, vals = gm.read_motif_profiles(prof)
    assert names == want["names"] and all(_same(a, b) for a, b in zip(vals, want["profiles"]))
    assert all(o.tolist() == list(range(-(L - 1), len(M))) for o, (_, M) in zip(offs, read))
    assert gm.main(["score-panel", "--field", "peak", ppath, mpath, out]) == 0
    wantp = gm.motif_scores_with_panel(gt.load_lmer_panel(ppath), read)
    members, mnames, values = gm.read_panel_motif_scores(out)
    assert members == ["a", "b", "c"] and mnames == want["names"] and _same(values, wantp["peak"])
    assert gm.main(["marginals", wpath, out]) == 0
    assert _same(gm.read_marginals(out), gm.position_marginals(gt.load_lmer_table(wpath)))
    assert "->" in capsys.readouterr().err


MOTIF = np.array([0, 3, 2, 0, 1, 2, 3, 1, 0, 3, 2, 2], np.uint8)        # ATGACGTCATGG


def _consensus_pwm(codes):
    M = np.full((len(codes), 4), 0.05)
    M[np.arange(len(codes)), codes] = 0.85
    return M


def test_a_planted_motif_ranks_first_against_the_trained_table(gm, tmp_path):
    """Trained on 150 + 150 random 200-bp sequences, the positives carrying ATGACGTCATGG (type 4, L = 10, k = 6, d = 3), folded
    into a table: the planted consensus as a PWM (0.85 on the consensus base) has the largest enrichment among itself and
    40 random consensus PWMs of widths 6..14.  A condition, not a margin."""
    from gkmqc_amd import gkmpredict as gp
    from gkmqc_amd import synth
    from tests.test_explain_gpu import _planted
    pos, _ = _planted(1, 150, 200, MOTIF)
    neg, _ = _planted(2, 150, 200, None)
    pf, nf = str(tmp_path / "p.fa"), str(tmp_path / "n.fa")
    synth.write_fasta(pf, [gp.codes_to_text(s).encode() for s in pos], "p")
    synth.write_fasta(nf, [gp.codes_to_text(s).encode() for s in neg], "n")
    table = gp.lmer_weights(gp.train(pf, nf, kernel_type=4, L=10, k=6, d=3))
    rng = np.random.default_rng(2024)
    motifs = [("planted", _consensus_pwm(MOTIF))]
    motifs += [("random%d" % i, _consensus_pwm(rng.integers(0, 4, size=int(rng.integers(6, 15))))) for i in range(40)]
    r = gm.motif_scores(table, motifs)
    order = np.argsort(-r["enrichment"])
    print("enrichment: planted %.6g; the next three: %s" % (r["enrichment"][0], ", ".join(
        "%s %.6g" % (r["names"][i], r["enrichment"][i]) for i in order[order != 0][:3])))
    assert order[0] == 0, [(r["names"][i], float(r["enrichment"][i])) for i in order[:5]]
    assert -9 <= r["peak_offset"][0] <= 11
