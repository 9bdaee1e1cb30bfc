"""The score of every single-base mutant on the GPU (gkmhip_ism_rbf_block, gkmpredict.mutant_scores): the RBF fold
against the CPU reference (tests/mutscores_ref.py) term by term, agreement with `score` on every explicit mutant of
trained RBF and linear models, the own-base column, determinism across blocks, runs and neighbours, bounds of the output,
the entry's refusals, the command line on a saved model, and plausibility on sequences with a planted motif."""
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import helpers
from tests import mutscores_ref as MR

pytestmark = pytest.mark.gpu

POS = os.path.join(helpers.GOLDEN, "motif_pos.fa")
NEG = os.path.join(helpers.GOLDEN, "motif_neg.fa")


@pytest.fixture(scope="module")
def gp(built):
    from gkmqc_amd import gkmpredict
    return gkmpredict


def _motif_seqs():
    from gkmqc_amd import device as dv
    pos, _, _, _ = dv.read_fasta(POS)
    neg, _, _, _ = dv.read_fasta(NEG)
    return pos, neg


@pytest.fixture(scope="module")
def models(gp):
    out = {(t, g): gp.train(POS, NEG, kernel_type=t, L=10, k=6, d=3, gamma=g) for t in (3, 5) for g in (1.0, 2.0)}
    out["lin4"] = gp.train(POS, NEG, kernel_type=4, L=10, k=6, d=3)
    pos, neg = _motif_seqs()
    rng = np.random.default_rng(5)
    z = [2.0 * np.mean((np.array(s) == 1) | (np.array(s) == 2)) + 0.1 * rng.normal() for s in pos]
    out["svr3"] = gp.train_svr(POS, z, kernel_type=3, L=10, k=6, d=3, gamma=1.0)
    # (12, 4, 8) tiles a 2 047-base query; 130 support vectors are three row chunks of 64, 64 and 2
    svs = [np.array(neg[i]) for i in range(65)] + [np.array(pos[i]) for i in range(65)]
    alpha = np.linspace(0.05, 1.0, len(svs))
    out["hand3"] = gp.Model(3, 12, 4, 8, 50, 50.0, 2.0, 1.0, 1e-3, False, -0.375, 65, alpha,
                            ["sv%d" % i for i in range(len(svs))], svs)
    # the hand-built k = 0 model of tests/test_ism_gpu.py (training on such a kernel is degenerate)
    svs = [np.array(neg[i]) for i in range(0, 40, 4)] + [np.array(pos[i]) for i in range(0, 40, 4)]
    out["k0"] = gp.Model(2, 5, 0, 5, 50, 50.0, 1.0, 1.0, 1e-3, False, 0.125, 10, np.linspace(0.1, 1.0, len(svs)),
                         ["sv%d" % i for i in range(len(svs))], svs)
    return out


def _ragged_queries(seed=21, L=10, lens=(None, None, 37, 600, 2047)):
    rng = np.random.default_rng(seed)
    lens = [L if i == 0 else L + 1 if i == 1 else n for i, n in enumerate(lens)]
    return [rng.integers(0, 4, size=n, dtype=np.uint8) for n in lens]


def _split(flat, queries, per_base):
    cuts = np.cumsum([len(x) for x in queries])[:-1]
    return [v.reshape(len(x), *per_base) for v, x in zip(np.split(flat, cuts * int(np.prod(per_base))), queries)]


class _Launcher:
    """one fresh context over `seqs` (the first n_sv of them support vectors) with the real inputs of the RBF entry: exact
    norms, the raw Gram block of (support vectors) x [c0, c1) and the mutants' norms from ism_self_profiles"""

    def __init__(self, gp, dv, params, gamma, seqs, n_sv, c0, c1):
        import torch
        self.torch = torch
        t, L, k, d = params
        self.ctx = dv.GramContext(t, L, k, d, 50, 50.0, gamma, 0)
        self.stream = torch.cuda.current_stream().cuda_stream
        self.ctx.set_sequences(seqs, self.stream)
        self.seqs, self.c0, self.c1 = seqs, c0, c1
        self.rows = np.arange(n_sv, dtype=np.int32)
        self.nb = sum(len(s) for s in seqs[c0:c1])
        c = dv.mismatch_weights(t, L, k)[:d + 1]
        self.sq = torch.empty(len(seqs), dtype=torch.float64, device="cuda")
        from gkmqc_amd import gkmquery
        gkmquery._exact_norms(self.ctx, len(seqs), c, self.sq, self.stream)
        self.ld = c1 - c0 + 3
        self.gx = torch.zeros((n_sv, self.ld), dtype=torch.float64, device="cuda")
        self.ctx.gram_block(self.rows, c0, c1, self.gx.data_ptr(), self.ld, self.stream)
        prof = torch.empty((self.nb, 4, d + 1), dtype=torch.int64, device="cuda")
        self.ctx.ism_self_profiles(c0, c1, prof.data_ptr(), self.stream)
        self.ysq = gkmquery._mutant_norms_sq(prof, c).sqrt_()

    def block(self, fu, fb, dual, pad=0, sentinel=-7.25, want_base=True):
        torch = self.torch
        out = torch.full((4 * self.nb + 2 * pad,), sentinel, dtype=torch.float64, device="cuda")
        base = torch.full((self.c1 - self.c0 + 2 * pad,), sentinel, dtype=torch.float64, device="cuda")
        d_dual = torch.tensor(np.asarray(dual, dtype=np.float64), device="cuda")
        self.ctx.ism_rbf_block(self.rows, self.c0, self.c1, fu, fb, d_dual.data_ptr(), self.sq.data_ptr(),
                               self.gx.data_ptr(), self.ld, self.ysq.data_ptr(), out.data_ptr() + 8 * pad,
                               base.data_ptr() + 8 * pad if want_base else None, self.stream)
        torch.cuda.synchronize()
        assert self.ctx.last_kernel_name() == "k_ism_rbf"
        return out.cpu().numpy(), base.cpu().numpy()

    def host_inputs(self):
        """(sq, gx[:, :ncols], [ysq (T, 4) per query]) as the device holds them"""
        queries = self.seqs[self.c0:self.c1]
        return (self.sq.cpu().numpy(), self.gx.cpu().numpy()[:, :self.c1 - self.c0],
                _split(self.ysq.cpu().numpy().reshape(-1), queries, (4,)))

    def close(self):
        self.ctx.close()


def _model_for(gp, t, L, k, d):
    """a model of the given kernel, for its fold coefficients only"""
    return gp.Model(t, L, k, d, 50, 50.0, 1.0, 1.0, 1e-3, False, 0.0, 0, [1.0], ["s"], [np.zeros(L, np.uint8)])


# (5, 12, 4, 8) tiles the 2 047-base query (1 094 positions per tile)
@pytest.mark.parametrize("t,L,k,d", [(3, 10, 6, 3), (5, 10, 6, 3), (3, 5, 1, 4), (5, 12, 4, 8)])
def test_entry_equals_the_reference_term_by_term(gp, t, L, k, d):
    """one support vector with pairs at every mismatch count, the real fold coefficients, Gram block and mutant norms:
    every out and base within 1e-12 max(1, gamma) |dual| of the numpy fold of the reference's exact tallies (1e-12: the
    project's bound for device exp against libm, tests/test_predict_gpu.py; an error in K enters the exponent times
    gamma); 0.0 at the own base"""
    from gkmqc_amd import device as dv
    rng = np.random.default_rng(L * 13 + d)
    queries = _ragged_queries(L, L)
    sv = rng.integers(0, 4, size=317, dtype=np.uint8)
    sv[100:140] = (3 - queries[3][300:340])[::-1]             # a reverse-strand copy of a piece of the 600-base query
    sv[200:230] = queries[4][-30:]                            # the last l-mers of the longest query
    seqs = [sv] + queries
    fu, fb, _ = gp.ism_coefficients(_model_for(gp, t, L, k, d))
    dg = [[MR.delta_g(x, sv, t, L, d, fu, fb)] for x in queries]
    dual = [-1.75]
    moved = 0.0
    for gamma in (0.25, 1.0, 2.0):
        run = _Launcher(gp, dv, (t, L, k, d), gamma, seqs, 1, 1, len(seqs))
        try:
            out, base = run.block(fu, fb, dual)
            sq, gx, ysq = run.host_inputs()
        finally:
            run.close()
        want, wbase = MR.rbf_block(queries, [sv], t, L, d, fu, fb, dual, sq[:1], sq[1:], gx, ysq, gamma, dg=dg)
        tol = 1e-12 * max(1.0, gamma) * abs(dual[0])
        for qi, (g, w, x) in enumerate(zip(_split(out, queries, (4,)), want, queries)):
            own = g[np.arange(len(x)), x]
            assert (own == 0.0).all() and not np.signbit(own).any(), (t, L, d, gamma, qi)
            err = np.abs(g - w).max()
            print("type %d (%d, %d, %d) gamma %g query %d (%d bases): worst |out - ref| %.3g, base %.3g (bound %.3g)"
                  % (t, L, k, d, gamma, qi, len(x), err, abs(base[qi] - wbase[qi]), tol))
            assert err <= tol, (t, L, d, gamma, qi, err, tol)
            assert abs(base[qi] - wbase[qi]) <= tol, (t, L, d, gamma, qi, base[qi], wbase[qi])
            off = np.ones_like(w, dtype=bool)
            off[np.arange(len(x)), x] = False
            moved = max(moved, np.abs(w - wbase[qi])[off].max())
    assert moved > 1e3 * 2e-12 * abs(dual[0])                 # (the mutants' terms differ from the query's own)


def _check_equals_score(gp, model, tol):
    pos, _ = _motif_seqs()
    queries = [np.array(pos[0]), np.array(pos[7])] + _ragged_queries(5, model.L, (None, None, 37, 2047))
    names, got = gp.mutant_scores(model, queries)
    assert names == ["seq%d" % i for i in range(len(queries))]
    want = MR.brute_force(gp, model, queries)
    moved = 0.0
    for qi, (g, w, x) in enumerate(zip(got, want, queries)):
        assert g.dtype == np.float64 and g.shape == (len(x), 4)
        own = g[np.arange(len(x)), x]
        assert len(set(own.tobytes()[8 * i:8 * i + 8] for i in range(len(x)))) == 1, qi    # one bit pattern at every t
        err = np.abs(g - w).max()
        print("query %d (%d bases): worst |ms - score| %.3g (bound %.3g)" % (qi, len(x), err, tol))
        assert err <= tol, (qi, len(x), err, tol)
        moved = max(moved, np.abs(g - own[:, None]).max())
    return moved


@pytest.mark.parametrize("which", [(3, 1.0), (3, 2.0), (5, 1.0), (5, 2.0), "svr3", "hand3"])
def test_rbf_mutant_scores_equal_the_score_of_every_mutant(gp, models, which):
    """|ms - score(y)| <= 1e-12 max(1, gamma) sum |dual_coef| for every mutant, the own-base column against score(x)
    included; and the mutants move the score by far more than that"""
    model = models[which]
    tol = 1e-12 * max(1.0, model.gamma) * np.abs(model.dual_coef()).sum()
    moved = _check_equals_score(gp, model, tol)
    assert moved > 1e3 * tol                                   # (not a vacuous comparison)


@pytest.mark.parametrize("which", ["lin4", "k0"])
def test_linear_mutant_scores_equal_the_score_of_every_mutant(gp, models, which):
    """the linear route (k_ism and ism's finish, plus rho): |ms - score(y)| <= 1e-12 sum |dual_coef|"""
    model = models[which]
    tol = 1e-12 * np.abs(model.dual_coef()).sum()
    moved = _check_equals_score(gp, model, tol)
    if which != "k0":                                           # (k = 0: every pair counts alike, the differences are ~0)
        assert moved > 1e3 * tol


@pytest.mark.parametrize("which", [(5, 1.0), "hand3", "lin4"])
def test_own_base_column_is_one_bit_pattern(gp, models, which):
    """ms[t, x[t]] is score(x)'s double at every t, on the tiled shape ((12, 4, 8), 2 047 bases: two tiles) too"""
    model = models[which]
    queries = _ragged_queries(17, model.L, (None, None, 37, 2047))
    _, got = gp.mutant_scores(model, queries, block=3)
    _, sx = gp.score(model, queries)
    tol = 1e-12 * max(1.0, model.gamma) * np.abs(model.dual_coef()).sum()
    for g, x, s in zip(got, queries, sx):
        own = np.ascontiguousarray(g[np.arange(len(x)), x])
        assert own.tobytes() == own[:1].tobytes() * len(x)
        assert abs(own[0] - s) <= tol
        assert (g != own[0]).any()


def test_bit_identical_across_blocks_runs_and_neighbours(gp, models):
    model = models[(5, 1.0)]
    queries = _ragged_queries(3, 10, (None, None, 37, 600, 211)) + _ragged_queries(4, 10, (None, None, 90, 1023))
    _, ref = gp.mutant_scores(model, queries)
    for block in (1, 3, len(queries)):
        _, got = gp.mutant_scores(model, queries, block=block)
        assert all(a.tobytes() == b.tobytes() for a, b in zip(got, ref)), block
    _, again = gp.mutant_scores(model, queries)
    assert all(a.tobytes() == b.tobytes() for a, b in zip(again, ref))
    rng = np.random.default_rng(4)
    for trial in range(3):
        others = [rng.integers(0, 4, size=int(rng.integers(10, 2048)), dtype=np.uint8)
                  for _ in range(int(rng.integers(1, 5)))]
        mixed = others[:2] + [queries[3]] + others[2:] + [queries[8]]
        at = len(others[:2])
        _, got = gp.mutant_scores(model, mixed, block=len(mixed) - trial)
        assert got[at].tobytes() == ref[3].tobytes() and got[-1].tobytes() == ref[8].tobytes(), trial


@pytest.mark.parametrize("L,k,d", [(10, 6, 3), (12, 4, 8)])
def test_nothing_outside_the_block_is_written(gp, L, k, d):
    """columns [c0, c1) with c0 > 0 among longer and shorter neighbours; 64 sentinels either side of the output and of
    base stay, no entry inside keeps one, and the values are the reference's (three support vectors, summed)"""
    from gkmqc_amd import device as dv
    rng = np.random.default_rng(8)
    svs = [rng.integers(0, 4, size=n, dtype=np.uint8) for n in (150, 80, 2047)]
    queries = _ragged_queries(9, L, (None, None, 37, 600, 211)) + [rng.integers(0, 4, size=2047, dtype=np.uint8)]
    queries[3][100:180] = svs[1]                                # a support vector inside a query: K near 1 for its terms
    seqs = svs + queries
    pad, sentinel = 64, -7.25
    c0, c1 = len(svs) + 2, len(seqs) - 1
    dual = [0.5, -1.25, 2.0]
    gamma = 2.0
    fu, fb, _ = gp.ism_coefficients(_model_for(gp, 5, L, k, d))
    run = _Launcher(gp, dv, (5, L, k, d), gamma, seqs, len(svs), c0, c1)
    try:
        out, base = run.block(fu, fb, dual, pad, sentinel)
        sq, gx, ysq = run.host_inputs()
        out2, base2 = run.block(fu, fb, dual, pad, sentinel, want_base=False)       # base = NULL: out alone
    finally:
        run.close()
    for arr in (out, base):
        assert (arr[:pad] == sentinel).all() and (arr[-pad:] == sentinel).all()
        assert not (arr[pad:-pad] == sentinel).any()
    assert out2.tobytes() == out.tobytes() and (base2 == sentinel).all()
    want, wbase = MR.rbf_block(seqs[c0:c1], svs, 5, L, d, fu, fb, dual, sq[:len(svs)], sq[c0:c1], gx, ysq, gamma)
    tol = 1e-12 * gamma * np.abs(dual).sum()
    for qi, (g, w) in enumerate(zip(_split(out[pad:-pad], seqs[c0:c1], (4,)), want)):
        assert np.abs(g - w).max() <= tol, (qi, np.abs(g - w).max())
        assert abs(base[pad + qi] - wbase[qi]) <= tol, qi


def test_entry_refuses_a_linear_context_and_bad_arguments(gp):
    from gkmqc_amd import device as dv
    import torch
    rng = np.random.default_rng(2)
    seqs = [rng.integers(0, 4, size=n, dtype=np.uint8) for n in (40, 30, 25)]
    buf = torch.zeros(4 * 55 + 64, dtype=torch.float64, device="cuda")
    fu = fb = np.zeros(4)
    stream = torch.cuda.current_stream().cuda_stream
    for t, fails in ((4, True), (5, False)):
        ctx = dv.GramContext(t, 10, 6, 3, 50, 50.0, 1.0, 0)
        try:
            ctx.set_sequences(seqs, stream)
            p = buf.data_ptr()
            sq = torch.ones(3, dtype=torch.float64, device="cuda")
            ysq = torch.ones(4 * 55, dtype=torch.float64, device="cuda")
            args = ([0], 1, 3, fu, fb, p, sq.data_ptr(), p, 2, ysq.data_ptr(), p + 64, None, stream)
            if fails:
                with pytest.raises(dv.GkmError) as e:
                    ctx.ism_rbf_block(*args)
                assert "kernel type" in str(e.value)
            else:
                ctx.ism_rbf_block(*args)
                torch.cuda.synchronize()
                assert ctx.last_kernel_name() == "k_ism_rbf"
                with pytest.raises(dv.GkmError):                  # leading dimension below the range
                    ctx.ism_rbf_block(*(args[:8] + (1,) + args[9:]))
                with pytest.raises(dv.GkmError):                  # an empty range
                    ctx.ism_rbf_block(*((args[0], 2, 2) + args[3:]))
                with pytest.raises(dv.GkmError):                  # no mutant norms
                    ctx.ism_rbf_block(*(args[:9] + (None,) + args[10:]))
        finally:
            ctx.close()


def test_cli_on_a_saved_rbf_model_equals_the_api(gp, models, tmp_path):
    model = models[(5, 2.0)]
    mpath, qpath, opath = str(tmp_path / "m.txt"), str(tmp_path / "q.fa"), str(tmp_path / "ms.txt")
    model.save(mpath)
    from gkmqc_amd import synth
    synth.write_fasta(qpath, [b"ACGT" * 5 + b"NNACGGTACCA" * 7, b"GGGTTTACCAGTAC" * 30, b"ACGTACGTACGTAC"], "q")
    r = subprocess.run([sys.executable, "-m", "gkmqc_amd.gkmpredict", "mutant-scores", "--block", "2", qpath, mpath,
                        opath], cwd=helpers.ROOT, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    names, got = gp.read_ism(opath)
    want_names, want = gp.mutant_scores(gp.load(mpath), qpath)
    assert names == want_names and len(got) == 3
    assert all(a.tobytes() == b.tobytes() for a, b in zip(got, want))


MOTIF = np.array([0, 3, 2, 0, 1, 2, 3, 1, 0, 3, 2, 2], np.uint8)        # ATGACGTCATGG


def _planted(seed, n, length, motif):
    """n random sequences; if motif is given, each carries it (either strand) at a recorded position"""
    rng = np.random.default_rng(seed)
    seqs, at = [], []
    for _ in range(n):
        s = rng.integers(0, 4, size=length, dtype=np.uint8)
        if motif is not None:
            p = int(rng.integers(0, length - len(motif) + 1))
            s[p:p + len(motif)] = motif if rng.random() < 0.5 else (3 - motif)[::-1]
            at.append(p)
        seqs.append(s)
    return seqs, at


def test_most_negative_mutations_fall_inside_the_planted_motif(gp, tmp_path):
    """A type-5 model trained on 150 + 150 random 200-bp sequences, the positives carrying ATGACGTCATGG: on each of 20
    held-out positives the most negative entry of ms - ms_own lies inside the motif."""
    from gkmqc_amd import synth
    pos, _ = _planted(1, 150, 200, MOTIF)
    neg, _ = _planted(2, 150, 200, None)
    pf, nf = str(tmp_path / "p.fa"), str(tmp_path / "n.fa")
    synth.write_fasta(pf, [gp.codes_to_text(s).encode() for s in pos], "p")
    synth.write_fasta(nf, [gp.codes_to_text(s).encode() for s in neg], "n")
    model = gp.train(pf, nf, kernel_type=5, L=10, k=6, d=3)
    held, at = _planted(3, 20, 200, MOTIF)
    held_neg, _ = _planted(4, 20, 200, None)
    _, sp = gp.score(model, held)
    _, sn = gp.score(model, held_neg)
    auc = np.mean(sp[:, None] > sn[None, :]) + 0.5 * np.mean(sp[:, None] == sn[None, :])
    print("held-out AUC of the type-5 model: %.3f" % auc)
    assert auc >= 0.9                                          # (the premise: the model separates the sets)
    _, ms = gp.mutant_scores(model, held)
    I = [v - v[np.arange(len(x)), x][:, None] for v, x in zip(ms, held)]
    inside = [p <= int(np.argmin(v.min(axis=1))) < p + len(MOTIF) for v, p in zip(I, at)]
    on = np.concatenate([v[p:p + len(MOTIF)].min(axis=1) for v, p in zip(I, at)])
    off = np.concatenate([np.delete(v.min(axis=1), np.arange(p, p + len(MOTIF))) for v, p in zip(I, at)])
    print("most negative entry inside the motif in %d of %d queries; worst per-position entry: motif mean %.4g, "
          "elsewhere mean %.4g" % (sum(inside), len(inside), on.mean(), off.mean()))
    assert all(inside), inside
