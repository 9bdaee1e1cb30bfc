"""In-silico mutagenesis on the GPU (gkmhip_ism_block, gkmhip_ism_self_profiles, gkmpredict.ism): exact tallies and self
profiles against the CPU reference (tests/ism_ref.py), agreement with `score` on every explicit mutant of trained models,
determinism across blocks, runs and neighbours, bounds of the output, the command line on a saved model, and
plausibility on sequences with a planted motif."""
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import helpers
from tests import ism_ref as R

pytestmark = pytest.mark.gpu

POS = os.path.join(helpers.GOLDEN, "motif_pos.fa")
NEG = os.path.join(helpers.GOLDEN, "motif_neg.fa")


@pytest.fixture(scope="module")
def gp(built):
    from gkmqc_amd import gkmpredict
    return gkmpredict


@pytest.fixture(scope="module")
def models(gp):
    out = {t: gp.train(POS, NEG, kernel_type=t, L=10, k=6, d=3) for t in (0, 2, 4)}
    # k = 0 allows d = L; every pair then counts with the same c_m, so training on such a kernel is degenerate: a model
    # built by hand from the motif sequences serves (ism must still equal the score differences, which are ~0 here)
    from gkmqc_amd import device as dv
    pos, _, _, _ = dv.read_fasta(POS)
    neg, _, _, _ = dv.read_fasta(NEG)
    svs = [np.array(neg[i]) for i in range(0, 40, 4)] + [np.array(pos[i]) for i in range(0, 40, 4)]
    alpha = np.linspace(0.1, 1.0, len(svs))
    out["k0"] = gp.Model(2, 5, 0, 5, 50, 50.0, 1.0, 1.0, 1e-3, False, 0.125, 10, alpha,
                         ["sv%d" % i for i in range(len(svs))], svs)
    return out


def _ragged_queries(seed=21, L=10, lens=(None, None, 37, 600, 2047)):
    rng = np.random.default_rng(seed)
    lens = [L if i == 0 else L + 1 if i == 1 else n for i, n in enumerate(lens)]
    return [rng.integers(0, 4, size=n, dtype=np.uint8) for n in lens]


class _Launcher:
    """one fresh context over `seqs`; ism_block / ism_self_profiles into sentinel-padded device buffers"""

    def __init__(self, dv, params, seqs):
        import torch
        self.torch = torch
        t, L, k, d, M, H = params
        self.d = d
        self.seqs = seqs
        self.ctx = dv.GramContext(t, L, k, d, M, H, 1.0, 0)
        self.stream = torch.cuda.current_stream().cuda_stream
        self.ctx.set_sequences(seqs, self.stream)

    def block(self, rows, c0, c1, fu, fb, gc, coef, pad=0, sentinel=-7.25):
        torch = self.torch
        nb = sum(len(s) for s in self.seqs[c0:c1])
        out = torch.full((4 * nb + 2 * pad,), sentinel, dtype=torch.float64, device="cuda")
        base = torch.full((c1 - c0 + 2 * pad,), sentinel, dtype=torch.float64, device="cuda")
        d_coef = torch.tensor(np.asarray(coef, dtype=np.float64), device="cuda")
        self.ctx.ism_block(rows, c0, c1, fu, fb, gc, d_coef.data_ptr(), out.data_ptr() + 8 * pad,
                           base.data_ptr() + 8 * pad, self.stream)
        torch.cuda.synchronize()
        assert self.ctx.last_kernel_name() == "k_ism"
        return out.cpu().numpy(), base.cpu().numpy()

    def self_profiles(self, c0, c1, pad=0, sentinel=-77):
        torch = self.torch
        nb = sum(len(s) for s in self.seqs[c0:c1])
        prof = torch.full((4 * (self.d + 1) * nb + 2 * pad,), sentinel, dtype=torch.int64, device="cuda")
        self.ctx.ism_self_profiles(c0, c1, prof.data_ptr() + 8 * pad, self.stream)
        torch.cuda.synchronize()
        assert self.ctx.last_kernel_name() == "k_ism_self"
        return prof.cpu().numpy()

    def close(self):
        self.ctx.close()


def _split(flat, queries, per_base):
    cuts = np.cumsum([len(x) for x in queries])[:-1]
    return [v.reshape(len(x), *per_base) for v, x in zip(np.split(flat, cuts * int(np.prod(per_base))), queries)]


def _unit(n, i):
    e = np.zeros(n)
    if i is not None:
        e[i] = 1.0
    return e


# (L, d) = (12, 8) and (8, 6) tile a 2 047-base query (1 094 and 1 407 positions per tile); (5, 5) is k = 0
@pytest.mark.parametrize("t,L,k,d", [(0, 3, 1, 2), (4, 10, 6, 3), (2, 5, 1, 4), (2, 5, 0, 5), (4, 12, 4, 8),
                                     (0, 8, 2, 6), (1, 2, 1, 1)])
def test_single_tallies_are_exact(gp, t, L, k, d):
    """one support vector, coef 1, one unit fold coefficient: every out[t, b] is the reference's U[t, m] or B[t, m, b] and
    base is P_m(x, s), bit for bit; 0.0 at the query's own base"""
    from gkmqc_amd import device as dv
    rng = np.random.default_rng(L * 13 + d)
    queries = _ragged_queries(L, L)
    sv = rng.integers(0, 4, size=317, dtype=np.uint8)
    sv[100:140] = (3 - queries[3][300:340])[::-1]             # a reverse-strand copy of a piece of the 600-base query
    sv[200:230] = queries[4][-30:]                            # the last l-mers of the longest query
    seqs = [sv] + queries
    want = [R.tallies(x, sv, t, L, d) for x in queries]
    mb = min(d + 1, L)
    run = _Launcher(dv, (t, L, k, d, 50, 50.0), seqs)
    try:
        for m in range(d + 1):
            out, base = run.block([0], 1, len(seqs), _unit(d + 1, m), _unit(d + 1, None), _unit(d + 1, m), [1.0])
            for qi, (g, x, (U, _)) in enumerate(zip(_split(out, queries, (4,)), queries, want)):
                w = np.repeat(U[:, m:m + 1].astype(np.float64), 4, axis=1)
                w[np.arange(len(x)), x] = 0.0
                assert np.array_equal(g, w), (t, L, d, "U", m, qi)
                assert base[qi] == float(R.profile(x, sv, t, L, d)[m]), (t, L, d, "P", m, qi)
        for m in range(1, mb + 1):
            out, _ = run.block([0], 1, len(seqs), _unit(d + 1, None), _unit(d + 1, m - 1), _unit(d + 1, None), [1.0])
            for qi, (g, (_, B)) in enumerate(zip(_split(out, queries, (4,)), want)):
                assert np.array_equal(g, B[:, m].astype(np.float64)), (t, L, d, "B", m, qi)
    finally:
        run.close()
    assert sum(w[0][:, 0].sum() for w in want) > 0 and sum(w[1][:, 1].sum() for w in want) > 0


@pytest.mark.parametrize("t,L,k,d", [(4, 10, 6, 3), (0, 6, 3, 3), (2, 5, 0, 5), (1, 12, 4, 8)])
def test_self_profiles_are_exact(gp, t, L, k, d):
    from gkmqc_amd import device as dv
    rng = np.random.default_rng(L + d)
    queries = _ragged_queries(L + 100, L, (None, None, 37, 200))
    queries[3][150:170] = (3 - queries[3][20:40])[::-1]        # its own reverse complement inside
    long = rng.integers(0, 4, size=2047, dtype=np.uint8)
    queries.append(long)
    seqs = [rng.integers(0, 4, size=50, dtype=np.uint8)] + queries
    run = _Launcher(dv, (t, L, k, d, 50, 50.0), seqs)
    try:
        pad = 32
        got = run.self_profiles(1, len(seqs), pad)
    finally:
        run.close()
    assert (got[:pad] == -77).all() and (got[-pad:] == -77).all()
    for qi, (g, x) in enumerate(zip(_split(got[pad:-pad], queries, (4, d + 1)), queries)):
        positions = None if len(x) < 1000 else [0, 1, L - 1, 1000, len(x) - L, len(x) - 1]
        want = R.self_profiles(x, t, L, d, positions=positions)
        rows = np.arange(len(x)) if positions is None else np.array(positions)
        assert np.array_equal(g[rows], want[rows]), (t, L, d, qi)


def _brute_force(gp, model, queries):
    """score(y) - score(x) for every explicit single-base mutant, through `score`"""
    mutants, index = [], []
    for qi, x in enumerate(queries):
        for t in range(len(x)):
            for b in range(4):
                if b != x[t]:
                    mutants.append(R.mutant(x, t, b))
                    index.append((qi, t, b))
    _, sx = gp.score(model, queries)
    _, sy = gp.score(model, mutants)
    want = [np.zeros((len(x), 4)) for x in queries]
    for (qi, t, b), s in zip(index, sy):
        want[qi][t, b] = s - sx[qi]
    return want


@pytest.mark.parametrize("which", [0, 2, 4, "k0"])
def test_ism_equals_the_score_of_every_mutant(gp, models, which):
    model = models[which]
    from gkmqc_amd import device as dv
    pos, _, _, _ = dv.read_fasta(POS)
    queries = [np.array(pos[0]), np.array(pos[7])] + _ragged_queries(5, model.L, (None, None, 37, 2047))
    names, got = gp.ism(model, queries)
    assert names == ["seq%d" % i for i in range(len(queries))]
    want = _brute_force(gp, model, queries)
    tol = 1e-12 * np.abs(model.dual_coef()).sum()
    for qi, (g, w, x) in enumerate(zip(got, want, queries)):
        assert g.dtype == np.float64 and g.shape == (len(x), 4)
        own = g[np.arange(len(x)), x]
        assert (own == 0.0).all() and not np.signbit(own).any(), qi
        err = np.abs(g - w).max()
        assert err <= tol, (which, qi, len(x), err, tol)
    if which != "k0":
        assert max(np.abs(w).max() for w in want) > 1e3 * tol      # (not a vacuous comparison)


def test_bit_identical_across_blocks_runs_and_neighbours(gp, models):
    model = models[4]
    queries = _ragged_queries(3, 10, (None, None, 37, 600, 211)) + _ragged_queries(4, 10, (None, None, 90, 1023))
    _, ref = gp.ism(model, queries)
    for block in (1, 3, len(queries)):
        _, got = gp.ism(model, queries, block=block)
        assert all(a.tobytes() == b.tobytes() for a, b in zip(got, ref)), block
    _, again = gp.ism(model, queries)
    assert all(a.tobytes() == b.tobytes() for a, b in zip(again, ref))
    rng = np.random.default_rng(4)
    for trial in range(3):
        others = [rng.integers(0, 4, size=int(rng.integers(10, 2048)), dtype=np.uint8)
                  for _ in range(int(rng.integers(1, 5)))]
        mixed = others[:2] + [queries[3]] + others[2:] + [queries[8]]
        at = len(others[:2])
        _, got = gp.ism(model, mixed, block=len(mixed) - trial)
        assert got[at].tobytes() == ref[3].tobytes() and got[-1].tobytes() == ref[8].tobytes(), trial


@pytest.mark.parametrize("L,k,d", [(10, 6, 3), (12, 4, 8)])
def test_nothing_outside_the_block_is_written(gp, L, k, d):
    """columns [c0, c1) with c0 > 0 among longer and shorter neighbours; 64 sentinels either side of the output and of
    base stay, no entry inside keeps one, and the values are the reference's tallies folded with the given coefficients"""
    from gkmqc_amd import device as dv
    rng = np.random.default_rng(8)
    svs = [rng.integers(0, 4, size=n, dtype=np.uint8) for n in (150, 80, 2047)]
    queries = _ragged_queries(9, L, (None, None, 37, 600, 211)) + [rng.integers(0, 4, size=2047, dtype=np.uint8)]
    seqs = svs + queries
    pad, sentinel = 64, -7.25
    c0, c1 = len(svs) + 2, len(seqs) - 1
    coef = [0.5, -1.25, 2.0]
    fu = np.linspace(1.0, 0.125, d + 1)
    fb = np.linspace(-0.3, 1.7, d + 1)
    gc = np.arange(1.0, d + 2)
    run = _Launcher(dv, (4, L, k, d, 50, 50.0), seqs)
    try:
        out, base = run.block([0, 1, 2], c0, c1, fu, fb, gc, coef, pad, sentinel)
    finally:
        run.close()
    for arr in (out, base):
        assert (arr[:pad] == sentinel).all() and (arr[-pad:] == sentinel).all()
        assert not (arr[pad:-pad] == sentinel).any()
    mb = min(d + 1, L)
    for qi, (g, x) in enumerate(zip(_split(out[pad:-pad], seqs[c0:c1], (4,)), seqs[c0:c1])):
        want, bound, gwant = 0.0, 0.0, 0.0
        for cf, s in zip(coef, svs):
            U, B = R.tallies(x, s, 4, L, d)
            U, B = U.astype(np.float64), B[:, 1:mb + 1].astype(np.float64)
            want = want + cf * ((U @ fu)[:, None] + np.einsum("tmb,m->tb", B, fb[:mb]))
            bound = bound + abs(cf) * ((U @ np.abs(fu))[:, None] + np.einsum("tmb,m->tb", B, np.abs(fb[:mb])))
            gwant = gwant + cf * float(R.profile(x, s, 4, L, d).astype(np.float64) @ gc)
        want[np.arange(len(x)), x] = 0.0
        assert (g[np.arange(len(x)), x] == 0.0).all(), qi
        assert (np.abs(g - want) <= 1e-14 * bound).all(), (qi, np.max(np.abs(g - want) - 1e-14 * bound))
        assert np.isclose(base[pad + qi], gwant, rtol=1e-14, atol=0), qi


def test_cli_on_a_saved_model_equals_the_api(gp, models, tmp_path):
    model = models[2]
    mpath, qpath, opath = str(tmp_path / "m.txt"), str(tmp_path / "q.fa"), str(tmp_path / "i.txt")
    model.save(mpath)
    from gkmqc_amd import synth
    synth.write_fasta(qpath, [b"ACGT" * 5 + b"NNACGGTACCA" * 7, b"GGGTTTACCAGTAC" * 30, b"ACGTACGTACGTAC"], "q")
    r = subprocess.run([sys.executable, "-m", "gkmqc_amd.gkmpredict", "ism", "--block", "2", qpath, mpath, opath],
                       cwd=helpers.ROOT, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    names, got = gp.read_ism(opath)
    want_names, want = gp.ism(gp.load(mpath), qpath)
    assert names == want_names and len(got) == 3
    assert all(a.tobytes() == b.tobytes() for a, b in zip(got, want))
    rbf = gp.train(POS, NEG, kernel_type=5, L=10, k=6, d=3)
    rbf.save(mpath)
    os.remove(opath)
    r = subprocess.run([sys.executable, "-m", "gkmqc_amd.gkmpredict", "ism", qpath, mpath, opath], cwd=helpers.ROOT,
                       capture_output=True, text=True)
    assert r.returncode == 1 and "RBF" in r.stderr
    assert not os.path.exists(opath)


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
    """Trained on 150 + 150 random 200-bp sequences, the positives carrying ATGACGTCATGG: on each of 20 held-out
    positives the most negative entry of the ISM table lies inside the motif."""
    from gkmqc_amd import synth
    pos, _ = _planted(1, 150, 200, MOTIF)
    neg, _ = _planted(2, 150, 200, None)
    pf, nf = str(tmp_path / "p.fa"), str(tmp_path / "n.fa")
    synth.write_fasta(pf, [gp.codes_to_text(s).encode() for s in pos], "p")
    synth.write_fasta(nf, [gp.codes_to_text(s).encode() for s in neg], "n")
    model = gp.train(pf, nf, kernel_type=4, L=10, k=6, d=3)
    held, at = _planted(3, 20, 200, MOTIF)
    _, I = gp.ism(model, held)
    inside = [p <= int(np.argmin(v.min(axis=1))) < p + len(MOTIF) for v, p in zip(I, at)]
    on = np.concatenate([v[p:p + len(MOTIF)].min(axis=1) for v, p in zip(I, at)])
    off = np.concatenate([np.delete(v.min(axis=1), np.arange(p, p + len(MOTIF))) for v, p in zip(I, at)])
    print("most negative entry inside the motif in %d of %d queries; worst per-position entry: motif mean %.4g, "
          "elsewhere mean %.4g" % (sum(inside), len(inside), on.mean(), off.mean()))
    assert all(inside), inside
