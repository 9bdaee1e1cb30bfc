"""Hypothetical importance on the GPU (gkmhip_hyp_block, gkmpredict.hypothetical): exact single tallies against the CPU
reference (tests/ism_ref.py), the own column against `explain` of the query and every mutant column against `explain` of
that mutant, bit for bit, agreement with tests/hyp_ref.py, determinism across blocks, runs and neighbours, bounds of the
output, the command line on a saved model, and plausibility on sequences with a planted motif."""
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import explain_ref as E
from tests import helpers
from tests import hyp_ref as HR
from tests import ism_ref as R

pytestmark = pytest.mark.gpu

POS = os.path.join(helpers.GOLDEN, "motif_pos.fa")
NEG = os.path.join(helpers.GOLDEN, "motif_neg.fa")


@pytest.fixture(scope="module")
def gp(built):
    from gkmqc_amd import gkmpredict
    return gkmpredict


def _motif_svs():
    from gkmqc_amd import device as dv
    pos, _, _, _ = dv.read_fasta(POS)
    neg, _, _, _ = dv.read_fasta(NEG)
    return [np.array(neg[i]) for i in range(0, 40, 4)] + [np.array(pos[i]) for i in range(0, 40, 4)]


@pytest.fixture(scope="module")
def models(gp):
    out = {t: gp.train(POS, NEG, kernel_type=t, L=10, k=6, d=3) for t in (0, 2, 4)}
    # (L, k, d) = (12, 4, 8) and (8, 2, 6) tile a 2 047-base query (1 094 and 1 407 positions per tile):
    # models built by hand from the motif sequences
    svs = _motif_svs()
    alpha = np.linspace(0.1, 1.0, len(svs))
    for t, L, k, d in ((4, 12, 4, 8), (2, 8, 2, 6)):
        out[(L, d)] = gp.Model(t, L, k, d, 50, 50.0, 1.0, 1.0, 1e-3, False, 0.125, 10, alpha,
                               ["sv%d" % i for i in range(len(svs))], svs)
    return out


TILE = {(12, 8): 1094, (8, 6): 1407}


def _ragged_queries(seed=21, L=10, lens=(None, None, 37, 600, 2047)):
    rng = np.random.default_rng(seed)
    lens = [L if i == 0 else L + 1 if i == 1 else n for i, n in enumerate(lens)]
    return [rng.integers(0, 4, size=n, dtype=np.uint8) for n in lens]


class _Launcher:
    """one fresh context over `seqs`; hyp_block into sentinel-padded device buffers"""

    def __init__(self, dv, params, seqs):
        import torch
        self.torch = torch
        t, L, k, d, M, H = params
        self.seqs = seqs
        self.ctx = dv.GramContext(t, L, k, d, M, H, 1.0, 0)
        self.stream = torch.cuda.current_stream().cuda_stream
        self.ctx.set_sequences(seqs, self.stream)

    def block(self, rows, c0, c1, share, coef, pad=0, sentinel=-7.25):
        torch = self.torch
        nb = sum(len(s) for s in self.seqs[c0:c1])
        out = torch.full((4 * nb + 2 * pad,), sentinel, dtype=torch.float64, device="cuda")
        d_coef = torch.tensor(np.asarray(coef, dtype=np.float64), device="cuda")
        self.ctx.hyp_block(rows, c0, c1, share, d_coef.data_ptr(), out.data_ptr() + 8 * pad, self.stream)
        torch.cuda.synchronize()
        assert self.ctx.last_kernel_name() == "k_ism<true>"
        return out.cpu().numpy()

    def close(self):
        self.ctx.close()


def _split(flat, queries, per_base):
    cuts = np.cumsum([len(x) for x in queries])[:-1]
    return [v.reshape(len(x), *per_base) for v, x in zip(np.split(flat, cuts * int(np.prod(per_base))), queries)]


def _unit(n, i):
    e = np.zeros(n)
    e[i] = 1.0
    return e


@pytest.mark.parametrize("t,L,k,d", [(0, 3, 1, 2), (4, 10, 6, 3), (2, 5, 1, 4), (4, 12, 4, 8), (0, 8, 2, 6),
                                     (1, 2, 1, 1)])
def test_single_tallies_are_exact(gp, t, L, k, d):
    """one support vector, coef 1, a unit share[m]: out[t, x[t]] is the reference's U[t, m] and out[t, b] its
    B[t, m + 1, b], bit for bit"""
    from gkmqc_amd import device as dv
    rng = np.random.default_rng(L * 13 + d)
    queries = _ragged_queries(L, L)
    sv = rng.integers(0, 4, size=317, dtype=np.uint8)
    sv[100:140] = (3 - queries[3][300:340])[::-1]             # a reverse-strand copy of a piece of the 600-base query
    sv[200:230] = queries[4][-30:]                            # the last l-mers of the longest query
    sv[250:290] = queries[4][1070:1110]                       # across (12, 8)'s tile boundary
    seqs = [sv] + queries
    want = [R.tallies(x, sv, t, L, d) for x in queries]
    run = _Launcher(dv, (t, L, k, d, 50, 50.0), seqs)
    try:
        for m in range(d + 1):
            out = run.block([0], 1, len(seqs), _unit(d + 1, m), [1.0])
            for qi, (g, x, (U, B)) in enumerate(zip(_split(out, queries, (4,)), queries, want)):
                w = B[:, m + 1].astype(np.float64)
                w[np.arange(len(x)), x] = U[:, m]
                assert np.array_equal(g, w), (t, L, d, m, qi)
    finally:
        run.close()
    assert sum(w[0][:, 0].sum() for w in want) > 0 and sum(w[1][:, 1].sum() for w in want) > 0


def _mutant_positions(x, L, tile=None):
    if len(x) < 700:
        return list(range(len(x)))
    pos = {0, 1, L - 1, L, len(x) // 2, len(x) - L, len(x) - 1}
    if tile:
        pos |= {tile - L, tile - 1, tile, tile + 1, tile + L - 1}
    return sorted(p for p in pos if 0 <= p < len(x))


@pytest.mark.parametrize("which", [0, 2, 4, (12, 8), (8, 6)])
def test_columns_equal_explain_of_the_query_and_of_each_mutant(gp, models, which):
    """hyp[t, x[t]] == explain(x)[t] and hyp[t, b] == explain(y)[t], y = x with base t set to b, bit for bit (2 047-base
    queries: the ends and around the tile boundaries)"""
    model = models[which]
    from gkmqc_amd import device as dv
    pos, _, _, _ = dv.read_fasta(POS)
    queries = [np.array(pos[0]), np.array(pos[7])] + _ragged_queries(5, model.L, (None, None, 37, 2047))
    names, got = gp.hypothetical(model, queries)
    assert names == ["seq%d" % i for i in range(len(queries))]
    _, own = gp.explain(model, queries)
    mutants, index = [], []
    for qi, x in enumerate(queries):
        g = got[qi]
        assert g.dtype == np.float64 and g.shape == (len(x), 4)
        assert g[np.arange(len(x)), x].tobytes() == own[qi].tobytes(), (which, qi)
        for t in _mutant_positions(x, model.L, TILE.get(which)):
            for b in range(4):
                if b != x[t]:
                    mutants.append(R.mutant(x, t, b))
                    index.append((qi, t, b))
    _, ey = gp.explain(model, mutants)
    bad = [(qi, t, b) for (qi, t, b), e in zip(index, ey) if got[qi][t, b] != e[t] or np.signbit(got[qi][t, b])
           != np.signbit(e[t])]
    assert not bad, (which, len(bad), bad[:5])
    assert max(np.abs(e).max() for e in ey) > 0


@pytest.mark.parametrize("which", [0, 4])
def test_agrees_with_the_cpu_reference(gp, models, which):
    model = models[which]
    norms = E.sv_norms(model)
    queries = _ragged_queries(17, model.L, (None, None, 37, 64))
    _, got = gp.hypothetical(model, queries)
    tol = 1e-12 * np.abs(model.dual_coef()).sum()
    big = 0.0
    for qi, (g, x) in enumerate(zip(got, queries)):
        want, _ = HR.hypothetical(model, x, norms)
        err = np.abs(g - want).max()
        assert err <= tol, (which, qi, err, tol)
        big = max(big, np.abs(want).max())
    assert big > 1e3 * tol                                   # (not a vacuous comparison)


def test_bit_identical_across_blocks_runs_and_neighbours(gp, models):
    model = models[4]
    queries = _ragged_queries(3, 10, (None, None, 37, 600, 211)) + _ragged_queries(4, 10, (None, None, 90, 1023))
    _, ref = gp.hypothetical(model, queries)
    for block in (1, 3, len(queries)):
        _, got = gp.hypothetical(model, queries, block=block)
        assert all(a.tobytes() == b.tobytes() for a, b in zip(got, ref)), block
    _, again = gp.hypothetical(model, queries)
    assert all(a.tobytes() == b.tobytes() for a, b in zip(again, ref))
    rng = np.random.default_rng(4)
    for trial in range(3):
        others = [rng.integers(0, 4, size=int(rng.integers(10, 2048)), dtype=np.uint8)
                  for _ in range(int(rng.integers(1, 5)))]
        mixed = others[:2] + [queries[3]] + others[2:] + [queries[8]]
        at = len(others[:2])
        _, got = gp.hypothetical(model, mixed, block=len(mixed) - trial)
        assert got[at].tobytes() == ref[3].tobytes() and got[-1].tobytes() == ref[8].tobytes(), trial


@pytest.mark.parametrize("L,k,d", [(10, 6, 3), (12, 4, 8)])
def test_nothing_outside_the_block_is_written(gp, L, k, d):
    """columns [c0, c1) with c0 > 0 among longer and shorter neighbours; 64 sentinels either side of the output stay, no
    entry inside keeps one, and the values are the reference's tallies folded with the given share"""
    from gkmqc_amd import device as dv
    rng = np.random.default_rng(8)
    svs = [rng.integers(0, 4, size=n, dtype=np.uint8) for n in (150, 80, 2047)]
    queries = _ragged_queries(9, L, (None, None, 37, 600, 211)) + [rng.integers(0, 4, size=2047, dtype=np.uint8)]
    seqs = svs + queries
    pad, sentinel = 64, -7.25
    c0, c1 = len(svs) + 2, len(seqs) - 1
    coef = [0.5, -1.25, 2.0]
    share = np.linspace(1.0, 0.125, d + 1)
    run = _Launcher(dv, (4, L, k, d, 50, 50.0), seqs)
    try:
        out = run.block([0, 1, 2], c0, c1, share, coef, pad, sentinel)
    finally:
        run.close()
    assert (out[:pad] == sentinel).all() and (out[-pad:] == sentinel).all()
    assert not (out[pad:-pad] == sentinel).any()
    for qi, (g, x) in enumerate(zip(_split(out[pad:-pad], seqs[c0:c1], (4,)), seqs[c0:c1])):
        want, bound = 0.0, 0.0
        for cf, s in zip(coef, svs):
            U, B = R.tallies(x, s, 4, L, d)
            raw = HR.raw_from_tallies(x, U, B, share, d)
            want = want + cf * raw
            bound = bound + abs(cf) * raw
        assert (np.abs(g - want) <= 1e-14 * bound).all(), (qi, np.max(np.abs(g - want) - 1e-14 * bound))


def test_cli_on_a_saved_model_equals_the_api(gp, models, tmp_path):
    model = models[2]
    mpath, qpath, opath = str(tmp_path / "m.txt"), str(tmp_path / "q.fa"), str(tmp_path / "h.txt")
    model.save(mpath)
    from gkmqc_amd import synth
    synth.write_fasta(qpath, [b"ACGT" * 5 + b"NNACGGTACCA" * 7, b"GGGTTTACCAGTAC" * 30, b"ACGTACGTACGTAC"], "q")
    r = subprocess.run([sys.executable, "-m", "gkmqc_amd.gkmpredict", "hypothetical", "--block", "2", qpath, mpath,
                        opath], cwd=helpers.ROOT, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    names, got = gp.read_ism(opath)
    want_names, want = gp.hypothetical(gp.load(mpath), qpath)
    assert names == want_names and len(got) == 3
    assert all(a.tobytes() == b.tobytes() for a, b in zip(got, want))


MOTIF = np.array([0, 3, 2, 0, 1, 2, 3, 1, 0, 3, 2, 2], np.uint8)        # ATGACGTCATGG


def _planted(seed, n, length, motif):
    """n random sequences; if motif is given, each carries it (either strand) at a recorded position and strand"""
    rng = np.random.default_rng(seed)
    seqs, at = [], []
    for _ in range(n):
        s = rng.integers(0, 4, size=length, dtype=np.uint8)
        if motif is not None:
            p = int(rng.integers(0, length - len(motif) + 1))
            fwd = bool(rng.random() < 0.5)
            s[p:p + len(motif)] = motif if fwd else (3 - motif)[::-1]
            at.append((p, fwd))
        seqs.append(s)
    return seqs, at


def test_the_motif_base_scores_highest_at_every_motif_position(gp, tmp_path):
    """Trained on 150 + 150 random 200-bp sequences, the positives carrying ATGACGTCATGG: summed over 20 held-out
    positives (in the motif's own frame, reverse-strand copies complemented and mirrored), the motif's base has the
    largest hypothetical score at each of its 12 positions."""
    from gkmqc_amd import synth
    pos, _ = _planted(1, 150, 200, MOTIF)
    neg, _ = _planted(2, 150, 200, None)
    pf, nf = str(tmp_path / "p.fa"), str(tmp_path / "n.fa")
    synth.write_fasta(pf, [gp.codes_to_text(s).encode() for s in pos], "p")
    synth.write_fasta(nf, [gp.codes_to_text(s).encode() for s in neg], "n")
    model = gp.train(pf, nf, kernel_type=4, L=10, k=6, d=3)
    held, at = _planted(3, 20, 200, MOTIF)
    _, Hyp = gp.hypothetical(model, held)
    total = np.zeros((len(MOTIF), 4))
    for h, (p, fwd) in zip(Hyp, at):
        win = h[p:p + len(MOTIF)]
        total += win if fwd else win[::-1, ::-1]             # reverse strand: mirrored positions, complemented bases
    print("summed hypothetical scores over the motif (rows: motif positions, columns A, C, G, T):\n%s" % total)
    assert (np.argmax(total, axis=1) == MOTIF).all(), np.argmax(total, axis=1)
