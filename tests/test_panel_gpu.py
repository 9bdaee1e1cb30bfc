"""L-mer weight panels on the GPU (gkm_panel.hip, gkmpredict's *_with_panel).  The whole contract is
"column m of a panel result is the single-table result of member m, bit for bit": random panels of every lane split
(n_models 1 .. 64, so mp = 8, 16, 32, 64 with and without padding columns) at L = 5 for an unweighted and a weighted
kernel type, against score_with_table, scan, delta and delta_saturation; a trained panel at gkmQC's shape; the device
layer's guard bands, padding columns, refusals and kernel names; and the command line.

The single-table references of the 64 random members are computed once per kernel type and shared; a panel of n models
holds the first n of them.  A chunk of one window (chunk = W) is Python's loop once per window: where the record has more
than 100 windows it is run for the panel of 9 models only (mp = 16 with padding columns), everywhere else for every
n_models; the chunks of 1000 and 2500 bases run for every n_models."""
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import helpers

pytestmark = pytest.mark.gpu

POS = os.path.join(helpers.GOLDEN, "motif_pos.fa")
NEG = os.path.join(helpers.GOLDEN, "motif_neg.fa")
L = 5
N_MODELS = (1, 2, 3, 8, 9, 17, 33, 64)
TYPES = (0, 4)


@pytest.fixture(scope="module")
def dv(built):
    from gkmqc_amd import device
    return device


@pytest.fixture(scope="module")
def gp(built):
    from gkmqc_amd import gkmpredict
    return gkmpredict


def _same(got, want):
    """bit for bit, NaN where and only where the reference has NaN"""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    nan = np.isnan(want)
    return got.shape == want.shape and np.array_equal(np.isnan(got), nan) and got[~nan].tobytes() == want[~nan].tobytes()


def _random_tables(gp, ktype, n=64, length=L):
    """n tables with W[u] == W[rc(u)], weights of mixed magnitude and sign so that the order of additions shows; d = 1
    keeps hits rare enough at L = 5 for k_scan_profiles, which every scan runs, to stay quick on the long windows"""
    rc = gp.lmer_rc(np.arange(4 ** length, dtype=np.uint32), length)
    out = []
    for m in range(n):
        rng = np.random.default_rng(1000 * ktype + m)
        W = rng.standard_normal(4 ** length) * 10.0 ** rng.integers(-6, 7, size=4 ** length)
        out.append(gp.LmerTable(W + W[rc], ktype, length, length - 1, 1, 50, 50.0, 0.25 * m - 3.0))
    return out


class _Shared:
    """per kernel type: the 64 random members, their panels by size and the single-table references, each made once"""

    def __init__(self, gp):
        self.gp, self.tables, self.panels, self.refs = gp, {}, {}, {}

    def members(self, ktype):
        if ktype not in self.tables:
            self.tables[ktype] = _random_tables(self.gp, ktype)
        return self.tables[ktype]

    def panel(self, ktype, n):
        if (ktype, n) not in self.panels:
            self.panels[ktype, n] = self.gp.LmerPanel(self.members(ktype)[:n])
        return self.panels[ktype, n]

    def ref(self, key, ktype, one):
        """one(table) for each of the 64 members, stacked along a new last axis -> a read-only array"""
        if (key, ktype) not in self.refs:
            a = np.stack([np.asarray(one(t)) for t in self.members(ktype)], axis=-1)
            a.setflags(write=False)
            self.refs[key, ktype] = a
        return self.refs[key, ktype]


@pytest.fixture(scope="module")
def shared(gp):
    return _Shared(gp)


# ------------------------------------------------------------------ score_with_panel
def _queries():
    """1, 2, 63, 64, 65, 128, 129 and 591 l-mers -- the residue and block edges of the 64-way split -- and 2 047 bases"""
    rng = np.random.default_rng(11)
    return [rng.integers(0, 4, size=T, dtype=np.uint8) for T in [n + L - 1 for n in (1, 2, 63, 64, 65, 128, 129, 591)] + [2047]]


@pytest.mark.parametrize("n", N_MODELS)
@pytest.mark.parametrize("ktype", TYPES)
def test_score_columns_equal_score_with_table(gp, shared, ktype, n):
    queries = _queries()
    want = shared.ref("score", ktype, lambda t: gp.score_with_table(t, queries)[1])[:, :n]
    panel = shared.panel(ktype, n)
    seen = []
    names, got = gp.score_with_panel(panel, queries, on_block=seen.append)
    assert names == ["seq%d" % i for i in range(9)] and got.shape == (9, n) and np.isfinite(got).all()
    for m in range(n):
        assert got[:, m].tobytes() == want[:, m].tobytes(), (ktype, n, m)
    assert len(seen) == 1 and seen[0]["kernel"] == "k_panel_score" and seen[0]["models"] == n
    assert seen[0]["lmers"] == float(sum(len(q) - L + 1 for q in queries))           # rows, not rows x models
    for block in (1, 7):
        assert gp.score_with_panel(panel, queries, block=block)[1].tobytes() == got.tobytes(), block


# ------------------------------------------------------------------ scan_with_panel
def _locus():
    x = np.random.default_rng(12).integers(0, 4, size=6000, dtype=np.uint8)
    x[[700, 701, 3999]] = 4
    return x


SCAN_SHAPES = [(L, 1), (L + 1, 1), (L + 63, 7), (L + 64, 1), (600, 10), (2047, 500)]


@pytest.mark.parametrize("W,s", SCAN_SHAPES)
@pytest.mark.parametrize("ktype", TYPES)
def test_scan_columns_equal_scan(gp, shared, ktype, W, s):
    x = _locus()
    other = np.random.default_rng(13).integers(0, 4, size=2100, dtype=np.uint8)
    want = shared.ref(("scan", W, s), ktype, lambda t: gp.scan(t, [x], W, s)[0][2])
    nw = gp.scan_window_count(6000, W, s)
    assert want.shape == (nw, 64) and np.isnan(want).any() and not np.isnan(want).all()
    calls = {chunk: len(gp.scan_chunk_plan(6000, W, s, max(chunk, W))) for chunk in (W, 1000, 2500)}
    for chunk in (1000, 2500):
        seen = []
        gp.scan(shared.members(ktype)[0], [x], W, s, chunk=max(chunk, W), on_chunk=seen.append)
        assert len(seen) == calls[chunk]                                              # scan's own number of chunks
    for n in N_MODELS:
        panel = shared.panel(ktype, n)
        (name, starts, got), = gp.scan_with_panel(panel, [x], W, s)
        assert name == "seq0" and np.array_equal(starts, np.arange(nw) * s) and got.shape == (nw, n)
        for m in range(n):
            assert _same(got[:, m], want[:, m]), (ktype, W, s, n, m)
        assert np.array_equal(np.isnan(got).any(axis=1), np.isnan(got).all(axis=1))   # NaN in every column or in none
        for chunk in (W, 1000, 2500):
            if chunk == W and nw > 100 and n != 9:
                continue
            seen = []
            res = gp.scan_with_panel(panel, [x], W, s, chunk=max(chunk, W), on_chunk=seen.append)
            assert _same(res[0][2], got), (ktype, W, s, n, chunk)
            assert len(seen) == calls[chunk]                                          # not multiplied by n_models
            assert sum(c["windows"] for c in seen) == nw
            assert all(c["kernel"] == "k_scan_profiles" and c["score_kernel"] == "k_panel_scan_score" and
                       c["models"] == n for c in seen)
        behind = gp.scan_with_panel(panel, [other, x], W, s)
        assert len(behind) == 2 and _same(behind[1][2], got)


# ------------------------------------------------------------------ delta_with_panel
def _delta_case(gp):
    """-> (records, variants): SNVs, MNVs, insertions, deletions and VCF-style alleles all over a record of 400 bases with
    invalid characters, at pos 0 and at the last base; a record shorter than L; equal alleles"""
    rng = np.random.default_rng(14)
    x = rng.integers(0, 4, size=400, dtype=np.uint8)
    x[[150, 151, 390]] = 4
    short = np.array([0, 1, 2], dtype=np.uint8)
    text = lambda a, b: gp.codes_to_text(np.where(x[a:b] < 4, x[a:b], 0))
    other = lambda t: "ACGT"[(int(x[t]) + 1 + int(rng.integers(0, 3))) & 3]
    v = []
    for t in [0, 1, 3, 4, 5, 100, 146, 147, 155, 156, 200, 394, 395, 396, 398, 399]:      # SNVs; 147 and 155 over N
        v.append((0, t, text(t, t + 1), other(t)))
    for t, r in [(0, 2), (10, 3), (50, 5), (395, 5), (300, 9), (143, 4)]:                     # MNVs
        v.append((0, t, text(t, t + r), "".join(other(q) for q in range(t, t + r))))
    for t, alt in [(0, "A"), (1, "CG"), (60, "ACGTACGTA"), (400, "T"), (399, "GGG"), (152, "A")]:   # insertions
        v.append((0, t, "", alt))
    for t, r in [(0, 1), (0, 7), (70, 2), (396, 4), (399, 1), (250, 12)]:                     # deletions
        v.append((0, t, text(t, t + r), ""))
    for t in (20, 80, 397):                                                                   # VCF style: shared bases
        v.append((0, t, text(t, t + 1), text(t, t + 1) + "TG"))
        v.append((0, t, text(t, t + 3), text(t, t + 1)))
        v.append((0, t, text(t, t + 3), text(t, t + 1) + other(t + 1) + text(t + 2, t + 3)))
    v += [(0, 30, "", ""), (0, 31, text(31, 32), text(31, 32)), (0, 32, text(32, 36), text(32, 36))]   # equal alleles
    v += [(1, 0, "A", "T"), (1, 2, "G", ""), (1, 1, "", "ACGTACGT"), (1, 3, "", "CCCCCCC")]          # shorter than L
    return [x, short], v


@pytest.mark.parametrize("n", N_MODELS)
@pytest.mark.parametrize("ktype", TYPES)
def test_delta_columns_equal_delta(gp, shared, ktype, n):
    records, variants = _delta_case(gp)
    want = shared.ref("delta", ktype, lambda t: gp.delta(t, records, variants))[:, :n]
    nan = np.isnan(want[:, 0])
    assert 2 <= nan.sum() < len(variants) / 2
    panel = shared.panel(ktype, n)
    seen = []
    got = gp.delta_with_panel(panel, records, variants, on_chunk=seen.append)
    assert got.shape == (len(variants), n)
    for m in range(n):
        assert _same(got[:, m], want[:, m]), (ktype, n, m)
    assert np.array_equal(np.isnan(got).all(axis=1), nan) and np.array_equal(np.isnan(got).any(axis=1), nan)
    equal = [i for i, v in enumerate(variants) if v[2] == v[3]]
    assert len(equal) == 3 and not got[equal].any() and not np.signbit(got[equal]).any()      # +0.0
    assert len(seen) == 2 and all(c["kernel"] == "k_panel_delta_variants" and c["models"] == n for c in seen)
    assert sum(c["variants"] for c in seen) == len(variants)
    order = np.random.default_rng(15).permutation(len(variants))
    shuffled = gp.delta_with_panel(panel, records, [variants[i] for i in order], chunk=300)
    assert _same(shuffled, got[order])
    empty = gp.delta_with_panel(panel, records, [])
    assert empty.shape == (0, n) and empty.dtype == np.float64


# ------------------------------------------------------------------ delta_saturation_with_panel
def _saturation_records():
    rng = np.random.default_rng(16)
    long = rng.integers(0, 4, size=3000, dtype=np.uint8)
    long[[0, 1234, 1236, 2999]] = 4
    return [rng.integers(0, 4, size=L, dtype=np.uint8), rng.integers(0, 4, size=L + 1, dtype=np.uint8), long]


@pytest.mark.parametrize("n", N_MODELS)
@pytest.mark.parametrize("ktype", TYPES)
def test_saturation_columns_equal_delta_saturation(gp, shared, ktype, n):
    records = _saturation_records()
    want = shared.ref("saturation", ktype, lambda t: np.concatenate([D for _, D in gp.delta_saturation(t, records)]))
    panel = shared.panel(ktype, n)
    seen = []
    res = gp.delta_saturation_with_panel(panel, records, on_chunk=seen.append)
    assert [name for name, _ in res] == ["seq0", "seq1", "seq2"]
    assert [D.shape for _, D in res] == [(L, 4, n), (L + 1, 4, n), (3000, 4, n)]
    got = np.concatenate([D for _, D in res])
    for m in range(n):
        assert _same(got[:, :, m], want[:, :, m]), (ktype, n, m)
    assert all(c["kernel"] == "k_panel_delta_sat" and c["models"] == n for c in seen) and len(seen) == 3
    chunked = gp.delta_saturation_with_panel(panel, records, chunk=700)
    assert _same(np.concatenate([D for _, D in chunked]), got)
    # the own-base column is +0.0; D[t, b, m] is delta_with_panel's value of that SNV
    x, D = records[2], res[2][1]
    ok = ~np.isnan(D).any(axis=(1, 2))
    assert 2900 < ok.sum() < 3000 and np.array_equal(ok, ~np.isnan(D).all(axis=(1, 2)))
    own = D[np.flatnonzero(ok), x[ok]]
    assert not own.any() and not np.signbit(own).any()
    snvs = [(2, t, "ACGT"[x[t]] if x[t] < 4 else "A", "ACGT"[b]) for t in range(3000) for b in range(4)]
    S = gp.delta_with_panel(panel, records, snvs).reshape(3000, 4, n)
    mine = np.zeros((3000, 4), dtype=bool)
    mine[np.flatnonzero(x < 4), x[x < 4]] = True                            # (the allele that is there already ...
    assert _same(S[~mine], D[~mine])
    rows = mine & ok[:, None]                                               # ... trims to nothing: delta's N rule differs)
    assert rows.sum() == ok.sum() and S[rows].tobytes() == D[rows].tobytes()


# ------------------------------------------------------------------ a trained panel at gkmQC's shape
@pytest.fixture(scope="module")
def trained(gp, dv, tmp_path_factory):
    """C-SVC at C = 0.1, 1, 10 and one epsilon-SVR: type 4, L = 10, k = 6, d = 3 -> (tables, names)"""
    tables = [gp.lmer_weights(gp.train(POS, NEG, kernel_type=4, L=10, k=6, d=3, C=C)) for C in (0.1, 1.0, 10.0)]
    fa = str(tmp_path_factory.mktemp("panel") / "train.fa")
    with open(fa, "w") as f:
        f.write(open(POS).read().rstrip("\n") + "\n" + open(NEG).read())
    seqs, _, _, _ = dv.read_fasta(fa)
    rng = np.random.default_rng(5)
    z = [2.0 * np.mean((np.asarray(s) == 1) | (np.asarray(s) == 2)) + (1.0 if i < 150 else 0.0) + 0.1 * rng.normal()
         for i, s in enumerate(seqs)]
    tables.append(gp.lmer_weights(gp.train_svr(fa, z, kernel_type=4, L=10, k=6, d=3)))
    return tables, ["c0.1", "c1", "c10", "svr"]


def test_trained_panel_matches_its_members(gp, dv, trained):
    tables, names = trained
    panel = gp.LmerPanel(tables, names)
    pos, _, _, _ = dv.read_fasta(POS)
    neg, _, _, _ = dv.read_fasta(NEG)
    queries = [pos[i] for i in range(6)] + [neg[i] for i in range(6)]
    locus = np.concatenate(queries).copy()
    locus[1000] = 4
    variants = [(0, t, "ACGT"[locus[t]], "ACGT"[(locus[t] + 1 + t % 3) & 3]) for t in range(3, len(locus), 97) if locus[t] < 4]
    variants += [(0, 500, "", "GATTACA"), (0, 900, gp.codes_to_text(locus[900:904]), ""), (0, 995, "", "C")]
    got = [gp.score_with_panel(panel, queries)[1], gp.scan_with_panel(panel, [locus], 600, 10)[0][2],
           gp.delta_with_panel(panel, [locus], variants), gp.delta_saturation_with_panel(panel, [locus[:1200]])[0][1]]
    for m, t in enumerate(tables):
        want = [gp.score_with_table(t, queries)[1], gp.scan(t, [locus], 600, 10)[0][2], gp.delta(t, [locus], variants),
                gp.delta_saturation(t, [locus[:1200]])[0][1]]
        for what, g, w in zip(("score", "scan", "delta", "saturation"), got, want):
            assert _same(g[..., m], w), (what, names[m])
    for what, g in zip(("score", "scan", "delta", "saturation"), got):
        flat = g.reshape(-1, 4)
        flat = flat[~np.isnan(flat).any(axis=1)]
        assert len(flat) > 10 and np.isfinite(flat).all(), what
        for a in range(4):
            for b in range(a):
                assert (flat[:, a] != flat[:, b]).any(), (what, names[a], names[b])
    assert np.isnan(got[1]).any() and np.isnan(got[2][-1]).all() and np.isnan(got[3][1000]).all()


# ------------------------------------------------------------------ the device layer
GUARD = 512
SENTINEL = -7.25


def _guarded(torch, rows, nm):
    """rows x nm doubles with one sentinel row and a guard band behind them"""
    return torch.full((rows * nm + nm + GUARD,), SENTINEL, dtype=torch.float64, device="cuda")


def _untouched(buf, rows, nm):
    tail = buf[rows * nm:].cpu().numpy()
    return (tail == SENTINEL).all()


@pytest.mark.parametrize("nm,ms", [(1, 8), (3, 8), (8, 8), (8, 16), (9, 16), (17, 24), (17, 64), (33, 40), (64, 64), (64, 72)])
def test_device_layer_guards_padding_and_names(dv, gp, shared, nm, ms):
    """every entry through GramContext with padding columns full of NaN: no padded value surfaces, the sentinel row and
    the guard band behind the output stay untouched, the launch reports its kernel and the rows it looked up"""
    import torch
    tables = shared.members(4)[:nm]
    P = np.full((4 ** L, ms), np.nan)
    P[:, :nm] = np.stack([t.W for t in tables], axis=1)
    queries = _queries()[2:6]
    x = _locus()[:900]
    valid = (x < 4)
    W, s = 70, 3
    nwin = gp.scan_window_count(900, W, s)
    var = np.array([[0, 1, 0, 1], [899, 1, 1, 0], [450, 0, 1, 3], [10, 4, 4, 0]], dtype=np.int32)
    alt = np.array([1, 2, 3, 0], dtype=np.uint8)
    ctx = dv.GramContext(*tables[0].kernel_params(), device=0)
    try:
        stream = torch.cuda.current_stream().cuda_stream
        d_P = torch.from_numpy(P).cuda()
        d_W = [torch.from_numpy(t.W).cuda() for t in tables]
        d_x = torch.from_numpy(np.where(valid, x, 0).astype(np.uint8)).cuda()
        d_v = torch.from_numpy(valid.astype(np.uint8)).cuda()
        nlm = 900 - L + 1
        lm = torch.empty(nlm, dtype=torch.int32, device="cuda")
        ctx.scan_lmers(d_x.data_ptr(), d_v.data_ptr(), 900, lm.data_ptr(), stream)
        wt = torch.from_numpy(dv.position_weights(4, W - L + 1, 50, 50.0)).cuda()
        ctx.set_sequences(queries, stream)
        p = lambda t: t.data_ptr()

        def both(rows, per_row, panel_call, single_call, name, count):
            buf = _guarded(torch, rows * per_row, nm)
            panel_call(p(buf))
            torch.cuda.synchronize()
            assert ctx.last_kernel_name() == name and ctx.last_comparisons() == count
            assert _untouched(buf, rows * per_row, nm)
            got = buf[:rows * per_row * nm].cpu().numpy().reshape(rows * per_row, nm)
            one = torch.empty(rows * per_row, dtype=torch.float64, device="cuda")
            for m in range(nm):
                single_call(p(d_W[m]), p(one))
                assert _same(got[:, m], one.cpu().numpy()), (name, m)
            assert ctx.last_comparisons() == count                                        # the counterpart's count
            return got

        both(3, 1, lambda o: ctx.panel_score(1, 4, p(d_P), nm, ms, o, stream),
             lambda w, o: ctx.lmer_score(1, 4, w, o, stream), "k_panel_score", float(64 + 65 + 128))
        both(nwin, 1, lambda o: ctx.panel_scan_score(p(lm), nlm, p(wt), W, s, nwin, p(d_P), nm, ms, o, stream),
             lambda w, o: ctx.scan_score(p(lm), nlm, p(wt), W, s, nwin, w, o, stream), "k_panel_scan_score",
             float(nwin * (W - L + 1)))
        sat = both(300, 4, lambda o: ctx.panel_delta_sat(p(lm), nlm, 600, 900, p(d_P), nm, ms, o, stream),
                   lambda w, o: ctx.delta_sat(p(lm), nlm, 600, 900, w, o, stream), "k_panel_delta_sat",
                   4.0 * (300 * L - sum(range(1, L))))
        assert np.isnan(sat).any() and not np.isnan(sat).all()                            # x[700], x[701] are invalid
        both(4, 1, lambda o: ctx.panel_delta_variants(p(lm), p(d_x), 900, var, alt, p(d_P), nm, ms, o, stream),
             lambda w, o: ctx.delta_variants(p(lm), p(d_x), 900, var, alt, w, o, stream), "k_panel_delta_variants",
             26.0)                                                                        # 2 + 1 + 11 + 12
    finally:
        ctx.close()


def test_device_layer_refusals(dv, gp, shared):
    import torch
    ctx = dv.GramContext(4, L, 3, 2, device=0)
    try:
        P = torch.zeros((4 ** L, 16), dtype=torch.float64, device="cuda")
        out = torch.zeros(4 * 1100 * 16, dtype=torch.float64, device="cuda")
        lm = torch.zeros(1000, dtype=torch.int32, device="cuda")
        codes = torch.zeros(1004, dtype=torch.uint8, device="cuda")
        wt = torch.ones(2047, dtype=torch.uint8, device="cuda")
        ctx.set_sequences(_queries()[:3])
        var, alt = [[5, 1, 0, 1]], np.zeros(10, dtype=np.uint8)
        p = lambda t: t.data_ptr()
        entries = {
            "score": lambda P_, nm, ms: ctx.panel_score(0, 3, P_, nm, ms, p(out)),
            "scan": lambda P_, nm, ms: ctx.panel_scan_score(p(lm), 1000, p(wt), 70, 1, 900, P_, nm, ms, p(out)),
            "sat": lambda P_, nm, ms: ctx.panel_delta_sat(p(lm), 1000, 0, 1004, P_, nm, ms, p(out)),
            "variants": lambda P_, nm, ms: ctx.panel_delta_variants(p(lm), p(codes), 1004, var, alt, P_, nm, ms, p(out)),
        }
        for name, call in entries.items():
            for P_, nm, ms in ((None, 9, 16), (p(P), 0, 16), (p(P), -1, 16), (p(P), 65, 72), (p(P), 9, 8), (p(P), 17, 16),
                               (p(P), 9, 12), (p(P), 9, 17), (p(P), 1, 1), (p(P), 4, 4)):
                with pytest.raises(dv.GkmError):
                    call(P_, nm, ms)
            call(p(P), 9, 16)                                                             # and the good call goes through
            call(p(P), 16, 16)
        # null outputs and inputs
        for call in (lambda: ctx.panel_score(0, 3, p(P), 9, 16, None),
                     lambda: ctx.panel_scan_score(None, 1000, p(wt), 70, 1, 900, p(P), 9, 16, p(out)),
                     lambda: ctx.panel_scan_score(p(lm), 1000, None, 70, 1, 900, p(P), 9, 16, p(out)),
                     lambda: ctx.panel_scan_score(p(lm), 1000, p(wt), 70, 1, 900, p(P), 9, 16, None),
                     lambda: ctx.panel_delta_sat(None, 1000, 0, 1004, p(P), 9, 16, p(out)),
                     lambda: ctx.panel_delta_sat(p(lm), 1000, 0, 1004, p(P), 9, 16, None),
                     lambda: ctx.panel_delta_variants(None, p(codes), 1004, var, alt, p(P), 9, 16, p(out)),
                     lambda: ctx.panel_delta_variants(p(lm), None, 1004, var, alt, p(P), 9, 16, p(out)),
                     lambda: ctx.panel_delta_variants(p(lm), p(codes), 1004, var, alt, p(P), 9, 16, None)):
            with pytest.raises(dv.GkmError):
                call()
        # what the single-table counterparts refuse
        for a, b in ((-1, 2), (2, 2), (3, 2), (0, 4)):
            with pytest.raises(dv.GkmError):
                ctx.panel_score(a, b, p(P), 9, 16, p(out))
        for width, stride, nwin in ((L - 1, 1, 10), (2048, 1, 1), (70, 0, 10), (70, 1, 0), (70, 1, 936), (70, 100, 11)):
            with pytest.raises(dv.GkmError):
                ctx.panel_scan_score(p(lm), 1000, p(wt), width, stride, nwin, p(P), 9, 16, p(out))
        ctx.panel_scan_score(p(lm), 1000, p(wt), 70, 1, 935, p(P), 9, 16, p(out))         # exactly fits
        for nlm, t0, t1 in ((0, 0, 1), (1000, -1, 5), (1000, 5, 5), (1000, 6, 5), (1000, 0, 1005)):
            with pytest.raises(dv.GkmError):
                ctx.panel_delta_sat(p(lm), nlm, t0, t1, p(P), 9, 16, p(out))
        for bad in ([[-1, 1, 0, 1]], [[1004, 1, 0, 1]], [[5, 256, 0, 1]], [[5, 1, 10, 1]], [[5, 1, -1, 1]], [[5, 1, 0, -1]],
                    [[5, -1, 0, 1]], [[5, 1, 0, 1], [5, 1, 8, 3]], []):
            with pytest.raises(dv.GkmError):
                ctx.panel_delta_variants(p(lm), p(codes), 1004, bad, alt, p(P), 9, 16, p(out))
        with pytest.raises(dv.GkmError):
            ctx.panel_delta_variants(p(lm), p(codes), 0, var, alt, p(P), 9, 16, p(out))
        ctx.panel_delta_variants(p(lm), p(codes), 1004, [[1003, 1, 7, 3], [1004, 0, 0, 10], [0, 0, 10, 0]], alt, p(P), 9, 16,
                                 p(out))
        torch.cuda.synchronize()
    finally:
        ctx.close()


# ------------------------------------------------------------------ the command line
def test_command_line_from_train_to_the_panel_commands(gp, tmp_path, capsys):
    m1, m2, w1, w2, pan = (str(tmp_path / n) for n in ("m1.txt", "m2.txt", "low.w.txt", "high.w.txt", "p.npz"))
    qfa, sfa, var = (str(tmp_path / n) for n in ("q.fa", "s.fa", "v.tsv"))
    rng = np.random.default_rng(17)
    x = rng.integers(0, 4, size=1500, dtype=np.uint8)
    body = np.frombuffer(gp.codes_to_text(x).encode(), dtype=np.uint8).copy()
    body[[300, 1499]] = ord("N")
    body[600:700] |= 0x20
    body = body.tobytes().decode()
    with open(sfa, "w") as f:
        f.write(">chrT test locus\n" + "\n".join(body[i:i + 60] for i in range(0, 1500, 60)) + "\n>tiny\nACGTACGTACGT\n")
    with open(qfa, "w") as f:
        f.write("".join(">q%d\n%s\n" % (i, gp.codes_to_text(x[100 * i:100 * i + 40 + 17 * i])) for i in (0, 1, 2, 4, 5)))
    up = body.upper()
    variants = [("chrT test locus", t, up[t], "ACGT"[(x[t] + 1) & 3], "id%d" % t) for t in (0, 50, 298, 640, 1400, 1495)]
    variants += [("chrT test locus", 700, "", "GATT", "ins"), ("chrT test locus", 800, up[800:803], "", "del"),
                 ("tiny", 4, "A", "AT", "last")]
    with open(var, "w") as f:
        f.write("# name\tpos\tref\talt\tid\n")
        f.write("".join("\t".join([v[0], str(v[1] + 1), v[2] or ".", v[3] or ".", v[4]]) + "\n" for v in variants))

    def run(*args):
        capsys.readouterr()
        assert gp.main(list(args)) == 0, (args, capsys.readouterr().err)
        return capsys.readouterr().err

    run("train", "-t", "4", "-L", "6", "-k", "4", "-d", "2", "-C", "0.1", POS, NEG, m1)
    run("train", "-t", "4", "-L", "6", "-k", "4", "-d", "2", "-C", "10", POS, NEG, m2)
    run("weights", m1, w1)
    run("weights", m2, w2)
    # `panel` needs no GPU: as a process of its own
    r = subprocess.run([sys.executable, "-m", "gkmqc_amd.gkmpredict", "panel", pan, w1, w2], cwd=helpers.ROOT,
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    panel = gp.load_lmer_panel(pan)
    assert panel.names == ["low.w.txt", "high.w.txt"] and (panel.L, panel.k, panel.d) == (6, 4, 2)
    singles = []
    for i, w in enumerate((w1, w2)):
        outs = [str(tmp_path / ("%s%d.tsv" % (c, i))) for c in ("predict", "scan", "delta")]
        run("predict-table", qfa, w, outs[0])
        run("scan", "--width", "300", "--stride", "25", sfa, w, outs[1])
        run("delta", w, sfa, var, outs[2])
        singles.append(outs)
    po, so, do = (str(tmp_path / n) for n in ("pp.tsv", "sp.tsv", "dp.tsv"))
    run("predict-panel", qfa, pan, po)
    err = run("scan-panel", "--width", "300", "--stride", "25", "--chunk", "700", sfa, pan, so)
    names, lead, values = gp.read_panel_output(so, 3)
    left_out = gp.scan_window_count(1500, 300, 25) - len(lead)
    assert left_out > 0 and "%d windows scored for 2 models, %d over a non-ACGT character left out" % (len(lead), left_out) in err
    err = run("delta-panel", "--chunk", "600", sfa, var, pan, do)
    assert "%d variants scored for 2 models, 2 over a non-ACGT character (nan)" % (len(variants) - 2) in err

    names, lead, values = gp.read_panel_output(po, 1)
    assert names == ["low.w.txt", "high.w.txt"] and lead == [("q%d" % i,) for i in (0, 1, 2, 4, 5)]
    assert open(po).read().startswith("#name\tlow.w.txt\thigh.w.txt\nq0\t")
    for m in range(2):
        want = np.array([float(line.split("\t")[1]) for line in open(singles[m][0]).read().split("\n")[:-1]])
        assert values[:, m].tobytes() == want.tobytes()
    assert (values[:, 0] != values[:, 1]).all()
    names, lead, values = gp.read_panel_output(so, 3)
    assert names == ["low.w.txt", "high.w.txt"] and open(so).read().startswith("#name\tstart\tend\tlow.w.txt\thigh.w.txt\n")
    for m in range(2):
        rows = gp.read_scan(singles[m][1])
        assert [(r[0], str(r[1]), str(r[2])) for r in rows] == lead
        assert values[:, m].tobytes() == np.array([r[3] for r in rows]).tobytes()
    names, lead, values = gp.read_panel_output(do, 5)
    assert names == ["low.w.txt", "high.w.txt"]
    assert open(do).read().startswith("#name\tpos\tref\talt\tid\tlow.w.txt\thigh.w.txt\n")
    for m in range(2):
        back, want = gp.read_delta(singles[m][2])
        assert back == variants and _same(values[:, m], want)
        assert [(v[0], str(v[1] + 1), v[2] or ".", v[3] or ".", v[4]) for v in back] == lead
    assert np.isnan(values).any(axis=1).sum() == 2
