"""Variant effects on the GPU (gkmhip_delta_sat, gkmhip_delta_variants, gkmpredict.delta and delta_saturation): both
kernels against the CPU reference (tests/delta_ref.py) bit for bit, variants of every kind and placement, independence
of the chunking, the order of the variants and the other records, trained tables against gkmhip_lmer_score on the edited
sequences, and the command line from `train` to `delta` and `delta-saturation`."""
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import delta_ref as DR
from tests import helpers

pytestmark = pytest.mark.gpu

POS = os.path.join(helpers.GOLDEN, "motif_pos.fa")
NEG = os.path.join(helpers.GOLDEN, "motif_neg.fa")


@pytest.fixture(scope="module")
def dv(built):
    from gkmqc_amd import device
    return device


@pytest.fixture(scope="module")
def gp(built):
    from gkmqc_amd import gkmpredict
    return gkmpredict


@pytest.fixture(scope="module")
def locus(dv):
    """the golden sequences back to back: 6 000 bases that the trained models have something to say about"""
    pos, _, _, _ = dv.read_fasta(POS)
    neg, _, _, _ = dv.read_fasta(NEG)
    return np.concatenate([pos[i] for i in range(15)] + [neg[i] for i in range(15)])


@pytest.fixture(scope="module")
def tables(gp, tmp_path_factory, dv):
    """{name: LmerTable}: C-SVC models of types 0, 1, 2 and 4, and one epsilon-SVR"""
    out = {"svc%d" % t: gp.lmer_weights(gp.train(POS, NEG, kernel_type=t, L=10, k=6, d=3)) for t in (0, 1, 2, 4)}
    tmp = tmp_path_factory.mktemp("delta")
    fa = str(tmp / "train.fa")
    with open(fa, "w") as f:
        f.write(open(POS).read().rstrip("\n") + "\n" + open(NEG).read())
    seqs, _, _, _ = dv.read_fasta(fa)
    rng = np.random.default_rng(5)
    z = [2.0 * np.mean((np.asarray(s) == 1) | (np.asarray(s) == 2)) + (1.0 if i < 150 else 0.0) + 0.1 * rng.normal()
         for i, s in enumerate(seqs)]
    out["svr4"] = gp.lmer_weights(gp.train_svr(fa, z, kernel_type=4, L=10, k=6, d=3))
    return out


def _random_table(gp, L):
    k = max(1, L - 3)
    return gp.LmerTable(np.random.default_rng(L).standard_normal(4 ** L), 0, L, k, L - k, 50, 50.0, 0.0)


def _record(L, T):
    """T random bases; the records of 200 carry invalid bases at 0, 97 and 199"""
    x = np.random.default_rng(1000 * L + T).integers(0, 4, size=T, dtype=np.uint8)
    if T == 200:
        x[[0, 97, 199]] = 4
    return x


def _same(got, want):
    """bit for bit, NaN where and only where the reference has NaN"""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    nan = np.isnan(want)
    return got.shape == want.shape and np.array_equal(np.isnan(got), nan) and got[~nan].tobytes() == want[~nan].tobytes()


def _text(x):
    return "".join("ACGT"[b] for b in x)


SAT_SHAPES = [(L, T) for L in (2, 5, 8, 10) for T in (L, L + 1, 2 * L - 1, 200)] + [(12, 200)]


@pytest.mark.parametrize("L,T", SAT_SHAPES)
def test_saturation_kernel_against_the_reference(dv, gp, L, T):
    """the whole (T, 4) array equals the reference, NaN rows included; the sign bit of D[t][x_t] is clear; a guard band
    behind the output stays untouched; the launch reports its gathers"""
    import torch
    table = _random_table(gp, L)
    x = _record(L, T)
    want = DR.saturation(table.W, L, x)
    ctx = dv.GramContext(*table.kernel_params()[:4], device=0)
    try:
        stream = torch.cuda.current_stream().cuda_stream
        valid = (x < 4).astype(np.uint8)
        d_x = torch.from_numpy(np.where(x < 4, x, 0).astype(np.uint8)).cuda()
        d_v = torch.from_numpy(valid).cuda()
        nlm = T - L + 1
        lm = torch.empty(nlm, dtype=torch.int32, device="cuda")
        ctx.scan_lmers(d_x.data_ptr(), d_v.data_ptr(), T, lm.data_ptr(), stream)
        W = torch.from_numpy(table.W).cuda()
        out = torch.full((T + 16, 4), -7.0, dtype=torch.float64, device="cuda")
        ctx.delta_sat(lm.data_ptr(), nlm, 0, T, W.data_ptr(), out.data_ptr(), stream)
        torch.cuda.synchronize()
        assert ctx.last_kernel_name() == "k_delta_sat"
        assert ctx.last_comparisons() == 4.0 * L * nlm                      # every l-mer covers L positions
        got = out.cpu().numpy()
        assert (got[T:] == -7.0).all()
        assert _same(got[:T], want), np.nonzero(~(got[:T] == want) & ~np.isnan(want))[0][:5]
        clean = np.flatnonzero(~np.isnan(want).any(axis=1))
        own = got[clean, x[clean]]
        assert (own == 0.0).all() and not np.signbit(own).any()
        assert len(clean) > 0 and (T < 200 or len(clean) < T)
        if T == 200:                                                        # a range of positions inside the words given
            part = torch.full((60 + 1, 4), -7.0, dtype=torch.float64, device="cuda")
            ctx.delta_sat(lm.data_ptr(), nlm, 70, 130, W.data_ptr(), part.data_ptr(), stream)
            torch.cuda.synchronize()
            assert _same(part[:60].cpu().numpy(), want[70:130]) and (part[60] == -7.0).all()
            for t0, t1 in ((-1, 5), (5, 5), (0, T + 1)):
                with pytest.raises(dv.GkmError):
                    ctx.delta_sat(lm.data_ptr(), nlm, t0, t1, W.data_ptr(), out.data_ptr(), stream)
    finally:
        ctx.close()
    # ... and through the public call
    res = gp.delta_saturation(table, [x])
    assert len(res) == 1 and res[0][0] == "seq0" and res[0][1].dtype == np.float64 and _same(res[0][1], want)


def _variant_cases(x, L):
    """MNVs of 2 and 5 bases, insertions of 1, L-1, L, 64 and 255, deletions of 1, L and 40: each at pos = 0 (behind the
    invalid first base of the record), at the first valid base, in the clear, ending at the last base (invalid) and at
    the last valid one, and next to the invalid base in the middle; and VCF-style untrimmed indels"""
    T = len(x)
    rng = np.random.default_rng(77)
    text = _text(np.where(x < 4, x, 0))                                     # (an invalid base matches any allele)
    out = []

    def other(seg):
        return "".join("ACGT"[("ACGT".index(ch) + 1 + i) % 4] for i, ch in enumerate(seg))

    for n in (2, 5):
        for pos in (0, 1, 20, 50, 60, 130, 150, 97 - L - n + 1, 97 - L - n + 2, 98, T - n, T - n - 1):
            out.append((0, pos, text[pos:pos + n], other(text[pos:pos + n])[:n - 1] + "ACGT"[(int(x[pos + n - 1]) + 1) % 4]))
    for n in (1, L - 1, L, 64, 255):
        ins = _text(rng.integers(0, 4, size=n))
        for pos in (0, 1, L - 1, 20, 50, 60, 130, 150, 97 - L + 1, 97 - L + 2, 97, 98, T - 1, T):
            out.append((0, pos, "", ins))
    for n in (1, L, 40):
        for pos in (0, 1, 20, 50, 130, 150, 97 - L - n + 1, 97 - L - n + 2, 96 - n + 1, 98, T - n, T - n - 1):
            out.append((0, pos, text[pos:pos + n], ""))
    # VCF style: the base before the event repeated in both alleles, and a shared suffix as well
    out.append((0, 40, text[40], text[40] + "GATTACA"))
    out.append((0, 40, text[40:44], text[40]))
    out.append((0, 40, text[40:46], text[40:42] + "CC" + text[44:46]))
    out.append((0, T - 2, text[T - 2], text[T - 2] + "T"))
    out.append((0, 120, text[120:125], text[120:125]))
    return out


@pytest.mark.parametrize("L", [2, 5, 10, 12])
def test_variants_against_the_reference(gp, L):
    table = _random_table(gp, L)
    x = _record(L, 200)
    # every SNV of the record is the saturation entry
    D = gp.delta_saturation(table, [x])[0][1]
    text = _text(np.where(x < 4, x, 0))
    snvs = [(0, t, text[t], "ACGT"[b]) for t in range(200) for b in range(4)]
    got = gp.delta(table, [x], snvs).reshape(200, 4)
    own = np.zeros((200, 4), dtype=bool)
    own[np.flatnonzero(x < 4), x[x < 4]] = True                             # (the allele that is there already)
    assert _same(got[~own], D[~own])
    # ... which gives +0.0 in both wherever the map has a row; where the map's row is NaN the variant, whose alleles
    # trim to nothing, has the context of an empty variant, one base shorter on the right (the reference below)
    rows = own & ~np.isnan(D).any(axis=1)[:, None]
    assert rows.sum() > 100 and (got[rows] == 0.0).all() and got[rows].tobytes() == D[rows].tobytes()
    assert _same(got, [[DR.delta(table.W, L, x, t, text[t], "ACGT"[b]) for b in range(4)] for t in range(200)])
    # MNVs, insertions, deletions, untrimmed alleles
    cases = _variant_cases(x, L)
    want = np.array([DR.delta(table.W, L, x, p, r, a) for _, p, r, a in cases])
    seen = []
    got = gp.delta(table, [x], cases, on_chunk=seen.append)
    assert got.dtype == np.float64 and _same(got, want), [cases[i] for i in np.nonzero(~(got == want) & ~np.isnan(want))[0][:5]]
    assert np.isnan(want).sum() > 10 and (~np.isnan(want)).sum() > 40
    assert want[-1] == 0.0 and not np.signbit(got[-1])
    assert len(seen) == 1 and seen[0]["kernel"] == "k_delta_variants" and seen[0]["variants"] == len(cases)
    gathers = 0
    for _, p, r, a in cases:
        p, r, a = DR.trim(p, r, a)
        lo, hi = max(0, p - (L - 1)), min(200, p + len(r) + L - 1)
        gathers += max(0, hi - lo - L + 1) + max(0, hi - lo - len(r) + len(a) - L + 1)
    assert seen[0]["gathers"] == gathers


def test_short_records_and_device_layer_refusals(dv, gp):
    """a record shorter than L has no l-mer words: its insertions still have a value; the launch refuses a variant
    outside the bases or alternate bases given"""
    import torch
    table = _random_table(gp, 5)
    x = np.array([0, 1, 2], dtype=np.uint8)
    cases = [(0, 0, "", "ACGTACG"), (0, 3, "", "TTTTT"), (0, 1, "C", "CGGGGG"), (0, 0, "ACG", "T"), (0, 1, "C", "G")]
    want = np.array([DR.delta(table.W, 5, x, p, r, a) for _, p, r, a in cases])
    assert (want[:3] != 0.0).all() and (want[3:] == 0.0).all()
    assert _same(gp.delta(table, [x], cases), want)
    ctx = dv.GramContext(*table.kernel_params()[:4], device=0)
    try:
        codes = torch.zeros(100, dtype=torch.uint8, device="cuda")
        lm = torch.zeros(96, dtype=torch.int32, device="cuda")
        W = torch.from_numpy(table.W).cuda()
        out = torch.zeros(4, dtype=torch.float64, device="cuda")
        alt = np.zeros(10, dtype=np.uint8)
        for var in ([[100, 1, 0, 1]], [[-1, 1, 0, 1]], [[0, 1, 0, 1], [98, 3, 0, 1]], [[5, 1, 8, 3]], [[5, 1, -1, 3]],
                    [[5, 256, 0, 1]], [[5, -1, 0, 1]], [[5, 1, 0, -1]]):
            with pytest.raises(dv.GkmError, match="variant %d" % (len(var) - 1)):
                ctx.delta_variants(lm.data_ptr(), codes.data_ptr(), 100, var, alt, W.data_ptr(), out.data_ptr())
        with pytest.raises(dv.GkmError):
            ctx.delta_variants(None, codes.data_ptr(), 100, [[5, 1, 0, 1]], alt, W.data_ptr(), out.data_ptr())
        ctx.delta_variants(lm.data_ptr(), codes.data_ptr(), 100, [[99, 1, 7, 3], [100, 0, 0, 10], [0, 0, 10, 0]], alt, W.data_ptr(), out.data_ptr())
        torch.cuda.synchronize()
        assert np.isfinite(out.cpu().numpy()).all()
    finally:
        ctx.close()


def _mixed_variants(x, n, seed):
    """n variants over a record without invalid bases: SNVs, MNVs, insertions and deletions, some VCF style"""
    rng = np.random.default_rng(seed)
    text = _text(x)
    out = []
    for i in range(n):
        kind = i % 6
        pos = int(rng.integers(0, len(x) - 50))
        if kind == 0:
            out.append((pos, text[pos], "ACGT"[(int(x[pos]) + 1 + i % 3) % 4]))
        elif kind == 1:
            m = int(rng.integers(2, 6))
            out.append((pos, text[pos:pos + m], _text((x[pos:pos + m] + 1 + rng.integers(0, 3, size=m)) % 4)))
        elif kind == 2:
            out.append((pos, "", _text(rng.integers(0, 4, size=int(rng.choice([1, 3, 9, 10, 64, 255]))))))
        elif kind == 3:
            m = int(rng.choice([1, 2, 10, 40]))
            out.append((pos, text[pos:pos + m], ""))
        elif kind == 4:
            out.append((pos, text[pos], text[pos] + _text(rng.integers(0, 4, size=int(rng.integers(1, 8))))))
        else:
            out.append((pos, text[pos:pos + int(rng.integers(2, 12))], text[pos]))
    out[0] = (0, text[0], "ACGT"[(int(x[0]) + 1) % 4])
    out[1] = (len(x), "", "ACGTTGCA")
    return out


def test_independence(gp, tables, locus):
    """the same 300 variants of the 6 000-base locus: identical arrays at the smallest chunk, at 1 000 bases and at the
    default, with the list shuffled, and with 500 random bases in front as another record; the saturation map likewise
    for the three chunk sizes"""
    table = tables["svc4"]
    L = table.L
    mixed = _mixed_variants(locus, 300, 9)
    variants = [(0,) + v for v in mixed]
    whole = gp.delta(table, [locus], variants)
    assert np.isfinite(whole).all() and (whole != 0.0).sum() > 250
    chunks_seen = []
    for chunk in (gp.delta_min_chunk(L), 1000, None):
        seen = []
        got = gp.delta(table, [locus], variants, chunk=chunk, on_chunk=seen.append)
        assert got.tobytes() == whole.tobytes(), chunk
        assert sum(c["variants"] for c in seen) == 300 and all(c["kernel"] == "k_delta_variants" for c in seen)
        chunks_seen.append(len(seen))
    assert chunks_seen[0] > chunks_seen[1] > chunks_seen[2] == 1
    order = np.random.default_rng(1).permutation(300)
    got = gp.delta(table, [locus], [variants[i] for i in order], chunk=1000)
    assert got.tobytes() == whole[order].tobytes()
    other = np.random.default_rng(8).integers(0, 4, size=500, dtype=np.uint8)
    behind = [(1,) + v for v in mixed] + [(0, 10, _text(other[10:12]), "")]
    got = gp.delta(table, [other, locus], behind, chunk=1000)
    assert got[:300].tobytes() == whole.tobytes() and np.isfinite(got[300])
    got = gp.delta(table, [other, locus], [("seq1",) + v for v in mixed])  # ... and by name
    assert got.tobytes() == whole.tobytes()
    sat = gp.delta_saturation(table, [locus])[0][1]
    assert sat.shape == (6000, 4) and np.isfinite(sat).all()
    counts = []
    for chunk in (gp.delta_min_chunk(L), 1000, None):
        seen = []
        res = gp.delta_saturation(table, [other, locus], chunk=chunk, on_chunk=seen.append)
        assert [r[0] for r in res] == ["seq0", "seq1"] and res[1][1].tobytes() == sat.tobytes(), chunk
        assert sum(c["positions"] for c in seen) == 6500 and all(c["kernel"] == "k_delta_sat" for c in seen)
        counts.append(len(seen))
    assert counts[0] > counts[1] > counts[2] == 2
    # the SNVs among the variants are entries of the map
    for (pos, ref, alt), v in zip(mixed, whole):
        if len(ref) == 1 and len(alt) == 1:
            assert v.tobytes() == sat[pos, "ACGT".index(alt)].tobytes()


@pytest.mark.parametrize("name", ["svc0", "svc1", "svc2", "svc4", "svr4"])
def test_trained_tables(dv, gp, tables, locus, name):
    """20 variants in 40-base sequences, bit for bit against the reference.  For the types without positional weights (0,
    1, 2) also against T(y) - T(x), both T from gkmhip_lmer_score on the whole edited and unedited sequences: the l-mers
    outside a variant's context are in both and cancel up to rounding -- four sums of at most n terms in whatever order
    and the subtractions, |error| <= 4 n 2^-53 A, n the l-mers of the longer sequence, A the sum of |W| over both
    sequences' l-mers."""
    import torch
    table = tables[name]
    L = table.L
    rng = np.random.default_rng(21)
    xs, ys, variants = [], [], []
    for i in range(20):
        a = int(rng.integers(0, len(locus) - 40))
        x = locus[a:a + 40]
        text, pos, kind = _text(x), int(rng.integers(0, 30)), i % 4
        if kind == 0:
            ref, alt = text[pos], "ACGT"[(int(x[pos]) + 1 + i % 3) % 4]
        elif kind == 1:
            m = int(rng.integers(2, 6))
            ref, alt = text[pos:pos + m], _text((x[pos:pos + m] + 1 + rng.integers(0, 3, size=m)) % 4)
        elif kind == 2:                                                     # VCF-style insertion and deletion
            ref, alt = text[pos], text[pos] + _text(rng.integers(0, 4, size=int(rng.integers(1, 7))))
        else:
            ref, alt = text[pos:pos + int(rng.integers(2, 7))], text[pos]
        xs.append(x)
        ys.append(np.array(DR.edit(x, pos, ref, alt), dtype=np.uint8))
        variants.append((i, pos, ref, alt))
    got = gp.delta(table, xs, variants)
    want = np.array([DR.delta(table.W, L, xs[i], p, r, a) for i, p, r, a in variants])
    assert _same(got, want) and np.isfinite(got).all() and (got != 0.0).all()
    if name not in ("svc0", "svc1", "svc2"):
        return
    ctx = dv.GramContext(*table.kernel_params()[:4], device=0)
    try:
        stream = torch.cuda.current_stream().cuda_stream
        ctx.set_sequences(xs + ys, stream)
        W = torch.from_numpy(table.W).cuda()
        T = torch.empty(40, dtype=torch.float64, device="cuda")
        ctx.lmer_score(0, 40, W.data_ptr(), T.data_ptr(), stream)
        T = T.cpu().numpy()
    finally:
        ctx.close()
    for i in range(20):
        n = max(len(xs[i]), len(ys[i])) - L + 1
        A = DR.total(table.W, xs[i], L)[1] + DR.total(table.W, ys[i], L)[1]
        err, bound = abs(got[i] - (T[20 + i] - T[i])), 4 * n * 2.0 ** -53 * A
        print("%s variant %d: |delta - (T(y) - T(x))| = %.3g, bound %.3g" % (name, i, err, bound))
        assert err <= bound, (variants[i], err, bound)


def test_command_line_from_train_to_delta(gp, locus, tmp_path):
    model, weights, fa = str(tmp_path / "m.txt"), str(tmp_path / "w.txt"), str(tmp_path / "s.fa")
    var, out, sat = str(tmp_path / "v.tsv"), str(tmp_path / "d.tsv"), str(tmp_path / "sat.tsv")
    x = locus[:1500].copy()
    text = np.frombuffer(gp.codes_to_text(x).encode(), dtype=np.uint8).copy()
    text[[300, 1499]] = ord("N")
    text[600:700] |= 0x20                                                   # lower case counts as upper case
    body = text.tobytes().decode()
    with open(fa, "w") as f:
        f.write(">chrT test locus\n" + "\n".join(body[i:i + 60] for i in range(0, 1500, 60)) + "\n>tiny\nACGTACGTACGT\n")
    mixed = _mixed_variants(x[:1400], 40, 4)[2:] + [(295, gp.codes_to_text(x[295:297]), "T"), (1495, "", "GG")]
    variants = [("chrT test locus", p, r, a) + (("id%d" % i,) if i % 2 else ()) for i, (p, r, a) in enumerate(mixed)]
    variants.append(("tiny", 4, "A", "AT", "last"))
    with open(var, "w") as f:
        f.write("# name\tpos\tref\talt\tid\n")
        f.write("".join("\t".join([v[0], str(v[1] + 1), v[2] or ".", v[3] or "."] + list(v[4:])) + "\n" for v in variants))

    def run(*args):
        r = subprocess.run([sys.executable, "-m", "gkmqc_amd.gkmpredict"] + list(args), cwd=helpers.ROOT,
                           capture_output=True, text=True)
        assert r.returncode == 0, (args, r.stderr)
        return r

    run("train", "-t", "4", "-L", "10", "-k", "6", "-d", "3", POS, NEG, model)
    run("weights", model, weights)
    r = run("delta", "--chunk", "500", weights, fa, var, out)
    table = gp.load_lmer_table(weights)
    assert gp.read_variants(var) == variants
    want = gp.delta(table, fa, variants)
    nan = int(np.isnan(want).sum())
    assert nan >= 2 and "%d variants scored, %d over a non-ACGT character (nan)" % (len(variants) - nan, nan) in r.stderr
    back, got = gp.read_delta(out)
    assert back == variants and _same(got, want)
    r = run("delta-saturation", "--chunk", "500", weights, fa, sat)
    res = gp.delta_saturation(table, fa)
    assert [n for n, _ in res] == ["chrT test locus", "tiny"] and [len(D) for _, D in res] == [1500, 12]
    left_out = sum(int(np.isnan(D).any(axis=1).sum()) for _, D in res)
    assert left_out == 19 + 10
    assert "%d positions scored, %d near a non-ACGT character left out" % (1512 - left_out, left_out) in r.stderr
    rows = gp.read_saturation(sat)
    keep = [(n, t) for n, D in res for t in np.flatnonzero(~np.isnan(D).any(axis=1)).tolist()]
    assert [(r[0], r[1]) for r in rows] == keep
    upper = body.upper()
    assert all(r[2] == (upper[r[1]] if r[0] != "tiny" else "ACGTACGTACGT"[r[1]]) for r in rows)
    flat = {n: D for n, D in res}
    assert np.array([r[3] for r in rows]).tobytes() == np.array([flat[n][t] for n, t in keep]).tobytes()
