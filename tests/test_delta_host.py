"""Variant effects without a GPU: allele trimming and the CPU reference (tests/delta_ref.py) against whole-record sums,
the chunk plans, every refusal of gkmpredict.check_delta and of the variant resolver, the variant, delta and saturation
files, and the command line's refusals (gkmqc_amd/gkmpredict.py)."""
import numpy as np
import pytest

from tests import delta_ref as DR


@pytest.fixture(scope="module")
def gp(built):
    from gkmqc_amd import gkmpredict
    return gkmpredict


def _table(gp, L=5, seed=1):
    rng = np.random.default_rng(seed)
    W = rng.standard_normal(4 ** L)
    u = np.arange(4 ** L, dtype=np.uint32)
    W = W + W[gp.lmer_rc(u, L)]
    return gp.LmerTable(W, 4, L, L - 2, 2, 50, 50.0, 0.125)


TRIM_CASES = [
    ((7, "A", "C"), (7, "A", "C")),                    # SNV
    ((7, "ACG", "TCA"), (7, "ACG", "TCA")),            # MNV
    ((7, "ACG", "TTT"), (7, "ACG", "TTT")),
    ((7, "A", "AT"), (8, "", "T")),                    # VCF-style insertion
    ((7, "AT", "A"), (8, "T", "")),                    # VCF-style deletion
    ((7, "A", "A"), (7, "", "")),                      # identical: the suffix goes first, so pos stays
    ((7, "ACGT", "ACGT"), (7, "", "")),
    ((7, "GATTC", "GACTC"), (9, "T", "C")),            # shared prefix and suffix
    ((7, "GAC", "GATTAC"), (8, "", "ATT")),            # the suffix AC goes first, which leaves the prefix G only
    ((7, "AA", "A"), (7, "A", "")),                    # a repeat: suffix first leaves the first base
    ((7, "", "T"), (7, "", "T")),
    ((7, "ac", "aT"), (8, "C", "T")),                  # either case
]


@pytest.mark.parametrize("given,want", TRIM_CASES)
def test_trimming(gp, given, want):
    assert gp.delta_trim(*given) == want
    assert DR.trim(given[0], given[1].upper(), given[2].upper()) == want


def test_reference_delta_against_whole_record_sums(gp):
    """For a random W (L = 5) and a record of 60 bases the delta of a variant equals T(y) - T(x), T the plain sum of W
    over all l-mers of the whole edited / unedited record: the l-mers outside the context are the same in both and
    cancel up to rounding.  Four recursive sums of at most n terms and the subtractions: |error| <= 4 n 2^-53 A, n the
    l-mers of the longer record, A the sum of |W| over both records' l-mers."""
    L = 5
    table = _table(gp, L, seed=11)
    rng = np.random.default_rng(12)
    x = rng.integers(0, 4, size=60).tolist()
    text = "".join("ACGT"[b] for b in x)
    cases = []
    for pos in (0, 1, 4, 5, 30, 55, 56, 59):
        cases.append((pos, text[pos], "ACGT"[(x[pos] + 1) % 4]))                          # SNV
        cases.append((pos, text[pos], text[pos] + "T"))                                   # A -> AT
        cases.append((pos, text[pos], text[pos]))                                         # identical
        if pos + 2 <= 60:
            cases.append((pos, text[pos:pos + 2], text[pos]))                             # AT -> A
        if pos + 3 <= 60:
            cases.append((pos, text[pos:pos + 3], "".join("ACGT"[(b + 2) % 4] for b in x[pos:pos + 3])))   # MNV
        if pos + 5 <= 60:
            cases.append((pos, text[pos:pos + 5], text[pos] + "GG" + text[pos + 3:pos + 5]))    # shared prefix and suffix
    cases += [(60, "", "ACGTACGT"), (0, "", "G"), (10, text[10:50], ""), (0, text, "A")]
    for pos, ref, alt in cases:
        got = DR.delta(table.W, L, x, pos, ref, alt)
        y = DR.edit(x, pos, ref, alt)
        ty, ay = DR.total(table.W, y, L)
        tx, ax = DR.total(table.W, x, L)
        n = max(len(x), len(y)) - L + 1
        assert abs(got - (ty - tx)) <= 4 * n * 2.0 ** -53 * (ax + ay), (pos, ref, alt)
        if DR.trim(pos, ref, alt)[1:] == ("", ""):
            assert got == 0.0 and not np.signbit(got)
        # the production trimming and context agree with the reference's
        p2, r2, a2 = gp.delta_trim(pos, ref, alt)
        a, e = gp.delta_context(len(x), L, p2, len(r2))
        assert got == DR.S(table.W, x[a:p2] + DR.codes_of(a2) + x[p2 + len(r2):e], L) - DR.S(table.W, x[a:e], L)


def test_reference_saturation_is_the_reference_delta_of_every_snv(gp):
    L = 5
    table = _table(gp, L, seed=3)
    x = np.random.default_rng(4).integers(0, 4, size=23).tolist()
    x[9] = 4
    D = DR.saturation(table.W, L, x)
    for t in range(len(x)):
        near = abs(t - 9) < L
        assert np.isnan(D[t]).all() if near else not np.isnan(D[t]).any()
        if near:
            continue
        for b in range(4):
            want = DR.delta(table.W, L, x, t, "ACGT"[x[t]], "ACGT"[b])
            assert D[t, b] == want and np.signbit(D[t, b]) == np.signbit(want)
        assert D[t, x[t]] == 0.0 and not np.signbit(D[t, x[t]])


def _random_variants(rng, T, n):
    pos = np.sort(rng.integers(0, T, size=n))
    rlen = np.minimum(rng.choice([0, 1, 1, 1, 3, 40, 255], size=n), T - pos)
    return pos.astype(np.int64), rlen.astype(np.int64)


@pytest.mark.parametrize("T", [300, 5000])
@pytest.mark.parametrize("L", [2, 10])
def test_chunk_plan(gp, L, T):
    """every variant in exactly one chunk, its context inside that chunk, at the smallest chunk, in between and at one
    larger than the record"""
    rng = np.random.default_rng(T + L)
    pos, rlen = _random_variants(rng, T, 400)
    pos[:3], rlen[:3] = 0, (0, 1, 255)                                      # at the first base
    pos[-2:], rlen[-2:] = (T - 1, T), (1, 0)                                # ending at, and an insertion behind, the last
    a, e = gp.delta_context(T, L, pos, rlen)
    assert (a == np.maximum(0, pos - L + 1)).all() and (e == np.minimum(T, pos + rlen + L - 1)).all()
    counts = []
    for chunk in (gp.delta_min_chunk(L), 1000, T + 1):
        plan = gp.delta_chunk_plan(T, L, pos, rlen, chunk)
        seen = np.zeros(len(pos), dtype=int)
        for v0, v1, b0, b1 in plan:
            assert v0 < v1 and 0 <= b0 < b1 <= T and b1 - b0 <= chunk
            seen[v0:v1] += 1
            assert (a[v0:v1] >= b0).all() and (e[v0:v1] <= b1).all()
            # what the kernel clips inside the chunk is what the record clips
            assert (np.maximum(0, pos[v0:v1] - b0 - (L - 1)) == a[v0:v1] - b0).all()
            assert (np.minimum(b1 - b0, pos[v0:v1] - b0 + rlen[v0:v1] + L - 1) == e[v0:v1] - b0).all()
        assert (seen == 1).all()
        assert [p[0] for p in plan[1:]] == [p[1] for p in plan[:-1]]
        counts.append(len(plan))
    assert counts[0] >= counts[1] >= counts[2] == 1 and counts[0] > 1
    assert gp.delta_chunk_plan(T, L, pos[:0], rlen[:0], 1000) == []
    with pytest.raises(gp.ModelError):
        gp.delta_chunk_plan(T, L, np.array([50]), np.array([255]), 100)


@pytest.mark.parametrize("L,T", [(2, 2), (5, 5), (5, 9), (5, 200), (10, 6000)])
def test_saturation_chunk_plan(gp, L, T):
    for chunk in (gp.delta_min_chunk(L), 1000, T + 1):
        plan = gp.delta_saturation_chunk_plan(T, L, chunk)
        assert plan[0][0] == 0 and plan[-1][1] == T
        assert [p[0] for p in plan[1:]] == [p[1] for p in plan[:-1]]
        for t0, t1, b0, b1 in plan:
            assert t0 < t1 and b1 - b0 <= max(chunk, 2 * L - 1) and b1 - b0 >= L
            assert b0 == max(0, t0 - (L - 1)) and b1 == min(T, t1 + L - 1)
        assert len(plan) == 1 or chunk <= T


def _records(gp):
    x = np.array(DR.codes_of("ACGTTGCAACGTACGTTTGACCA"), dtype=np.uint8)
    valid = np.ones(len(x), dtype=bool)
    valid[5] = False                                                        # (reads G in the code array, N in the file)
    return [("chr1 first", x, valid), ("two", x[:8].copy(), valid[8:16].copy())]


def test_refusals(gp):
    table = _table(gp)
    recs = _records(gp)

    class NotATable:
        kernel_type, L = 4, 5

    for bad in (NotATable(), None, "weights.txt"):
        with pytest.raises(gp.ModelError, match="not a model"):
            gp.check_delta(bad)
    gp.check_delta(table)
    gp.check_delta(table, chunk=gp.delta_min_chunk(5))
    assert gp.delta_min_chunk(5) == 2 * 4 + 255 + 1
    with pytest.raises(gp.ModelError, match="chunk"):
        gp.check_delta(table, chunk=gp.delta_min_chunk(5) - 1)
    ok = [("chr1 first", 0, "A", "C"), (0, 7, "AACG", "A", "rs1"), ("two", 8, "", "T"), ("chr1 first", 4, "TA", "TC")]
    gp.check_delta(table, ok, recs)
    gp.check_delta(table, ok)
    refused = {
        "character": [("two", 1, "C", "N"), ("two", 1, "C", "A-"), ("two", 1, "c*", "A"), ("two", 1, "C", "R")],
        "string": [("two", 1, "C", None), ("two", 1, 1, "A")],
        "position": [("two", -1, "A", "C"), ("two", 1.0, "C", "A"), ("two", "1", "C", "A")],
        "outside": [("two", 8, "A", "C"), ("two", 6, "CAA", "C"), ("two", 9, "", "C")],
        "no such record": [("three", 1, "C", "A"), (2, 1, "C", "A"), (-1, 1, "C", "A")],
        "at most 255": [("two", 1, "C", "C" + "A" * 256), ("two", 1, "", "A" * 256)],
        "variant is": [("two", 1, "C")],
    }
    for what, cases in refused.items():
        for v in cases:
            with pytest.raises(gp.ModelError, match=what):
                gp.check_delta(table, ok + [v], recs)
    for what in ("character", "string", "position", "at most 255", "variant is"):    # ... and without the records
        with pytest.raises(gp.ModelError, match=what):
            gp.check_delta(table, refused[what])
    gp.check_delta(table, [("two", 1, "C", "C" + "A" * 255), ("two", 1, "CG", "C" + "A" * 255 + "G")], recs)   # trimmed to 255
    # an error names the variant
    with pytest.raises(gp.ModelError, match=r"variant 4 \('two', 1, 'C', 'N'\)"):
        gp.check_delta(table, ok + [("two", 1, "C", "N")], recs)


def test_reference_allele_must_match_the_record(gp):
    from gkmqc_amd.gkmdelta import _resolve_variants
    recs = _records(gp)
    rec, pos, rlen, alts = _resolve_variants(recs, [("chr1 first", 7, "AACG", "A"), (0, 4, "TTC", "TTA"),
                                                   ("chr1 first", 5, "A", "T"), ("two", 8, "", "ac")])
    assert rec.tolist() == [0, 0, 0, 1] and pos.tolist() == [8, 6, 5, 8] and rlen.tolist() == [3, 1, 1, 0]
    assert alts == [b"", b"\x00", b"\x03", b"\x00\x01"]                     # base 5 is invalid: any allele matches there
    with pytest.raises(gp.ModelError, match=r"variant 1 \('chr1 first', 7, 'AAGG', 'A'\).*does not match.*AACG"):
        _resolve_variants(recs, [("two", 0, "A", "C"), ("chr1 first", 7, "AAGG", "A")])
    with pytest.raises(gp.ModelError, match="does not match"):
        _resolve_variants(recs, [("chr1 first", 0, "C", "C")])
    gp.check_delta(_table(gp), [("chr1 first", 0, "C", "C")], recs)        # (not check_delta's: it reads no bases)


def test_variant_file(gp, tmp_path):
    path = str(tmp_path / "v.tsv")
    with open(path, "w") as f:
        f.write("# name\tpos\tref\talt\tid\n")
        f.write("chr1 first\t1\tA\tC\n")
        f.write("\n")
        f.write("two\t9\t.\tT\trs2\r\n")
        f.write("#two\t9\t.\tT\trs2\n")
        f.write("two\t3\tGT\t-\n")
        f.write("chr1 first\t8\tAACG\tA\tindel 1")
    got = gp.read_variants(path)
    assert got == [("chr1 first", 0, "A", "C"), ("two", 8, "", "T", "rs2"), ("two", 2, "GT", ""),
                   ("chr1 first", 7, "AACG", "A", "indel 1")]
    for bad in ("two\t0\tA\tC\n", "two\tx\tA\tC\n", "two\t1\tA\n", "two\t1\tA\tC\tid\textra\n", "two 1 A C\n"):
        with open(path, "w") as f:
            f.write("two\t1\tA\tC\n" + bad)
        with pytest.raises(gp.ModelError, match="v.tsv:2"):
            gp.read_variants(path)


def test_delta_file_round_trip_keeps_nan_rows(gp, tmp_path):
    path = str(tmp_path / "d.tsv")
    variants = [("chr1 first", 0, "A", "C"), ("two", 8, "", "T", "rs2"), ("two", 2, "GT", ""), (1, 3, "T", "G", "x")]
    values = np.array([0.1, float("nan"), -1.0 / 3.0, 0.0])
    gp.write_delta(path, variants, values)
    lines = open(path).read().split("\n")
    assert lines[-1] == "" and len(lines) == 5
    assert lines[0] == "chr1 first\t1\tA\tC\t%.17g" % 0.1 and lines[1] == "two\t9\t.\tT\trs2\tnan"
    assert lines[2].startswith("two\t3\tGT\t.\t-0.3333") and lines[3] == "1\t4\tT\tG\tx\t0"
    back, got = gp.read_delta(path)
    assert back == variants[:3] + [("1", 3, "T", "G", "x")]
    assert got.dtype == np.float64 and np.isnan(got[1]) and got[[0, 2, 3]].tobytes() == values[[0, 2, 3]].tobytes()


def test_saturation_file_round_trip_omits_nan_rows(gp, tmp_path):
    path = str(tmp_path / "s.tsv")
    rng = np.random.default_rng(2)
    x = np.array(DR.codes_of("ACGTTGCA"), dtype=np.uint8)
    y = np.array([0, 1, 4, 3], dtype=np.uint8)
    D1, D2 = rng.standard_normal((8, 4)), rng.standard_normal((4, 4))
    D1[np.arange(8), x] = 0.0
    D1[[0, 5]] = np.nan
    D2[1:] = np.nan
    assert gp.write_saturation(path, [("seq0", D1), ("seq1", D2)], [x, y]) == 5
    rows = gp.read_saturation(path)
    assert [(r[0], r[1], r[2]) for r in rows] == [("seq0", t, "ACGTTGCA"[t]) for t in (1, 2, 3, 4, 6, 7)] + [("seq1", 0, "A")]
    assert np.array([r[3] for r in rows]).tobytes() == np.concatenate((D1[[1, 2, 3, 4, 6, 7]], D2[:1])).tobytes()
    first = open(path).read().split("\n")[0].split("\t")
    assert first[:3] == ["seq0", "2", "C"] and first[3:] == ["%.17g" % v for v in D1[1]]


def test_api_refuses_before_it_touches_the_device(gp):
    """a model in place of a table, a small chunk, a bad variant and a short record are refused without a GPU"""
    table = _table(gp)
    x = np.array(DR.codes_of("ACGTTGCAACGT"), dtype=np.uint8)
    with pytest.raises(gp.ModelError, match="not a model"):
        gp.delta(object(), [x], [(0, 0, "A", "C")])
    with pytest.raises(gp.ModelError, match="not a model"):
        gp.delta_saturation(object(), [x])
    with pytest.raises(gp.ModelError, match="chunk"):
        gp.delta(table, [x], [(0, 0, "A", "C")], chunk=100)
    with pytest.raises(gp.ModelError, match="chunk"):
        gp.delta_saturation(table, [x], chunk=100)
    with pytest.raises(gp.ModelError, match="does not match"):
        gp.delta(table, [x], [(0, 0, "C", "A")])
    with pytest.raises(gp.ModelError, match="no such record"):
        gp.delta(table, [x], [("seq1", 0, "A", "C")])
    with pytest.raises(gp.ModelError, match="fewer than L"):
        gp.delta_saturation(table, [x, x[:4]])
    assert gp.delta(table, [x], []).shape == (0,)


def test_command_line_refusals(gp, tmp_path, capsys):
    table = _table(gp)
    weights, fa, var, out = (str(tmp_path / n) for n in ("w.txt", "x.fa", "v.tsv", "o.tsv"))
    table.save(weights)
    with open(fa, "w") as f:
        f.write(">a\nACGTTGCAACGT\n")
    with open(var, "w") as f:
        f.write("a\t1\tC\tA\n")
    assert gp.main(["delta", weights, str(tmp_path / "none.fa"), var, out]) == 1
    assert gp.main(["delta", weights, fa, str(tmp_path / "none.tsv"), out]) == 1
    assert gp.main(["delta", "--chunk", "10", weights, fa, var, out]) == 1
    assert gp.main(["delta", weights, fa, var, out]) == 1                  # the reference allele does not match
    assert "does not match" in capsys.readouterr().err
    assert gp.main(["delta-saturation", "--chunk", "10", weights, fa, out]) == 1
    assert gp.main(["delta-saturation", fa, fa, out]) == 1                 # not a weights file
    import os
    assert not os.path.exists(out) and not os.path.exists(out + ".tmp")
