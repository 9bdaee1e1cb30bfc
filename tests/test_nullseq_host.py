"""Null-sequence generation without a GPU (gkmqc_amd/nullseq.py): the two CPU restatements of the index agree, an index
directory written by the tests loads, every rule of the sampler holds by brute force (shortfalls included), seeds,
the BED and FASTA writers, refusals, and the `sample` command line on a prebuilt directory."""
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import helpers
from tests import nullidx_ref as NR

T, W = 30000, 50


def check_sample(index, positives, negatives, margin_gc, margin_rp):
    """Every rule of nullseq.sample for ONE subset, by brute force.  Returns the number of positives left unmatched."""
    t = index.width
    mg, mr = int(margin_gc * t), int(margin_rp * t)
    assert len(negatives) == len(positives)
    base = np.zeros(256, bool)
    base[list(b"ACGTacgt")] = True
    info = {}
    for chrom in {c for c, _ in positives}:
        raw = index.chrom(chrom).text
        ref = NR.index_vectorised(raw, t)
        key = ref["key"].astype(np.int64)
        bad = np.concatenate(([0], np.cumsum(~base[raw])))
        clean = (bad[t:t + len(key)] - bad[:len(key)]) == 0          # no byte outside ACGTacgt
        info[chrom] = (key, clean, [s for c, s in positives if c == chrom])
    short = 0
    taken = {chrom: [] for chrom in info}          # the negatives of the positives in front, per chromosome
    for (chrom, start), neg in zip(positives, negatives):
        key, clean, pos_here = info[chrom]
        w = index.chrom(chrom).text[start:start + t].tobytes()
        c, r = sum(w.count(x) for x in b"cgCG"), sum(w.count(x) for x in b"acgt")
        kc, kr = np.divmod(key, t + 1)
        adm = (key != NR.NOKEY) & clean & (np.abs(kc - c) <= mg) & (np.abs(kr - r) <= mr)
        i = np.arange(len(key))
        for o in pos_here + taken[chrom]:
            adm &= np.abs(i - o) >= t
        if neg is None:
            short += 1
            assert not adm.any(), "a positive was left unmatched although %d admissible windows remained" % adm.sum()
            continue
        nc, ns = neg
        assert nc == chrom and 0 <= ns < len(key)
        assert adm[ns], "the negative %s:%d breaks a rule" % (nc, ns)
        # nearest first: no admissible window sits in a cell nearer than the one chosen
        dist = np.abs(kc - c) + np.abs(kr - r)
        assert dist[ns] == dist[adm].min()
        taken[chrom].append(ns)
    return short


@pytest.fixture(scope="module")
def genome():
    """two records of 30 000 bases: soft-masked, with N gaps and a few IUPAC bytes"""
    recs = []
    for name, seed in (("chr1", 1), ("chr2", 2)):
        raw = NR.soft_masked(T, seed=seed, n_gaps=3, gap=400)
        rng = np.random.default_rng(seed + 100)
        raw[rng.integers(0, T, 40)] = ord("R")
        recs.append((name, raw))
    return recs


@pytest.fixture(scope="module")
def index_dir(genome, tmp_path_factory):
    d = str(tmp_path_factory.mktemp("nullidx"))
    NR.write_index(d, W, genome)
    return d


@pytest.fixture(scope="module")
def ns():
    from gkmqc_amd import nullseq
    return nullseq


@pytest.fixture(scope="module")
def subsets(genome):
    """about 100 positives in two subsets: one spread over both records, one crowding a stretch of chr1 whose cells are
    rare (all C/G, upper case), so that admissible windows run out"""
    rng = np.random.default_rng(9)
    spread = [("chr1" if i % 2 else "chr2", int(s)) for i, s in enumerate(rng.choice(np.arange(0, T - W, 97), 60, False))]
    crowded = [("chr1", 12000 + 10 * i) for i in range(40)]
    return [spread, crowded]


@pytest.fixture(scope="module")
def crowded_genome(genome, tmp_path_factory):
    """the same genome with a GC-rich island under the crowded subset; few windows elsewhere match it"""
    recs = [(n, r.copy()) for n, r in genome]
    rng = np.random.default_rng(4)
    recs[0][1][11900:12600] = np.frombuffer(b"CG", np.uint8)[rng.integers(0, 2, 700)]
    recs[0][1][20000:20300] = np.frombuffer(b"CG", np.uint8)[rng.integers(0, 2, 300)]   # the only other source
    d = str(tmp_path_factory.mktemp("nullidx_crowded"))
    NR.write_index(d, W, recs)
    return d


def test_the_two_reference_functions_agree():
    rng = np.random.default_rng(0)
    raw = np.frombuffer(b"ACGTacgtNnRr", np.uint8)[rng.choice(12, 900, p=[.12] * 8 + [.005, .005, .015, .015])]
    for t in (1, 2, 7, 64, 200):
        a, b = NR.index_direct(raw, t), NR.index_vectorised(raw, t)
        assert a["len"] == b["len"]
        for name in ("key", "pos", "ptr", "na", "cg", "rp"):
            assert a[name].tobytes() == b[name].tobytes(), (t, name)
    for T_ in (6, 7, 8):
        a, b = NR.index_direct(raw[:T_], 7), NR.index_vectorised(raw[:T_], 7)
        assert a["len"] == b["len"] and a["pos"].tobytes() == b["pos"].tobytes() and a["ptr"].tobytes() == b["ptr"].tobytes()


def test_a_written_index_loads(ns, genome, index_dir):
    index = ns.load_index(index_dir, W)
    assert index.names == ["chr1", "chr2"]
    for name, raw in genome:
        ref = NR.index_vectorised(raw, W)
        c = index.chrom(name)
        assert isinstance(c.pos, np.memmap)
        assert c.pos.tobytes() == ref["pos"].tobytes() and (c.ptr == ref["ptr"]).all() and c.len == ref["len"]
        assert c.text.tobytes() == raw.tobytes()
        k = int(ref["key"][ref["pos"][5]])
        cell = c.cell(*divmod(k, W + 1))
        assert (np.diff(cell) > 0).all() and (ref["key"][cell] == k).all() and (ref["key"] == k).sum() == len(cell)
        assert c.cell_of(int(ref["pos"][5])) == divmod(k, W + 1)
    assert [n for n, _ in ns.read_genome_fasta(os.path.join(index_dir, "fa", "chr1.fa"))] == ["chr1"]


def test_the_sampler_keeps_its_rules(ns, index_dir, crowded_genome, subsets):
    index = ns.load_index(index_dir, W)
    got = ns.sample(index, subsets, 0.06, 0.06, seed=1)
    assert [len(g) for g in got] == [60, 40]
    assert check_sample(index, subsets[0], got[0], 0.06, 0.06) == 0
    check_sample(index, subsets[1], got[1], 0.06, 0.06)
    crowded = ns.load_index(crowded_genome, W)
    got = ns.sample(crowded, subsets, 0.02, 0.02, seed=1)
    short = check_sample(crowded, subsets[1], got[1], 0.02, 0.02)
    assert 0 < short < 40, "the crowded subset must run out of admissible windows, but not at once"
    check_sample(crowded, subsets[0], got[0], 0.02, 0.02)


def test_seeds(ns, index_dir, subsets):
    index = ns.load_index(index_dir, W)
    a = ns.sample(index, subsets, 0.06, 0.06, seed=3)
    assert a == ns.sample(ns.load_index(index_dir, W), subsets, 0.06, 0.06, seed=3)
    assert a != ns.sample(index, subsets, 0.06, 0.06, seed=4)
    # a subset's result is its own: the subsets behind it do not enter
    assert ns.sample(index, [subsets[0]], 0.06, 0.06, seed=3)[0] == a[0]


def test_writers_round_trip(ns, index_dir, genome, tmp_path):
    index = ns.load_index(index_dir, W)
    sites = [("chr1", 0), ("chr2", 1234), ("chr1", T - W)]
    bed, fa = str(tmp_path / "x.bed"), str(tmp_path / "x.fa")
    ns.write_bed(bed, sites, W)
    assert open(bed).read() == "chr1\t0\t50\nchr2\t1234\t1284\nchr1\t%d\t%d\n" % (T - W, T)
    assert ns.read_bed(bed) == sites
    ns.write_fasta(fa, index, sites)
    lines = open(fa).read().split("\n")
    raw = dict(genome)
    assert lines[0] == ">chr1:1-50" and lines[2] == ">chr2:1235-1284" and lines[4] == ">chr1:%d-%d" % (T - W + 1, T)
    for (chrom, s), text in zip(sites, lines[1::2]):
        assert text == raw[chrom][s:s + W].tobytes().decode().upper()
    with open(bed, "a") as f:
        f.write("# a comment\n\nchr2\t7\t57\tname\n")
    assert ns.read_bed(bed) == sites + [("chr2", 7)]


def test_genome_reader_keeps_case_and_joins_lines(ns, tmp_path):
    p = tmp_path / "g.fa"
    p.write_bytes(b"junk\n>a first\nACgt\r\nnNRr\n\n>b\n>c\tx\nacgtacgtac\ngt")
    got = [(n, r.tobytes()) for n, r in ns.read_genome_fasta(str(p))]
    assert got == [("a", b"ACgtnNRr"), ("b", b""), ("c", b"acgtacgtacgt")]
    (tmp_path / "e.fa").write_bytes(b"no record here\n")
    assert list(ns.read_genome_fasta(str(tmp_path / "e.fa"))) == []


def test_refusals(ns, index_dir, tmp_path):
    from gkmqc_amd import device
    for bad in (0, 2048, -3):
        with pytest.raises(device.GkmError):
            ns.load_index(index_dir, bad)
        with pytest.raises(device.GkmError):
            ns.build_index(str(tmp_path / "none.fa"), str(tmp_path / "o"), bad)
    with pytest.raises(device.GkmError):
        device.nullidx_check(2 ** 31 - 1, 600)
    with pytest.raises(ns.NullseqError):
        ns.load_index(index_dir, W + 1)                      # no such width in the directory
    index = ns.load_index(index_dir, W)
    with pytest.raises(ns.NullseqError):
        ns.sample(index, [[("chrX", 5)]])
    for start in (T - W + 1, -1):
        with pytest.raises(ns.NullseqError):
            ns.sample(index, [[("chr1", start)]])
    assert ns.sample(index, [[("chr1", T - W)]], 0.5, 0.5)[0][0] is not None   # the last full window is a fine positive


def test_cli_sample_on_a_prebuilt_directory(ns, index_dir, subsets, tmp_path):
    pos_bed, neg_bed = str(tmp_path / "pos.bed"), str(tmp_path / "neg.bed")
    pos_fa, neg_fa = str(tmp_path / "pos.fa"), str(tmp_path / "neg.fa")
    ns.write_bed(pos_bed, subsets[0], W)
    env = dict(os.environ, PYTHONPATH=helpers.ROOT)
    cmd = [sys.executable, "-m", "gkmqc_amd.nullseq", "sample", "--width", str(W), "--margin-gc", "0.06", "--margin-rp",
           "0.06", "--seed", "3", index_dir, pos_bed, neg_bed, "--fasta", pos_fa, neg_fa]
    r = subprocess.run(cmd, env=env, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    want = ns.sample(ns.load_index(index_dir, W), [subsets[0]], 0.06, 0.06, seed=3)[0]
    assert ns.read_bed(neg_bed) == [n for n in want if n is not None]
    assert open(neg_fa).read().count(">") == len(ns.read_bed(neg_bed)) and open(pos_fa).read().count(">") == 60
    r = subprocess.run(cmd[:-6] + [index_dir, str(tmp_path / "missing.bed"), neg_bed], env=env, capture_output=True, text=True)
    assert r.returncode == 1 and "error" in r.stderr
