"""The genome window index on the GPU (gkmhip_nullidx_keys, gkmhip_nullidx_cells, gkmhip_nullidx_sort through
device.nullidx_build): key, pos, ptr, len and the three bit planes against the CPU restatement of tests/nullidx_ref.py byte
for byte, at the sizes where the kernels change path (window widths around a lane and a wave, T around multiples of the
tile, one cell over many sort blocks, the highest key), with N and other odd bytes, twice for determinism, and from a
genome FASTA to a trained model through the command line."""
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import helpers
from tests import nullidx_ref as NR
from tests.test_nullseq_host import check_sample

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dv(built):
    from gkmqc_amd import device
    return device


def _same(got, ref, what=""):
    assert got["len"] == ref["len"], what
    for name in ("key", "pos", "ptr", "na", "cg", "rp"):
        assert got[name].dtype == ref[name].dtype and got[name].shape == ref[name].shape, (what, name)
        assert got[name].tobytes() == ref[name].tobytes(), (what, name)


def _check(dv, raw, t, direct=False, what=""):
    raw = NR.as_bytes(raw)
    got = dv.nullidx_build(raw, t)
    _same(got, (NR.index_direct if direct else NR.index_vectorised)(raw, t), what or "T=%d t=%d" % (len(raw), t))
    return got


@pytest.fixture(scope="module")
def seq5000():
    return NR.soft_masked(5000, seed=11, n_gaps=2, gap=40)


@pytest.mark.parametrize("T", [6, 7, 8])
def test_empty_and_single_window(dv, T):
    """t = 7: T = t - 1 and T = t hold no window (ptr all zero, len 0), T = t + 1 holds one"""
    got = _check(dv, b"ACgTTGCA"[:T], 7, direct=True)
    assert len(got["key"]) == max(0, T - 7)
    if T <= 7:
        assert got["len"] == 0 and not got["ptr"].any() and len(got["pos"]) == 0
    else:
        assert got["len"] == 1 and got["pos"].tolist() == [0]


@pytest.mark.parametrize("t", [1, 2, 7, 63, 64, 65, 600, 2047])
def test_widths_across_lane_and_wave_boundaries(dv, seq5000, t):
    _check(dv, seq5000, t)


def test_small_input_against_the_direct_recount(dv, seq5000):
    _check(dv, seq5000[:700], 7, direct=True)
    _check(dv, seq5000[:700], 64, direct=True)


@pytest.mark.parametrize("k", [1, 3])
def test_tile_edges(dv, k):
    tile, t = dv.nullidx_tile(), 600
    assert tile > 0
    raw = NR.soft_masked(tile * k + t + 1, seed=20 + k, n_gaps=2, gap=300)
    for T in (tile * k - 1, tile * k, tile * k + 1, tile * k + t, tile * k + t + 1):
        _check(dv, raw[:T], t)


def test_a_single_cell_across_many_blocks(dv):
    """one cell holds every window: the sort keeps the starts ascending across its blocks"""
    got = _check(dv, b"A" * 70000, 600)
    assert got["len"] == 70000 - 600 and (np.diff(got["pos"]) == 1).all()


def test_the_highest_key_and_all_key_bits(dv):
    t = 2047
    got = _check(dv, b"g" * 10000, t)
    assert got["len"] == 10000 - t and (got["key"] == (t + 1) ** 2 - 1).all()
    assert got["ptr"][t, t] == 0


def test_n_and_odd_bytes(dv):
    rng = np.random.default_rng(3)
    T, t = 9000, 600
    base = np.frombuffer(b"ACGTacgt", np.uint8)[rng.integers(0, 8, T)]
    cases = {}
    for name, at, what in (("N at base 0", [0], b"N"), ("N at base T - 1", [T - 1], b"N"),
                           ("a run of exactly t", list(range(3000, 3000 + t)), b"N"), ("a lone n", [4321], b"n"),
                           ("R", [100, 5000], b"R"), ("r", [100, 5000], b"r")):
        raw = base.copy()
        raw[at] = what[0]
        cases[name] = raw
    for name, raw in cases.items():
        got = _check(dv, raw, t, what=name)
        if name in ("R", "r"):       # no flag: every window is indexed, and the byte counts as neither C/G nor a repeat
            assert got["len"] == T - t
    mixed = base.copy()
    mixed[[0, 4321, T - 1]] = ord("N")
    mixed[[100, 5000]] = ord("r")
    mixed[[101, 7000]] = ord("Y")
    _check(dv, mixed[:3000], 7, direct=True, what="mixed, against the direct recount")


def test_the_last_start_is_never_indexed(dv):
    """T - t would be the only window with t C/G bytes; its cell stays empty"""
    t = 64
    raw = np.frombuffer(b"A" * 1000 + b"G" * t, np.uint8)
    got = _check(dv, raw, t)
    ref_key = t * (t + 1)
    assert not (got["key"] == ref_key).any()
    assert got["ptr"][t, 0] == got["len"] == len(raw) - t      # nothing under or behind that cell
    assert got["key"].max() == (t - 1) * (t + 1)


@pytest.fixture(scope="module")
def large(dv):
    raw = NR.soft_masked(3000000, seed=7, n_gaps=6, gap=40000)
    return raw, dv.nullidx_build(raw, 600)


def test_a_large_input(dv, large):
    raw, got = large
    ref = NR.index_vectorised(raw, 600)
    _same(got, ref, "3 000 000 bases")
    assert (np.diff(ref["ptr"].ravel()) > 0).sum() > 2000 and 0 < ref["len"] < len(raw) - 600


def test_two_builds_give_identical_bytes(dv, large):
    raw, first = large
    _same(dv.nullidx_build(raw, 600), first, "second build")


def test_refusals_launch_nothing(dv):
    lib = dv.load()
    for T, t in ((100, 0), (100, 2048), (2 ** 31 - 1, 600)):
        assert lib.gkmhip_nullidx_keys(0, None, T, t, None, None, None, None, None) == 2
        assert lib.gkmhip_nullidx_cells(0, None, T, t, None, None, 0, None) == 2
        assert lib.gkmhip_nullidx_sort(0, None, T, t, None, None, 0, None) == 2
        assert lib.gkmhip_nullidx_scratch_bytes(T, t) == -1
    with pytest.raises(dv.GkmError):
        dv.nullidx_build(np.zeros(10, np.uint8), 2048)


def test_from_a_genome_to_a_trained_model(dv, tmp_path):
    """build-index and sample through the command line, then gkmpredict.train on the two FASTA files written"""
    from gkmqc_amd import gkmpredict, nullseq
    rng = np.random.default_rng(17)
    t, motif = 200, np.frombuffer(b"TGACTCAGCA", np.uint8)
    recs, bed = [], []
    for name, T in (("chrA", 90000), ("chrB", 70000), ("chrC", 40000)):
        raw = NR.soft_masked(T, seed=int(rng.integers(1 << 30)), n_gaps=2, gap=500)
        grid = [s for s in range(1000, T - 2000, 1000) if ord("N") not in raw[s:s + t]]
        for s in np.sort(rng.choice(grid, size=20, replace=False)):
            for off in (40, 110):
                raw[s + off:s + off + len(motif)] = motif        # a positive: the genome as it is, with the motif in it
            bed.append((name, int(s)))
        recs.append((name, raw))
    fa = tmp_path / "genome.fa"
    with open(fa, "wb") as f:
        for name, raw in recs:
            f.write(b">" + name.encode() + b" synthetic\n")
            for a in range(0, len(raw), 70):
                f.write(raw[a:a + 70].tobytes() + b"\n")
    pos_bed = tmp_path / "pos.bed"
    nullseq.write_bed(str(pos_bed), bed, t)
    idx, neg_bed = tmp_path / "idx", tmp_path / "neg.bed"
    pos_fa, neg_fa = tmp_path / "pos.fa", tmp_path / "neg.fa"
    env = dict(os.environ, PYTHONPATH=helpers.ROOT)
    for args in (["build-index", "--width", str(t), str(fa), str(idx)],
                 ["sample", "--width", str(t), "--seed", "5", str(idx), str(pos_bed), str(neg_bed),
                  "--fasta", str(pos_fa), str(neg_fa)]):
        r = subprocess.run([sys.executable, "-m", "gkmqc_amd.nullseq"] + args, env=env, capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
    index = nullseq.load_index(str(idx), t)
    for name, raw in recs:                                    # the files are the reference's, byte for byte
        ref = NR.index_vectorised(raw, t)
        c = index.chrom(name)
        assert c.pos.tobytes() == ref["pos"].tobytes() and c.ptr.tobytes() == ref["ptr"].tobytes() and c.len == ref["len"]
        for pl in ("na", "cg", "rp"):
            assert open(idx / "bit" / ("%s.%s.bit" % (name, pl)), "rb").read() == ref[pl].tobytes()
        assert c.text.tobytes() == raw.tobytes()
    neg = nullseq.read_bed(str(neg_bed))
    # the positives are ordinary windows of this genome, so most cells they fall into hold other windows; where one
    # does not, check_sample below verifies that nothing admissible was left
    assert len(bed) == 60 and 45 <= len(neg) <= 60
    again = nullseq.sample(index, [bed], seed=5)[0]
    assert [n for n in again if n is not None] == neg
    check_sample(index, bed, again, 0.02, 0.02)
    model = gkmpredict.train(str(pos_fa), str(neg_fa), kernel_type=2, L=10, k=6, d=3)
    assert model is not None
