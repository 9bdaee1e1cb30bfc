"""Scanning on the GPU (gkmhip_scan_lmers, gkmhip_scan_profiles, gkmhip_scan_score, gkmpredict.scan): exact window
profiles against the oracle's self profiles of the windows cut out, bit identity with score_with_table on the
materialised windows for trained models, independence of the chunking and of what precedes a record, windows over
invalid characters, the comparisons a launch shares between windows, and the command line from `train` to `scan`."""
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import dense_inputs as DI
from tests import helpers
from tests import scan_ref as SR
from tests.window_launch import scan_profiles as _device_profiles

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
    tmp = tmp_path_factory.mktemp("scan")
    fa = str(tmp / "train.fa")
    with open(fa, "w") as f:
        f.write(open(POS).read().rstrip("\n") + "\n" + open(NEG).read())
    seqs, _, _, _ = dv.read_fasta(fa)
    rng = np.random.default_rng(5)
    z = [2.0 * np.mean((np.asarray(s) == 1) | (np.asarray(s) == 2)) + (1.0 if i < 150 else 0.0) + 0.1 * rng.normal()
         for i, s in enumerate(seqs)]
    out["svr4"] = gp.lmer_weights(gp.train_svr(fa, z, kernel_type=4, L=10, k=6, d=3))
    return out


_ORACLE = {}


def _oracle_profiles(x, W, s, t, L, k, d):
    """the oracle's self profile of every window cut out (identical windows looked up once)"""
    out = []
    for _, w in SR.windows(x, W, s):
        key = (t, L, k, d, w.tobytes())
        if key not in _ORACLE:
            _ORACLE[key] = SR.self_profile(w, t, L, k, d)
        out.append(_ORACLE[key])
    return np.array(out, dtype=np.int64).reshape(-1, d + 1)


@pytest.mark.parametrize("t", [0, 4])
@pytest.mark.parametrize("L,d", [(5, 2), (8, 3), (10, 3), (12, 4)])
def test_exact_profiles(dv, t, L, d):
    """every window's profile equals the oracle's P_m(w, w) of the window cut out, for W in {L, L + 1, 64, 600} and
    strides {1, 7, W, W + 3}, on iid bases and on a homopolymer (every forward pair a hit)"""
    k = L - d
    rng = np.random.default_rng(100 * L + d)
    inputs = {"iid": rng.integers(0, 4, size=2500, dtype=np.uint8), "polyA": DI.homopolymer(DI.A, 1300)}
    for name, x in inputs.items():
        for W in (L, L + 1, 64, 600):
            for s in (1, 7, W, W + 3):
                got, _, lm = _device_profiles(dv, t, L, k, d, x, W, s)
                want = _oracle_profiles(x, W, s, t, L, k, d)
                assert got.shape == want.shape and len(want) == (len(x) - W) // s + 1
                assert np.array_equal(got, want), (name, t, L, d, W, s, np.nonzero((got != want).any(axis=1))[0][:5])
                assert np.array_equal(lm, SR.R.pack(x, L))
        assert (_oracle_profiles(inputs["polyA"], 600, 600, t, L, k, d)[:, 0] > 0).all()


def test_lmer_words_flag_every_lmer_over_an_invalid_base(dv):
    rng = np.random.default_rng(3)
    L = 10
    x = rng.integers(0, 4, size=500, dtype=np.uint8)
    valid = np.ones(500, dtype=np.uint8)
    valid[[0, 100, 101, 499]] = 0
    _, _, lm = _device_profiles(dv, 0, L, 6, 3, x, 64, 5, valid)
    flagged = (lm >> 31).astype(bool)
    want = np.array([not valid[p:p + L].all() for p in range(500 - L + 1)])
    assert np.array_equal(flagged, want)
    assert np.array_equal(lm & 0x00FFFFFF, SR.R.pack(x, L))


def _materialised(gp, table, x, W, s):
    wins = [w for _, w in SR.windows(x, W, s)]
    _, want = gp.score_with_table(table, wins)
    return want


@pytest.mark.parametrize("name", ["svc0", "svc1", "svc2", "svc4", "svr4"])
def test_bit_identity_with_score_with_table(gp, tables, locus, name):
    table = tables[name]
    for W, s in ((10, 3), (11, 1), (64, 7), (200, 1), (200, 200), (600, 10), (600, 603), (2047, 500)):
        res = gp.scan(table, [locus], W, s)
        assert len(res) == 1 and res[0][0] == "seq0"
        _, starts, got = res[0]
        assert starts.dtype == np.int64 and starts.tolist() == SR.starts(len(locus), W, s)
        want = _materialised(gp, table, locus, W, s)
        assert got.dtype == np.float64 and np.array_equal(got, want), (name, W, s, np.nonzero(got != want)[0][:5])
        assert np.isfinite(got).all()


def test_scores_against_the_cpu_reference(gp, tables, locus):
    """the definition, window by window on the CPU: the table's gathers and the oracle's profile.  Both sum the same
    n <= 191 products wt[p] W(f_p) in another order, divided by sq >= sqrt(c_0 sum wt^2): an error of a few ulps of
    sum wt |W| / sq <= sqrt(n) max|W| < 14 max|W|; the bound below leaves two orders of magnitude over that."""
    table = tables["svc4"]
    x = locus[:900]
    _, starts, got = gp.scan(table, [x], 200, 50)[0]
    ref = SR.scores(table, x, 200, 50)
    assert starts.tolist() == [a for a, _ in ref]
    want = np.array([v for _, v in ref])
    assert (np.abs(got - want) <= 1e-12 * np.abs(table.W).max() * 200).all()


def test_launch_independence(gp, tables, locus):
    """bit identity across chunk sizes, and for a record scanned alone or behind another"""
    table = tables["svc4"]
    for W, s in ((600, 1), (64, 7), (200, 200)):
        _, _, whole = gp.scan(table, [locus], W, s)[0]
        chunks_seen = []
        for chunk in (W, 1000, 2500):
            seen = []
            _, _, got = gp.scan(table, [locus], W, s, chunk=chunk, on_chunk=seen.append)[0]
            assert got.tobytes() == whole.tobytes(), (W, s, chunk)
            assert sum(c["windows"] for c in seen) == len(whole) and all(c["kernel"] == "k_scan_profiles" for c in seen)
            chunks_seen.append(len(seen))
        assert chunks_seen[0] > chunks_seen[1] > chunks_seen[2] >= 1
    other = np.random.default_rng(8).integers(0, 4, size=1234, dtype=np.uint8)
    short = locus[:50]
    res = gp.scan(table, [other, short, locus], 600, 10)
    assert [r[0] for r in res] == ["seq0", "seq1", "seq2"]
    assert len(res[1][1]) == 0 and len(res[1][2]) == 0                     # shorter than the width: no windows
    alone = gp.scan(table, [locus], 600, 10)[0]
    assert res[2][2].tobytes() == alone[2].tobytes() and np.array_equal(res[2][1], alone[1])


def test_invalid_windows(gp, tables, locus, tmp_path):
    """windows touching an N are NaN, every other window keeps its value, and the written file omits exactly those"""
    table = tables["svc4"]
    W, s = 200, 9
    x = locus[:3000].copy()
    clean = gp.scan(table, [x], W, s)[0][2]
    bad_at = [0, 700, 701, 702, 1999, 2999]
    y = x.copy()
    y[bad_at] = 4
    _, starts, got = gp.scan(table, [y], W, s)[0]
    touched = np.array([any(a <= b < a + W for b in bad_at) for a in starts])
    assert touched.any() and not touched.all()
    assert np.isnan(got[touched]).all()
    assert got[~touched].tobytes() == clean[~touched].tobytes()
    # the same through files: N and lower case in the FASTA, chunked
    text = np.frombuffer(b"ACGT", dtype=np.uint8)[x].copy()
    text[bad_at] = ord("N")
    text[1000:1500] |= 0x20                                                # lower case counts as upper case
    fa, weights, out = str(tmp_path / "x.fa"), str(tmp_path / "w.txt"), str(tmp_path / "o.bedgraph")
    with open(fa, "w") as f:
        body = text.tobytes().decode()
        f.write(">locus one\n" + "\n".join(body[i:i + 60] for i in range(0, len(body), 60)) + "\n>tiny\nACGT\n")
    table.save(weights)
    r = subprocess.run([sys.executable, "-m", "gkmqc_amd.gkmpredict", "scan", "--width", str(W), "--stride", str(s),
                        "--chunk", "777", fa, weights, out], cwd=helpers.ROOT, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert "%d over a non-ACGT character left out" % int(touched.sum()) in r.stderr
    rows = gp.read_scan(out)
    assert [(n, a, b) for n, a, b, _ in rows] == [("locus one", int(a), int(a) + W) for a in starts[~touched]]
    assert np.array([v for _, _, _, v in rows]).tobytes() == clean[~touched].tobytes()


@pytest.mark.parametrize("L,W,s,T", [(10, 600, 1, 3000), (10, 600, 73, 6000), (10, 600, 10, 1230), (5, 64, 7, 600),
                                     (12, 2047, 254, 2047 + 63 * 254)])
def test_shared_comparisons(dv, L, W, s, T):
    """at a stride of at most n / 8 over at least 64 windows a launch compares at most a quarter of the pairs the
    materialised path compares (2 n^2 per window)"""
    n = W - L + 1
    assert 8 * s <= n
    x = np.random.default_rng(T).integers(0, 4, size=T, dtype=np.uint8)
    prof, comparisons, _ = _device_profiles(dv, 0, L, L - 3, 3, x, W, s)
    assert len(prof) >= 64
    assert 0 < comparisons <= 0.25 * 2.0 * n * n * len(prof), (comparisons, 2.0 * n * n * len(prof))
    # disjoint windows: one stretch each, half the band plus the diagonal
    prof, comparisons, _ = _device_profiles(dv, 0, L, L - 3, 3, x[:min(T, 5 * W)], W, W)
    assert comparisons == (n * n + n) * len(prof) <= 2.0 * n * n * len(prof)


def test_group_is_a_function_of_the_shape_only(dv):
    ctx = dv.GramContext(4, 10, 6, 3, device=0)
    try:
        assert ctx.scan_group(600, 1) == 64 and ctx.scan_group(600, 600) == 1 and ctx.scan_group(600, 591) == 1
        assert ctx.scan_group(600, 590) == 6 and ctx.scan_group(2047, 254) == 9
        assert ctx.scan_group(9, 1) == 0 and ctx.scan_group(2048, 1) == 0 and ctx.scan_group(600, 0) == 0
    finally:
        ctx.close()


def test_device_layer_refusals(dv):
    import torch
    ctx = dv.GramContext(4, 10, 6, 3, device=0)
    try:
        lm = torch.zeros(1000, dtype=torch.int32, device="cuda")
        wt = torch.ones(2047, dtype=torch.uint8, device="cuda")
        out = torch.zeros((410, 4), dtype=torch.int64, device="cuda")
        for args in ((9, 1, 10), (2048, 1, 1), (600, 0, 10), (600, 1, 0), (600, 1, 411), (600, 100, 6)):
            with pytest.raises(dv.GkmError):
                ctx.scan_profiles(lm.data_ptr(), 1000, wt.data_ptr(), args[0], args[1], args[2], out.data_ptr())
        ctx.scan_profiles(lm.data_ptr(), 1000, wt.data_ptr(), 600, 1, 410, out.data_ptr())   # exactly fits
        torch.cuda.synchronize()
    finally:
        ctx.close()


def test_command_line_from_train_to_scan(gp, locus, tmp_path):
    model, weights = str(tmp_path / "m.txt"), str(tmp_path / "w.txt")
    fa, out, qfa, qout = str(tmp_path / "s.fa"), str(tmp_path / "o.bedgraph"), str(tmp_path / "q.fa"), str(tmp_path / "q.txt")
    x = locus[:2000]
    with open(fa, "w") as f:
        f.write(">chrT test locus\n%s\n" % gp.codes_to_text(x))
    wins = SR.windows(x, 300, 100)
    with open(qfa, "w") as f:
        f.write("".join(">w%d\n%s\n" % (a, gp.codes_to_text(w)) for a, w in wins))

    def run(*args):
        r = subprocess.run([sys.executable, "-m", "gkmqc_amd.gkmpredict"] + list(args), cwd=helpers.ROOT,
                           capture_output=True, text=True)
        assert r.returncode == 0, (args, r.stderr)
        return r

    run("train", "-t", "4", "-L", "10", "-k", "6", "-d", "3", POS, NEG, model)
    run("weights", model, weights)
    r = run("scan", "--width", "300", "--stride", "100", fa, weights, out)
    assert "18 windows scored, 0 over a non-ACGT character left out" in r.stderr
    run("predict-table", qfa, weights, qout)
    rows = gp.read_scan(out)
    want = [ln.split("\t") for ln in open(qout).read().split("\n")[:-1]]
    assert len(rows) == len(want) == 18
    for (name, a, b, v), (a_w, _), (_, text) in zip(rows, wins, want):
        assert (name, a, b) == ("chrT test locus", a_w, a_w + 300)
        assert np.float64(v).tobytes() == np.float64(float(text)).tobytes()
    for ln in open(out).read().split("\n")[:-1]:
        assert ln.split("\t")[3] == "%.17g" % float(ln.split("\t")[3])
