"""Window alignment without a GPU: the block-wise carry protocol of tests/walign_ref.py against its whole-matrix DP, the
planted cases the GPU tests share (asserted here for the reference alone, on the oracle's K), every refusal of
gkmwindows.window_align and of the command line, the output file, and the two entry points of the device layer that
need no device."""
import os

import numpy as np
import pytest

from tests import walign_ref as R
from tests import wsim_ref as WR

NAN = float("nan")
P = R.PLANT


@pytest.fixture(scope="module")
def gw(built):
    from gkmqc_amd import gkmwindows
    return gkmwindows


@pytest.fixture(scope="module")
def dv(built):
    from gkmqc_amd import device
    return device


def plant_kernel(x, y):
    """the oracle's K of the planted case's parameters (tests/wsim_ref.kernel)"""
    return WR.kernel(x, y, P["width"], P["stride"], P["stride"], P["kernel_type"], P["L"], P["k"], P["d"])


def bases(a, K, orientation):
    """the matched pairs of an R.align result as (x_start, y_start)"""
    return [(i * P["stride"], R.y_index(c, K.shape[1], orientation) * P["stride"]) for i, c in a["pairs"]]


@pytest.mark.parametrize("seed", range(10))
def test_blocks_equal_the_whole_matrix(seed):
    """tie-heavy matrices with NaNs, both orientations, three chunkings, 1 x 1 among them: the same score, end cell and
    every direction byte"""
    rng = np.random.default_rng(seed)
    m, n = (int(v) for v in rng.integers(3, 45, size=2))
    K = np.array([0.0, 0.25, 0.5, 0.75, 1.0, NAN])[rng.integers(0, 6, size=(m, n))]
    for orientation in ("forward", "reverse"):
        whole = R.align(K, 0.5, 0.25, orientation)
        assert whole["score"] > 0 and whole["pairs"] and whole["pairs"][-1] == whole["end"]
        for bx, by in ((7, 5), (1, 1), (13, 40), (m, n)):
            score, end, D = R.align_blocks(K, 0.5, 0.25, orientation, bx, by)
            assert score == whole["score"] and end == whole["end"] and np.array_equal(D, whole["D"]), (orientation, bx, by)
    # the reverse orientation is the forward one of the mirrored columns
    mirrored = R.align(np.ascontiguousarray(K[:, ::-1]), 0.5, 0.25, "forward")
    back = R.align(K, 0.5, 0.25, "reverse")
    assert mirrored["score"] == back["score"] and mirrored["pairs"] == back["pairs"]


def test_ties_and_the_order_of_the_comparisons():
    assert R.cell(0.5, 0.0, 0.0, 0.0, 0.5, 0.25) == (0.0, R.STOP)           # nothing beats 0: STOP
    assert R.cell(1.0, 0.5, 1.25, 1.25, 0.5, 0.25) == (1.0, R.DIAG)         # DIAG = UP = LEFT = 1: the first taken
    assert R.cell(NAN, 9.0, 1.25, 1.25, 0.5, 0.25) == (1.0, R.UP)           # a NaN takes no diagonal step; UP before LEFT
    assert R.cell(NAN, 9.0, 0.0, 1.25, 0.5, 0.25) == (1.0, R.LEFT)
    H = np.array([[0.0, 2.0, 1.0], [2.0, 0.0, 2.0]])
    assert R.best_cell(H) == (2.0, 0, 1) and R.best_cell(np.zeros((2, 2))) == (0.0, -1, -1)
    assert R.better((2.0, 0, 1), (2.0, 1, 0)) and not R.better((2.0, 1, 0), (2.0, 0, 1)) and R.better((2.0, 1, 0), (2.0, 1, 2))
    assert not R.better((0.0, 0, 0), (0.0, -1, -1)) and R.better((1e-300, 5, 5), (0.0, -1, -1))


def test_planted_segment_with_a_deletion():
    """every pair on the two planted diagonals, both present, the deletion bridged by two UP steps, in one path"""
    x, y = R.planted()
    K = plant_kernel(x, y)
    assert K.shape == (65, 55) and not np.isnan(K).any()
    a = R.align(K, P["offset"], P["gap"], "forward")
    pairs = bases(a, K, "forward")
    diagonals = [px - py for px, py in pairs]
    assert len(pairs) >= 25 and set(diagonals) == set(R.PLANT_DIAGONALS) and diagonals == sorted(diagonals)
    steps = [(b[0] - a_[0], b[1] - a_[1]) for a_, b in zip(a["pairs"], a["pairs"][1:])]
    assert sorted(set(steps)) == [(1, 1), (3, 1)] and steps.count((3, 1)) == 1
    assert all(200 - P["width"] < px < 500 and 100 - P["width"] < py < 380 for px, py in pairs)
    assert a["score"] > 8.0 and a["stop"] == (a["pairs"][0][0] - 1, a["pairs"][0][1] - 1)
    assert R.align(K, P["offset"], P["gap"], "reverse")["score"] < 2.0
    assert R.align_both(K, P["offset"], P["gap"])[0] == "forward"
    # nothing reaches the offset: an empty path
    none = R.align(K, 2.0, P["gap"], "forward")
    assert (none["score"], none["end"], none["pairs"]) == (0.0, (-1, -1), []) and not none["D"].any()


def test_planted_reverse_complement():
    x, y = R.planted(reverse=True)
    K = plant_kernel(x, y)
    fwd, rev = R.align(K, P["offset"], P["gap"], "forward"), R.align(K, P["offset"], P["gap"], "reverse")
    assert rev["score"] > 8.0 and fwd["score"] < 2.0 and R.align_both(K, P["offset"], P["gap"])[0] == "reverse"
    pairs = bases(rev, K, "reverse")
    # window [a, a + 60) of x matches y from 520 - a before the deletion and from 540 - a after it
    assert len(pairs) >= 25 and {px + py for px, py in pairs} == {520, 540}
    assert [p[0] for p in pairs] == sorted(p[0] for p in pairs) and [p[1] for p in pairs] == sorted((p[1] for p in pairs), reverse=True)


def test_an_n_run_is_crossed_by_gap_steps():
    x, y = R.planted(n_run=(230, 240))
    K = plant_kernel(x, y)
    dead = np.isnan(K).all(axis=0)
    assert dead.sum() == 6 and np.array_equal(np.isnan(K), np.broadcast_to(dead, K.shape))
    a = R.align(K, P["offset"], P["gap"], "forward")
    pairs = bases(a, K, "forward")
    ys = [py for _, py in pairs]
    assert not any(dead[py // P["stride"]] for py in ys)
    assert min(ys) < 180 - P["stride"] and max(ys) > 230 + P["stride"] and {px - py for px, py in pairs} == set(R.PLANT_DIAGONALS)
    assert (a["D"][:, dead] != R.DIAG).all() and (a["D"][:, dead] == R.LEFT).any()


def test_api_refusals_come_before_any_device_work(gw):
    """(no GPU here: anything that reached the device would fail otherwise)"""
    x, y = np.zeros(100, dtype=np.uint8), np.zeros(90, dtype=np.uint8)
    ok = dict(offset=0.3, gap=0.1)
    cases = [(dict(width=20, kernel_type=4), "position"), (dict(width=20, kernel_type=5), "position"),
             (dict(width=10), "below L"), (dict(width=2048), "above 2047"), (dict(width=20, stride_x=0), "stride"),
             (dict(width=20, stride_y=0), "stride"), (dict(width=95), "record y"), (dict(width=101), "record x"),
             (dict(width=20, gamma=NAN, kernel_type=3), "gamma"), (dict(width=20, chunk=19), "chunk"),
             (dict(width=20, L=11, k=12), "window_align"), (dict(width=20, d=9), "window_align"),
             (dict(width=20, offset=NAN), "offset"), (dict(width=20, offset=float("inf")), "offset"),
             (dict(width=20, offset=None), "offset"), (dict(width=20, gap=None), "gap"), (dict(width=20, gap=-0.1), "gap"),
             (dict(width=20, gap=NAN), "gap"), (dict(width=20, gap=float("inf")), "gap"),
             (dict(width=20, orientation="backward"), "orientation"), (dict(width=20, orientation=None), "orientation"),
             (dict(width=20, trace_bytes=81 * 71 - 1), "larger strides.*path=False.*larger trace_bytes")]
    for kw, msg in cases:
        with pytest.raises(gw.WindowError, match=msg):
            gw.window_align(x, y, **{**ok, **kw})
    with pytest.raises(gw.WindowError, match="one-dimensional"):
        gw.window_align(np.zeros((2, 50), np.uint8), y, 20, **ok)
    with pytest.raises(gw.WindowError, match="trace_bytes"):
        gw.check_window_align(10 ** 6, 10 ** 6, 300, 1, offset=0.3, gap=0.1)       # the default of 2^32 direction bytes
    # and what is served passes: the same pairs without a path, larger strides, a larger budget
    gw.check_window_align(100, 90, 20, offset=0.3, gap=0.0, trace_bytes=81 * 71)
    gw.check_window_align(100, 90, 20, offset=-0.3, gap=0.1, orientation="both", trace_bytes=1, path=False)
    gw.check_window_align(10 ** 6, 10 ** 6, 300, 20, None, 3, 11, 7, 3, 0.5, 0.3, 0.1, "reverse")


def test_best_cells_of_blocks_combine_to_the_best_of_the_whole(gw):
    rng = np.random.default_rng(4)
    H = rng.integers(0, 4, size=(30, 40)).astype(np.float64)                 # few values: the maximum is tied
    assert (H == H.max()).sum() > 5
    best = (0.0, -1, -1)
    for i0 in (20, 0, 10):                                                   # any order of the blocks
        for c0 in (30, 0, 10, 20):
            h, i, c = R.best_cell(H[i0:i0 + 10, c0:c0 + 10])
            if i >= 0 and gw.better_cell((h, i + i0, c + c0), best):
                best = (h, i + i0, c + c0)
    assert best == R.best_cell(H)
    assert not gw.better_cell((0.0, 3, 3), (0.0, -1, -1))


def test_align_file_round_trip(gw, tmp_path):
    r = dict(score=np.pi / 3, orientation="reverse", end=(7, 2), start=(3, 9), x_start=np.array([30, 40, 70], dtype=np.int64),
             y_start=np.array([90, 80, 1 << 40], dtype=np.int64))
    path = str(tmp_path / "a.tsv")
    gw.write_window_align(path, r)
    with open(path) as f:
        lines = f.read().split("\n")
    assert lines[0].split("\t")[:4] == ["#score", "%.17g" % (np.pi / 3), "orientation", "reverse"] and lines[1:] == \
        ["30\t90", "40\t80", "70\t%d" % (1 << 40), ""]
    back = gw.read_window_align(path)
    assert back["score"] == r["score"] and back["orientation"] == "reverse" and back["end"] == (7, 2) and back["start"] == (3, 9)
    assert np.array_equal(back["x_start"], r["x_start"]) and np.array_equal(back["y_start"], r["y_start"])
    empty = dict(score=0.0, orientation="forward", end=(-1, -1), start=(-1, -1), x_start=np.zeros(0, np.int64),
                 y_start=np.zeros(0, np.int64))
    gw.write_window_align(path, empty)
    back = gw.read_window_align(path)
    assert back["score"] == 0.0 and back["end"] == (-1, -1) and len(back["x_start"]) == 0 and back["x_start"].dtype == np.int64
    for text in ("", "1\t2\n", "#score\t1.0\n", lines[0] + "\n30\t90\n", lines[0] + "\n30\t90\n40\tx\n70\t1\n",
                 lines[0].replace("reverse", "both") + "\n30\t90\n40\t80\n70\t1\n"):
        with open(path, "w") as f:
            f.write(text)
        with pytest.raises(gw.WindowError):
            gw.read_window_align(path)


def test_command_line_refusals_exit_1_and_write_nothing(gw, tmp_path, capsys):
    xfa, yfa, two = str(tmp_path / "x.fa"), str(tmp_path / "y.fa"), str(tmp_path / "two.fa")
    with open(xfa, "w") as f:
        f.write(">x\n" + "ACGT" * 10 + "\n")
    with open(yfa, "w") as f:
        f.write(">y\n" + "ACGGT" * 7 + "\n")
    with open(two, "w") as f:
        f.write(">a\n" + "ACGT" * 10 + "\n>b\n" + "ACGT" * 10 + "\n")
    out = str(tmp_path / "o.tsv")
    ok = ["--offset", "0.3", "--gap", "0.1"]
    cases = [(["--width", "10"] + ok + [xfa, yfa, out], "below L"),
             (["--width", "20", "--stride-x", "0"] + ok + [xfa, yfa, out], "stride"),
             (["--width", "20", "--chunk", "10"] + ok + [xfa, yfa, out], "chunk"),
             (["--width", "36"] + ok + [xfa, yfa, out], "record y"),
             (["--width", "20", "-t", "4"] + ok + [xfa, yfa, out], "position"),
             (["--width", "20", "--offset", "nan", "--gap", "0.1", xfa, yfa, out], "offset"),
             (["--width", "20", "--offset", "0.3", "--gap", "-1", xfa, yfa, out], "gap"),
             (["--width", "20", "--offset", "0.3", "--gap", "inf", xfa, yfa, out], "gap"),
             (["--width", "20", "--orientation", "sideways"] + ok + [xfa, yfa, out], "orientation"),
             (["--width", "20"] + ok + [str(tmp_path / "missing.fa"), yfa, out], "cannot read"),
             (["--width", "20"] + ok + [xfa, two, out], "2 records")]
    for args, msg in cases:
        assert gw.main(["align"] + args) == 1, args
        err = capsys.readouterr().err
        assert msg in err and err.startswith("gkmwindows: error: ") and err.count("\n") == 1, args
        assert not os.path.exists(out) and not os.path.exists(out + ".tmp")
    for args in (["--width", "20", xfa, yfa, out], ["--width", "20", "--offset", "0.3", xfa, yfa, out],
                 ["--width", "20", "--gap", "0.3", xfa, yfa, out], ok + [xfa, yfa, out]):
        with pytest.raises(SystemExit):
            gw.main(["align"] + args)                                         # --width, --offset and --gap are required
    with pytest.raises(SystemExit):
        gw.main(["matrix", "--width", "20"] + ok + [xfa, yfa, out])           # and belong to `align` alone


def test_tile_shape_and_scratch_need_no_device(dv):
    r, c = dv.walign_tile()
    assert r == 64 and c >= 64 and c % 8 == 0
    tiles = lambda m, n: ((m + r - 1) // r, (n + c - 1) // c)                 # noqa: E731
    for m, n in ((1, 1), (r, c), (r + 1, c + 1), (4986, 4986), (1 << 20, 1 << 20)):
        tx, ty = tiles(m, n)
        need = dv.walign_scratch_bytes(m, n)
        assert need >= 8 * (tx + 1) * (ty + 1) + 24 * tx * ty and need % 8 == 0
    if (r, c) == (64, 128):
        assert sum(tiles(4986, 4986)) - 1 == 116                              # launches of the measured shape (§5r)
    for m, n in ((0, 5), (5, 0), (-1, 5), ((1 << 20) + 1, 5), (5, (1 << 20) + 1)):
        assert dv.walign_scratch_bytes(m, n) == -1
