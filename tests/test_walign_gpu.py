"""Window alignment on the GPU (gkmwindows.window_align over gkmhip_walign_block and gkmhip_walign_trace): the score's
bits and the whole path against the plain-loop reference (tests/walign_ref.py) run on window_kernel's K of the same
call, the planted cases tests/test_walign_host.py asserts for the reference, invalid bases, independence of the chunking,
the score-only run, the trace budget and the command line."""
import subprocess
import sys

import numpy as np
import pytest

from tests import helpers
from tests import walign_ref as R

pytestmark = pytest.mark.gpu

P = R.PLANT
PLANT_ARGS = (P["width"], P["stride"], P["stride"], P["kernel_type"], P["L"], P["k"], P["d"])


@pytest.fixture(scope="module")
def gw(built):
    from gkmqc_amd import gkmwindows
    return gkmwindows


def same_as_reference(got, K, offset, gap, orientation, sx, sy):
    """every field of a window_align result against the reference run on K"""
    name, want = R.align_both(K, offset, gap) if orientation == "both" else (orientation, R.align(K, offset, gap, orientation))
    nB = K.shape[1]
    assert got["orientation"] == name
    assert np.float64(got["score"]).tobytes() == np.float64(want["score"]).tobytes(), (got["score"], want["score"])
    ei, ec = want["end"]
    assert tuple(got["end"]) == ((ei, R.y_index(ec, nB, name)) if ei >= 0 else (-1, -1))
    if "x_index" not in got:
        return want
    xi = [i for i, _ in want["pairs"]]
    yi = [R.y_index(c, nB, name) for _, c in want["pairs"]]
    assert got["x_index"].tolist() == xi and got["y_index"].tolist() == yi
    assert got["x_start"].tolist() == [i * sx for i in xi] and got["y_start"].tolist() == [j * sy for j in yi]
    assert tuple(got["start"]) == ((xi[0], yi[0]) if xi else (-1, -1))
    assert got["x_index"].dtype == got["y_index"].dtype == got["x_start"].dtype == got["y_start"].dtype == np.int64
    return want


@pytest.mark.parametrize("t", [0, 3])
@pytest.mark.parametrize("L,k,d", [(8, 5, 2), (11, 7, 3)])
def test_bit_identity_with_the_reference(gw, t, L, k, d):
    """a diverged copy, a copy of its reverse complement and an N in either record; the offset at K's 0.8 quantile, so
    that a fifth of the window pairs gain and D holds every direction"""
    rng = np.random.default_rng(10 * L + t)
    W, sx, sy = 64, 7, 5
    x, y = rng.integers(0, 4, size=900, dtype=np.uint8), rng.integers(0, 4, size=760, dtype=np.uint8)
    seg = x[100:400].copy()
    hit = rng.random(300) < 0.1
    seg[hit] = (seg[hit] + 1) % 4
    y[50:350] = seg
    y[420:620] = R.complement_reverse(x[600:800])
    x[250] = 4
    y[700] = 4
    gamma = 2.0
    full = gw.window_kernel(x, y, W, sx, sy, t, L, k, d, gamma)
    K = full["K"]
    assert K.shape == (120, 140) and np.isnan(K).any()
    offset = float(np.nanquantile(K, 0.8))
    gap = (float(np.nanmax(K)) - offset) / 4
    scores = {}
    for orientation in ("forward", "reverse", "both"):
        got = gw.window_align(x, y, W, sx, sy, t, L, k, d, gamma, offset, gap, orientation)
        want = same_as_reference(got, K, offset, gap, orientation, sx, sy)
        scores[orientation] = got["score"]
        assert len(got["x_index"]) > 10 and set(np.unique(want["D"])) == {0, 1, 2, 3}
        assert np.array_equal(got["x_valid"], full["x_valid"]) and np.array_equal(got["y_valid"], full["y_valid"])
        assert got["x_valid"][got["x_index"]].all() and got["y_valid"][got["y_index"]].all()
    assert scores["both"] == max(scores["forward"], scores["reverse"]) and scores["forward"] != scores["reverse"]


def test_planted_cases(gw):
    """what tests/test_walign_host.py asserts for the reference on the oracle's K, for window_align"""
    sx = P["stride"]
    x, y = R.planted()
    fwd = gw.window_align(x, y, *PLANT_ARGS, 1.0, P["offset"], P["gap"], "forward")
    K = gw.window_kernel(x, y, *PLANT_ARGS)["K"]
    same_as_reference(fwd, K, P["offset"], P["gap"], "forward", sx, sx)
    diagonals = (fwd["x_start"] - fwd["y_start"]).tolist()
    assert len(diagonals) >= 25 and set(diagonals) == set(R.PLANT_DIAGONALS) and diagonals == sorted(diagonals)
    steps = list(zip(np.diff(fwd["x_index"]).tolist(), np.diff(fwd["y_index"]).tolist()))
    assert sorted(set(steps)) == [(1, 1), (3, 1)] and steps.count((3, 1)) == 1 and fwd["score"] > 8.0
    both = gw.window_align(x, y, *PLANT_ARGS, 1.0, P["offset"], P["gap"], "both")
    assert both["orientation"] == "forward" and both["score"] == fwd["score"] and np.array_equal(both["y_index"], fwd["y_index"])
    assert gw.window_align(x, y, *PLANT_ARGS, 1.0, P["offset"], P["gap"], "reverse")["score"] < 2.0
    # nothing reaches the offset: an empty path
    none = gw.window_align(x, y, *PLANT_ARGS, 1.0, 2.0, P["gap"], "both")
    assert (none["score"], none["orientation"], tuple(none["end"]), tuple(none["start"])) == (0.0, "forward", (-1, -1), (-1, -1))
    assert len(none["x_index"]) == len(none["y_start"]) == 0
    # the reverse complement planted instead
    xr, yr = R.planted(reverse=True)
    Kr = gw.window_kernel(xr, yr, *PLANT_ARGS)["K"]
    rev = gw.window_align(xr, yr, *PLANT_ARGS, 1.0, P["offset"], P["gap"], "both")
    same_as_reference(rev, Kr, P["offset"], P["gap"], "both", sx, sx)
    assert rev["orientation"] == "reverse" and rev["score"] > 8.0
    assert set((rev["x_start"] + rev["y_start"]).tolist()) == {520, 540} and (np.diff(rev["y_index"]) < 0).all()
    assert gw.window_align(xr, yr, *PLANT_ARGS, 1.0, P["offset"], P["gap"], "forward")["score"] < 2.0


def test_invalid_bases_are_crossed_not_matched(gw):
    sx = P["stride"]
    x, y = R.planted(n_run=(230, 240))
    x = x.copy()
    x[640] = 255                                                           # (beyond the planted segment)
    got = gw.window_align(x, y, *PLANT_ARGS, 1.0, P["offset"], P["gap"], "forward")
    full = gw.window_kernel(x, y, *PLANT_ARGS)
    same_as_reference(got, full["K"], P["offset"], P["gap"], "forward", sx, sx)
    assert (~got["y_valid"]).sum() == 6 and (~got["x_valid"]).sum() == 6
    assert np.array_equal(got["x_valid"], full["x_valid"]) and np.array_equal(got["y_valid"], full["y_valid"])
    assert got["y_valid"][got["y_index"]].all() and got["x_valid"][got["x_index"]].all()
    assert got["y_start"].min() < 180 - sx and got["y_start"].max() > 230 + sx
    assert set((got["x_start"] - got["y_start"]).tolist()) == set(R.PLANT_DIAGONALS)


@pytest.mark.parametrize("orientation", ["forward", "reverse"])
def test_chunk_invariance(gw, orientation):
    """one block (3 x 3 DP tiles), 2 x 3 blocks and 3 x 7 blocks whose edges fall inside DP tiles: the same bytes; the
    score-only run agrees on the score and the end"""
    from gkmqc_amd import device as dv
    from gkmqc_amd import gkmpredict as gp
    rng = np.random.default_rng(23)
    W, sx, sy, args = 64, 5, 3, (2, 10, 6, 3, 1.0)
    x, y = rng.integers(0, 4, size=759, dtype=np.uint8), rng.integers(0, 4, size=1621, dtype=np.uint8)
    seg = x[100:600].copy()
    hit = rng.random(500) < 0.12
    seg[hit] = (seg[hit] + 2) % 4
    seg = np.concatenate((seg[:200], rng.integers(0, 4, size=40, dtype=np.uint8), seg[200:]))   # an insertion of 40 bases
    y[300:840] = R.complement_reverse(seg) if orientation == "reverse" else seg
    y[1300] = 4
    K = gw.window_kernel(x, y, W, sx, sy, *args)["K"]
    r, c = dv.walign_tile()
    assert K.shape == (140, 520) and K.shape[0] > 2 * r and K.shape[1] > 2 * c
    offset = float(np.nanquantile(K, 0.85))
    gap = (float(np.nanmax(K)) - offset) / 3
    seen = []
    whole = gw.window_align(x, y, W, sx, sy, *args, offset, gap, orientation, on_chunk=seen.append)
    want = same_as_reference(whole, K, offset, gap, orientation, sx, sy)
    assert len(seen) == 1 and seen[0]["align_kernel_ms"] >= 0 and seen[0]["kernel"] == "k_wsim_profiles"
    assert len(whole["x_index"]) > 40 and {1, 2, 3} <= set(np.unique(want["D"]))
    gaps = set(zip(np.diff(whole["x_index"]).tolist(), np.abs(np.diff(whole["y_index"])).tolist())) - {(1, 1)}
    assert gaps                                                             # the path holds gap steps
    blocks = []
    for chunk in (700, 300):
        px, py = len(gp.scan_chunk_plan(759, W, sx, chunk)), len(gp.scan_chunk_plan(1621, W, sy, chunk))
        blocks.append((px, py))
        seen = []
        got = gw.window_align(x, y, W, sx, sy, *args, offset, gap, orientation, chunk=chunk, on_chunk=seen.append)
        assert len(seen) == px * py and sum(s["x_windows"] * s["y_windows"] for s in seen) == K.size
        assert any(s["y_windows"] % c and s["x_windows"] % r for s in seen)
        assert got.keys() == whole.keys()
        for key in whole:
            a, b = got[key], whole[key]
            assert (a.tobytes() == b.tobytes() and a.dtype == b.dtype) if isinstance(b, np.ndarray) else a == b, (chunk, key)
        assert np.float64(got["score"]).tobytes() == np.float64(whole["score"]).tobytes()
        short = gw.window_align(x, y, W, sx, sy, *args, offset, gap, orientation, chunk=chunk, path=False)
        assert short == dict(score=whole["score"], orientation=orientation, end=whole["end"])
    assert blocks == [(2, 3), (3, 7)]
    short = gw.window_align(x, y, W, sx, sy, *args, offset, gap, "both", path=False, trace_bytes=1)
    assert short == dict(score=whole["score"], orientation=orientation, end=whole["end"])


def test_the_trace_budget_is_checked_before_any_launch(gw):
    x, y = R.planted()
    seen = []
    with pytest.raises(gw.WindowError, match="larger strides.*path=False.*larger trace_bytes"):
        gw.window_align(x, y, *PLANT_ARGS, 1.0, P["offset"], P["gap"], trace_bytes=65 * 55 - 1, on_chunk=seen.append)
    assert not seen
    got = gw.window_align(x, y, *PLANT_ARGS, 1.0, P["offset"], P["gap"], trace_bytes=65 * 55, on_chunk=seen.append)
    assert len(seen) == 1 and got["score"] > 8.0


def test_command_line(gw, tmp_path):
    from gkmqc_amd import gkmpredict as gp
    x, y = R.planted(reverse=True)
    xfa, yfa = str(tmp_path / "x.fa"), str(tmp_path / "y.fa")
    text = gp.codes_to_text(x)
    text = text[:650] + "N" + text[651:]
    with open(xfa, "w") as f:
        f.write(">locus x\n" + "\n".join(text[i:i + 60] for i in range(0, len(text), 60)) + "\n")
    with open(yfa, "w") as f:
        f.write(">locus y\n" + gp.codes_to_text(y).lower() + "\n")
    xn = x.copy()
    xn[650] = 4
    out = str(tmp_path / "a.tsv")
    r = subprocess.run([sys.executable, "-m", "gkmqc_amd.gkmwindows", "align", "--width", str(P["width"]), "--stride-x",
                        str(P["stride"]), "--offset", str(P["offset"]), "--gap", str(P["gap"]), "--orientation", "both",
                        "--chunk", "250", "-t", "0", "-L", str(P["L"]), "-k", str(P["k"]), "-d", str(P["d"]), xfa, yfa, out],
                       cwd=helpers.ROOT, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    want = gw.window_align(xn, y, *PLANT_ARGS, 1.0, P["offset"], P["gap"], "both")
    assert "reverse, %d matched window pairs" % len(want["x_start"]) in r.stderr and want["orientation"] == "reverse"
    back = gw.read_window_align(out)
    assert back["score"] == want["score"] and back["orientation"] == "reverse"
    assert back["end"] == tuple(want["end"]) and back["start"] == tuple(want["start"])
    assert back["x_start"].tobytes() == want["x_start"].tobytes() and back["y_start"].tobytes() == want["y_start"].tobytes()
    assert set((back["x_start"] + back["y_start"]).tolist()) == {520, 540}
