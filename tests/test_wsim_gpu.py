"""Windowed kernel matrices on the GPU (gkmhip_wsim_profiles, gkmhip_wsim_normalize, gkmhip_wsim_best,
gkmwindows.window_kernel / window_best): every pair's exact profile against the oracle's profile of the two windows cut
out, bit identity of K with device.cross_kernel on the materialised windows, tile and chunk edges, windows over invalid
characters, independence of the chunking, the best window per row, and the comparisons a launch shares between window
pairs."""
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import dense_inputs as DI
from tests import helpers
from tests import wsim_ref as WR
from tests.window_launch import cross as _cross
from tests.window_launch import record as _record
from tests.window_launch import tile_count as _tile_count
from tests.window_launch import wsim_profiles as _device_profiles

pytestmark = pytest.mark.gpu

SR = WR.SR
K_TOL = 1e-12        # device exp() against the host's libm, as tests/test_gpu_parity.py holds the RBF types


@pytest.fixture(scope="module")
def dv(built):
    from gkmqc_amd import device
    return device


@pytest.fixture(scope="module")
def gw(built):
    from gkmqc_amd import gkmwindows
    return gkmwindows


@pytest.mark.parametrize("t", [0, 1, 2])
@pytest.mark.parametrize("L,k,d", [(5, 3, 2), (8, 5, 3), (11, 7, 3), (12, 8, 4), (10, 4, 6)])
def test_exact_profiles(dv, t, L, k, d):
    """every pair's profile equals the oracle's P_m of the two windows cut out, and G the Gram epilogue's sum of it, for
    W in {L, L + 1, 64, 300} and strides {(1, 1), (7, 3), (W, 1), (W + 3, W)}, on iid bases, on a homopolymer (every
    forward pair a hit) and with y = x; up to 34 windows of x (more than one tile) by 12 of y"""
    rng = np.random.default_rng(100 * L + d)
    iid_x, iid_y = rng.integers(0, 4, size=1500, dtype=np.uint8), rng.integers(0, 4, size=1500, dtype=np.uint8)
    poly = DI.homopolymer(DI.A, 1500)
    c = dv.mismatch_weights(t, L, k)[:d + 1]
    ctx = dv.GramContext(t, L, k, d, device=0)
    try:
        for name, (x, y) in {"iid": (iid_x, iid_y), "polyA": (poly, poly), "y = x": (iid_x, iid_x)}.items():
            for W in (L, L + 1, 64, 300):
                for sx, sy in ((1, 1), (7, 3), (W, 1), (W + 3, W)):
                    xs, ys = _record(x, W, sx, 34), _record(y, W, sy, 12)
                    got, G, _ = _device_profiles(ctx, xs, ys, W, sx, sy)
                    want = WR.profiles(xs, ys, W, sx, sy, t, L, k, d)
                    what = (name, t, L, d, W, sx, sy)
                    assert got.shape == want.shape and want.shape[0] >= 1 and want.shape[1] >= 1, what
                    assert np.array_equal(got, want), (what, np.argwhere((got != want).any(axis=2))[:5])
                    assert helpers.raw_from_profiles(want, c).tobytes() == G.tobytes(), what
        assert (WR.profiles(poly[:300], poly[:300], 300, 1, 1, t, L, k, d)[:, :, 0] == (300 - L + 1) ** 2).all()
    finally:
        ctx.close()
        WR.forget()


@pytest.mark.parametrize("sx,sy", [(1, 1), (3, 1), (1, 5), (20, 20)])
def test_tile_edges(dv, sx, sy):
    """1, g - 1, g, g + 1 and 2 g + 1 windows on each axis independently, g from gkmhip_wsim_group, at W = 64"""
    L, k, d, W = 8, 5, 3, 64
    gx, gy = dv.wsim_group(L, d, W, sx, sy)
    assert gx == 32 and gy == 32                                           # (n = 57: every stride here is below it)
    rng = np.random.default_rng(sx + 10 * sy)
    x = rng.integers(0, 4, size=W + 2 * gx * sx, dtype=np.uint8)
    y = rng.integers(0, 4, size=W + 2 * gy * sy, dtype=np.uint8)
    y[70:100] = x[20:50]                                                   # something shared beyond chance
    ctx = dv.GramContext(0, L, k, d, device=0)
    try:
        whole = WR.profiles(x, y, W, sx, sy, 0, L, k, d)
        assert whole.shape[:2] == (2 * gx + 1, 2 * gy + 1)
        counts = lambda g: (1, g - 1, g, g + 1, 2 * g + 1)                 # noqa: E731
        for nx in counts(gx):
            for ny in (counts(gy) if nx in (1, gx + 1) else (gy, 2 * gy + 1)):
                got, _, comparisons = _device_profiles(ctx, _record(x, W, sx, nx), _record(y, W, sy, ny), W, sx, sy)
                assert got.shape[:2] == (nx, ny)
                assert np.array_equal(got, whole[:nx, :ny]), (nx, ny, np.argwhere((got != whole[:nx, :ny]).any(axis=2))[:5])
                assert comparisons == 2 * _tile_count(W - L + 1, sx, gx, nx) * _tile_count(W - L + 1, sy, gy, ny)
    finally:
        ctx.close()


@pytest.mark.parametrize("t", [0, 1, 2, 3])
@pytest.mark.parametrize("L,k,d,W,sx,sy,T", [(11, 7, 3, 300, 20, 13, 1300), (8, 5, 3, 64, 1, 3, 160), (10, 4, 6, 10, 1, 1, 60),
                                             (12, 8, 4, 200, 200, 7, 900)])
def test_bit_identity_with_cross_kernel(dv, gw, t, L, k, d, W, sx, sy, T):
    rng = np.random.default_rng(T + t)
    x = rng.integers(0, 4, size=T, dtype=np.uint8)
    y = rng.integers(0, 4, size=T - 37 if T > 100 else T, dtype=np.uint8)
    y[5:5 + min(W, 40)] = x[9:9 + min(W, 40)]
    gamma = 1.7 if t == 3 else 1.0
    r = gw.window_kernel(x, y, W, sx, sy, t, L, k, d, gamma)
    assert r["x_starts"].tolist() == SR.starts(len(x), W, sx) and r["y_starts"].tolist() == SR.starts(len(y), W, sy)
    assert r["x_valid"].all() and r["y_valid"].all() and r["K"].dtype == np.float64
    want = _cross(dv, x, y, W, sx, sy, t, L, k, d, gamma)
    assert r["K"].shape == want.shape and r["K"].tobytes() == want.tobytes(), np.argwhere(r["K"] != want)[:5]
    assert np.isfinite(r["K"]).all() and (r["K"] > 0).any()
    # a record against itself: no unit diagonal is forced, the entry is what the division gives; cross_kernel's
    # off-diagonal entry of two identical sequences is the same division
    s = gw.window_kernel(x[:W + 5 * sx], x[:W + 5 * sx], W, sx, sx, t, L, k, d, gamma)["K"]
    twice = _cross(dv, x[:W + 5 * sx], x[:W + 5 * sx], W, sx, sx, t, L, k, d, gamma)
    assert s.tobytes() == twice.tobytes() and np.abs(np.diag(s) - 1.0).max() < 1e-15


@pytest.mark.parametrize("t", [0, 2, 3])
def test_k_against_the_cpu_reference(gw, t):
    """the definition, pair by pair on the CPU from the oracle's profiles: the same sums, square roots and one division;
    type 3 passes through the device's exp()"""
    rng = np.random.default_rng(31 + t)
    x, y = rng.integers(0, 4, size=400, dtype=np.uint8), rng.integers(0, 4, size=330, dtype=np.uint8)
    y[100:180] = x[40:120]
    got = gw.window_kernel(x, y, 100, 25, 10, t, 10, 6, 3, 2.0)["K"]
    want = WR.kernel(x, y, 100, 25, 10, t, 10, 6, 3, 2.0)
    assert got.shape == want.shape == (13, 24)
    err = helpers.max_rel_err(got, want)
    print("type %d: max relative error against the reference %.3g" % (t, err))
    assert err < K_TOL


def test_invalid_bases(gw):
    """an N in x makes exactly the rows of the windows over it NaN, an N in y the columns; every other entry keeps its
    bytes"""
    rng = np.random.default_rng(12)
    W, sx, sy = 64, 5, 9
    x, y = rng.integers(0, 4, size=400, dtype=np.uint8), rng.integers(0, 4, size=500, dtype=np.uint8)
    clean = gw.window_kernel(x, y, W, sx, sy, 2, 10, 6, 3)
    bad_x, bad_y = [0, 130, 131, 399], [77, 300]
    xb, yb = x.copy(), y.copy()
    xb[bad_x] = 4
    yb[bad_y] = 255
    rows = np.array([any(a <= b < a + W for b in bad_x) for a in clean["x_starts"]])
    cols = np.array([any(a <= b < a + W for b in bad_y) for a in clean["y_starts"]])
    assert rows.any() and not rows.all() and cols.any() and not cols.all()
    for xs, ys, r, c in ((xb, y, rows, np.zeros_like(cols)), (x, yb, np.zeros_like(rows), cols), (xb, yb, rows, cols)):
        got = gw.window_kernel(xs, ys, W, sx, sy, 2, 10, 6, 3, chunk=150)
        assert np.array_equal(got["x_valid"], ~r) and np.array_equal(got["y_valid"], ~c)
        dead = r[:, None] | c[None, :]
        assert np.array_equal(np.isnan(got["K"]), dead)
        assert got["K"][~dead].tobytes() == clean["K"][~dead].tobytes()
    best = gw.window_best(xb, yb, W, sx, sy, 2, 10, 6, 3)
    assert (best["y_start"][rows] == -1).all() and np.isnan(best["K"][rows]).all()
    assert (best["y_start"][~rows] >= 0).all() and not cols[best["y_start"][~rows] // sy].any()


def test_chunk_invariance(gw):
    """chunks that cut each axis into 1, 2 and 5 pieces: identical bytes from window_kernel and window_best"""
    from gkmqc_amd import gkmpredict as gp
    rng = np.random.default_rng(13)
    W, sx, sy = 100, 7, 4
    x, y = rng.integers(0, 4, size=1000, dtype=np.uint8), rng.integers(0, 4, size=1000, dtype=np.uint8)
    y[300:500] = x[100:300]
    x[640] = 4
    whole = gw.window_kernel(x, y, W, sx, sy, 3, 11, 7, 3, 0.5)
    whole_best = gw.window_best(x, y, W, sx, sy, 3, 11, 7, 3, 0.5, min_separation=50)
    pieces = []
    for chunk in (1000, 550, 280):
        px, py = len(gp.scan_chunk_plan(1000, W, sx, chunk)), len(gp.scan_chunk_plan(1000, W, sy, chunk))
        pieces.append((px, py))
        seen = []
        got = gw.window_kernel(x, y, W, sx, sy, 3, 11, 7, 3, 0.5, chunk=chunk, on_chunk=seen.append)
        assert len(seen) == px * py and all(c["kernel"] == "k_wsim_profiles" for c in seen)
        assert sum(c["x_windows"] * c["y_windows"] for c in seen) == whole["K"].size
        for key in ("K", "x_starts", "y_starts", "x_valid", "y_valid"):
            assert got[key].tobytes() == whole[key].tobytes(), (chunk, key)
        got = gw.window_best(x, y, W, sx, sy, 3, 11, 7, 3, 0.5, chunk=chunk, min_separation=50)
        for key in ("x_starts", "y_start", "K"):
            assert got[key].tobytes() == whole_best[key].tobytes(), (chunk, key)
    assert pieces == [(1, 1), (2, 2), (5, 5)]


def test_best_equals_the_argmax_of_the_matrix(gw):
    rng = np.random.default_rng(14)
    W, sx, sy = 64, 3, 2
    x, y = rng.integers(0, 4, size=500, dtype=np.uint8), rng.integers(0, 4, size=700, dtype=np.uint8)
    y[:200] = x[100:300]
    y[400:600] = x[100:300]                                                # twice: ties, the lower start wins
    y[650] = 4
    full = gw.window_kernel(x, y, W, sx, sy, 0, 8, 5, 3)
    for sep in (0, 1, 150, 10 ** 6):
        want_j, want_k = WR.best(full["K"], full["x_starts"], full["y_starts"], sep)
        got = gw.window_best(x, y, W, sx, sy, 0, 8, 5, 3, min_separation=sep, chunk=200)
        assert np.array_equal(got["y_start"], want_j) and got["K"].tobytes() == want_k.tobytes(), sep
        assert np.array_equal(got["x_starts"], full["x_starts"])
    assert (want_j == -1).all() and np.isnan(want_k).all()                 # nothing is 10^6 bases away: -1 / NaN
    tied = gw.window_best(x, y, W, sx, sy, 0, 8, 5, 3)
    at = np.flatnonzero((full["x_starts"] >= 100) & (full["x_starts"] + W <= 300) & (full["x_starts"] % 2 == 0))
    assert len(at) > 10 and np.array_equal(tied["y_start"][at], full["x_starts"][at] - 100)


def test_best_against_itself_finds_a_planted_copy_and_never_overlaps(gw):
    rng = np.random.default_rng(15)
    W = 64
    x = rng.integers(0, 4, size=900, dtype=np.uint8)
    x[700:764] = x[120:184]                                                # a copy of 64 bases, 580 further on
    r = gw.window_best(x, x, W, 4, 4, 2, 11, 7, 3, min_separation=W)
    assert (np.abs(r["y_start"] - r["x_starts"]) >= W).all() and (r["y_start"] >= 0).all()
    i = int(np.flatnonzero(r["x_starts"] == 120)[0])
    assert r["y_start"][i] == 700 and abs(r["K"][i] - 1.0) < 1e-15
    j = int(np.flatnonzero(r["x_starts"] == 700)[0])
    assert r["y_start"][j] == 120
    assert set(np.argsort(r["K"])[-2:].tolist()) == {i, j}
    # without a separation every window finds itself; the copy ties with its original, and the lower start wins
    own = gw.window_best(x, x, W, 4, 4, 2, 11, 7, 3)
    assert own["y_start"][j] == 120 and np.array_equal(np.delete(own["y_start"], j), np.delete(own["x_starts"], j))
    # a separation nothing satisfies: -1 / NaN in every row
    none = gw.window_best(x[:200], x[:200], W, 4, 4, 2, 11, 7, 3, min_separation=137)
    assert (none["y_start"] == -1).all() and np.isnan(none["K"]).all()
    some = gw.window_best(x[:200], x[:200], W, 4, 4, 2, 11, 7, 3, min_separation=100)
    assert ((some["y_start"] == -1) == ((some["x_starts"] < 100) & (some["x_starts"] > 36))).all()


@pytest.mark.parametrize("L,s", [(11, 1), (11, 20), (11, 36), (5, 7)])
def test_shared_comparisons(dv, L, s):
    """64 x 64 windows of 300 bases at sx = sy <= n / 8: at most an eighth of the 2 n^2 pairs per window pair the
    materialised path compares; the CPU rendering counts the same"""
    W = 300
    n = W - L + 1
    assert 8 * s <= n
    x = np.random.default_rng(s).integers(0, 4, size=W + 63 * s, dtype=np.uint8)
    ctx = dv.GramContext(0, L, L - 3, 3, device=0)
    try:
        P, _, comparisons = _device_profiles(ctx, x, x[::-1].copy(), W, s, s)
        assert P.shape[:2] == (64, 64)
        assert 0 < comparisons <= 2.0 * n * n * 64 * 64 / 8
        gx, gy = ctx.wsim_group(W, s, s)
        assert comparisons == 2 * _tile_count(n, s, gx, 64) * _tile_count(n, s, gy, 64)
        if L == 11:                                                        # (at L = 5 a third of all pairs are hits)
            ref_P, ref_comparisons = WR.tile_profiles(x, x[::-1].copy(), W, s, s, gx, gy, L, 3)
            assert ref_comparisons == comparisons <= 2.0 * n * n * 64 * 64 / 8 and np.array_equal(ref_P, P)
        # disjoint windows: one pair per tile, the materialised count
        z = np.random.default_rng(2).integers(0, 4, size=3 * W, dtype=np.uint8)
        P, _, comparisons = _device_profiles(ctx, z, z[:2 * W], W, W, W)
        assert P.shape[:2] == (3, 2) and comparisons == 2 * n * n * 6
    finally:
        ctx.close()
    small = np.random.default_rng(1).integers(0, 4, size=40 + 11 * 2, dtype=np.uint8)
    _, ref = WR.tile_profiles(small, small, 40, 2, 2, 8, 8, 5, 2)          # 12 x 12 windows, n = 36, s <= n / 8
    assert ref <= 2 * 36 * 36 * 12 * 12 / 8


def test_command_line(gw, tmp_path):
    rng = np.random.default_rng(16)
    x, y = rng.integers(0, 4, size=700, dtype=np.uint8), rng.integers(0, 4, size=600, dtype=np.uint8)
    y[200:400] = x[300:500]
    from gkmqc_amd import gkmpredict as gp
    xfa, yfa = str(tmp_path / "x.fa"), str(tmp_path / "y.fa")
    text = gp.codes_to_text(x)
    text = text[:50] + "N" + text[51:]
    with open(xfa, "w") as f:
        f.write(">locus x\n" + "\n".join(text[i:i + 60] for i in range(0, len(text), 60)) + "\n")
    with open(yfa, "w") as f:
        f.write(">locus y\n" + gp.codes_to_text(y).lower() + "\n")
    xn = x.copy()
    xn[50] = 4

    def run(*args):
        r = subprocess.run([sys.executable, "-m", "gkmqc_amd.gkmwindows"] + list(args), cwd=helpers.ROOT,
                           capture_output=True, text=True)
        assert r.returncode == 0, (args, r.stderr)
        return r

    out = str(tmp_path / "k.npz")
    r = run("matrix", "--width", "100", "--stride-x", "10", "--stride-y", "20", "--chunk", "300", "-t", "3", "-L", "10", "-k", "6",
            "-d", "3", "-G", "0.5", xfa, yfa, out)
    want = gw.window_kernel(xn, y, 100, 10, 20, 3, 10, 6, 3, 0.5)
    assert "61 x 26 windows, 6 and 0 over a non-ACGT character" in r.stderr
    back = gw.read_window_kernel(out)
    assert back["width"] == 100
    for key in ("K", "x_starts", "y_starts", "x_valid", "y_valid"):
        assert back[key].tobytes() == want[key].tobytes(), key
    out = str(tmp_path / "b.tsv")
    run("best", "--width", "100", "--stride-x", "10", "--min-separation", "30", "-t", "2", "-L", "10", "-k", "6", "-d", "3",
        xfa, yfa, out)
    want = gw.window_best(xn, y, 100, 10, None, 2, 10, 6, 3, min_separation=30)
    back = gw.read_window_best(out)
    for key in ("x_starts", "y_start", "K"):
        assert back[key].tobytes() == want[key].tobytes(), key
    i = int(np.flatnonzero(want["x_starts"] == 300)[0])
    assert want["y_start"][i] == 200
    assert not os.path.exists(out + ".tmp")
