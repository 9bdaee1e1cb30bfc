"""Windowed kernel matrices without a GPU: the CPU reference's tile and difference-array rendering (tests/wsim_ref.py)
against the oracle's profile of every pair of windows cut out, the tile shape of the device layer (gkmhip_wsim_group needs
no device) against the chunk plans, every refusal of gkmwindows.window_kernel / window_best and of the command line, the
combination of the chunks' best columns, and the two output files (gkmqc_amd/gkmwindows.py)."""
import os

import numpy as np
import pytest

from tests import wsim_ref as WR

NAN = float("nan")


@pytest.fixture(scope="module")
def gw(built):
    from gkmqc_amd import gkmwindows
    return gkmwindows


@pytest.fixture(scope="module")
def dv(built):
    from gkmqc_amd import device
    return device


@pytest.mark.parametrize("t,L,k,d", [(0, 5, 3, 2), (2, 6, 4, 1), (1, 6, 3, 3)])
@pytest.mark.parametrize("W,sx,sy,gx,gy", [(5, 1, 1, 4, 3), (6, 1, 2, 32, 32), (20, 1, 1, 5, 7), (20, 3, 7, 4, 2),
                                           (20, 20, 1, 1, 6), (20, 23, 20, 1, 1), (33, 2, 5, 16, 3)])
def test_tile_formulation_equals_the_oracle_per_pair(built, t, L, k, d, W, sx, sy, gx, gy):
    """every l-mer pair of a tile compared once per strand and credited to the rectangle of window pairs that hold it =
    the oracle's P_m of the two windows cut out; one window pair per tile compares 2 n^2 pairs, the materialised count"""
    W = max(W, L)
    rng = np.random.default_rng(W + sx + 7 * sy + L)
    x = rng.integers(0, 4, size=80, dtype=np.uint8)
    y = rng.integers(0, 4, size=70, dtype=np.uint8)
    x[20:38] = 0                                                           # a homopolymer stretch: dense hits
    y[10:30] = 0
    y[40:50] = np.tile([0, 3], 5)                                          # (AT)n: reverse-complement hits
    x[50:60] = np.tile([0, 3], 5)
    got, comparisons = WR.tile_profiles(x, y, W, sx, sy, gx, gy, L, d)
    want = WR.profiles(x, y, W, sx, sy, t, L, k, d)
    assert got.shape == want.shape == (len(WR.SR.starts(80, W, sx)), len(WR.SR.starts(70, W, sy)), d + 1)
    assert np.array_equal(got, want)
    n = W - L + 1
    if gx == 1 and gy == 1:
        assert comparisons == 2 * n * n * want.shape[0] * want.shape[1]


def test_tile_formulation_with_y_equal_to_x(built):
    x = np.random.default_rng(5).integers(0, 4, size=60, dtype=np.uint8)
    got, _ = WR.tile_profiles(x, x, 16, 3, 3, 4, 4, 6, 2)
    want = WR.profiles(x, x, 16, 3, 3, 0, 6, 4, 2)
    assert np.array_equal(got, want)
    assert np.array_equal(got, np.swapaxes(got, 0, 1))                     # P(i, j) = P(j, i) for one record


def test_reference_kernel_follows_the_definition(built):
    from tests import explain_ref as R
    rng = np.random.default_rng(0)
    x = rng.integers(0, 4, size=40, dtype=np.uint8)
    y = rng.integers(0, 4, size=36, dtype=np.uint8)
    x[17] = 4
    K = WR.kernel(x, y, 12, 5, 4, 0, 5, 3, 2)
    assert K.shape == (6, 7)
    c = WR.coefficients(0, 5, 3, 2)
    for i, (a, wx) in enumerate(WR.SR.windows(x, 12, 5)):
        for j, (b, wy) in enumerate(WR.SR.windows(y, 12, 4)):
            if a <= 17 < a + 12:
                assert np.isnan(K[i, j])
            else:
                g = WR.raw(R.profile(wx, wy, 0, 5, 3, 2), c)
                assert K[i, j] == g / (R.self_norm(wx, 0, 5, 3, 2) * R.self_norm(wy, 0, 5, 3, 2))
    same = WR.kernel(y, y, 12, 4, 4, 0, 5, 3, 2)
    assert np.allclose(np.diag(same), 1.0, rtol=0, atol=1e-15)            # not forced, what the division gives
    rbf = WR.kernel(y, y, 12, 4, 4, 3, 5, 3, 2, gamma=2.0)
    lin = WR.kernel(y, y, 12, 4, 4, 2, 5, 3, 2)
    assert np.array_equal(rbf, np.exp(2.0 * (lin - 1)))


SHAPES = [(11, 3, 300, 1, 1), (11, 3, 300, 20, 20), (11, 3, 300, 300, 1), (11, 3, 300, 7, 290), (11, 3, 300, 289, 291),
          (5, 2, 5, 1, 1), (5, 2, 6, 1, 2), (12, 12, 2047, 1, 254), (10, 6, 2047, 66, 65), (8, 3, 64, 1, 3), (5, 0, 2047, 2042, 2043)]


@pytest.mark.parametrize("L,d,W,sx,sy", SHAPES)
def test_tile_shape_is_consistent(dv, L, d, W, sx, sy):
    """gx x gy windows: one along an axis whose windows share no l-mer, at most 32, a stretch of at most 4 096 words, the
    LDS of a tile well under 160 KiB, g >= 8 wherever the stride is at most n / 8, and the same along x and y"""
    n = W - L + 1
    gx, gy = dv.wsim_group(L, d, W, sx, sy)
    for g, s in ((gx, sx), (gy, sy)):
        assert 1 <= g <= 32
        assert (g == 1) == (s >= n or n + s > 4096)
        assert n + (g - 1) * s <= 4096
        if g < 32 and s < n:
            assert n + g * s > 4096                                        # the largest that fits
        if 8 * s <= n:
            assert g >= 8
    assert (gx, gy) == dv.wsim_group(L, d, W, sx, sy) and (gy, gx) == dv.wsim_group(L, d, W, sy, sx)
    assert dv.wsim_group(L, 0, W, sx, sy) == (gx, gy)                      # (d enters the LDS size, not the shape)
    lds = (d + 1) * (gx + 1) * (gy + 1) * 4 + 6 * (n + (gy - 1) * sy)
    assert lds <= 96 * 1024


def test_tile_shape_refusals(dv):
    for args in ((11, 3, 10, 1, 1), (11, 3, 2048, 1, 1), (11, 3, 300, 0, 1), (11, 3, 300, 1, 0), (11, 3, 300, -2, 1),
                 (13, 3, 300, 1, 1), (11, 13, 300, 1, 1), (0, 0, 300, 1, 1)):
        assert dv.wsim_group(*args) == (0, 0)


@pytest.mark.parametrize("T,W,s", [(1000, 60, 1), (1000, 60, 7), (1000, 60, 63), (61, 60, 1), (5000, 600, 10)])
@pytest.mark.parametrize("chunk", [60, 100, 601, 10 ** 6])
def test_chunks_of_whole_windows_fit_the_budget(gw, T, W, s, chunk):
    from gkmqc_amd import gkmpredict as gp
    chunk = max(chunk, W)
    plan = gp.scan_chunk_plan(T, W, s, chunk)
    per = gw.windows_per_chunk(W, s, chunk)
    assert max(w1 - w0 for w0, w1, _, _ in plan) == min(per, gp.scan_window_count(T, W, s))
    assert sum(w1 - w0 for w0, w1, _, _ in plan) == gp.scan_window_count(T, W, s)
    cx, cy = gw.default_chunks(W, s, 3 * s)
    assert gw.windows_per_chunk(W, s, cx) == gw.windows_per_chunk(W, 3 * s, cy)
    assert gw.windows_per_chunk(W, s, cx) ** 2 * 8 <= gw.BLOCK_BYTES < (gw.windows_per_chunk(W, s, cx) + 1) ** 2 * 8


def test_api_refusals_come_before_any_device_work(gw):
    """(no GPU here: anything that reached the device would fail otherwise)"""
    x, y = np.zeros(100, dtype=np.uint8), np.zeros(90, dtype=np.uint8)
    cases = [(dict(width=20, kernel_type=4), "position"), (dict(width=20, kernel_type=5), "position"),
             (dict(width=10), "below L"), (dict(width=2048), "above 2047"), (dict(width=20, stride_x=0), "stride"),
             (dict(width=20, stride_y=0), "stride"), (dict(width=20, stride_x=-1), "stride"),
             (dict(width=95), "record y"), (dict(width=101), "record x"), (dict(width=20, gamma=NAN, kernel_type=3), "gamma"),
             (dict(width=20, gamma=float("inf")), "gamma"), (dict(width=20, chunk=19), "chunk"),
             (dict(width=20, L=11, k=12), "window_"), (dict(width=20, d=9), "window_"), (dict(width=20, kernel_type=6), "window_")]
    for fn in (gw.window_kernel, gw.window_best):
        for kw, msg in cases:
            with pytest.raises(gw.WindowError, match=msg):
                fn(x, y, **kw)
    with pytest.raises(gw.WindowError, match="negative"):
        gw.window_best(x, y, 20, min_separation=-1)
    with pytest.raises(gw.WindowError, match="window_best"):
        gw.window_best(x, y, 10)
    with pytest.raises(gw.WindowError, match="one-dimensional"):
        gw.window_kernel(np.zeros((2, 50), np.uint8), y, 20)
    with pytest.raises(gw.WindowError, match="device budget"):
        gw.check_window_kernel(10 ** 6, 10 ** 6, 20, chunk=10 ** 6)
    gw.check_window_kernel(100, 90, 20, 3, None, 3, 11, 7, 3, 0.5, 50, 7)  # and what is served passes


def _best_of(K, lo, hi):
    """(best_j, best_k) of the columns [lo, hi) of K by a plain loop, columns global; NaN never wins"""
    out_j, out_k = [], []
    for row in K:
        bj, bv = -1, NAN
        for j in range(lo, hi):
            if row[j] == row[j] and (bj < 0 or row[j] > bv):
                bj, bv = j, row[j]
        out_j.append(bj)
        out_k.append(bv)
    return np.array(out_j, dtype=np.int64), np.array(out_k)


@pytest.mark.parametrize("seed", range(6))
def test_best_of_chunks_equals_best_of_the_whole(gw, seed):
    rng = np.random.default_rng(seed)
    K = rng.integers(0, 4, size=(40, 23)).astype(np.float64) / 4.0       # few values: ties everywhere
    K[rng.random(K.shape) < 0.3] = NAN
    K[5] = NAN                                                             # a row without any candidate
    K[6, :-1], K[6, -1] = NAN, 0.25
    K[7] = 0.5                                                             # one value in every column
    K[8] = [-0.0, 0.0] * 11 + [-0.0]                                       # zeros of either sign tie
    want_j, want_k = _best_of(K, 0, 23)
    assert want_j[5] == -1 and np.isnan(want_k[5]) and want_j[6] == 22 and want_j[7] == 0 and want_j[8] == 0
    for _ in range(5):
        cuts = [0] + sorted(rng.choice(np.arange(1, 23), size=rng.integers(0, 6), replace=False).tolist()) + [23]
        parts = [_best_of(K, lo, hi) for lo, hi in zip(cuts[:-1], cuts[1:])]
        for order in (parts, parts[::-1], [parts[i] for i in rng.permutation(len(parts))]):
            got_j, got_k = gw.combine_best(order)
            assert np.array_equal(got_j, want_j) and got_k.tobytes() == want_k.tobytes()
    none = gw.combine_best([(np.full(3, -1), np.full(3, NAN)), (np.full(3, -1), np.full(3, NAN))])
    assert none[0].tolist() == [-1, -1, -1] and np.isnan(none[1]).all()


def test_reference_best_applies_the_separation(built):
    K = np.array([[0.9, 0.8, 0.7, NAN], [0.1, 0.5, 0.5, 0.2], [NAN, NAN, NAN, NAN]])
    xs, ys = np.array([0, 10, 20]), np.array([0, 5, 10, 15])
    j, v = WR.best(K, xs, ys)
    assert j.tolist() == [0, 5, -1] and v[:2].tolist() == [0.9, 0.5] and np.isnan(v[2])
    j, v = WR.best(K, xs, ys, 6)
    assert j.tolist() == [10, 0, -1] and v[:2].tolist() == [0.7, 0.1]
    j, v = WR.best(K, xs, ys, 100)
    assert j.tolist() == [-1, -1, -1] and np.isnan(v).all()


def test_matrix_file_round_trip(gw, tmp_path):
    rng = np.random.default_rng(9)
    K = rng.standard_normal((5, 3)) * 10.0 ** rng.integers(-8, 8, size=(5, 3))
    K[2] = NAN
    K[0, 1] = -0.0
    r = dict(K=K, x_starts=np.arange(5, dtype=np.int64) * 7, y_starts=np.arange(3, dtype=np.int64) * 2,
             x_valid=np.array([1, 1, 0, 1, 1], bool), y_valid=np.ones(3, bool))
    path = str(tmp_path / "k.npz")
    gw.write_window_kernel(path, r, 300)
    back = gw.read_window_kernel(path)
    assert back["width"] == 300 and back["K"].tobytes() == K.tobytes() and back["K"].shape == (5, 3)
    for key in ("x_starts", "y_starts", "x_valid", "y_valid"):
        assert back[key].dtype == r[key].dtype and np.array_equal(back[key], r[key])
    import zipfile
    with zipfile.ZipFile(path) as z:
        assert all(i.compress_type == zipfile.ZIP_STORED for i in z.infolist())   # uncompressed
    other = str(tmp_path / "o.npz")
    np.savez(other, K=K)
    with pytest.raises(gw.WindowError, match="is not a"):
        gw.read_window_kernel(other)
    pickled = str(tmp_path / "p.npz")
    np.savez(pickled, **{**{k: v for k, v in r.items()}, "format": np.array(gw.MATRIX_FORMAT), "width": np.array([{}], dtype=object)})
    with pytest.raises(ValueError):
        gw.read_window_kernel(pickled)                                     # allow_pickle=False


def test_best_file_round_trip(gw, tmp_path):
    r = dict(x_starts=np.arange(5, dtype=np.int64) * 20, y_start=np.array([40, -1, 0, 1 << 40, 7], dtype=np.int64),
             K=np.array([np.pi / 3, NAN, -0.0, 5e-324, 1.0 - 2.0 ** -53]))
    path = str(tmp_path / "b.tsv")
    gw.write_window_best(path, r)
    back = gw.read_window_best(path)
    for key in ("x_starts", "y_start"):
        assert back[key].dtype == np.int64 and np.array_equal(back[key], r[key])
    assert back["K"].tobytes() == r["K"].tobytes()
    lines = open(path).read().split("\n")
    assert lines[-1] == "" and lines[0] == "0\t40\t%.17g" % (np.pi / 3) and lines[1] == "20\t-1\tnan"
    with open(path, "a") as f:
        f.write("1\t2\n")
    with pytest.raises(gw.WindowError, match=":6:"):
        gw.read_window_best(path)


def test_command_line_refusals_exit_1_and_write_nothing(gw, tmp_path, capsys):
    xfa, yfa, two = str(tmp_path / "x.fa"), str(tmp_path / "y.fa"), str(tmp_path / "two.fa")
    with open(xfa, "w") as f:
        f.write(">x\n" + "ACGT" * 10 + "\n")
    with open(yfa, "w") as f:
        f.write(">y\n" + "ACGGT" * 7 + "\n")
    with open(two, "w") as f:
        f.write(">a\n" + "ACGT" * 10 + "\n>b\n" + "ACGT" * 10 + "\n")
    for cmd, out in (("matrix", str(tmp_path / "o.npz")), ("best", str(tmp_path / "o.tsv"))):
        cases = [(["--width", "10", xfa, yfa, out], "below L"),
                 (["--width", "2048", xfa, yfa, out], "above 2047"),
                 (["--width", "20", "--stride-x", "0", xfa, yfa, out], "stride"),
                 (["--width", "20", "--stride-y", "0", xfa, yfa, out], "stride"),
                 (["--width", "20", "--chunk", "10", xfa, yfa, out], "chunk"),
                 (["--width", "36", xfa, yfa, out], "record y"),
                 (["--width", "20", "-t", "4", xfa, yfa, out], "position"),
                 (["--width", "20", "-t", "5", xfa, yfa, out], "position"),
                 (["--width", "20", "-t", "3", "-G", "nan", xfa, yfa, out], "gamma"),
                 (["--width", "20", "-L", "11", "-k", "12", xfa, yfa, out], "gkmwindows: error"),
                 (["--width", "20", str(tmp_path / "missing.fa"), yfa, out], "cannot read"),
                 (["--width", "20", xfa, two, out], "2 records")]
        if cmd == "best":
            cases.append((["--width", "20", "--min-separation", "-1", xfa, yfa, out], "negative"))
        for args, msg in cases:
            assert gw.main([cmd] + args) == 1, args
            assert msg in capsys.readouterr().err, args
            assert not os.path.exists(out) and not os.path.exists(out + ".tmp")
        with pytest.raises(SystemExit):
            gw.main([cmd, xfa, yfa, out])                                  # --width is required
    with pytest.raises(SystemExit):
        gw.main(["matrix", "--width", "20", "--min-separation", "5", xfa, yfa, str(tmp_path / "o.npz")])
    with pytest.raises(SystemExit):
        gw.main(["--width", "20", xfa, yfa, str(tmp_path / "o.npz")])      # a command is required
