"""The window kernels over the whole legal (L, k, d, W, stride) region on the GPU (tests/window_cases.py; the conditions the
cases are there for are held by tests/test_window_region_host.py): k_wsim_profiles at L < 5, d up to 12 and d = L, launches
with more than 64 KiB of dynamic LDS, tiles cut short by the 4 096-word stretch, window_kernel / window_best on top of
them, k_scan_profiles' values at wide windows (n > 1024, stretch-limited groups), k_scan_score at the same widths, and the
shared word counts at the widest window.  Everything is compared as the older window tests compare it: integer profiles
bit for bit with the oracle's profile of the windows cut out, G with helpers.raw_from_profiles, K with
device.cross_kernel on the materialised windows, sentinels in the guard rows, last_kernel_name."""
import re

import numpy as np
import pytest

from tests import helpers
from tests import dist_launch as TD
from tests import regions_launch as TR
from tests import regions_ref as RR
from tests import window_cases as WC
from tests import window_launch as WL
from tests import wsim_ref as WR

pytestmark = pytest.mark.gpu

SR = WR.SR
K_TOL = 1e-12        # device exp() against the host's libm, as tests/test_wsim_gpu.py holds type 3
NAN, INF = float("nan"), float("inf")


@pytest.fixture(scope="module")
def dv(built):
    from gkmqc_amd import device
    return device


@pytest.fixture(scope="module")
def gw(built):
    from gkmqc_amd import gkmwindows
    return gkmwindows


@pytest.fixture(scope="module")
def gp(built):
    from gkmqc_amd import gkmpredict
    return gkmpredict


def _want(x, y, c, t, rows=None, cols=None):
    """the oracle's profile of window i of x against window j of y for i in rows, j in cols (all by default)"""
    wx, wy = SR.windows(x, c.W, c.sx), SR.windows(y, c.W, c.sy)
    rows = range(len(wx)) if rows is None else rows
    cols = range(len(wy)) if cols is None else cols
    return np.array([[WR.pair_profile(wx[i][1], wy[j][1], t, c.L, c.k, c.d) for j in cols] for i in rows], dtype=np.int64)


def _launch(dv, ctx, t, c, x, y, rows=None, cols=None):
    """one k_wsim_profiles launch over every window pair of (x, y): profiles, G and the comparison count against the oracle
    on the window pairs rows x cols -> the launch's (nA, nB)"""
    got, G, comparisons = WL.wsim_profiles(ctx, x, y, c.W, c.sx, c.sy)
    nA, nB = got.shape[:2]
    rows = list(range(nA) if rows is None else rows)
    cols = list(range(nB) if cols is None else cols)
    want = _want(x, y, c, t, rows, cols)
    what = (c, t, nA, nB)
    assert got.shape == (len(SR.starts(len(x), c.W, c.sx)), len(SR.starts(len(y), c.W, c.sy)), c.d + 1), what
    sub = got[np.ix_(rows, cols)]
    assert np.array_equal(sub, want), (what, np.argwhere((sub != want).any(axis=2))[:5])
    coef = dv.mismatch_weights(t, c.L, c.k)[:c.d + 1]
    assert helpers.raw_from_profiles(want, coef).tobytes() == np.ascontiguousarray(G[np.ix_(rows, cols)]).tobytes(), what
    n = c.W - c.L + 1
    gx, gy = ctx.wsim_group(c.W, c.sx, c.sy)
    assert comparisons == 2 * WL.tile_count(n, c.sx, gx, nA) * WL.tile_count(n, c.sy, gy, nB), what
    return nA, nB


@pytest.mark.parametrize("t", [0, 1, 2])
@pytest.mark.parametrize("L,k,d", WC.WSIM_LKD)
def test_wsim_profiles_over_the_region(dv, t, L, k, d):
    """L < 5, d > 6, d = L and d = L - 1: up to 13 planes of the difference array and 13 coefficients of the epilogue, at
    W in {L, L + 1, 64} (300 where d >= 9), strides (1, 1), (7, 3), (W, 1), 34 x 12 windows; inputs in which every class
    m = 0..d occurs, a homopolymer and y = x"""
    ctx = dv.GramContext(t, L, k, d, device=0)
    try:
        for c in WC.wsim_region_launches(L, k, d):
            x, y = WC.records(c.seed, c.comp, L, d, c.W, c.sx, c.sy, c.nx, c.ny)
            assert _launch(dv, ctx, t, c, x, y) == (c.nx, c.ny)
    finally:
        ctx.close()
        WR.forget()


LDS_PARAMS = [(case, col) for case in WC.WSIM_LDS for col in ((0, 1) if case.launch.W == 2047 else (None,))]


@pytest.mark.parametrize("case,col", LDS_PARAMS, ids=["%s%s" % (c.name, "" if col is None else "-y%d" % col) for c, col in LDS_PARAMS])
def test_wsim_profiles_above_64_kib_of_lds(dv, case, col, monkeypatch, capfd):
    """launches whose dynamic LDS passes 64 KiB (the limit hipFuncSetAttribute raises), two tiles on each axis, and the
    largest launch below it; the byte count is read from the launch's own GKM_TRACE line.  At W = 2047 a window pair
    costs the oracle 29 ms: one test per window of y."""
    c = case.launch
    x, y = WC.records(c.seed, c.comp, c.L, c.d, c.W, c.sx, c.sy, c.nx, c.ny)
    monkeypatch.setenv("GKM_TRACE", "1")
    ctx = dv.GramContext(0, c.L, c.k, c.d, device=0)
    try:
        capfd.readouterr()
        assert _launch(dv, ctx, 0, c, x, y, cols=None if col is None else [col]) == (c.nx, c.ny)
        lds = [int(v) for v in re.findall(r"k_wsim_profiles \(.*?(\d+) bytes of LDS", capfd.readouterr().err)]
        assert lds == [case.lds] and (lds[0] > WC.LDS_64K) == case.above
    finally:
        ctx.close()
        WR.forget()


@pytest.mark.parametrize("other", [0, 1])
@pytest.mark.parametrize("sx,sy", WC.STRETCH_STRIDES)
def test_wsim_stretch_limited_tiles(dv, sx, sy, other):
    """L = 11, W = 2047: 21 windows fill the 4 096-word stretch of a tile (1 < g < 32); g - 1, g and g + 1 windows on that
    axis, 2 on the other -- beside a tile of 21 x 21, of 1 x 21, of 21 x 1 and of 32 x 21.  One test per window of the
    other axis (22 pairs of the oracle each)."""
    c, axis = WC.stretch_launch(sx, sy)
    x, y = WC.records(c.seed, c.comp, c.L, c.d, c.W, sx, sy, c.nx, c.ny)
    ctx = dv.GramContext(0, c.L, c.k, c.d, device=0)
    try:
        g = ctx.wsim_group(c.W, sx, sy)[axis]
        assert g == WC.STRETCH_G
        for count in (g - 1, g, g + 1):
            if axis == 0:
                shape = _launch(dv, ctx, 0, c, x[:WC.record_length(c.W, sx, count)], y, cols=[other])
            else:
                shape = _launch(dv, ctx, 0, c, x, y[:WC.record_length(c.W, sy, count)], rows=[other])
            assert shape == ((count, 2) if axis == 0 else (2, count))
    finally:
        ctx.close()
        WR.forget()


def _same_k(got, want):
    return got.shape == want.shape and got.tobytes() == want.tobytes()


@pytest.mark.parametrize("t", [0, 3])
def test_window_kernel_end_to_end_at_d_equal_to_l(dv, gw, t):
    """window_kernel at (9, 0, 9): bit for bit device.cross_kernel on the windows cut out; type 3 against the CPU definition
    at K_TOL with NaN in the same cells; window_best against the plain argmax; windows over invalid bases"""
    c = WC.E2E_DL
    gamma = 1.7 if t == 3 else 1.0
    x, y = WC.records(c.seed, c.comp, c.L, c.d, c.W, c.sx, c.sy, c.nx, c.ny)
    r = gw.window_kernel(x, y, c.W, c.sx, c.sy, t, c.L, c.k, c.d, gamma)
    want = WL.cross(dv, x, y, c.W, c.sx, c.sy, t, c.L, c.k, c.d, gamma)
    assert r["K"].shape == (c.nx, c.ny) and _same_k(r["K"], want), np.argwhere(r["K"] != want)[:5]
    assert np.isfinite(r["K"]).all() and (r["K"] > 0).all()                # (d = L: every l-mer pair counts)
    ref = WR.kernel(x, y, c.W, c.sx, c.sy, t, c.L, c.k, c.d, gamma)
    same, err = helpers.same_nonfinite_rel_err(r["K"], ref)
    print("type %d: max relative error against the reference %.3g" % (t, err))
    assert same and err < K_TOL
    for sep in (0, 30):
        want_j, want_k = WR.best(r["K"], r["x_starts"], r["y_starts"], sep)
        got = gw.window_best(x, y, c.W, c.sx, c.sy, t, c.L, c.k, c.d, gamma, min_separation=sep, chunk=c.W + 10 * c.sx)
        assert np.array_equal(got["y_start"], want_j) and got["K"].tobytes() == want_k.tobytes(), sep
    xb, yb = WC.records(c.seed, c.comp, c.L, c.d, c.W, c.sx, c.sy, c.nx, c.ny, invalid=2)
    assert np.array_equal(np.where(xb < 4, xb, x), x) and np.array_equal(np.where(yb < 4, yb, y), y)
    bad = gw.window_kernel(xb, yb, c.W, c.sx, c.sy, t, c.L, c.k, c.d, gamma)
    okx, oky = np.array(SR.valid_windows(xb, c.W, c.sx)), np.array(SR.valid_windows(yb, c.W, c.sy))
    dead = ~okx[:, None] | ~oky[None, :]
    assert dead.any() and not dead.all() and np.array_equal(bad["x_valid"], okx) and np.array_equal(bad["y_valid"], oky)
    assert np.array_equal(np.isnan(bad["K"]), dead) and bad["K"][~dead].tobytes() == r["K"][~dead].tobytes()
    same, err = helpers.same_nonfinite_rel_err(bad["K"], WR.kernel(xb, yb, c.W, c.sx, c.sy, t, c.L, c.k, c.d, gamma))
    assert same and err < K_TOL
    WR.forget()


@pytest.mark.parametrize("t", [0, 3])
def test_window_kernel_end_to_end_at_the_widest_window(dv, gw, t):
    """W = 2047 at stride 100 (tiles of 21 windows): bit identity with cross_kernel, and the same bytes from chunks of ten
    windows, whose edges lie inside the whole launch's stretch-limited tiles"""
    c = WC.E2E_WIDE
    gamma = 0.5 if t == 3 else 1.0
    x, y = WC.records(c.seed, c.comp, c.L, c.d, c.W, c.sx, c.sy, c.nx, c.ny)
    seen = []
    whole = gw.window_kernel(x, y, c.W, c.sx, c.sy, t, c.L, c.k, c.d, gamma, on_chunk=seen.append)
    assert len(seen) == 1 and seen[0]["kernel"] == "k_wsim_profiles" and (seen[0]["x_windows"], seen[0]["y_windows"]) == (c.nx, c.ny)
    want = WL.cross(dv, x, y, c.W, c.sx, c.sy, t, c.L, c.k, c.d, gamma)
    assert _same_k(whole["K"], want), np.argwhere(whole["K"] != want)[:5]
    assert np.isfinite(whole["K"]).all() and (whole["K"] > 0).all()
    seen = []
    cut = gw.window_kernel(x, y, c.W, c.sx, c.sy, t, c.L, c.k, c.d, gamma, chunk=WC.E2E_WIDE_CHUNK, on_chunk=seen.append)
    assert [(s["x_windows"], s["y_windows"]) for s in seen] == [(a, b) for a in (10, 10, 6) for b in (10, 10, 4)]
    for key in ("K", "x_starts", "y_starts", "x_valid", "y_valid"):
        assert cut[key].tobytes() == whole[key].tobytes(), key
    want_j, want_k = WR.best(whole["K"], whole["x_starts"], whole["y_starts"], 150)
    for chunk in (None, WC.E2E_WIDE_CHUNK):
        got = gw.window_best(x, y, c.W, c.sx, c.sy, t, c.L, c.k, c.d, gamma, min_separation=150, chunk=chunk)
        assert np.array_equal(got["y_start"], want_j) and got["K"].tobytes() == want_k.tobytes(), chunk


def _stretch_comparisons(n, s, g, windows):
    """gkmhip_scan_profiles' count: per stretch of gw windows the pairs (p, p + delta), 0 <= delta < n, once per strand"""
    total = 0
    for w0 in range(0, windows, g):
        S = n + (min(g, windows - w0) - 1) * s
        total += 2 * S * n - n * (n - 1)
    return total


@pytest.mark.parametrize("t", [0, 4])
@pytest.mark.parametrize("L,k,d,W,s", WC.SCAN_WIDE)
def test_scan_profiles_at_wide_windows(dv, t, L, k, d, W, s):
    """k_scan_profiles' values where no test read them: n > 1024 (the delta loop runs past a workgroup's lanes) and groups
    cut short by the stretch, at g - 1, g, g + 1 and 2 g + 1 windows, against the oracle's self profile of the windows
    cut out (at W = 2047 of at most 19 of them: the ends of every stretch and evenly spaced ones)"""
    n = W - L + 1
    g = WC.group(n, s, WC.SP_GMAX)
    counts = WC.scan_counts(g, W)
    x = WC.scan_record(100 * L + s, "planted", W, s, max(counts))
    oracle = {}
    for windows in counts:
        xs = x[:WC.record_length(W, s, windows)]
        got, comparisons, lm = WL.scan_profiles(dv, t, L, k, d, xs, W, s)
        assert got.shape == (windows, d + 1) and np.array_equal(lm, SR.R.pack(xs, L))
        assert comparisons == _stretch_comparisons(n, s, g, windows)
        at = WC.scan_compared(L, W, g, windows)
        for i in at:
            if i not in oracle:
                oracle[i] = SR.self_profile(x[i * s:i * s + W], t, L, k, d)
        want = np.array([oracle[i] for i in at], dtype=np.int64)
        assert np.array_equal(got[at], want), (t, L, W, s, windows, [at[i] for i in np.flatnonzero((got[at] != want).any(axis=1))[:5]])
        assert (want[:, 0] > 0).all()


def _scan_score(dv, t, L, x, W, s, table):
    """gkmhip_scan_lmers + gkmhip_scan_score over every window of x with the weights of kernel type t -> (scores, wt)"""
    import torch
    ctx = dv.GramContext(t, L, 3, 3, device=0)
    try:
        stream = torch.cuda.current_stream().cuda_stream
        d_x = torch.from_numpy(np.ascontiguousarray(x, dtype=np.uint8)).cuda()
        d_v = torch.ones(len(x), dtype=torch.uint8, device="cuda")
        nlm = len(x) - L + 1
        lm = torch.full((nlm + 64,), -1, dtype=torch.int32, device="cuda")
        ctx.scan_lmers(d_x.data_ptr(), d_v.data_ptr(), len(x), lm.data_ptr(), stream)
        nwin = len(SR.starts(len(x), W, s))
        wt = dv.position_weights(t, W - L + 1)
        d_wt = torch.from_numpy(wt).cuda()
        d_tab = torch.from_numpy(np.ascontiguousarray(table, dtype=np.float64)).cuda()
        out = torch.full((nwin + 1,), -7.5, dtype=torch.float64, device="cuda")
        ctx.scan_score(lm.data_ptr(), nlm, d_wt.data_ptr(), W, s, nwin, d_tab.data_ptr(), out.data_ptr(), stream)
        torch.cuda.synchronize()
        assert ctx.last_kernel_name() == "k_scan_score" and ctx.last_comparisons() == nwin * (W - L + 1)
        assert (lm[nlm:] == -1).all() and out[nwin] == -7.5
        return out[:nwin].cpu().numpy(), wt
    finally:
        ctx.close()


@pytest.mark.parametrize("t", [0, 4])
def test_scan_score_of_an_integer_table_at_wide_windows(dv, t):
    """a table of small integers: every product and every partial sum is an exact integer below 2^53, so any summation
    order gives the exact sum and numpy's integer sum must match bit for bit"""
    L = WC.SCORE_L
    table = np.random.default_rng(6).integers(-50, 51, size=4 ** L)
    for _, _, _, W, s in WC.SCAN_WIDE:
        x = WC.scan_record(W + s, "planted", W, s, 22)
        got, wt = _scan_score(dv, t, L, x, W, s, table)
        codes = SR.R.pack(x, L).astype(np.int64)
        n = W - L + 1
        want = np.array([int(np.dot(wt.astype(np.int64), table[codes[a:a + n]])) for a in SR.starts(len(x), W, s)])
        assert len(want) == 22 and np.abs(wt.astype(np.int64)).sum() * 50 < 2 ** 53 and (want != 0).any()
        assert got.tobytes() == want.astype(np.float64).tobytes(), (t, W, s, np.flatnonzero(got != want)[:5])


@pytest.mark.parametrize("t", [0, 4])
def test_scan_of_a_table_of_random_doubles_at_wide_windows(gp, t):
    """`scan` with a table of random doubles: byte for byte score_with_table on the windows cut out"""
    from gkmqc_amd import gkmtables
    from tests import lmer_ref as LR
    L = WC.SCORE_L
    rng = np.random.default_rng(7 + t)
    W_ = rng.standard_normal(4 ** L) * 10.0 ** rng.integers(-3, 3, size=4 ** L)
    u = np.arange(4 ** L)
    W_ = np.where(u <= LR.rc_codes(u, L), W_, W_[LR.rc_codes(u, L)])       # W[u] == W[rc u], as a folded model's
    table = gkmtables.LmerTable(W_, t, L, 3, 3, 50, 50.0, 0.25)
    for _, _, _, W, s in WC.SCAN_WIDE:
        x = WC.scan_record(W + s + 1, "planted", W, s, 22)
        (_, starts, got), = gp.scan(table, [x], W, s)
        assert starts.tolist() == SR.starts(len(x), W, s) and len(starts) == 22
        _, want = gp.score_with_table(table, [w for _, w in SR.windows(x, W, s)])
        assert got.dtype == np.float64 and got.tobytes() == np.asarray(want).tobytes(), (t, W, s, np.flatnonzero(got != want)[:5])
        assert np.isfinite(got).all()


@pytest.fixture(scope="module")
def ctx10(dv):
    c = dv.GramContext(4, TR.L, 6, 3, device=0)
    yield c
    c.close()


@pytest.mark.parametrize("stride,nwin", [(1, 300), (2100, 6)])
def test_word_counts_at_the_widest_window(ctx10, stride, nwin):
    """the prefix counts of flagged words (gkm_wordcnt.h) through gkmhip_regions_count / fill and gkmhip_dist_edges at
    width 2047: a flagged word at a window's first l-mer, at a window's last, and (stride 2100) in the gap between two
    disjoint windows, where it fails no window"""
    L, width = TR.L, 2047
    n = width - L + 1
    nlm = (nwin - 1) * stride + n
    first, last = (100, 250) if stride == 1 else (1, 3)
    flags = np.zeros(nlm, bool)
    flags[[first * stride, last * stride + n - 1]] = True
    if stride > n:
        flags[4 * stride + n + 20] = True                                  # between windows 4 and 5
        assert 4 * stride + n + 20 < 5 * stride
    covers = np.array([flags[i * stride:i * stride + n].any() for i in range(nwin)])
    valid = TR._valid(flags, nwin, width, stride)
    assert np.array_equal(valid, ~covers) and np.array_equal(valid, TD._valid(flags, nwin, width, stride))
    want_valid = (np.arange(nwin) > 100) & (np.arange(nwin) < 250) if stride == 1 else np.array([1, 0, 1, 0, 1, 1], bool)
    assert np.array_equal(valid, want_valid)
    s = np.random.default_rng(stride).standard_normal(nwin)
    s[first] = s[last] = 9.0                                               # the largest scores sit at failed windows
    launch = TR.Launch(ctx10, s, -INF, 0, width=width, stride=stride, flags=flags)
    want = TR._check(launch, "every valid window")
    assert want["windows"].sum() == valid.sum() and 9.0 not in want["peak"]
    assert len(want["first"]) == (1 if stride == 1 else 3)
    TR._check(TR.Launch(ctx10, s, 0.0, 1, width=width, stride=stride, flags=flags), "thresholded")
    dist = TD.Launch(ctx10, s, width=width, stride=stride, flags=flags)
    edges = np.array([-1.0, 0.0, 0.5, 8.0])
    got = dist.edges(edges)
    assert np.array_equal(got, dist.want_edges(edges)) and got.sum() == valid.sum() and got[-1] == 0
    assert RR.window_regions(launch.ref_scores, -INF, 0)["windows"].sum() == valid.sum()
