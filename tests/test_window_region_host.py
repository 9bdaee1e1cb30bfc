"""The window kernels' case table (tests/window_cases.py) held to its conditions without a GPU: with the oracle and host
arithmetic alone, every case is what tests/test_window_region_gpu.py runs it for -- the LDS of a launch on the side of
64 KiB it claims, a stretch-limited group where one is claimed, a window pair of every mismatch class in the planted
inputs, the reference side of every test inside the budget -- and the numpy rendering of the tile formulation
(tests/wsim_ref.py) equals the oracle at d = L and on tiles of unequal, cut-short shape."""
import numpy as np
import pytest

from tests import window_cases as WC
from tests import wsim_ref as WR


@pytest.fixture(scope="module")
def dv(built):
    from gkmqc_amd import device
    return device


def _classes_seen(launch):
    """which classes m = 0..d have a window pair with P_m > 0 in the oracle's profiles of the launch's planted input
    (pairs are looked at until every class was seen: at W = 2047 a pair costs 29 ms)"""
    c = launch
    x, y = WC.records(c.seed, c.comp, c.L, c.d, c.W, c.sx, c.sy, c.nx, c.ny)
    wx, wy = WR.SR.windows(x, c.W, c.sx), WR.SR.windows(y, c.W, c.sy)
    assert len(wx) == c.nx and len(wy) == c.ny
    seen = np.zeros(c.d + 1, dtype=bool)
    for _, a in wx:
        for _, b in wy:
            seen |= WR.R.profile(a, b, 0, c.L, c.k, c.d) > 0
            if seen.all():
                return seen
    return seen


@pytest.mark.parametrize("L,k,d", WC.WSIM_LKD)
def test_region_launches_hold_every_class_within_the_budget(built, L, k, d):
    launches = WC.wsim_region_launches(L, k, d)
    assert {c.W for c in launches} == {L, L + 1, 64} | ({300} if d >= 9 else set())
    assert {(c.sx, c.sy) for c in launches if c.W == 64} == {(1, 1), (7, 3), (64, 1)}
    assert all((c.nx, c.ny) == (34, 12) for c in launches)
    assert all(c.comp == "planted" for c in launches if c.W == 300)        # dense inputs at the small shapes only
    for c in launches:
        if c.comp == "planted":
            assert _classes_seen(c).all(), c
    assert sum(WC.pair_cost(L, c.W, c.nx * c.ny) for c in launches) <= WC.BUDGET


def test_region_tuples_are_legal_and_reach_the_corners(dv):
    from oracle import oracle as O
    for L, k, d in WC.WSIM_LKD:
        assert dv.check_parameters(0, L, k, d) is None and O.lib().gkmo_check_params(0, L, k, d) is None
    assert min(L for L, _, _ in WC.WSIM_LKD) == 2 and max(d for _, _, d in WC.WSIM_LKD) == 12
    assert any(d == L for L, _, d in WC.WSIM_LKD) and any(d == L - 1 for L, _, d in WC.WSIM_LKD)
    assert sum(d >= 9 for _, _, d in WC.WSIM_LKD) == 5


@pytest.mark.parametrize("case", WC.WSIM_LDS, ids=[c.name for c in WC.WSIM_LDS])
def test_lds_cases_lie_on_their_side_of_64_kib(dv, case):
    c = case.launch
    n = c.W - c.L + 1
    gx, gy = dv.wsim_group(c.L, c.d, c.W, c.sx, c.sy)
    assert (gx, gy) == (WC.group(n, c.sx, WC.WS_GMAX), WC.group(n, c.sy, WC.WS_GMAX))
    words = n + (gy - 1) * c.sy
    lds = (c.d + 1) * (gx + 1) * (gy + 1) * 4 + 4 * words + ((2 * words + 3) // 4) * 4
    assert lds == WC.wsim_lds_bytes(c.L, c.d, c.W, c.sx, c.sy) == case.lds
    assert (lds > WC.LDS_64K) == case.above and lds <= 81204
    assert c.nx > gx and (c.ny > gy or c.W == 2047)                        # more than one tile
    pairs = c.nx * (1 if c.W == 2047 else c.ny)                            # (W = 2047: one test per window of y)
    assert WC.pair_cost(c.L, c.W, pairs) <= WC.BUDGET
    assert _classes_seen(c).all()
    if c.W == 2047:
        assert 1 < gx < WC.WS_GMAX and c.nx == gx + 1


def test_the_most_lds_below_d_9_is_the_control(built):
    """at d = 8 no shape passes 64 KiB: the control is the largest there is"""
    most = max(WC.wsim_lds_bytes(12, 8, W, s, s) for W in (300, 1000, 2047) for s in range(1, 200))
    full = 9 * 33 * 33 * 4 + 6 * 4096
    assert most <= full < WC.LDS_64K and [c.lds for c in WC.WSIM_LDS if not c.above] == [63632]


@pytest.mark.parametrize("sx,sy", WC.STRETCH_STRIDES)
def test_stretch_limited_tiles(dv, sx, sy):
    c, axis = WC.stretch_launch(sx, sy)
    g = dv.wsim_group(c.L, c.d, c.W, sx, sy)
    n = c.W - c.L + 1
    assert 1 < g[axis] == WC.STRETCH_G < WC.WS_GMAX and n + (g[axis] - 1) * 100 == 4037
    assert g[1 - axis] == {100: WC.STRETCH_G, 2037: 1, 1: 32}[(sx, sy)[1 - axis]]
    assert (c.nx, c.ny)[axis] == g[axis] + 1 and (c.nx, c.ny)[1 - axis] == 2
    assert WC.pair_cost(c.L, c.W, g[axis] + 1) <= WC.BUDGET                # (one test per window of the other axis)
    assert _classes_seen(c).all()


def test_scan_cases(dv):
    groups = []
    for L, k, d, W, s in WC.SCAN_WIDE:
        assert dv.check_parameters(0, L, k, d) is None and dv.check_parameters(4, L, k, d) is None
        n = W - L + 1
        g = WC.group(n, s, WC.SP_GMAX)
        groups.append(g)
        for windows in WC.scan_counts(g, W):
            at = WC.scan_compared(L, W, g, windows)
            assert at == sorted(set(at)) and 0 <= at[0] and at[-1] == windows - 1
            assert WC.pair_cost(L, W, len(at)) <= WC.BUDGET
            assert len(at) <= WC.SCAN_WIDE_CAP or W < 2047
            assert {i for i in (0, g - 2, g - 1, g) if i < windows} <= set(at)
    assert groups == [49, 9, 21, 63, 64]                                   # four stretch-limited groups ...
    assert all(1 < g < WC.SP_GMAX for g in groups[:4])
    assert sum(W - L + 1 > 1024 for L, _, _, W, _ in WC.SCAN_WIDE) == 4    # ... and n > 1024 with a full group of 64
    assert WC.scan_counts(9, 2047) == [8, 9, 10, 19] and WC.scan_counts(21, 2047) == [20, 21, 22]
    ctx_free = [WC.group(W - WC.SCORE_L + 1, s, WC.SP_GMAX) for _, _, _, W, s in WC.SCAN_WIDE]
    assert all(g >= 9 for g in ctx_free)


def test_end_to_end_cases(dv):
    from gkmqc_amd import gkmpredict as gp
    from gkmqc_amd import gkmwindows as gw
    c = WC.E2E_DL
    assert c.d == c.L and dv.check_parameters(3, c.L, c.k, c.d) is None
    assert WC.pair_cost(c.L, c.W, c.nx * c.ny + c.nx + c.ny) <= WC.BUDGET
    c = WC.E2E_WIDE
    gx, gy = dv.wsim_group(c.L, c.d, c.W, c.sx, c.sy)
    assert 1 < gx == gy == WC.STRETCH_G < c.ny <= c.nx
    plan = gp.scan_chunk_plan(WC.record_length(c.W, c.sx, c.nx), c.W, c.sx, WC.E2E_WIDE_CHUNK)
    edges = [w0 for w0, _, _, _ in plan[1:]]
    assert edges == [10, 20] and all(e % gx for e in edges)                # chunk edges inside the tiles of the whole launch
    assert gw.windows_per_chunk(c.W, c.sx, WC.E2E_WIDE_CHUNK) == 10


def test_generators_are_deterministic_and_exact_in_length(built):
    for comp in WC.COMPOSITIONS:
        a = WC.records(5, comp, 7, 7, 64, 7, 3, 34, 12, invalid=2)
        b = WC.records(5, comp, 7, 7, 64, 7, 3, 34, 12, invalid=2)
        assert all(np.array_equal(u, v) for u, v in zip(a, b))
        assert len(WR.SR.starts(len(a[0]), 64, 7)) == 34 and len(WR.SR.starts(len(a[1]), 64, 3)) == 12
        assert (a[0] >= 4).sum() == 2 and (a[1] >= 4).sum() == 2
    x, y = WC.records(6, "same", 5, 2, 20, 1, 1, 9, 9)
    assert np.array_equal(x, y) and (WC.records(6, "polyA", 5, 2, 20, 1, 1, 9, 9)[0] == 0).all()
    w = np.array([0, 1, 2, 3, 3, 0], dtype=np.uint8)
    assert WC.rc(w).tolist() == [3, 0, 0, 1, 2, 3]
    s = WC.substituted(np.random.default_rng(0), w, [1, 4])
    assert (s != w).tolist() == [False, True, False, False, True, False] and s.max() < 4
    assert WC.covered(20, 5, 6, 7).tolist() == [0, 1, 7, 8, 14, 15]
    z = WC.scan_record(3, "planted", 300, 10, 20, invalid=3)
    assert len(z) == 490 and (z >= 4).sum() == 3


def test_tile_rendering_equals_the_oracle_at_d_equal_to_l(built):
    """every pair is a hit (m <= L = d): all d + 1 planes of the difference array take corners"""
    L, k, d, W, sx, sy = 3, 0, 3, 8, 2, 3
    x, y = WC.records(1, "planted", L, d, W, sx, sy, 7, 5)
    got, comparisons = WR.tile_profiles(x, y, W, sx, sy, 3, 2, L, d)
    want = WR.profiles(x, y, W, sx, sy, 0, L, k, d)
    assert got.shape == want.shape == (7, 5, 4) and np.array_equal(got, want)
    assert (want.sum(axis=2) == 2 * 6 * 6).all() and (want > 0).any(axis=(0, 1)).all()
    assert comparisons == 2 * WC.tile_words(6, sx, 3, 7) * WC.tile_words(6, sy, 2, 5)


def test_tile_rendering_equals_the_oracle_on_cut_short_tiles(built):
    """the stretch-limited shapes at reduced size: as if a stretch held 64 words, n = 30 and stride 5 give g = 7 windows a
    tile; g - 1, g, g + 1 windows on that axis against 2 at a stride >= n (tiles of 1 x g), a stride of 1 and the same 5"""
    L, k, d, W, s = 11, 7, 3, 40, 5
    n = W - L + 1
    g = 1 + (64 - n) // s
    assert 1 < g == 7 < WC.WS_GMAX
    for other, g_other in ((30, 1), (1, 32), (5, g)):
        x, y = WC.records(other, "planted", L, d, W, other, s, 2, g + 1)
        whole = WR.profiles(x, y, W, other, s, 0, L, k, d)
        assert (whole > 0).any(axis=(0, 1)).all()
        for ny in (g - 1, g, g + 1):
            ys = y[:WC.record_length(W, s, ny)]
            got, comparisons = WR.tile_profiles(x, ys, W, other, s, g_other, g, L, d)
            assert np.array_equal(got, whole[:, :ny]), (other, ny)
            assert comparisons == 2 * WC.tile_words(n, other, g_other, 2) * WC.tile_words(n, s, g, ny)
            got_t, _ = WR.tile_profiles(ys, x, W, s, other, g, g_other, L, d)        # and with the limited axis along x
            assert np.array_equal(got_t, np.swapaxes(whole[:, :ny], 0, 1))
