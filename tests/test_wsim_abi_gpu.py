"""The window-pair entry points of include/gkm_hip.h on the GPU (gkm_wsim.hip: gkmhip_wsim_profiles,
gkmhip_wsim_normalize, gkmhip_wsim_best): a leading dimension larger than the block leaves the padding cells' bytes
alone, a NULL profile pointer writes only G, the work runs on the stream it is given, and refused arguments return error
2 and write nothing."""
import math

import numpy as np
import pytest

from tests import abi_cases as A

pytestmark = pytest.mark.gpu

L, K, D = 8, 5, 3
W, SX, SY = 40, 3, 5
TX, TY = W + 36 * SX, W + 33 * SY                      # 37 x 34 windows: two tiles on either axis
NWX, NWY = 37, 34


@pytest.fixture(scope="module")
def dv(built):
    from gkmqc_amd import device
    return device


@pytest.fixture(scope="module")
def ctx(dv):
    c = dv.GramContext(3, L, K, D, gamma=1.5, device=0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def words(ctx):
    """the l-mer words of two records (one flagged base in y) and the windows' norms, complete before any test reads them"""
    import torch
    rng = np.random.default_rng(77)
    out = []
    for T, bad in ((TX, None), (TY, 60)):
        x = torch.from_numpy(rng.integers(0, 4, size=T, dtype=np.uint8)).cuda()
        v = torch.ones(T, dtype=torch.uint8, device="cuda")
        if bad is not None:
            v[bad] = 0
        lm = torch.empty(T - L + 1, dtype=torch.int32, device="cuda")
        ctx.scan_lmers(x.data_ptr(), v.data_ptr(), T, lm.data_ptr(), 0)
        out.append(lm)
    sqx = torch.from_numpy(rng.random(NWX) + 20.0).cuda()
    sqy = torch.from_numpy(rng.random(NWY) + 20.0).cuda()
    sqy[12] = float("nan")
    torch.cuda.synchronize()
    return out[0], out[1], sqx, sqy


def _profiles(ctx, words, G, ld, P, stream=0, nwx=NWX, nwy=NWY):
    lmx, lmy, _, _ = words
    ctx.wsim_profiles(lmx.data_ptr(), lmx.numel(), lmy.data_ptr(), lmy.numel(), W, SX, SY, nwx, nwy, G.data_ptr(), ld,
                      None if P is None else P.data_ptr(), stream)


def _pad(ld):
    m = np.zeros((NWX + 1, ld), dtype=bool)
    m[:, NWY:] = True
    m[NWX] = True
    return m


@pytest.mark.parametrize("ld", [NWY, NWY + 3, 2 * NWY + 1])
def test_leading_dimension_and_untouched_cells(ctx, words, ld):
    import torch
    _, _, sqx, sqy = words
    ref_G, ref_P = A.sentinel_f64((NWX, NWY)), A.sentinel_i32((NWX, NWY, D + 1))
    _profiles(ctx, words, ref_G, NWY, ref_P)
    G, P = A.sentinel_f64((NWX + 1, ld)), A.sentinel_i32((NWX + 1, NWY, D + 1))
    _profiles(ctx, words, G, ld, P)
    torch.cuda.synchronize()
    assert A.untouched(G, _pad(ld)) and A.untouched(P[NWX:], np.ones((1, NWY), bool))
    assert A.same_bytes(G[:NWX, :NWY], ref_G) and A.same_bytes(P[:NWX], ref_P)
    assert not A.untouched(ref_G, np.ones((NWX, NWY), bool)) and (ref_P >= 0).all() and (ref_P[:, :, D] > 0).any()
    # a NULL profile pointer: the same G, nothing else
    G2 = A.sentinel_f64((NWX + 1, ld))
    _profiles(ctx, words, G2, ld, None)
    torch.cuda.synchronize()
    assert A.same_bytes(G2, G)
    # normalisation in place: the padding keeps its bytes, a NaN norm makes its column NaN and nothing else
    raw = G[:NWX, :NWY].cpu().numpy()
    ctx.wsim_normalize(G.data_ptr(), ld, NWX, NWY, sqx.data_ptr(), sqy.data_ptr(), 0)
    torch.cuda.synchronize()
    assert ctx.last_kernel_name() == "k_wsim_normalize" and A.untouched(G, _pad(ld))
    got = G[:NWX, :NWY].cpu().numpy()
    lin = raw / (sqx.cpu().numpy()[:, None] * sqy.cpu().numpy()[None, :])
    assert np.array_equal(np.isnan(got), np.isnan(lin)) and np.isnan(got[:, 12]).all() and np.isnan(got).sum() == NWX
    ok = ~np.isnan(lin)
    assert np.abs(got[ok] / np.exp(1.5 * (lin[ok] - 1)) - 1).max() < 1e-12
    # the best column per row from the padded matrix: the padding (sentinel NaNs) and the NaN column never win
    bj, bk = torch.full((NWX + 1,), -9, dtype=torch.int64, device="cuda"), A.sentinel_f64((NWX + 1,))
    ctx.wsim_best(G.data_ptr(), ld, NWX, NWY, 0, SX, 0, SY, 0, bj.data_ptr(), bk.data_ptr(), 0)
    torch.cuda.synchronize()
    assert ctx.last_kernel_name() == "k_wsim_best" and int(bj[NWX]) == -9 and A.untouched(bk[NWX:], np.ones(1, bool))
    want = np.nanargmax(got, axis=1)
    assert np.array_equal(bj[:NWX].cpu().numpy(), want) and 12 not in want
    assert bk[:NWX].cpu().numpy().tobytes() == got[np.arange(NWX), want].tobytes()


def test_flagged_words_take_part_in_no_pair(ctx, words):
    """(the flagged base of y sits in l-mers 53..60: a column over them counts fewer pairs than it would)"""
    import torch
    lmx, lmy, _, _ = words
    P = A.sentinel_i32((NWX, NWY, D + 1))
    G = A.sentinel_f64((NWX, NWY))
    _profiles(ctx, words, G, NWY, P)
    clean = lmy.clone()
    clean &= 0x7FFFFFFF
    P2, G2 = A.sentinel_i32((NWX, NWY, D + 1)), A.sentinel_f64((NWX, NWY))
    ctx.wsim_profiles(lmx.data_ptr(), lmx.numel(), clean.data_ptr(), clean.numel(), W, SX, SY, NWX, NWY, G2.data_ptr(), NWY,
                      P2.data_ptr(), 0)
    torch.cuda.synchronize()
    n = W - L + 1
    over = np.array([j * SY <= 60 and 53 < j * SY + n for j in range(NWY)])
    P, P2 = P.cpu().numpy(), P2.cpu().numpy()
    assert over.any() and not over.all()
    assert np.array_equal(P[:, ~over], P2[:, ~over]) and (P[:, over] <= P2[:, over]).all()
    assert (P[:, over].sum(axis=(0, 2)) < P2[:, over].sum(axis=(0, 2))).all()


def test_work_runs_on_the_given_stream(ctx, words):
    """the three calls behind a delay on a side stream, the outputs filled with sentinels on that stream just before:
    work put on another stream would run during the delay and be overwritten by the fill"""
    import torch
    _, _, sqx, sqy = words
    ld = NWY + 3

    def run(stream, G, P, bj, bk):
        _profiles(ctx, words, G, ld, P, stream)
        ctx.wsim_normalize(G.data_ptr(), ld, NWX, NWY, sqx.data_ptr(), sqy.data_ptr(), stream)
        ctx.wsim_best(G.data_ptr(), ld, NWX, NWY, 0, SX, 0, SY, 10, bj.data_ptr(), bk.data_ptr(), stream)

    def outputs():
        return (A.sentinel_f64((NWX, ld)), A.sentinel_i32((NWX, NWY, D + 1)),
                torch.full((NWX,), -9, dtype=torch.int64, device="cuda"), A.sentinel_f64((NWX,)))

    want = outputs()
    run(0, *want)
    torch.cuda.synchronize()
    ms = max(ctx.last_kernel_ms(), 0.0)
    got = outputs()
    buf = torch.empty(1 << 25, dtype=torch.float64, device="cuda")         # 256 MiB: a fill takes a fraction of a millisecond
    buf.fill_(0.0)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    fills = 64
    while True:
        with torch.cuda.stream(side):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for i in range(fills):
                buf.fill_(float(i))
            e1.record()
            A.refill(got[0])
            A.refill(got[1])
            got[2].fill_(-9)
            A.refill(got[3])
            run(side.cuda_stream, *got)
            side.synchronize()
        took = e0.elapsed_time(e1)
        if took >= max(20.0, 10.0 * ms) or fills >= 4096:
            break
        fills *= 2
    print("delay %.1f ms before calls whose last kernel took %.3f ms" % (took, ms))
    assert took >= 10.0 * ms
    for g, w in zip(got, want):
        assert A.same_bytes(g, w)
    assert not A.untouched(got[0][:, :NWY], np.ones((NWX, NWY), bool)) and (got[2] != -9).all()


def test_refused_arguments_return_error_2_and_write_nothing(ctx, dv, words):
    import torch
    lmx, lmy, sqx, sqy = words
    G, P = A.sentinel_f64((NWX, NWY)), A.sentinel_i32((NWX, NWY, D + 1))
    bj, bk = torch.full((NWX,), -9, dtype=torch.int64, device="cuda"), A.sentinel_f64((NWX,))
    good = dict(lmx=lmx.data_ptr(), nlmx=lmx.numel(), lmy=lmy.data_ptr(), nlmy=lmy.numel(), width=W, sx=SX, sy=SY, nwx=NWX,
                nwy=NWY, G=G.data_ptr(), ld=NWY, P=P.data_ptr())
    for kw in (dict(lmx=0), dict(lmy=0), dict(G=0), dict(width=L - 1), dict(width=2048), dict(sx=0), dict(sy=-1), dict(nwx=0),
               dict(nwy=0), dict(nwx=NWX + 1), dict(nwy=NWY + 1), dict(ld=NWY - 1), dict(nlmx=lmx.numel() - 1),
               dict(nlmy=lmy.numel() - 1), dict(nwx=(1 << 30) + 1), dict(nwx=1 << 20, nwy=1 << 20, nlmx=1 << 40, nlmy=1 << 40, ld=1 << 20)):
        with pytest.raises(dv.GkmError, match=r"gkmhip_wsim_profiles failed \(2\)"):
            ctx.wsim_profiles(*{**good, **kw}.values(), 0)
    ctx.wsim_profiles(*good.values(), 0)                                   # and the good arguments are served
    torch.cuda.synchronize()
    assert not A.untouched(G, np.ones((NWX, NWY), bool))
    A.refill(G)
    A.refill(P)
    for args in ((0, NWY, NWX, NWY, sqx.data_ptr(), sqy.data_ptr()), (G.data_ptr(), NWY - 1, NWX, NWY, sqx.data_ptr(), sqy.data_ptr()),
                 (G.data_ptr(), NWY, 0, NWY, sqx.data_ptr(), sqy.data_ptr()), (G.data_ptr(), NWY, NWX, NWY, 0, sqy.data_ptr()),
                 (G.data_ptr(), NWY, NWX, NWY, sqx.data_ptr(), 0)):
        with pytest.raises(dv.GkmError, match=r"gkmhip_wsim_normalize failed \(2\)"):
            ctx.wsim_normalize(*args, 0)
    g = G.data_ptr()
    for args in ((0, NWY, NWX, NWY, 0, SX, 0, SY, 0), (g, NWY - 1, NWX, NWY, 0, SX, 0, SY, 0), (g, NWY, NWX, 0, 0, SX, 0, SY, 0),
                 (g, NWY, NWX, NWY, -1, SX, 0, SY, 0), (g, NWY, NWX, NWY, 0, 0, 0, SY, 0), (g, NWY, NWX, NWY, 0, SX, 0, 0, 0),
                 (g, NWY, NWX, NWY, 0, SX, 0, SY, -1), (g, NWY, NWX, NWY, 0, SX, (1 << 40) + 1, SY, 0)):
        with pytest.raises(dv.GkmError, match=r"gkmhip_wsim_best failed \(2\)"):
            ctx.wsim_best(*args, bj.data_ptr(), bk.data_ptr(), 0)
    for outs in ((0, bk.data_ptr()), (bj.data_ptr(), 0)):
        with pytest.raises(dv.GkmError, match=r"\(2\)"):
            ctx.wsim_best(g, NWY, NWX, NWY, 0, SX, 0, SY, 0, *outs, 0)
    torch.cuda.synchronize()
    every = np.ones((NWX, NWY), bool)
    assert A.untouched(G, every) and A.untouched(P, every) and (bj == -9).all() and A.untouched(bk, np.ones(NWX, bool))
    assert math.isfinite(ctx.last_kernel_ms())
