"""The window contraction entry points of include/gkm_hip.h on the GPU (gkm_contract.hip: gkmhip_lmer_contract,
gkmhip_panel_contract): a leading dimension larger than the panel leaves the padding cells' bytes alone, the work runs on
the stream it is given, no windows means no launch, refused arguments return error 2 and write nothing, and the partial
values are the context's own: the calls take no scratch, and the size queries say what the context holds."""
import math

import numpy as np
import pytest

from tests import abi_cases as A
from tests import motif_ref as R

pytestmark = pytest.mark.gpu

NM, NWIN = 3, 37
LS = (5, 7)                 # one tile written straight to the output; four tiles and the fold launch


@pytest.fixture(scope="module")
def dv(built):
    from gkmqc_amd import device
    return device


@pytest.fixture(scope="module")
def problems(dv):
    """per L: a context, three tables on the device alone and as a panel image, NWIN windows; complete before any test"""
    import torch
    out = {}
    for L in LS:
        rng = np.random.default_rng(L)
        Ws = [R.symmetric_table(rng, L) for _ in range(NM)]
        rows = np.zeros((4 ** L, 8))
        rows[:, :NM] = np.stack(Ws, axis=1)
        P = rng.dirichlet(np.ones(4), size=(NWIN, L))
        out[L] = dict(ctx=dv.GramContext(2, L, L - 1, 1, device=0), W=[torch.from_numpy(W).cuda() for W in Ws],
                      rows=torch.from_numpy(rows).cuda(), P=torch.from_numpy(P).cuda(), hW=Ws, hP=P)
    torch.cuda.synchronize()
    yield out
    for p in out.values():
        p["ctx"].close()


def test_scratch_belongs_to_the_context(dv):
    assert dv.contract_scratch_bytes(5, 0, 1000) == 0 and dv.contract_scratch_bytes(6, 64, 1000) == 0
    assert dv.contract_scratch_bytes(7, 0, 10) == 10 * 4 * 8 and dv.contract_scratch_bytes(7, NM, 10) == 10 * 4 * 8 * 8
    assert dv.contract_scratch_bytes(12, 64, 1) == 4096 * 64 * 8
    assert dv.contract_max_windows(10, 0) == 65536 and dv.contract_max_windows(12, 64) == (1 << 32) // (4096 * 64 * 8)
    assert dv.contract_max_windows(1, 0) == dv.contract_max_windows(13, 0) == dv.contract_max_windows(5, 65) == -1
    assert dv.contract_scratch_bytes(7, 0, -1) == dv.contract_scratch_bytes(7, 0, 65537) == -1
    lib = dv.load()
    assert len(lib.gkmhip_lmer_contract.argtypes) == 6 and len(lib.gkmhip_panel_contract.argtypes) == 9


@pytest.mark.parametrize("L", LS)
@pytest.mark.parametrize("ld", [NM, NM + 2, 2 * NM + 1])
def test_leading_dimension_and_untouched_cells(problems, L, ld):
    import torch
    p = problems[L]
    ctx = p["ctx"]
    single = [A.sentinel_f64((NWIN + 1,)) for _ in range(NM)]
    for W, o in zip(p["W"], single):
        ctx.lmer_contract(W.data_ptr(), p["P"].data_ptr(), NWIN, o.data_ptr(), 0)
    assert ctx.last_kernel_name() == "k_lmer_contract" and ctx.last_comparisons() == NWIN * 4.0 ** L
    out = A.sentinel_f64((NWIN + 1, ld))
    ctx.panel_contract(p["rows"].data_ptr(), NM, 8, p["P"].data_ptr(), NWIN, out.data_ptr(), ld, 0)
    torch.cuda.synchronize()
    assert ctx.last_kernel_name() == "k_panel_contract" and ctx.last_comparisons() == NWIN * NM * 4.0 ** L
    assert math.isfinite(ctx.last_kernel_ms()) and ctx.last_kernel_ms() > 0
    pad = np.zeros((NWIN + 1, ld), dtype=bool)
    pad[:, NM:] = True
    pad[NWIN] = True
    assert A.untouched(out, pad)
    for m in range(NM):
        assert A.untouched(single[m][NWIN:], np.ones(1, bool))
        assert A.same_bytes(out[:NWIN, m].contiguous(), single[m][:NWIN])
        assert single[m][:NWIN].cpu().numpy().tobytes() == R.contract_many(p["hW"][m], p["hP"]).tobytes()


@pytest.mark.parametrize("L", LS)
def test_no_windows_launch_nothing(dv, problems, L):
    import torch
    p = problems[L]
    fresh = dv.GramContext(2, L, L - 1, 1, device=0)
    try:
        out = A.sentinel_f64((4, NM))
        fresh.lmer_contract(p["W"][0].data_ptr(), p["P"].data_ptr(), 0, out.data_ptr(), 0)
        fresh.panel_contract(p["rows"].data_ptr(), NM, 8, p["P"].data_ptr(), 0, out.data_ptr(), NM, 0)
        torch.cuda.synchronize()
        assert fresh.last_kernel_name() == "none" and fresh.last_comparisons() == 0
        assert A.untouched(out, np.ones((4, NM), bool))
    finally:
        fresh.close()


@pytest.mark.parametrize("L", LS)
def test_work_runs_on_the_given_stream(problems, L):
    """the two calls behind a delay on a side stream, the outputs filled with sentinels on that stream just before: work put
    on another stream would run during the delay and be overwritten by the fill"""
    import torch
    p = problems[L]
    ctx = p["ctx"]

    def run(stream, one, many):
        ctx.lmer_contract(p["W"][1].data_ptr(), p["P"].data_ptr(), NWIN, one.data_ptr(), stream)
        ctx.panel_contract(p["rows"].data_ptr(), NM, 8, p["P"].data_ptr(), NWIN, many.data_ptr(), NM + 1, stream)

    def outputs():
        return A.sentinel_f64((NWIN,)), A.sentinel_f64((NWIN, NM + 1))

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
    assert not A.untouched(got[0], np.ones(NWIN, bool)) and A.untouched(got[1][:, NM:], np.ones((NWIN, 1), bool))


@pytest.mark.parametrize("L", LS)
def test_refused_arguments_return_error_2_and_write_nothing(dv, problems, L):
    import torch
    p = problems[L]
    ctx = p["ctx"]
    one, many = A.sentinel_f64((NWIN,)), A.sentinel_f64((NWIN, NM + 1))
    good = dict(W=p["W"][0].data_ptr(), P=p["P"].data_ptr(), nwin=NWIN, out=one.data_ptr())
    for kw in (dict(W=0), dict(P=0), dict(out=0), dict(nwin=-1), dict(nwin=65537), dict(nwin=1 << 40)):
        with pytest.raises(dv.GkmError, match=r"gkmhip_lmer_contract failed \(2\)"):
            ctx.lmer_contract(*{**good, **kw}.values(), 0)
    good = dict(rows=p["rows"].data_ptr(), nm=NM, ms=8, P=p["P"].data_ptr(), nwin=NWIN, out=many.data_ptr(), ld=NM + 1)
    for kw in (dict(rows=0), dict(P=0), dict(out=0), dict(nwin=-1), dict(nwin=65537), dict(ld=NM - 1), dict(ld=0), dict(nm=0),
               dict(nm=65, ms=72, ld=65), dict(nm=9), dict(ms=12), dict(ms=0)):
        with pytest.raises(dv.GkmError, match=r"gkmhip_panel_contract failed \(2\)"):
            ctx.panel_contract(*{**good, **kw}.values(), 0)
    torch.cuda.synchronize()
    assert A.untouched(one, np.ones(NWIN, bool)) and A.untouched(many, np.ones((NWIN, NM + 1), bool))
    ctx.panel_contract(*good.values(), 0)                                  # and the good arguments are served
    torch.cuda.synchronize()
    assert not A.untouched(many[:, :NM], np.ones((NWIN, NM), bool)) and A.untouched(many[:, NM:], np.ones((NWIN, 1), bool))
