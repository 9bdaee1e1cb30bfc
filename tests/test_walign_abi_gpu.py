"""The window-alignment entry points of include/gkm_hip.h on the GPU (gkm_walign.hip: gkmhip_walign_block,
gkmhip_walign_trace) driven with synthetic K and D tensors against tests/walign_ref.py: every direction byte, the edge
vectors updated in place and the best cell across the tile edges, ties, NaNs, both column orders and non-zero edges;
leading dimensions and untouched cells, the score-only run, the launch bracket, the stream, refusals; the traceback."""
import numpy as np
import pytest

from tests import abi_cases as A
from tests import walign_ref as R

pytestmark = pytest.mark.gpu

OFFSET, GAP = 0.75, 0.25
BYTE = 0xEE                      # what an untouched cell of D holds (no direction)
TIES = np.array([0.0, 0.25, 0.5, 0.75, 1.0, np.nan])


@pytest.fixture(scope="module")
def dv(built):
    from gkmqc_amd import device
    return device


@pytest.fixture(scope="module")
def ctx(dv):
    c = dv.GramContext(0, 8, 5, 3, device=0)
    yield c
    c.close()


def _values(rng, kind, shape):
    """tie-heavy: quarters and NaNs, so that equal candidates meet in most cells; iid: uniform doubles, a few NaNs"""
    if kind == "ties":
        return TIES[rng.integers(0, len(TIES), size=shape)]
    v = rng.random(shape)
    v[rng.random(shape) < 0.03] = np.nan
    return v


def _edges(rng, kind, m, n):
    """non-zero cells beyond the upper and left edge: (top, left, corner)"""
    if kind == "ties":
        return rng.integers(0, 9, size=n) * 0.25, rng.integers(0, 9, size=m) * 0.25, float(rng.integers(1, 9)) * 0.25
    return rng.random(n) * 2, rng.random(m) * 2, float(rng.random()) * 2


class Run:
    """one call of gkmhip_walign_block on sentinel-padded device arrays"""

    def __init__(self, K, top, left, corner, ld=None, ldd=None, with_D=True):
        import torch
        m, n = K.shape
        self.m, self.n = m, n
        self.ld, self.ldd = ld or n, ldd or n
        self.K = torch.full((m + 1, self.ld), 1e30, dtype=torch.float64, device="cuda")   # a pad that would win every cell
        self.K[:m, :n] = torch.from_numpy(K).cuda()
        self.top, self.left = A.sentinel_f64((n + 1,)), A.sentinel_f64((m + 1,))
        self.top[:n] = torch.from_numpy(np.asarray(top, dtype=np.float64)).cuda()
        self.left[:m] = torch.from_numpy(np.asarray(left, dtype=np.float64)).cuda()
        self.corner = torch.tensor([corner], dtype=torch.float64, device="cuda")
        self.D = torch.full((m + 1, self.ldd), BYTE, dtype=torch.uint8, device="cuda") if with_D else None
        self.bh = A.sentinel_f64((2,))
        self.bic = torch.full((3,), -9, dtype=torch.int64, device="cuda")

    def call(self, ctx, dv, flip, offset=OFFSET, gap=GAP, stream=0, **kw):
        import torch
        need = dv.walign_scratch_bytes(self.m, self.n)
        self.scratch = torch.zeros(max(need, 8) // 8 + 1, dtype=torch.int64, device="cuda")
        args = dict(K=self.K.data_ptr(), ld=self.ld, nwx=self.m, nwy=self.n, flip=flip, offset=offset, gap=gap,
                    top=self.top.data_ptr(), left=self.left.data_ptr(), corner=self.corner.data_ptr(),
                    D=None if self.D is None else self.D.data_ptr(), ldd=self.ldd, bh=self.bh.data_ptr(),
                    bic=self.bic.data_ptr(), scratch=self.scratch.data_ptr(), scratch_bytes=need)
        args.update(kw)
        ctx.walign_block(*args.values(), stream)

    def check(self, H, D, what):
        """every byte against the reference's H and D of the same inputs"""
        m, n = self.m, self.n
        if self.D is not None:
            got = self.D.cpu().numpy()
            assert np.array_equal(got[:m, :n], D), (what, np.argwhere(got[:m, :n] != D)[:5])
            assert (got[:m, n:] == BYTE).all() and (got[m] == BYTE).all(), what
        assert A.same_bytes(self.top[:n], H[-1]) and A.same_bytes(self.left[:m], H[:, -1]), what
        assert A.untouched(self.top[n:], np.ones(1, bool)) and A.untouched(self.left[m:], np.ones(1, bool)), what
        h, i, c = R.best_cell(H)
        assert A.same_bytes(self.bh[:1], np.array([h])) and self.bic.tolist() == [i, c, -9], (what, self.bh[0].item(), self.bic)
        assert A.untouched(self.bh[1:], np.ones(1, bool)), what

    def untouched(self):
        n, m = self.n, self.m
        return (A.untouched(self.bh, np.ones(2, bool)) and self.bic.tolist() == [-9, -9, -9]
                and (self.D is None or bool((self.D == BYTE).all()))
                and A.untouched(self.top[n:], np.ones(1, bool)) and A.untouched(self.left[m:], np.ones(1, bool)))


def test_tile_shape_needs_no_device(dv):
    r, c = dv.walign_tile()
    assert r == 64 and c >= 64 and dv.walign_scratch_bytes(r, c) > 0 and dv.walign_scratch_bytes(0, c) == -1


@pytest.mark.parametrize("flip", [0, 1])
@pytest.mark.parametrize("kind", ["ties", "iid"])
def test_tile_edges(ctx, dv, kind, flip):
    """1, R - 1, R, R + 1, 2 R + 1 rows by 1, C - 1, C, C + 1, 2 C + 1 columns of one matrix's upper left corner, with
    non-zero cells beyond the edges: D, the edge vectors and the best cell equal the reference"""
    import torch
    r, c = dv.walign_tile()
    rows, cols = (1, r - 1, r, r + 1, 2 * r + 1), (1, c - 1, c, c + 1, 2 * c + 1)
    rng = np.random.default_rng(11 + flip + 2 * (kind == "iid"))
    K = _values(rng, kind, (rows[-1], cols[-1]))
    top, left, corner = _edges(rng, kind, rows[-1], cols[-1])
    some_positive = False
    for m in rows:
        for n in cols:
            # the upper left corner in DP coordinates: with flip the LAST n columns of K's rows, mirrored by the call
            Kb = np.ascontiguousarray(K[:m, cols[-1] - n:] if flip else K[:m, :n])
            run = Run(Kb, top[:n], left[:m], corner)
            run.call(ctx, dv, flip)
            torch.cuda.synchronize()
            assert ctx.last_kernel_name() == "k_walign_tiles" and ctx.last_comparisons() == m * n
            H, D = R.dp_block(Kb, flip, OFFSET, GAP, top[:n], left[:m], corner)
            run.check(H, D, (kind, flip, m, n))
            some_positive |= bool((D == R.DIAG).any() and (D == R.UP).any() and (D == R.LEFT).any() and (D == R.STOP).any())
    assert some_positive


@pytest.mark.parametrize("flip", [0, 1])
def test_nan_rows_columns_and_zero_edges(ctx, dv, flip):
    """NaN rows, NaN columns and scattered NaNs: no diagonal step into them, gap steps across; zero edges, as a whole
    matrix has them; the best cell's ties broken by the lower i, then the lower c"""
    import torch
    r, c = dv.walign_tile()
    m, n = r + 7, c + 9
    rng = np.random.default_rng(13 + flip)
    K = _values(rng, "ties", (m, n))
    K[[3, 40, r - 1, r], :] = np.nan
    K[:, [0, c // 2, c - 1, c, n - 1]] = np.nan
    run = Run(K, np.zeros(n), np.zeros(m), 0.0)
    run.call(ctx, dv, flip)
    torch.cuda.synchronize()
    H, D = R.dp_block(K, flip, OFFSET, GAP, np.zeros(n), np.zeros(m), 0.0)
    run.check(H, D, flip)
    assert not (D[[3, 40, r - 1, r]] == R.DIAG).any() and (D[[40, r]] == R.UP).any()
    cols = [n - 1 - j for j in (0, c // 2, c - 1, c, n - 1)] if flip else [0, c // 2, c - 1, c, n - 1]
    assert not (D[:, cols] == R.DIAG).any() and (D[:, cols] == R.LEFT).any()
    assert (H == H.max()).sum() > 1                                        # the best value is tied
    # an all-NaN block and one below the offset: nothing positive
    for Kz in (np.full((m, n), np.nan), np.full((m, n), OFFSET)):
        run = Run(Kz, np.zeros(n), np.zeros(m), 0.0)
        run.call(ctx, dv, flip)
        torch.cuda.synchronize()
        run.check(np.zeros((m, n)), np.zeros((m, n), np.uint8), "nothing positive")
        assert run.bic.tolist()[:2] == [-1, -1] and run.bh[0].item() == 0.0


@pytest.mark.parametrize("flip", [0, 1])
def test_leading_dimensions_score_only_and_stream(ctx, dv, flip):
    import torch
    r, c = dv.walign_tile()
    m, n = r + 3, c + 5
    rng = np.random.default_rng(21 + flip)
    K = _values(rng, "iid", (m, n))
    top, left, corner = _edges(rng, "iid", m, n)
    H, D = R.dp_block(K, flip, OFFSET, GAP, top, left, corner)
    for ld, ldd in ((n + 3, n), (n, n + 5), (2 * n + 1, n + 8)):
        run = Run(K, top, left, corner, ld, ldd)
        run.call(ctx, dv, flip)
        torch.cuda.synchronize()
        run.check(H, D, (ld, ldd))
    run = Run(K, top, left, corner, n + 3, with_D=False)                   # D = NULL: the same edges and best cell
    run.call(ctx, dv, flip)
    torch.cuda.synchronize()
    run.check(H, D, "score only")
    # a side stream behind a delay, the outputs refilled with sentinels on that stream just before: work put on another
    # stream would run during the delay and be overwritten by the refill
    side = torch.cuda.Stream()
    buf = torch.empty(1 << 25, dtype=torch.float64, device="cuda")
    buf.fill_(0.0)
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        run = Run(K, top, left, corner, n + 3, n + 5)
        side.synchronize()
        for i in range(64):
            buf.fill_(float(i))
        run.D.fill_(BYTE)
        A.refill(run.bh)
        run.bic.fill_(-9)
        run.call(ctx, dv, flip, stream=side.cuda_stream)
        side.synchronize()
    run.check(H, D, "side stream")


def test_refused_arguments_return_error_2_and_write_nothing(ctx, dv):
    import torch
    m, n = 70, 300
    rng = np.random.default_rng(3)
    K = _values(rng, "iid", (m, n))
    top, left, corner = _edges(rng, "iid", m, n)
    run = Run(K, top, left, corner)
    before = (run.top.clone(), run.left.clone())
    need = dv.walign_scratch_bytes(m, n)
    for kw in (dict(K=None), dict(top=None), dict(left=None), dict(corner=None), dict(bh=None), dict(bic=None),
               dict(scratch=None), dict(ld=n - 1), dict(ldd=n - 1), dict(nwx=0), dict(nwy=0), dict(nwx=(1 << 20) + 1),
               dict(nwy=(1 << 20) + 1), dict(offset=float("nan")), dict(offset=float("inf")), dict(gap=-0.5),
               dict(gap=float("nan")), dict(gap=float("inf")), dict(scratch_bytes=need - 1), dict(scratch_bytes=0)):
        with pytest.raises(dv.GkmError, match=r"gkmhip_walign_block failed \(2\)"):
            run.call(ctx, dv, 0, **kw)
    torch.cuda.synchronize()
    assert run.untouched() and A.same_bytes(run.top, before[0]) and A.same_bytes(run.left, before[1])
    run.call(ctx, dv, 0)                                                   # and the good arguments are served
    torch.cuda.synchronize()
    run.check(*R.dp_block(K, 0, OFFSET, GAP, top, left, corner), "served")
    # the trace
    D = torch.full((m, n), 1, dtype=torch.uint8, device="cuda")
    path, count = A.sentinel_i32((m + 1, 2)), torch.full((3,), -9, dtype=torch.int64, device="cuda")
    good = dict(D=D.data_ptr(), ldd=n, nwx=m, nwy=n, end_i=m - 1, end_c=n - 1, path=path.data_ptr(), capacity=m,
                count=count.data_ptr())
    for kw in (dict(D=None), dict(path=None), dict(count=None), dict(ldd=n - 1), dict(nwx=0), dict(nwy=(1 << 20) + 1),
               dict(end_i=m), dict(end_i=-1), dict(end_c=n), dict(end_c=-1), dict(capacity=m - 1)):
        with pytest.raises(dv.GkmError, match=r"gkmhip_walign_trace failed \(2\)"):
            ctx.walign_trace(*{**good, **kw}.values(), 0)
    torch.cuda.synchronize()
    assert A.untouched(path, np.ones((m + 1, 2), bool)) and count.tolist() == [-9, -9, -9]


def _trace(ctx, D, end, ldd=None):
    """gkmhip_walign_trace on a numpy D -> (pairs from the end backwards, the cell at which the walk stopped)"""
    import torch
    m, n = D.shape
    ldd = ldd or n
    dD = torch.full((m + 1, ldd), 1, dtype=torch.uint8, device="cuda")     # (a pad of DIAG: a walk into it would go on)
    dD[:m, :n] = torch.from_numpy(D).cuda()
    cap = min(m, n)
    path, count = A.sentinel_i32((cap + 1, 2)), torch.full((4,), -9, dtype=torch.int64, device="cuda")
    ctx.walign_trace(dD.data_ptr(), ldd, m, n, end[0], end[1], path.data_ptr(), cap, count.data_ptr(), 0)
    torch.cuda.synchronize()
    assert ctx.last_kernel_name() == "k_walign_trace"
    k, si, sc, guard = count.tolist()
    assert guard == -9 and 0 <= k <= cap and A.untouched(path[k:], np.ones((cap + 1 - k, 2), bool))
    return [tuple(p) for p in path[:k].cpu().numpy().tolist()], (si, sc)


def test_trace(ctx):
    rng = np.random.default_rng(9)
    diag = lambda m, n: np.full((m, n), R.DIAG, dtype=np.uint8)            # noqa: E731
    cases = {}
    cases["longer than two squares, off both edges"] = (diag(200, 200), (199, 199))
    cases["off the top edge"] = (diag(50, 300), (49, 250))
    cases["off the left edge"] = (diag(300, 50), (280, 49))
    cases["an all-STOP start"] = (np.zeros((90, 130), dtype=np.uint8), (80, 100))
    gaps = diag(400, 500)
    gaps[150:, 300] = R.UP                                                 # 249 steps up column 300 ...
    gaps[150, 100:301] = R.LEFT                                            # ... 201 steps left along row 150, then the diagonal
    gaps[81, 30] = R.STOP
    cases["a long pure-gap run"] = (gaps, (399, 300))
    walk = rng.choice(np.array([R.DIAG, R.UP, R.LEFT], dtype=np.uint8), size=(300, 300), p=[0.5, 0.25, 0.25])
    cases["a random walk to an edge"] = (walk, (299, 299))
    stops = walk.copy()
    stops[rng.random((300, 300)) < 0.004] = R.STOP
    cases["a random walk to a STOP"] = (stops, (299, 290))
    corrupt = walk.copy()
    corrupt[rng.random((300, 300)) < 0.004] = 7
    cases["a byte that is no direction stops the walk"] = (corrupt, (299, 280))
    for name, (D, end) in cases.items():
        want_pairs, want_stop = R.trace(D, *end)
        for ldd in (None, D.shape[1] + 13):
            got_pairs, got_stop = _trace(ctx, D, end, ldd)
            assert got_stop == want_stop and got_pairs == want_pairs, (name, ldd, got_stop, want_stop, len(got_pairs))
    ref = lambda name: R.trace(cases[name][0], *cases[name][1])            # noqa: E731
    assert len(ref("longer than two squares, off both edges")[0]) == 200
    assert ref("off the top edge")[1] == (-1, 200) and ref("off the left edge")[1] == (230, -1)
    assert ref("an all-STOP start") == ([], (80, 100))
    assert ref("a long pure-gap run")[1] == (81, 30) and len(ref("a long pure-gap run")[0]) == 99 - 30
