"""The distribution entry points on the GPU (gkm_dist.hip: gkmhip_dist_digits, gkmhip_dist_edges, gkmhip_dist_collect;
DESIGN.md §5p): synthetic score arrays and l-mer words straight into the C calls, every histogram and every collected
multiset compared with numpy on the same arrays -- sizes around a wave's 64 lanes, a workgroup's 256 threads and its
span of 1024 windows, special values, flagged words, a leading dimension, guard bands, accumulation, every number of
prefixes, refusals, a capacity that is too small, and the same bytes on a second launch."""
import numpy as np
import pytest

from tests import dist_ref as DR

pytestmark = pytest.mark.gpu

L = 10
NAN, INF = float("nan"), float("inf")
GUARD, SPAN = 64, 1024                                                     # (a workgroup's windows: include/gkm_hip.h)
SIZES = (1, 63, 64, 65, 255, 256, 257, SPAN - 1, SPAN, SPAN + 1, 2 * SPAN + 3)
BITS = (12, 13, 13, 13, 13)
BOUNDS = (12, 25, 38, 51)


@pytest.fixture(scope="module")
def dv(built):
    from gkmqc_amd import device
    return device


@pytest.fixture(scope="module")
def ctx(dv):
    c = dv.GramContext(4, L, 6, 3, device=0)
    assert c.dist_digit_bits() == 13                                       # (BITS and BOUNDS above are written for it)
    yield c
    c.close()


def _valid(flags, nwin, width, stride):
    n = width - L + 1
    bad = np.concatenate(([0], np.cumsum(flags)))
    a = np.arange(nwin) * stride
    return bad[a + n] == bad[a]


def _special(n, rng):
    """normals with every special value among them, a NaN included"""
    s = rng.standard_normal(n)
    special = [INF, -INF, 0.0, -0.0, 5e-324, -5e-324, np.finfo(np.float64).max, -np.finfo(np.float64).max, 1.0,
               np.nextafter(1.0, 2.0), 1.0, NAN]
    at = rng.permutation(n)[:min(n, len(special))]
    s[at] = special[:len(at)]
    return s


class Launch:
    """one (scores, words, shape) on the device and its scratch with a guard band behind it"""

    def __init__(self, ctx, scores, width=L, stride=1, flags=None, ld=1, col=0, poison=INF):
        import torch
        self.ctx, self.width, self.stride, self.ld, self.col = ctx, width, stride, ld, col
        scores = np.asarray(scores, dtype=np.float64)
        self.nwin = len(scores)
        self.nlm = (self.nwin - 1) * stride + width - L + 1
        flags = np.zeros(self.nlm, bool) if flags is None else np.asarray(flags, bool)
        assert len(flags) == self.nlm
        self.ref = np.where(_valid(flags, self.nwin, width, stride), scores, NAN)   # unscored: NaN
        self.keys = DR.key(DR.scored(self.ref))
        host = np.full((self.nwin, ld), poison)
        host[:, col] = scores
        self.scores = torch.from_numpy(host).cuda()
        words = np.random.default_rng(1).integers(0, 4 ** L, size=self.nlm, dtype=np.uint32) | (flags.astype(np.uint32) << 31)
        self.lm = torch.from_numpy(words.view(np.int32)).cuda()
        self.sbytes = ctx.dist_scratch_bytes(self.nlm, self.nwin)
        assert self.sbytes > 0
        self.scratch = torch.full((self.sbytes + GUARD,), 0x5A, dtype=torch.uint8, device="cuda")
        self.stream = torch.cuda.current_stream().cuda_stream

    def args(self):
        return (self.scores.data_ptr() + 8 * self.col, self.ld, self.lm.data_ptr(), self.nlm, self.width, self.stride,
                self.nwin)

    def tail(self):
        return (self.scratch.data_ptr(), self.sbytes, self.stream)

    def intact(self):
        import torch
        torch.cuda.synchronize()
        return bool((self.scratch[self.sbytes:] == 0x5A).all())

    def counters(self, cells, start=0):
        """`cells` int64 counters at `start`, a 0x5A guard band behind them"""
        import torch
        buf = torch.full((cells + GUARD,), 0x5A5A5A5A5A5A5A5A, dtype=torch.int64, device="cuda")
        buf[:cells] = start
        return buf

    def digits(self, prefixes, prefix_bits, buf=None, times=1):
        """-> the (max(nprefix, 1), 2^bits) histogram after `times` accumulating calls; guards checked"""
        level = 0 if prefix_bits == 0 else BOUNDS.index(prefix_bits) + 1
        cells = max(len(prefixes), 1) << BITS[level]
        buf = self.counters(cells) if buf is None else buf
        for _ in range(times):
            self.ctx.dist_digits(*self.args(), prefixes, prefix_bits, buf.data_ptr(), *self.tail())
            assert self.ctx.last_kernel_name() == "k_dist_digits" and self.ctx.last_kernel_ms() >= 0.0
            assert self.ctx.last_comparisons() == self.nwin
        assert self.intact() and (buf[cells:] == 0x5A5A5A5A5A5A5A5A).all(), "a cell outside the histogram was written"
        return buf[:cells].cpu().numpy().reshape(max(len(prefixes), 1), -1)

    def want_digits(self, prefixes, prefix_bits):
        level = 0 if prefix_bits == 0 else BOUNDS.index(prefix_bits) + 1
        bits = BITS[level]
        digit = ((self.keys >> np.uint64(64 - prefix_bits - bits)) & np.uint64((1 << bits) - 1)).astype(np.int64)
        if prefix_bits == 0:
            return np.bincount(digit, minlength=1 << bits)[None, :]
        top = self.keys >> np.uint64(64 - prefix_bits)
        return np.stack([np.bincount(digit[top == np.uint64(p)], minlength=1 << bits) for p in prefixes])

    def prefixes_of(self, prefix_bits, most=64):
        """up to `most` distinct prefixes that scored windows carry, ascending"""
        have = np.unique(self.keys >> np.uint64(64 - prefix_bits))
        return have[np.linspace(0, len(have) - 1, min(most, len(have))).astype(int)] if len(have) else have

    def edges(self, edges, times=1):
        import torch
        d_edges = torch.from_numpy(np.asarray(edges, dtype=np.float64)).cuda()
        buf = self.counters(len(edges) + 1)
        for _ in range(times):
            self.ctx.dist_edges(*self.args(), d_edges.data_ptr(), len(edges), buf.data_ptr(), *self.tail())
            assert self.ctx.last_kernel_name() == "k_dist_edges" and self.ctx.last_comparisons() == self.nwin
        assert self.intact() and (buf[len(edges) + 1:] == 0x5A5A5A5A5A5A5A5A).all()
        return buf[:len(edges) + 1].cpu().numpy()

    def want_edges(self, edges):
        return np.bincount(np.searchsorted(edges, DR.scored(self.ref), side="right"), minlength=len(edges) + 1)

    def collect(self, prefixes, prefix_bits, capacity, start=0):
        """-> (the counter afterwards, the values written); the cells from `capacity` on stay untouched"""
        import torch
        out = torch.full((capacity + GUARD,), -7.5, dtype=torch.float64, device="cuda")
        counter = torch.full((1 + GUARD,), 0x5A5A5A5A5A5A5A5A, dtype=torch.int64, device="cuda")
        counter[0] = start
        self.ctx.dist_collect(*self.args(), prefixes, prefix_bits, out.data_ptr(), capacity, counter.data_ptr(), *self.tail())
        assert self.ctx.last_kernel_name() == "k_dist_collect" and self.ctx.last_comparisons() == self.nwin
        assert self.intact() and (out[capacity:] == -7.5).all() and (counter[1:] == 0x5A5A5A5A5A5A5A5A).all()
        return int(counter[0]), out[:capacity].cpu().numpy()

    def want_collect(self, prefixes, prefix_bits):
        take = np.isin(self.keys >> np.uint64(64 - prefix_bits), np.asarray(prefixes, dtype=np.uint64))
        return np.sort(self.keys[take])


@pytest.mark.parametrize("nwin", SIZES)
def test_every_call_at_every_size(ctx, nwin):
    rng = np.random.default_rng(nwin)
    launch = Launch(ctx, _special(nwin, rng))
    assert np.array_equal(launch.digits([], 0), launch.want_digits([], 0))
    assert launch.want_digits([], 0).sum() == len(launch.keys) == nwin - int(np.isnan(launch.ref).sum())
    for bits in BOUNDS:
        prefixes = launch.prefixes_of(bits, 5)
        assert np.array_equal(launch.digits(prefixes, bits), launch.want_digits(prefixes, bits)), bits
        want = launch.want_collect(prefixes, bits)
        n, got = launch.collect(prefixes, bits, len(want) + 3)
        assert n == len(want) and np.array_equal(np.sort(DR.key(got[:n])), want) and (got[n:] == -7.5).all()
    edges = np.sort(rng.standard_normal(7))
    assert np.array_equal(launch.edges(edges), launch.want_edges(edges))


def test_special_values_and_a_nan_at_an_unflagged_window(ctx):
    s = _special(700, np.random.default_rng(4))
    launch = Launch(ctx, s)
    assert np.isnan(s).sum() == 1 and len(launch.keys) == 699              # the NaN is unscored
    got = launch.digits([], 0)
    assert np.array_equal(got, launch.want_digits([], 0)) and got.sum() == 699
    assert got[0, 0] >= 1 and got[0, -1] == 1                              # -inf: the lowest digit; +inf alone: the highest
    edges = np.array([-INF, -5e-324, -0.0, 0.0, 5e-324, 1.0, np.nextafter(1.0, 2.0), INF])
    h = launch.edges(edges)
    assert np.array_equal(h, launch.want_edges(edges)) and h[0] == 0 and h[-1] == 1 and h.sum() == 699
    assert h[2] == 1 and h[3] == 0 and h[4] == 2                           # -0.0 and 0.0 both reach both zero edges
    assert h[6] == 2 and h[7] >= 2                                         # 1.0 twice, then its neighbour and the maximum
    # every value as its own 51-bit prefix: collected exactly
    for value in (-INF, INF, -0.0, 0.0, 1.0):
        p = DR.key(np.array([value])) >> np.uint64(13)
        n, got = launch.collect(p, 51, 8)
        assert n == int((launch.keys >> np.uint64(13) == p[0]).sum()) >= 1
        assert np.array_equal(np.sort(DR.key(got[:n])), launch.want_collect(p, 51))


@pytest.mark.parametrize("width,stride", [(L, 1), (L + 5, 1), (L + 5, 7), (600, 7)])
def test_flagged_words(ctx, width, stride):
    """a flagged word unscores exactly the windows that cover it: at a window's first l-mer, at its last, between strides"""
    n = width - L + 1
    nwin = 1500
    nlm = (nwin - 1) * stride + n
    flags = np.zeros(nlm, bool)
    flags[[0, 5 * stride, 300 * stride + n - 1, 700 * stride + n // 2, nlm - 1]] = True
    if stride > n:
        flags[900 * stride + n] = True                                     # between two windows: unscores none
    valid = _valid(flags, nwin, width, stride)
    covers = np.array([flags[i * stride:i * stride + n].any() for i in range(nwin)])
    assert np.array_equal(valid, ~covers) and not valid[[0, 5, 300, 700, nwin - 1]].any() and 2 * valid.sum() > nwin
    s = np.random.default_rng(5).standard_normal(nwin)
    s[300] = 1e300                                                         # would be the maximum: never counted
    launch = Launch(ctx, s, width=width, stride=stride, flags=flags)
    got = launch.digits([], 0)
    assert np.array_equal(got, launch.want_digits([], 0)) and got.sum() == valid.sum()
    prefixes = launch.prefixes_of(25)
    assert np.array_equal(launch.digits(prefixes, 25), launch.want_digits(prefixes, 25))
    edges = np.array([-1.0, 0.0, 1.0, 1e299])
    h = launch.edges(edges)
    assert np.array_equal(h, launch.want_edges(edges)) and h[-1] == 0
    top = np.unique(DR.key(s) >> np.uint64(52))
    n_all, got = launch.collect(top, 12, nwin)
    assert n_all == valid.sum() and np.array_equal(np.sort(DR.key(got[:n_all])), np.sort(launch.keys))


def test_leading_dimension_and_poison(ctx):
    rng = np.random.default_rng(6)
    nwin = SPAN + 300
    s = rng.standard_normal(nwin)
    alone = Launch(ctx, s)
    edges = np.array([-0.5, 0.0, 0.0, 2.0, INF])
    p12 = alone.prefixes_of(12)
    for ld, col, poison in ((3, 1, INF), (3, 1, NAN), (3, 0, -INF), (3, 2, 1.0), (64, 63, INF)):
        launch = Launch(ctx, s, ld=ld, col=col, poison=poison)
        before = launch.scores.clone()
        assert np.array_equal(launch.digits([], 0), alone.want_digits([], 0))
        assert np.array_equal(launch.digits(p12, 12), alone.want_digits(p12, 12))
        h = launch.edges(edges)
        assert np.array_equal(h, alone.want_edges(edges)) and h[-1] == 0   # +inf poison is never counted
        n, got = launch.collect(p12, 12, nwin)
        assert n == nwin and np.array_equal(np.sort(DR.key(got)), np.sort(alone.keys))
        assert launch.scores.cpu().numpy().tobytes() == before.cpu().numpy().tobytes()   # the score array is only read


def test_two_calls_accumulate(ctx):
    launch = Launch(ctx, np.random.default_rng(7).standard_normal(2 * SPAN + 9))
    assert np.array_equal(launch.digits([], 0, times=2), 2 * launch.want_digits([], 0))
    prefixes = launch.prefixes_of(12)
    assert np.array_equal(launch.digits(prefixes, 12, times=2), 2 * launch.want_digits(prefixes, 12))
    start = launch.counters(1 << 12, start=5)                              # and on top of what stands there
    assert np.array_equal(launch.digits([], 0, buf=start), 5 + launch.want_digits([], 0))
    edges = np.array([-1.0, 1.0])
    assert np.array_equal(launch.edges(edges, times=2), 2 * launch.want_edges(edges))
    # collect appends from the counter on
    n, got = launch.collect(prefixes, 12, launch.nwin + 10, start=10)
    assert n == 10 + launch.nwin and (got[:10] == -7.5).all()
    assert np.array_equal(np.sort(DR.key(got[10:])), np.sort(launch.keys))


@pytest.mark.parametrize("nprefix", [1, 2, 64])
def test_prefix_counts(ctx, nprefix):
    rng = np.random.default_rng(8)
    s = rng.standard_normal(3000) * 10.0 ** rng.integers(-40, 40, 3000)    # many exponents: many 12-bit prefixes
    launch = Launch(ctx, s)
    for bits in BOUNDS:
        prefixes = launch.prefixes_of(bits, nprefix)
        assert len(prefixes) == nprefix
        got = launch.digits(prefixes, bits)
        assert np.array_equal(got, launch.want_digits(prefixes, bits)) and (got.sum(axis=1) >= 1).all()
        want = launch.want_collect(prefixes, bits)
        n, out = launch.collect(prefixes, bits, len(want))
        assert n == len(want) >= nprefix and np.array_equal(np.sort(DR.key(out)), want)
    # a prefix no window carries, alone and among others: its row stays zero, nothing is collected for it
    absent = np.uint64(0x7FF)                                              # the exponent of negative zero and denormals
    assert absent not in (launch.keys >> np.uint64(52))
    n, out = launch.collect([absent], 12, 4)
    assert launch.digits([absent], 12).sum() == 0 and n == 0 and (out == -7.5).all()
    mixed = np.unique(np.append(launch.prefixes_of(12, 3), absent))
    got = launch.digits(mixed, 12)
    assert np.array_equal(got, launch.want_digits(mixed, 12)) and got[list(mixed).index(absent)].sum() == 0


def test_edges(ctx):
    rng = np.random.default_rng(9)
    s = _special(2 * SPAN + 3, rng)
    launch = Launch(ctx, s)
    scored = len(launch.keys)
    for edges in ([0.0], [-INF], [INF], [-INF, INF], [0.0, 0.0], np.sort(rng.standard_normal(4096)),
                  np.sort(np.concatenate([[-INF, -INF, INF, INF], np.repeat(rng.standard_normal(1023), 4)])),
                  np.sort(rng.standard_normal(4095)), np.sort(rng.standard_normal(1000))):
        edges = np.asarray(edges, dtype=np.float64)
        h = launch.edges(edges)
        assert np.array_equal(h, launch.want_edges(edges)) and h.sum() == scored, len(edges)
    assert launch.edges(np.array([-INF]))[0] == 0 and launch.edges(np.array([INF])).tolist() == [scored - 1, 1]


def test_collect_capacity(ctx):
    launch = Launch(ctx, np.random.default_rng(10).standard_normal(2 * SPAN + 9))
    prefixes = launch.prefixes_of(12)[1:]                                  # all but the lowest exponent
    want = launch.want_collect(prefixes, 12)
    assert 100 < len(want) < launch.nwin
    n, got = launch.collect(prefixes, 12, len(want))                       # exactly fits
    assert n == len(want) and np.array_equal(np.sort(DR.key(got)), want)
    n, got = launch.collect(prefixes, 12, len(want) - 1)                   # one short: the counter still advances
    assert n == len(want) and (got != -7.5).all()
    left = list(want.tolist())
    for k in DR.key(got).tolist():                                         # what was written is a sub-multiset
        left.remove(k)
    assert len(left) == 1
    n, got = launch.collect(prefixes, 12, 0)
    assert n == len(want)


def test_the_same_bytes_on_a_second_launch(ctx):
    rng = np.random.default_rng(11)
    s = rng.standard_normal(5 * SPAN + 123)
    s[rng.random(len(s)) < 0.2] = 1.0
    a, b = Launch(ctx, s), Launch(ctx, s)
    prefixes = a.prefixes_of(25)
    edges = np.sort(rng.standard_normal(100))
    for run in (lambda x: x.digits([], 0), lambda x: x.digits(prefixes, 25), lambda x: x.edges(edges)):
        ra, rb, rc = run(a), run(b), run(a)
        assert ra.tobytes() == rb.tobytes() == rc.tobytes()


def test_refusals(ctx, dv):
    import torch
    launch = Launch(ctx, np.random.default_rng(12).standard_normal(300))
    good = launch.args()
    hist = launch.counters(64 << 13)
    out = torch.empty(300, dtype=torch.float64, device="cuda")
    edges = torch.zeros(8, dtype=torch.float64, device="cuda")
    p12 = launch.prefixes_of(12, 2)

    def but(**kw):
        names = ("score", "ld", "lm", "nlm", "width", "stride", "nwin")
        return tuple(kw.get(k, v) for k, v in zip(names, good))

    def digits(args=good, prefixes=p12, bits=12, h=None, scratch=None, sbytes=None):
        ctx.dist_digits(*args, prefixes, bits, hist.data_ptr() if h is None else h,
                        launch.scratch.data_ptr() if scratch is None else scratch,
                        launch.sbytes if sbytes is None else sbytes, launch.stream)

    digits()
    digits(prefixes=[], bits=0)
    refused = [dict(args=a) for a in (but(ld=0), but(score=0), but(lm=0), but(nwin=0), but(nwin=301), but(width=L - 1),
                                      but(width=2048), but(stride=0))]
    refused += [dict(sbytes=launch.sbytes - 1), dict(scratch=launch.scratch.data_ptr() + 4), dict(h=0)]
    refused += [dict(bits=b) for b in (0, 1, 11, 13, 24, 26, 52, 63, 64, -1)]                     # no level boundary
    refused += [dict(prefixes=[], bits=12), dict(prefixes=np.arange(65), bits=25), dict(prefixes=[3, 3]),
                dict(prefixes=[4, 3]), dict(prefixes=[1 << 12]), dict(prefixes=[1, 1 << 25], bits=25)]
    hist[:] = 0
    for kw in refused:
        with pytest.raises(dv.GkmError, match=r"gkmhip_dist_digits failed \(2\)"):
            digits(**kw)
    with pytest.raises(dv.GkmError, match=r"\(2\).*no level boundary"):
        digits(bits=20)
    torch.cuda.synchronize()
    assert (hist[:64 << 13] == 0).all(), "a refused call counted something"
    for n in (0, 4097, -1):
        with pytest.raises(dv.GkmError, match=r"gkmhip_dist_edges failed \(2\)"):
            ctx.dist_edges(*good, edges.data_ptr(), n, hist.data_ptr(), *launch.tail())
    with pytest.raises(dv.GkmError, match=r"\(2\)"):
        ctx.dist_edges(*good, 0, 8, hist.data_ptr(), *launch.tail())
    counter = torch.zeros(1, dtype=torch.int64, device="cuda")
    for prefixes, bits, cap, cnt in (([], 0, 300, None), (p12, 20, 300, None), (p12, 64, 300, None), (p12, 12, -1, None),
                                     (p12, 12, 300, 0), ([2, 1], 12, 300, None)):
        with pytest.raises(dv.GkmError, match=r"gkmhip_dist_collect failed \(2\)"):
            ctx.dist_collect(*good, prefixes, bits, out.data_ptr(), cap, counter.data_ptr() if cnt is None else cnt,
                             *launch.tail())
    torch.cuda.synchronize()
    assert int(counter[0]) == 0 and (hist[:64 << 13] == 0).all() and launch.intact()
    assert ctx.dist_scratch_bytes(0, 1) == -1 and ctx.dist_scratch_bytes(10, 0) == -1
    assert ctx.dist_scratch_bytes(1 << 40, 5) == -1 and ctx.dist_scratch_bytes(10, (1 << 30) + 1) == -1
