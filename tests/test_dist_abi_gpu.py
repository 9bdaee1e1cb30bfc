"""The distribution entry points on the GPU (gkm_dist.hip: gkmhip_dist_digits, gkmhip_dist_edges, gkmhip_dist_collect;
DESIGN.md §5p): synthetic score arrays and l-mer words straight into the C calls, every histogram and every collected
multiset compared with numpy on the same arrays -- sizes around a wave's 64 lanes, a workgroup's 256 threads and its
span of 1024 windows, special values, flagged words, a leading dimension, guard bands, accumulation, every number of
prefixes, refusals, a capacity that is too small, and the same bytes on a second launch."""
import numpy as np
import pytest

from tests import dist_ref as DR
from tests.dist_launch import BITS, BOUNDS, GUARD, INF, L, NAN, SIZES, SPAN, Launch, _special, _valid  # noqa: F401

pytestmark = pytest.mark.gpu


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
