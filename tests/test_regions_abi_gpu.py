"""The region entry points on the GPU (gkm_regions.hip: gkmhip_regions_count, gkmhip_regions_fill):
synthetic score arrays and l-mer words straight into the C calls, every result compared with tests/regions_ref.py on the
same arrays -- sizes around a wave's 64 lanes, a wave's 256 windows and a workgroup's span, runs and gaps that cross
all three, special values, flagged words, a leading dimension, guard bands, a capacity that is too small, and the same
bytes on a second launch."""
import numpy as np
import pytest

from tests import regions_ref as RR
from tests.regions_launch import FILL_D, FILL_I, GUARD, INF, KEYS, L, NAN, Launch, _check, _valid  # noqa: F401

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dv(built):
    from gkmqc_amd import device
    return device


@pytest.fixture(scope="module")
def ctx(dv):
    c = dv.GramContext(4, L, 6, 3, device=0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def span(ctx):
    s = ctx.regions_span()
    assert s == 1024                                                       # (the sizes below are written around it)
    return s


def _scores(passing, rng):
    """distinct values: passing windows above 0, the others below"""
    v = rng.permutation(len(passing)) + 1.0
    return np.where(passing, v, -v)


SIZES = (1, 2, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 20000)


@pytest.mark.parametrize("nwin", SIZES)
def test_pass_patterns_at_every_size(ctx, span, nwin):
    rng = np.random.default_rng(nwin)
    i = np.arange(nwin)
    patterns = {
        "all": np.ones(nwin, bool), "none": np.zeros(nwin, bool), "alternating": i % 2 == 0, "alternating odd": i % 2 == 1,
        "runs end on lane 63": i % 64 >= 40, "runs begin on lane 0": i % 64 < 20,
        "runs end on a wave's last window": i % 256 >= 250, "runs begin on a wave's first": i % 256 < 3,
        "runs end on a workgroup's last window": i % span >= span - 30, "runs begin on a workgroup's first": i % span < 30,
        "last window only": i == nwin - 1, "random": rng.random(nwin) < 0.5, "sparse": rng.random(nwin) < 0.01,
    }
    for name, passing in patterns.items():
        want = _check(Launch(ctx, _scores(passing, rng), 0.0, 0), (nwin, name))
        if name == "alternating":
            assert len(want["first"]) == (nwin + 1) // 2                   # the most regions there can be
        if name == "all":
            assert want["windows"].tolist() == [nwin]


def test_one_run_over_several_workgroups(ctx, span):
    """the maximum in the first, a middle and the last workgroup; twice: the first of the two is the summit"""
    nwin = 3 * span + 500
    base = np.random.default_rng(2).random(nwin)
    for at in (5, span + 476, nwin - 100):
        s = base.copy()
        s[at] = 2.0
        want = _check(Launch(ctx, s, 0.0, 0), at)
        assert [want[k].tolist() for k in KEYS] == [[0], [nwin - 1], [at], [nwin], [2.0]]
    s = base.copy()
    s[[700, 2 * span + 3]] = 2.0
    assert _check(Launch(ctx, s, 0.0, 0), "twice")["summit"].tolist() == [700]
    # the run begins and ends inside workgroups, failing windows around it
    s = np.where((np.arange(nwin) >= 300) & (np.arange(nwin) < nwin - 300), base + 1.0, -1.0)
    want = _check(Launch(ctx, s, 0.0, 0), "inner")
    assert want["first"].tolist() == [300] and want["windows"].tolist() == [nwin - 600]


def test_all_scores_equal(ctx, span):
    nwin = 2 * span + 77
    for gap in (0, 5):
        want = _check(Launch(ctx, np.full(nwin, 1.25), 1.25, gap), gap)
        assert [want[k].tolist() for k in KEYS] == [[0], [nwin - 1], [0], [nwin], [1.25]]
    passing = (np.arange(nwin) % 700) < 650
    want = _check(Launch(ctx, np.where(passing, 1.25, 1.0), 1.25, 0), "runs")
    assert np.array_equal(want["summit"], want["first"]) and len(want["first"]) == 4


def test_gaps(ctx, span):
    """failing stretches of 1, 2, 64, 65, 300, 301 windows and of more than a workgroup's span, within the gap and beyond"""
    nwin = 5000
    at = [10, 11, 13, 16, 81, 147, 448, 750, 751, 1904, 3004, 4999]        # apart by 1 2 3 65 66 301 302 1 1153 1100 1995
    assert span < 1100 and max(np.diff(at)) > span
    s = np.full(nwin, -1.0)
    s[at] = [3.0, 1.0, 2.0, 5.0, 4.0, 9.0, 9.0, 6.0, 7.0, 8.0, 8.5, 1.5]
    seen = set()
    for gap in (0, 1, 2, 63, 64, 65, 299, 300, 301, 1098, 1099, 1151, 1152, 1993, 1994, nwin):
        want = _check(Launch(ctx, s, 0.0, gap), gap)
        assert want["windows"].sum() == len(at)
        seen.add(len(want["first"]))
    assert seen == set(range(1, 11))                                       # every merge happened at its own gap
    # a gap that bridges whole workgroups of failing windows, and one window short of it
    s = np.full(4 * span, -1.0)
    s[[span - 1, 3 * span]] = 1.0
    assert len(_check(Launch(ctx, s, 0.0, 2 * span), "bridged")["first"]) == 1
    assert len(_check(Launch(ctx, s, 0.0, 2 * span - 1), "not bridged")["first"]) == 2


def test_special_values(ctx):
    rng = np.random.default_rng(4)
    nwin = 700
    s = rng.standard_normal(nwin)
    s[rng.choice(nwin, 60, replace=False)] = NAN
    s[rng.choice(nwin, 40, replace=False)] = INF
    s[rng.choice(nwin, 40, replace=False)] = -INF
    for thr in (-INF, 0.0, INF, float(np.nanmedian(s)), float(s[np.isfinite(s)][7])):
        for gap in (0, 2):
            want = _check(Launch(ctx, s, thr, gap), (thr, gap))
            assert len(want["first"]) > 0
    assert _check(Launch(ctx, s, -INF, 0), "-inf")["windows"].sum() == nwin - int(np.isnan(s).sum())
    assert (_check(Launch(ctx, s, INF, 0), "+inf")["peak"] == INF).all()
    # a threshold equal to a score passes it; the next double above does not
    t = np.array([0.1, 0.3, 0.2, 0.3, 0.1])
    assert _check(Launch(ctx, t, 0.3, 0), "equal")["first"].tolist() == [1, 3]
    assert len(_check(Launch(ctx, t, np.nextafter(0.3, 1.0), 0), "above")["first"]) == 0
    # -0.0 passes a threshold of 0.0 and 0.0 one of -0.0; they tie, so the first of them is the summit, its sign kept
    z = np.array([-1.0, -0.0, 0.0, -1.0, 0.0, -0.0, -1.0])
    for thr in (0.0, -0.0):
        want = _check(Launch(ctx, z, thr, 0), "zeros")
        assert want["summit"].tolist() == [1, 4] and np.signbit(want["peak"]).tolist() == [True, False]
    assert len(_check(Launch(ctx, np.full(300, NAN), -INF, 9), "nan only")["first"]) == 0


@pytest.mark.parametrize("width,stride", [(L, 1), (L + 5, 1), (L + 5, 3), (L + 70, 1), (L + 70, 100), (600, 7)])
def test_flagged_words(ctx, width, stride):
    """a flagged word fails exactly the windows that cover it: at a window's first l-mer, at its last, and in between"""
    n = width - L + 1
    nwin = 1500
    nlm = (nwin - 1) * stride + n
    flags = np.zeros(nlm, bool)
    flags[[0, 5 * stride, 300 * stride + n - 1, 700 * stride + n // 2, 701 * stride + n // 2, nlm - 1]] = True
    flags[1100 * stride:1100 * stride + 3 * n] = True
    valid = _valid(flags, nwin, width, stride)
    covers = np.array([flags[i * stride:i * stride + n].any() for i in range(nwin)])
    assert np.array_equal(valid, ~covers) and not valid[[0, 5, 300, nwin - 1]].any() and 2 * valid.sum() > nwin
    s = np.random.default_rng(5).random(nwin)
    launch = Launch(ctx, s, -INF, 0, width=width, stride=stride, flags=flags)
    want = _check(launch, "every valid window")
    assert want["windows"].sum() == valid.sum() and len(want["first"]) >= 4
    _check(Launch(ctx, s, 0.5, 1, width=width, stride=stride, flags=flags), "thresholded")
    # a score that would pass at a failed window stays out even where it is the largest
    s[300] = 9.0
    assert 9.0 not in _check(Launch(ctx, s, -INF, 2, width=width, stride=stride, flags=flags), "bridged")["peak"]


def test_leading_dimension(ctx, span):
    rng = np.random.default_rng(6)
    nwin = span + 300
    s = rng.standard_normal(nwin)
    want = RR.window_regions(s, 0.25, 1)
    for ld, col, poison in ((3, 1, INF), (3, 1, NAN), (3, 0, INF), (3, 2, -INF), (64, 63, INF)):
        got = _check(Launch(ctx, s, 0.25, 1, ld=ld, col=col, poison=poison), (ld, col, poison))
        assert RR.same(got, want, KEYS)


def test_capacity(ctx, dv, span):
    import torch
    rng = np.random.default_rng(7)
    launch = Launch(ctx, rng.standard_normal(2 * span + 9), 0.0, 0)
    n = launch.count()
    assert n == len(launch.want()["first"]) > 100
    for capacity in (0, 1, n - 1):
        launch.outputs(n)
        with pytest.raises(dv.GkmError, match=r"gkmhip_regions_fill failed \(2\).*%d regions, capacity %d" % (n, capacity)):
            launch.fill(capacity)
        torch.cuda.synchronize()
        assert launch.untouched_from(0), "a refused fill wrote something"
    launch.outputs(n)
    launch.fill(n)                                                         # exactly fits
    torch.cuda.synchronize()
    assert launch.untouched_from(n) and (launch.ints[:, :n] != FILL_I).all()
    # nothing to report: the fill launches nothing, with or without arrays
    none = Launch(ctx, np.full(500, -1.0), 0.0, 3)
    assert none.count() == 0
    none.outputs(4)
    none.fill(4)
    ctx.regions_fill(*none.args(), 0, 0, 0, 0, 0, 0, none.stream)
    torch.cuda.synchronize()
    assert none.untouched_from(0)


def test_the_same_bytes_on_a_second_launch(ctx, span):
    rng = np.random.default_rng(8)
    s = rng.standard_normal(5 * span + 123)
    s[rng.random(len(s)) < 0.2] = 1.0                                      # ties
    a, b = Launch(ctx, s, 0.3, 2), Launch(ctx, s, 0.3, 2)
    ra, rb = a.run(), b.run()
    rc = a.run()                                                           # and on the same scratch again
    assert RR.same(ra, rb, KEYS) and RR.same(ra, rc, KEYS) and RR.same(ra, a.want(), KEYS)


def test_refusals(ctx, dv):
    import torch
    launch = Launch(ctx, np.random.default_rng(9).standard_normal(300), 0.0, 0)
    good = launch.args()

    def but(**kw):
        names = ("score", "ld", "lm", "nlm", "width", "stride", "nwin", "thr", "gap", "scratch", "sbytes")
        return tuple(kw.get(k, v) for k, v in zip(names, good))

    for args in (but(gap=-1), but(thr=NAN), but(ld=0), but(sbytes=launch.sbytes - 1), but(scratch=0), but(score=0), but(lm=0),
                 but(nwin=0), but(nwin=301), but(width=L - 1), but(width=2048), but(stride=0),
                 but(scratch=launch.scratch.data_ptr() + 4)):
        with pytest.raises(dv.GkmError, match=r"\(2\)"):
            ctx.regions_count(*args, launch.stream)
    assert ctx.regions_scratch_bytes(0, 1) == -1 and ctx.regions_scratch_bytes(10, 0) == -1
    assert ctx.regions_scratch_bytes(1 << 40, 5) == -1 and ctx.regions_scratch_bytes(10, (1 << 30) + 1) == -1
    # a fill needs the count call of the same arguments in its scratch
    launch.outputs(300)
    with pytest.raises(dv.GkmError, match=r"\(2\).*does not hold"):
        launch.fill(300)                                                   # (no count call yet: the scratch is 0x5A)
    n = launch.count()
    for args in (but(gap=1), but(thr=0.5), but(nwin=299), but(stride=1, width=L + 1, nwin=299)):
        with pytest.raises(dv.GkmError, match=r"\(2\).*does not hold"):
            ctx.regions_fill(*args, 300, *(launch.ints[k].data_ptr() for k in range(4)), launch.peak.data_ptr(), launch.stream)
    torch.cuda.synchronize()
    assert launch.untouched_from(0)
    launch.fill(300)
    torch.cuda.synchronize()
    assert launch.untouched_from(n) and n > 0
