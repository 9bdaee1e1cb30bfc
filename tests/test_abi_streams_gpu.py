"""When the device ABI of include/gkm_hip.h does its work: "work is enqueued on `stream`", and the two scratch slots of
launches that alternate between two streams.

The rest of the suite hands every call torch's current stream outside any stream context -- the null stream, which a
library's stray launch on stream 0 IS.  Here the caller's stream is a side stream that is kept busy:

    1. a delay on the stream (plain torch fills, timed with torch events);
    2. the sentinel fill of the outputs;
    3. the call under test;
    4. stream.synchronize().

Anything the library put on another stream runs during the delay: its result is then overwritten by the fill, or it read
an input that was still waiting behind the delay.  The upload goes through the same steps first, into a context that
holds OTHER sequences (a decoy of the same lengths), so that a table built early is built from the wrong bases.  The
result must equal the null-stream run's bytes.  Correct code is ordered behind the delay whatever its length, so it
cannot fail these tests; the delay only decides whether wrong code is caught.  It is repeated until it lasts ten times
the null-stream run's last_kernel_ms() (a margin for the queue's start-up, not a measurement) and at least FLOOR_MS, so
that the host-side preparation of a call (packing, planning) falls inside it; the ratio reached is printed."""
import math

import numpy as np
import pytest

from tests import abi_cases as A

pytestmark = pytest.mark.gpu

FLOOR_MS = 20.0      # host-side preparation of the calls here takes 0.1-2 ms
CAP_MS = 1500.0      # a test stays within a few seconds
RATIO = 10.0

L6 = (6, 4, 2)       # the small context of tests/test_launch_bracket_gpu.py
CODES = 4 ** 6
NV = 11
BASES = 30 + 41 + 50
WIDTH, STRIDE, RECORD = 40, 7, 120
NWIN = (RECORD - WIDTH) // STRIDE + 1


@pytest.fixture(scope="module")
def dev(built):
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    from gkmqc_amd import device
    device.load()
    return device


class Delay:
    """Repeated fills of one 512-MiB buffer on the current stream"""

    def __init__(self):
        import torch
        self.buf = torch.empty(1 << 26, dtype=torch.float64, device="cuda")
        self.buf.fill_(0.0)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for i in range(16):
            self.buf.fill_(float(i))
        e1.record()
        torch.cuda.synchronize()
        self.per_fill_ms = max(e0.elapsed_time(e1) / 16, 1e-3)

    def behind(self, stream, target_ms, work, before=None):
        """[before();] on `stream`: a delay of at least target_ms, then work(), then a wait for the stream; the whole
        thing again with twice the fills while the delay came out shorter.  -> the delay's ms"""
        import torch
        fills = int(math.ceil(1.5 * target_ms / self.per_fill_ms))
        while True:
            if before:
                before()
            with torch.cuda.stream(stream):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for i in range(fills):
                    self.buf.fill_(float(i))
                e1.record()
                work()
                stream.synchronize()
            took = e0.elapsed_time(e1)
            if took >= target_ms or took >= CAP_MS:
                return took
            fills *= 2

    def side_stream(self):
        """A torch stream that runs BESIDE the null stream.  HIP maps streams onto a few hardware queues, and two streams
        that share one execute in order: a stray launch on stream 0 would then wait behind the delay like correct code
        and go unseen.  A candidate is kept if a small fill on the null stream completes while a delay on the candidate
        is still running; the others stay alive meanwhile, so that the next one comes from another queue.  After eight
        candidates the last one is taken whatever it shares (the tests then still pass on correct code)."""
        import torch
        word = torch.zeros(16, device="cuda")
        fills = int(math.ceil(5.0 / self.per_fill_ms))
        tried = []
        for _ in range(8):
            s = torch.cuda.Stream()
            tried.append(s)
            torch.cuda.synchronize()
            busy, small = torch.cuda.Event(), torch.cuda.Event()
            with torch.cuda.stream(s):
                for i in range(fills):
                    self.buf.fill_(float(i))
                busy.record()
            word.fill_(1.0)
            small.record()
            small.synchronize()
            beside = not busy.query()
            s.synchronize()
            if beside:
                break
        print("side stream: candidate %d %s the null stream" % (len(tried), "runs beside" if beside else "SHARES A QUEUE WITH"))
        return s


@pytest.fixture(scope="module")
def delay(dev):
    return Delay()


def _null():
    import torch
    s = torch.cuda.current_stream().cuda_stream
    assert s == 0      # outside any stream context: the null stream
    return s


def _decoy(seqs):
    """other bases, the same lengths"""
    return [((np.asarray(x) + 1) % 4).astype(np.uint8) for x in seqs]


class Job:
    """One call under test: `outputs` (sentinel tensors), upload(seqs, stream), call(stream), and the context"""

    def __init__(self, ctx, seqs, outputs, call, check=None):
        self.ctx, self.seqs, self.outputs, self.call, self.check = ctx, seqs, outputs, call, check

    def upload(self, seqs, stream):
        self.ctx.set_sequences(seqs, stream)


def _on_both_streams(job, delay, what):
    """the null-stream run, then the upload and the call behind a delay on a side stream: the same bytes"""
    import torch
    try:
        null = _null()
        job.upload(job.seqs, null)
        for o in job.outputs:
            A.refill(o)
        job.call(null)
        torch.cuda.synchronize()
        if job.check:
            job.check()
        ms = max(job.ctx.last_kernel_ms(), 0.0)
        want = [A.bits(o).copy() for o in job.outputs]
        assert not any(A.untouched(o, np.ones(tuple(o.shape), dtype=bool)) for o in job.outputs)   # (something was written)
        target = max(RATIO * ms, FLOOR_MS)
        s = delay.side_stream()
        decoy = _decoy(job.seqs)

        def other_sequences():
            job.upload(decoy, null)
            torch.cuda.synchronize()

        def work():
            for o in job.outputs:
                A.refill(o)
            job.call(s.cuda_stream)

        took_upload = delay.behind(s, target, lambda: job.upload(job.seqs, s.cuda_stream), before=other_sequences)
        took = delay.behind(s, target, work)
        if job.check:
            job.check()
        print("%s: kernel %.3f ms, delays %.1f and %.1f ms: %.0f and %.0f times the kernel" %
              (what, ms, took_upload, took, took_upload / max(ms, 1e-3), took / max(ms, 1e-3)))
        assert min(took, took_upload) >= RATIO * ms, "the delay is capped below ten times the kernel"
        for o, w in zip(job.outputs, want):
            assert (A.bits(o) == w).all(), what
    finally:
        job.ctx.close()


# ------------------------------------------------------------------ the Gram launches
def _gram_job(dev, launch, t, kind):
    import torch
    seqs = launch.seqs()
    n, d = len(seqs), launch.d
    ctx = dev.GramContext(t, launch.L, launch.L - d, d, gamma=2.0)
    ctx.set_kernel(getattr(dev, launch.kernel))
    ld, ldp = n + 3, n + 5
    rows = A.subset_with_a_jump(n)
    p = torch.Tensor.data_ptr
    if kind == "gram_matrix":
        G, P, sq = A.sentinel_f64((n, ld)), A.sentinel_i32((n, ldp, d + 1)), A.sentinel_f64((n,))

        def call(s):
            ctx.gram_rows(np.arange(n), p(G), ld, p(P), ldp, False, s)
            ctx.normalize(p(G), ld, p(sq), True, s)
        return Job(ctx, seqs, [G, P, sq], call, lambda: A.assert_path(ctx, launch))
    if kind == "cross_kernel":
        G, sq = A.sentinel_f64((len(rows), ld)), A.sentinel_f64((n,))

        def call(s):
            ctx.self_norms(p(sq), s)
            ctx.gram_rows_full(rows, p(G), ld, True, s)
            ctx.normalize_rows_full(rows, p(G), ld, p(sq), True, s)
        return Job(ctx, seqs, [G, sq], call)
    if kind == "block":
        c0, c1 = 5, n - 2
        G, sq = A.sentinel_f64((len(rows), ld)), A.sentinel_f64((n,))

        def call(s):
            ctx.self_norms(p(sq), s)
            ctx.gram_block(rows, c0, c1, p(G), ld, s)
            ctx.normalize_block(rows, c0, c1, p(G), ld, p(sq), s)
        return Job(ctx, seqs, [G, sq], call)
    assert kind == "self_norms"
    sq = A.sentinel_f64((n,))
    return Job(ctx, seqs, [sq], lambda s: ctx.self_norms(p(sq), s))


@pytest.mark.parametrize("kind,name,t", [
    ("gram_matrix", "pk7", 4), ("gram_matrix", "packed", 5), ("gram_matrix", "direct", 4),
    ("cross_kernel", "packed", 5), ("cross_kernel", "direct", 4), ("cross_kernel", "pk7", 4),
    ("block", "packed", 5), ("block", "direct", 4), ("self_norms", "packed", 4), ("self_norms", "direct", 4),
])
def test_gram_calls_behind_a_delay_on_a_side_stream(dev, delay, kind, name, t):
    _on_both_streams(_gram_job(dev, A.by_name(name), t, kind), delay, "%s %s t=%d" % (kind, name, t))


# ------------------------------------------------------------------ one entry each of the other kernels
ENTRIES = ["explain", "ism", "hyp", "lmer_weights+lmer_score", "scan_lmers+scan_score", "delta_sat", "panel_score"]


def _entry_job(dev, entry):
    import torch
    Lm, k, d = L6
    rng = np.random.default_rng(20261)
    seqs = [rng.integers(0, 4, n).astype(np.uint8) for n in (40,) * 6 + (30, 41, 50)]
    ctx = dev.GramContext(4, Lm, k, d)
    f64 = dict(dtype=torch.float64, device="cuda")
    rows = np.arange(6)
    W = torch.from_numpy(rng.standard_normal(CODES)).cuda()
    panel = torch.from_numpy(rng.standard_normal((CODES, 8))).cuda()
    coef = torch.from_numpy(rng.standard_normal(6)).cuda()
    xscale = torch.from_numpy(rng.random(3) + 0.5).cuda()
    c = rng.random(d + 1)
    v = torch.from_numpy(rng.integers(0, CODES, NV).astype(np.int32)).cuda()
    cv = torch.from_numpy(rng.standard_normal(NV)).cuda()
    record = torch.from_numpy(rng.integers(0, 4, RECORD).astype(np.uint8)).cuda()
    valid = torch.ones(RECORD, dtype=torch.uint8, device="cuda")
    nlm = RECORD - Lm + 1
    wt = torch.from_numpy(rng.integers(1, 200, WIDTH - Lm + 1).astype(np.uint8)).cuda()
    lm_in = torch.empty(nlm, dtype=torch.int32, device="cuda")
    ctx.scan_lmers(record.data_ptr(), valid.data_ptr(), RECORD, lm_in.data_ptr(), _null())
    torch.cuda.synchronize()      # the inputs are complete before any stream reads them
    keep = (W, panel, coef, xscale, v, cv, record, valid, wt, lm_in)
    p = torch.Tensor.data_ptr
    if entry == "explain":
        out = [A.sentinel_f64((BASES,))]
        call = lambda s: ctx.explain_block(rows, 6, 9, c, p(coef), p(xscale), p(out[0]), s)      # noqa: E731
    elif entry == "ism":
        out = [A.sentinel_f64((BASES, 4)), A.sentinel_f64((3,))]
        call = lambda s: ctx.ism_block(rows, 6, 9, c, c, c, p(coef), p(out[0]), p(out[1]), s)      # noqa: E731
    elif entry == "hyp":
        out = [A.sentinel_f64((BASES, 4))]
        call = lambda s: ctx.hyp_block(rows, 6, 9, c, p(coef), p(out[0]), s)      # noqa: E731
    elif entry == "lmer_weights+lmer_score":
        out = [A.sentinel_f64((CODES,)), A.sentinel_f64((3,))]

        def call(s):
            ctx.lmer_weights(c, p(v), p(cv), NV, 0, CODES, p(out[0]), s)
            ctx.lmer_score(6, 9, p(out[0]), p(out[1]), s)
    elif entry == "scan_lmers+scan_score":
        out = [A.sentinel_i32((nlm,)), A.sentinel_f64((NWIN,))]

        def call(s):
            ctx.scan_lmers(p(record), p(valid), RECORD, p(out[0]), s)
            ctx.scan_score(p(out[0]), nlm, p(wt), WIDTH, STRIDE, NWIN, p(W), p(out[1]), s)
    elif entry == "delta_sat":
        out = [A.sentinel_f64((RECORD, 4))]
        call = lambda s: ctx.delta_sat(p(lm_in), nlm, 0, RECORD, p(W), p(out[0]), s)      # noqa: E731
    else:
        assert entry == "panel_score"
        out = [A.sentinel_f64((3, 3))]
        call = lambda s: ctx.panel_score(6, 9, p(panel), 3, 8, p(out[0]), s)      # noqa: E731
    job = Job(ctx, seqs, out, call)
    job.keep = keep
    return job


@pytest.mark.parametrize("entry", ENTRIES)
def test_other_entries_behind_a_delay_on_a_side_stream(dev, delay, entry):
    _on_both_streams(_entry_job(dev, entry), delay, entry)


def test_nullidx_build_behind_a_delay_on_a_side_stream(dev, delay):
    import torch
    from tests import nullidx_ref as NR
    raw = NR.as_bytes(NR.soft_masked(5000, seed=11, n_gaps=2, gap=40))
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    dev.nullidx_build(raw, 7)                     # (the first call loads the kernels)
    e0.record()
    want = dev.nullidx_build(raw, 7)
    e1.record()
    torch.cuda.synchronize()
    ms = e0.elapsed_time(e1)                      # the whole build, host waits included: longer than its kernels
    ref = NR.index_vectorised(raw, 7)
    got = {}
    s = delay.side_stream()
    took = delay.behind(s, max(RATIO * ms, FLOOR_MS), lambda: got.update(dev.nullidx_build(raw, 7)))
    print("nullidx_build: %.3f ms, delay %.1f ms: %.0f times" % (ms, took, took / ms))
    assert took >= RATIO * ms
    assert got["len"] == want["len"] == ref["len"]
    for name in ("key", "pos", "ptr", "na", "cg", "rp"):
        assert got[name].tobytes() == want[name].tobytes() == ref[name].tobytes(), name


# ------------------------------------------------------------------ tables built on one stream, read on another
@pytest.mark.parametrize("name,t", [("packed", 4), ("direct", 4), ("pk7", 2)])
def test_upload_on_one_stream_second_launch_on_another(dev, delay, name, t):
    """gkmhip_set_sequences and the first launch on a side stream s, the second launch on another side stream s2 that
    waits for s (and takes the other scratch slot): the per-sequence tables are complete before s2 reads them."""
    import torch
    launch = A.by_name(name)
    seqs = launch.seqs()
    n = len(seqs)
    ld = n + 3
    rows = A.subset_with_a_jump(n)
    ctx = dev.GramContext(t, launch.L, launch.L - launch.d, launch.d)
    try:
        ctx.set_kernel(getattr(dev, launch.kernel))
        G1, G2, sq = A.sentinel_f64((n, ld)), A.sentinel_f64((len(rows), ld)), A.sentinel_f64((n,))
        p = torch.Tensor.data_ptr

        def first(s):
            ctx.set_scratch_slot(0)
            ctx.gram_rows(np.arange(n), p(G1), ld, None, 0, False, s)

        def second(s):
            ctx.set_scratch_slot(1)
            ctx.self_norms(p(sq), s)
            ctx.gram_rows_full(rows, p(G2), ld, True, s)

        null = _null()
        ctx.set_sequences(seqs, null)
        first(null)
        ms = max(ctx.last_kernel_ms(), 0.0)
        second(null)
        torch.cuda.synchronize()
        want = [A.bits(o).copy() for o in (G1, G2, sq)]
        ctx.set_sequences(_decoy(seqs), null)
        torch.cuda.synchronize()
        s, s2 = delay.side_stream(), torch.cuda.Stream()

        def work():
            for o in (G1, G2, sq):
                A.refill(o)
            ctx.set_sequences(seqs, s.cuda_stream)
            first(s.cuda_stream)
            s2.wait_stream(s)
            with torch.cuda.stream(s2):
                second(s2.cuda_stream)
            s.wait_stream(s2)

        took = delay.behind(s, max(RATIO * ms, FLOOR_MS), work)
        print("%s: kernel %.3f ms, delay %.1f ms: %.0f times" % (name, ms, took, took / max(ms, 1e-3)))
        assert took >= RATIO * ms
        for o, w in zip((G1, G2, sq), want):
            assert (A.bits(o) == w).all()
    finally:
        ctx.close()


# ------------------------------------------------------------------ two slots, two streams
@pytest.mark.parametrize("name", ["packed", "pk7"])
def test_two_scratch_slots_on_two_streams(dev, name):
    """The header's protocol: consecutive launches alternate between two streams and the two scratch slots, with no host
    wait of the caller's in between; then one normalisation.  The same bytes as one launch on one stream."""
    import torch
    launch = A.by_name(name)
    seqs = launch.seqs()
    n = len(seqs)
    ld = n + 3
    ctx = dev.GramContext(4, launch.L, launch.L - launch.d, launch.d)
    try:
        ctx.set_kernel(getattr(dev, launch.kernel))
        null = _null()
        ctx.set_sequences(seqs, null)
        p = torch.Tensor.data_ptr
        one, sq1 = A.sentinel_f64((n, ld)), A.sentinel_f64((n,))
        ctx.gram_rows(np.arange(n), p(one), ld, None, 0, False, null)
        A.assert_path(ctx, launch)
        ctx.normalize(p(one), ld, p(sq1), False, null)
        two, sq2 = A.sentinel_f64((n, ld)), A.sentinel_f64((n,))
        torch.cuda.synchronize()
        streams = (torch.cuda.Stream(), torch.cuda.Stream())
        for i, rows in enumerate(np.array_split(np.arange(n, dtype=np.int32), 4)):
            ctx.set_scratch_slot(i & 1)
            ctx.gram_rows(rows, p(two), ld, None, 0, False, streams[i & 1].cuda_stream)
        streams[0].wait_stream(streams[1])
        ctx.set_scratch_slot(0)
        ctx.normalize(p(two), ld, p(sq2), False, streams[0].cuda_stream)
        streams[0].synchronize()
        assert (A.bits(two) == A.bits(one)).all() and (A.bits(sq2) == A.bits(sq1)).all()
        pad = np.zeros((n, ld), dtype=bool)
        pad[:, n:] = True
        pad[np.triu_indices(n, 1)] = True
        assert A.untouched(two, pad)
    finally:
        ctx.close()
