"""One launch of the region entry points (gkmhip_regions_count / gkmhip_regions_fill) on synthetic scores and l-mer words,
with guard bands behind the scratch and every output, and its comparison with tests/regions_ref.py.  Test infrastructure."""
import numpy as np

from tests import regions_ref as RR

L = 10
KEYS = ("first", "last", "summit", "windows", "peak")
NAN, INF = float("nan"), float("inf")
FILL_I, FILL_D, GUARD = -77, -7.5, 64


def _valid(flags, nwin, width, stride):
    """window i holds no flagged word among its width - L + 1"""
    n = width - L + 1
    bad = np.concatenate(([0], np.cumsum(flags)))
    a = np.arange(nwin) * stride
    return bad[a + n] == bad[a]


class Launch:
    """one (scores, words, shape) on the device, its scratch, and output arrays with a guard band behind each"""

    def __init__(self, ctx, scores, thr, gap, width=L, stride=1, flags=None, ld=1, col=0, poison=INF, spare=5):
        import torch
        self.ctx, self.thr, self.gap, self.width, self.stride, self.ld = ctx, thr, gap, width, stride, ld
        scores = np.asarray(scores, dtype=np.float64)
        self.nwin = len(scores)
        self.nlm = (self.nwin - 1) * stride + width - L + 1
        flags = np.zeros(self.nlm, bool) if flags is None else np.asarray(flags, bool)
        assert len(flags) == self.nlm
        self.ref_scores = np.where(_valid(flags, self.nwin, width, stride), scores, NAN)
        host = np.full((self.nwin, ld), poison)
        host[:, col] = scores
        self.scores = torch.from_numpy(host).cuda()
        words = np.random.default_rng(1).integers(0, 4 ** L, size=self.nlm, dtype=np.uint32) | (flags.astype(np.uint32) << 31)
        self.lm = torch.from_numpy(words.view(np.int32)).cuda()
        self.sbytes = ctx.regions_scratch_bytes(self.nlm, self.nwin)
        assert self.sbytes > 0
        self.scratch = torch.full((self.sbytes + GUARD,), 0x5A, dtype=torch.uint8, device="cuda")
        self.col, self.spare = col, spare
        self.stream = torch.cuda.current_stream().cuda_stream

    def args(self):
        return (self.scores.data_ptr() + 8 * self.col, self.ld, self.lm.data_ptr(), self.nlm, self.width, self.stride,
                self.nwin, self.thr, self.gap, self.scratch.data_ptr(), self.sbytes)

    def count(self):
        n = self.ctx.regions_count(*self.args(), self.stream)
        assert self.ctx.last_kernel_name() == "k_regions_summaries" and self.ctx.last_kernel_ms() >= 0.0
        assert (self.scratch[self.sbytes:] == 0x5A).all()
        return n

    def outputs(self, cells):
        import torch
        self.ints = torch.full((4, cells + GUARD), FILL_I, dtype=torch.int32, device="cuda")
        self.peak = torch.full((cells + GUARD,), FILL_D, dtype=torch.float64, device="cuda")

    def fill(self, capacity):
        self.ctx.regions_fill(*self.args(), capacity, *(self.ints[k].data_ptr() for k in range(4)), self.peak.data_ptr(),
                              self.stream)

    def untouched_from(self, n):
        return bool((self.ints[:, n:] == FILL_I).all()) and bool((self.peak[n:] == FILL_D).all())

    def run(self):
        """count, fill with `spare` cells of capacity to spare -> the regions; nothing beyond the count is written"""
        import torch
        n = self.count()
        self.outputs(n + self.spare)
        self.fill(n + self.spare)
        torch.cuda.synchronize()
        if n:
            assert self.ctx.last_kernel_name() == "k_regions_fill" and self.ctx.last_kernel_ms() >= 0.0
        assert self.untouched_from(n), "a cell beyond the count was written"
        h = self.ints[:, :n].cpu().numpy().astype(np.int64)
        return dict(first=h[0], last=h[1], summit=h[2], windows=h[3], peak=self.peak[:n].cpu().numpy())

    def want(self):
        return RR.window_regions(self.ref_scores, self.thr, self.gap)


def _check(launch, what):
    got, want = launch.run(), launch.want()
    assert RR.same(got, want, KEYS), (what, {k: (got[k][:6], want[k][:6]) for k in KEYS}, len(got["first"]), len(want["first"]))
    return want
