"""One launch of the distribution entry points (gkmhip_dist_digits / gkmhip_dist_edges / gkmhip_dist_collect) on synthetic
scores and l-mer words, with guard bands behind the scratch and every output, and numpy's count of the same.  Test infrastructure."""
import numpy as np

from tests import dist_ref as DR

L = 10
NAN, INF = float("nan"), float("inf")
GUARD, SPAN = 64, 1024                                                     # (a workgroup's windows: include/gkm_hip.h)
SIZES = (1, 63, 64, 65, 255, 256, 257, SPAN - 1, SPAN, SPAN + 1, 2 * SPAN + 3)
BITS = (12, 13, 13, 13, 13)
BOUNDS = (12, 25, 38, 51)


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
