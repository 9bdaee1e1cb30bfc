"""Hard inputs for the interpretation kernels (k_explain, k_ism, k_ism<true>, k_ism_self_base + k_ism_self, k_lmer_weights,
k_lmer_score): sequences on which most l-mer pairs are hits, where iid bases make a hit the rare event.  Seeded and
deterministic; everything returns base-code arrays (0..3 = A, C, G, T).  Also a small CPU model of the order in which
k_ism's waves queue their hits, which shows that the inputs chosen for the queue fill it to every depth it is designed
for.  Test infrastructure: shared by tests/test_dense_host.py, tests/test_dense_gpu.py and tools/fuzz_interpret.py."""
import collections

import numpy as np

A, C, G, T = 0, 1, 2, 3
MAX_LEN = 2047                      # the longest sequence the kernels accept

# name -> (kernel type, M, H).  (254, 1e6): every positional weight is 254; (255, 1e6): every weight 255 except the
# centre l-mer, whose byte wraps to 0 as in the reference; "unit": an unweighted kernel type (every weight 1)
WEIGHTS = collections.OrderedDict((("w50", (4, 50, 50.0)), ("w254", (4, 254, 1e6)), ("w255", (4, 255, 1e6)),
                                   ("unit", (0, 50, 50.0))))


def rc(x):
    return (3 - np.asarray(x, dtype=np.uint8))[::-1].copy()


def homopolymer(b, n):
    return np.full(n, b, dtype=np.uint8)


def repeat(unit, n):
    unit = np.asarray(unit, dtype=np.uint8)
    return np.tile(unit, n // len(unit) + 1)[:n].copy()


def lengths(L):
    """L, L + 1, exactly one wave of l-mers, 256 and 257 l-mers, the longest accepted"""
    return [L, L + 1, 64 + L - 1, 256 + L - 1, 257 + L - 1, MAX_LEN]


def unit_of(period, seed):
    """a repeat unit of `period` bases that is not itself a repeat of a shorter one"""
    rng = np.random.default_rng(1000 * period + seed)
    while True:
        u = rng.integers(0, 4, size=period, dtype=np.uint8)
        if all(period % q or not np.array_equal(u, np.tile(u[:q], period // q)) for q in range(1, period)):
            return u


def spliced(n, L, seed):
    """iid bases with low-complexity stretches (homopolymers, period-2 and period-3 repeats of 20 to 90 bases) spliced in
    at random places, so that one wave of l-mers holds hitting and non-hitting lanes"""
    rng = np.random.default_rng(seed)
    x = rng.integers(0, 4, size=n, dtype=np.uint8)
    at = 0
    while True:
        at += int(rng.integers(5, 70))
        run = int(rng.integers(20, 91))
        if at + run > n:
            return x
        kind = int(rng.integers(0, 3))
        unit = [int(rng.integers(0, 4))] if kind == 0 else [(A, T), (A, C), (C, G)][int(rng.integers(0, 3))] \
            if kind == 1 else unit_of(3, int(rng.integers(0, 9)))
        x[at:at + run] = repeat(unit, run)
        at += run


def substituted(x, n, L, seed):
    """a copy of x with n substitutions packed into one window of L bases near the middle (n <= L), so that the l-mers
    over the whole window see exactly n mismatches against the original and their neighbours see fewer, one by one"""
    rng = np.random.default_rng(seed)
    y = np.array(x, dtype=np.uint8)
    lo = max(0, (len(y) - L) // 2)
    for t in lo + rng.permutation(min(L, len(y)))[:n]:
        y[t] = (y[t] + 1 + int(rng.integers(0, 3))) & 3
    return y


def variants(s, L, d, seed=0):
    """[(name, sequence)]: an exact copy of s, its reverse complement, and copies with 1, d, d + 1 and d + 2 substitutions
    (m = d: the last hit of explain; d + 1: ISM's extra row; d + 2: just outside)"""
    out = [("copy", np.array(s, dtype=np.uint8)), ("rc", rc(s))]
    for n in sorted({1, d, d + 1, d + 2}):
        if 1 <= n <= L:
            out.append(("sub%d" % n, substituted(s, n, L, seed + n)))
    return out


def low_complexity(L, n, seed=0):
    """[(name, sequence of n bases)]: homopolymers of each base, (AC)n, the self-reverse-complementary (AT)n and (CG)n,
    periods 3 to 7, repeat units of L - 1, L and L + 1 bases"""
    out = [("poly%s" % "ACGT"[b], homopolymer(b, n)) for b in range(4)]
    out += [("AC", repeat((A, C), n)), ("AT", repeat((A, T), n)), ("CG", repeat((C, G), n))]
    out += [("period%d" % p, repeat(unit_of(p, seed), n)) for p in sorted({3, 4, 5, 6, 7, L - 1, L, L + 1}) if p >= 3]
    return out


def queries(L, d, seed=0):
    """[(name, sequence)]: the generator's whole family for one (L, d), every length of lengths(L) taken at least once and
    the low-complexity kinds spread over them"""
    out = []
    lens = lengths(L)
    for i, (name, _) in enumerate(low_complexity(L, L, seed)):
        n = lens[i % len(lens)]
        out.append(("%s_%d" % (name, n), dict(low_complexity(L, n, seed))[name]))
    for n in (64 + L - 1, 257 + L - 1, 600, MAX_LEN):
        out.append(("spliced_%d" % n, spliced(n, L, seed + n)))
    sv = spliced(120, L, seed + 7)
    out += [("sv_%s" % name, v) for name, v in variants(sv, L, d, seed)]
    return out


def small_set(L, d, seed=0, n=(64, 150, 300)):
    """[(name, sequence)]: a set small enough to run all against all through the CPU references: low-complexity
    sequences of 64 to 300 bases (and L, L + 1), a spliced one, and the variants of a spliced support vector"""
    out = [("polyA_%d" % n[1], homopolymer(A, n[1])), ("polyC_%d" % n[0], homopolymer(C, n[0])),
           ("polyT_%d" % (L + 1), homopolymer(T, L + 1)), ("AT_%d" % n[2], repeat((A, T), n[2])),
           ("AC_%d" % n[1], repeat((A, C), n[1])), ("CG_%d" % L, repeat((C, G), L)),
           ("period3_%d" % n[0], repeat(unit_of(3, seed), n[0])),
           ("periodL_%d" % n[2], repeat(unit_of(L, seed), n[2])),
           ("periodL+1_%d" % n[1], repeat(unit_of(L + 1, seed), n[1])),
           ("spliced_%d" % n[2], spliced(n[2], L, seed + 3))]
    sv = spliced(64 + L - 1, L, seed + 5)
    sv[10:10 + 2 * L] = A                                            # a homopolymer stretch inside the support vector
    return out + [("sv_%s" % name, v) for name, v in variants(sv, L, d, seed)]


# ------------------------------------------------------------------ k_ism's hit queue
QUEUE_THREADS, QUEUE_SLOTS, QUEUE_FLUSH, QUEUE_CAP = 256, 8, 64, 128


def queue_depths(x, s, L, d, tile):
    """A CPU model of the order in which k_ism queues hits, from the kernel's description (gkm_ism.hip),
    not from its code: a workgroup of 256 threads serves one tile of `tile` query positions; slot r of thread tid holds
    the l-mer pl0 + 256 r + tid of the l-mers [pl0, pl1) that cover the tile; each wave of 64 threads has a queue of its
    own.  For each l-mer of the support vector in order, for each slot r in which the wave has an l-mer, the wave pushes
    its forward hits (m <= min(d + 1, L)), flushes if the depth is >= 64, pushes its reverse-complement hits, flushes if
    the depth is >= 64; what is left is flushed at the end of the support vector.
    -> Counter {depth at a flush: how often}, over all tiles and waves."""
    from tests import ism_ref as R
    x = np.asarray(x, dtype=np.uint8)
    s = np.asarray(s, dtype=np.uint8)
    _, _, _, _, m = R._pairs(x, s, 0, L, 50, 50.0)
    hit = m <= min(d + 1, L)                                          # [nx, 2 ns]: forward l-mers of s, then reverse
    nx, ns = hit.shape[0], hit.shape[1] // 2
    out = collections.Counter()
    for t0 in range(0, len(x), tile):
        tlen = min(tile, len(x) - t0)
        pl0, pl1 = max(0, t0 - L + 1), min(nx, t0 + tlen)
        n = QUEUE_THREADS * QUEUE_SLOTS
        h = np.zeros((n, 2 * ns), dtype=np.int64)
        h[:pl1 - pl0] = hit[pl0:pl1]
        cnt = h.reshape(QUEUE_SLOTS, QUEUE_THREADS // 64, 64, 2 * ns).sum(axis=2)      # [slot, wave, l-mer of s]
        for w in range(QUEUE_THREADS // 64):
            slots = min(QUEUE_SLOTS, max(0, (pl1 - pl0 - 64 * w + QUEUE_THREADS - 1) // QUEUE_THREADS))
            depth = 0
            for q in range(ns):
                for r in range(slots):
                    for push in (int(cnt[r, w, q]), int(cnt[r, w, ns + q])):
                        depth += push
                        assert depth < QUEUE_CAP, "the model itself exceeds the queue's capacity"
                        if depth >= QUEUE_FLUSH:
                            out[depth] += 1
                            depth = 0
            if depth:
                out[depth] += 1
    return out


QUEUE_SHAPE = (4, 5, 2, 3)          # (kernel type, L, k, d) of the queue inputs: only an l-mer of five Cs misses AAAAA


def queue_inputs():
    """-> (support vector, [queries]) for QUEUE_SHAPE, built so that the queues see every depth 64 .. 127 at a flush.
    The support vector is AAAAA (one l-mer; its reverse complement TTTTT hits nothing made of A and C).  A query is A
    with runs of C: l-mer p is a hit unless all its five bases are C.  Per wave, slots (0, 1), (2, 3), .. pair up: the
    first pushes a hits, the second c, and a + c >= 64 is flushed.  Family 1: a = 63 (one l-mer of Cs at the head of the
    slot's 64 l-mers), c hits then Cs; family 2: a hits then Cs, c = 64; a short run of hits survives only at the very
    start of the query (elsewhere the C runs either side swallow it), which family 3 uses for depths 65 .. 68."""
    tl, L = QUEUE_SHAPE[1], QUEUE_SHAPE[1]
    sv = homopolymer(A, tl)
    out = []

    def build(plan):
        """plan: {(wave, slot): hits wanted among the slot's 64 l-mers, as (count, misses_first)}"""
        miss = np.zeros(MAX_LEN - L + 1, dtype=bool)
        for (w, r), (count, first) in plan.items():
            p0 = 256 * r + 64 * w
            if first:
                miss[p0:p0 + 64 - count] = True
            else:
                miss[p0 + count:p0 + 64] = True
        x = homopolymer(A, MAX_LEN)
        for p in np.nonzero(miss[:MAX_LEN - L + 1])[0]:
            x[p:p + L] = C
        return x

    depth = 64
    while depth <= 127:                                  # family 1: a = 63, c = depth - 63
        plan = {}
        for w in range(4):
            for r in (0, 2, 4):
                if depth <= 127:
                    plan[(w, r)] = (63, True)
                    plan[(w, r + 1)] = (depth - 63, False)
                    depth += 1
        out.append(build(plan))
    depth = 64
    while depth <= 127:                                  # family 2: a = depth - 64, c = 64
        plan = {}
        for w in range(4):
            for r in (0, 2, 4):
                if depth <= 127:
                    plan[(w, r)] = (depth - 64, False)
                    depth += 1
        out.append(build(plan))
    for a in (1, 2, 3, 4):                               # family 3: a hits at the very start, then Cs; slot 1 all hits
        out.append(build({(0, 0): (a, False)}))
    return sv, out


def ism_tile(L, d):
    """query positions per tile of k_ism: 4 (d + 1 + 3 min(d + 1, L)) bytes of tallies per position within
    160 KiB of LDS less 6 248 bytes of counters and queues, at most 2 048: 1 094 for (12, 8), 1 407 for (8, 6)"""
    return min(2048, (160 * 1024 - 6248) // (4 * (d + 1 + 3 * min(d + 1, L))))
