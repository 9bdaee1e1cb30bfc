"""The window kernels' case table (k_scan_lmers / k_scan_profiles / k_scan_score, k_wsim_profiles / k_wsim_normalize /
k_wsim_best), shared by tests/test_window_region_host.py (which holds every case to the condition it is
there for, with the oracle and host arithmetic alone), tests/test_window_region_gpu.py (the kernels against the oracle) and
tools/fuzz_windows.py (the randomised sweep, which draws its inputs from the same generators).  Plain numpy; nothing here
touches the device or the product library.

Inputs are base-code arrays (0..3; a code >= 4 is an invalid base), made by seeded generators:

  iid        independent uniform bases
  planted    iid, then l-mer pairs planted so that EVERY mismatch class m = 0..d occurs between an l-mer under a window of x
             and one under a window of y (at L = 12 iid pairs alone give no m <= 2), forward and reverse complement; where
             the records are long enough also a stretch of x copied into y diverged by substitutions, and one reverse
             complemented
  polyA      both records a homopolymer: every forward pair a hit
  same       y is x
  (polyA and same at the small shapes only: dense hits serialise the LDS atomics)

and `sprinkle_invalid` puts a few codes >= 4 into a record.
"""
from collections import namedtuple

import numpy as np

BUDGET = 3e8                          # l-mer comparisons the reference side of one test may cost, 2 n^2 per window pair
WS_GMAX, SP_GMAX, STRETCH = 32, 64, 4096
LDS_64K = 65536


# ------------------------------------------------------------------ host arithmetic restated from the launches
def group(n, s, gmax):
    """windows of one tile (wsim, gmax 32) or stretch (scan, gmax 64) along an axis: gkm_wsim.hip wsim_group, gkm_scan.hip
    scan_group"""
    return 1 if s >= n else min(gmax, 1 + (STRETCH - n) // s)


def wsim_lds_bytes(L, d, W, sx, sy):
    """dynamic LDS of a k_wsim_profiles launch, restated from gkmhip_wsim_profiles: the difference array of d + 1 classes,
    the words of y a full tile covers, and their 16-bit column intervals rounded up to 4 bytes"""
    n = W - L + 1
    gx, gy = group(n, sx, WS_GMAX), group(n, sy, WS_GMAX)
    words = n + (gy - 1) * sy
    return (d + 1) * (gx + 1) * (gy + 1) * 4 + words * 4 + ((words * 2 + 3) & ~3)


def tile_words(n, s, g, nw):
    """sum over the tiles of an axis of their l-mer words n + (windows - 1) s"""
    return sum(n + (min(g, nw - w0) - 1) * s for w0 in range(0, nw, g))


def record_length(W, s, windows):
    return W + (windows - 1) * s


def pair_cost(L, W, pairs):
    """comparisons the oracle makes for `pairs` window pairs (or self profiles): 2 n^2 each"""
    n = W - L + 1
    return 2 * n * n * pairs


# ------------------------------------------------------------------ generators
def rc(codes):
    return (3 - np.asarray(codes, dtype=np.uint8))[::-1].copy()


def substituted(rng, stretch, at):
    """a copy of `stretch` with the bases at the indices `at` replaced by another base"""
    out = np.array(stretch, dtype=np.uint8)
    at = np.asarray(at, dtype=np.int64)
    out[at] = (out[at] + rng.integers(1, 4, size=len(at))) % 4
    return out


def covered(T, L, W, s):
    """the l-mer positions under some window of a record of T bases, ascending"""
    n = W - L + 1
    seen = np.zeros(T - L + 1, dtype=bool)
    for a in range(0, T - W + 1, s):
        seen[a:a + n] = True
    return np.flatnonzero(seen)


def plant_classes(rng, x, y, L, d, W, sx, sy):
    """In place: an l-mer pair of every class m = 0..d between the covered l-mers of x and of y.  Where x holds d + 1
    covered positions at least L apart, the l-mer at the m-th becomes a covered l-mer of y (its reverse complement for odd
    m) with exactly m substitutions: y is not written, so no plant disturbs another.  Otherwise (short records at stride
    1) y's head becomes x's head with every base of [L, 2L) substituted: the l-mers at offset j of both then differ in
    exactly min(j, L) bases, and the classes the records are too short for are left to the iid pairs -- the host test
    holds the outcome, not this function."""
    cx, cy = covered(len(x), L, W, sx), covered(len(y), L, W, sy)
    slots, last = [], -L
    for p in cx:
        if p - last >= L:
            slots.append(int(p))
            last = p
    if len(slots) >= d + 1:
        step = max(1, len(slots) // (d + 1))                               # spread over the record: more than one tile
        for m in range(d + 1):
            q = int(cy[(m * 5) % len(cy)])
            word = substituted(rng, y[q:q + L], rng.permutation(L)[:m])
            x[slots[m * step]:slots[m * step] + L] = rc(word) if m % 2 else word
    else:
        T = min(len(x), len(y), 2 * L + 8)
        y[:T] = x[:T]
        y[L:min(T, 2 * L)] = substituted(rng, y[L:min(T, 2 * L)], np.arange(min(T, 2 * L) - L))


def plant_copies(rng, x, y, L):
    """In place, where both records hold 6 L bases: a stretch of x in y's last third with one base in eight substituted,
    and the reverse complement of another stretch in y's middle with one in twelve"""
    if min(len(x), len(y)) < 6 * L:
        return
    ln = min(len(x), len(y)) // 4
    a, b = len(x) // 2, len(y) - ln
    y[b:b + ln] = substituted(rng, x[a:a + ln], np.flatnonzero(rng.random(ln) < 0.125))
    a, b = len(x) - ln, len(y) // 3
    y[b:b + ln] = substituted(rng, rc(x[a:a + ln]), np.flatnonzero(rng.random(ln) < 1.0 / 12))


def sprinkle_invalid(rng, x, count):
    """In place: `count` bases become codes >= 4 (4, 5 or 255)"""
    at = rng.choice(len(x), size=min(count, len(x)), replace=False)
    x[at] = rng.choice(np.array([4, 5, 255], dtype=np.uint8), size=len(at))
    return np.sort(at)


COMPOSITIONS = ("iid", "planted", "polyA", "same")


def records(seed, comp, L, d, W, sx, sy, nx, ny, invalid=0):
    """(x, y): records that hold exactly nx and ny windows, of the composition `comp`; `invalid` codes >= 4 in each"""
    rng = np.random.default_rng(seed)
    Tx, Ty = record_length(W, sx, nx), record_length(W, sy, ny)
    x = rng.integers(0, 4, size=Tx, dtype=np.uint8)
    y = rng.integers(0, 4, size=Ty, dtype=np.uint8)
    if comp == "polyA":
        x[:], y[:] = 0, 0
    elif comp == "same":
        y = np.resize(x, Ty).copy()
    elif comp == "planted":
        plant_copies(rng, x, y, L)
        plant_classes(rng, x, y, L, d, W, sx, sy)
    elif comp != "iid":
        raise ValueError(comp)
    if invalid:
        sprinkle_invalid(rng, x, invalid)
        sprinkle_invalid(rng, y, invalid)
    return x, y


def scan_record(seed, comp, W, s, windows, invalid=0):
    """one record of `windows` windows for the scan: iid, with a repeat and an inverted repeat of itself when `planted`"""
    rng = np.random.default_rng(seed)
    x = rng.integers(0, 4, size=record_length(W, s, windows), dtype=np.uint8)
    if comp == "polyA":
        x[:] = 0
    elif comp == "planted":
        ln = min(200, len(x) // 5)
        x[len(x) - ln:] = substituted(rng, x[ln:2 * ln], np.flatnonzero(rng.random(ln) < 0.125))
        x[2 * ln:3 * ln] = substituted(rng, rc(x[:ln]), np.flatnonzero(rng.random(ln) < 1.0 / 12))
    if invalid:
        sprinkle_invalid(rng, x, invalid)
    return x


# ------------------------------------------------------------------ the named cases
# k_wsim_profiles over (L, k, d): the corners of the legal region no exact test reached -- L < 5, d > 6, d = L, d = L - 1
WSIM_LKD = [(2, 0, 2), (2, 1, 1), (3, 0, 3), (3, 3, 0), (4, 1, 3), (7, 0, 7), (9, 0, 9), (11, 1, 10), (12, 0, 12), (12, 1, 11),
            (12, 3, 9)]
WSIM_NX, WSIM_NY = 34, 12

WsimLaunch = namedtuple("WsimLaunch", "comp L k d W sx sy nx ny seed")


def wsim_region_launches(L, k, d):
    """the launches of one (L, k, d): W in {L, L + 1, 64} (and 300 where d >= 9), strides (1, 1), (7, 3), (W, 1), planted
    inputs everywhere, polyA and y = x below W = 300"""
    out = []
    for W in (L, L + 1, 64) + ((300,) if d >= 9 else ()):
        for sx, sy in ((1, 1), (7, 3), (W, 1)):
            for comp in ("planted",) if W == 300 else ("planted", "polyA", "same"):
                out.append(WsimLaunch(comp, L, k, d, W, sx, sy, WSIM_NX, WSIM_NY, 1000 * L + 10 * d + sx))
    return out


# more than 64 KiB of dynamic LDS, and the control just below: (name, launch, bytes, above)
LdsCase = namedtuple("LdsCase", "name launch lds above")
WSIM_LDS = [
    LdsCase("d12-s60", WsimLaunch("planted", 12, 0, 12, 300, 60, 60, 33, 33, 1), 69524, True),
    LdsCase("d12-s122", WsimLaunch("planted", 12, 0, 12, 300, 122, 122, 33, 33, 2), 81056, True),
    LdsCase("d9-s122", WsimLaunch("planted", 9, 0, 9, 300, 122, 122, 33, 33, 3), 68004, True),
    LdsCase("d12-w2047", WsimLaunch("planted", 12, 0, 12, 2047, 70, 70, 31, 2, 4), 74368, True),
    LdsCase("d8-control", WsimLaunch("planted", 12, 4, 8, 300, 122, 122, 33, 33, 5), 63632, False),
]

# tiles cut short by the 4 096-word stretch: L = 11, W = 2047, g = 21 at stride 100
STRETCH_LKD, STRETCH_W, STRETCH_G = (11, 7, 3), 2047, 21
STRETCH_STRIDES = [(100, 100), (2037, 100), (100, 2037), (1, 100)]


def stretch_launch(sx, sy):
    """(the launch with g + 1 windows on the limited axis and 2 on the other, the limited axis: 0 for x, 1 for y)"""
    L, k, d = STRETCH_LKD
    axis = 0 if (sx, sy) == (100, 2037) else 1
    nx, ny = (STRETCH_G + 1, 2) if axis == 0 else (2, STRETCH_G + 1)
    return WsimLaunch("planted", L, k, d, STRETCH_W, sx, sy, nx, ny, 7 * sx + sy), axis


# window_kernel / window_best end to end: one d = L tuple, one W = 2047 tuple whose chunks cut a stretch-limited tile
E2E_DL = WsimLaunch("planted", 9, 0, 9, 64, 3, 2, 40, 37, 11)
E2E_WIDE = WsimLaunch("planted", 11, 7, 3, 2047, 100, 100, 26, 24, 12)
E2E_WIDE_CHUNK = 2047 + 9 * 100       # ten windows per chunk: the chunk edges at windows 10 and 20 lie inside the tiles of 21

# k_scan_profiles values at wide windows: (L, k, d, W, s)
SCAN_WIDE = [(10, 6, 3, 600, 73), (12, 8, 4, 2047, 254), (11, 7, 3, 2047, 100), (4, 1, 3, 2047, 33), (10, 4, 6, 1100, 47)]
SCAN_WIDE_CAP = 19                    # windows compared with the oracle at W = 2047
SCORE_L = 6                           # k_scan_score at the same (W, s)


def scan_counts(g, W):
    """window counts around a stretch: g - 1, g, g + 1, and 2 g + 1 where W < 2047 or it stays within the cap"""
    out = [g - 1, g, g + 1]
    if W < 2047 or 2 * g + 1 <= SCAN_WIDE_CAP:
        out.append(2 * g + 1)
    return [c for c in out if c >= 1]


def scan_compared(L, W, g, windows):
    """the windows of a launch of `windows` windows whose profile is compared with the oracle's: all of them where that
    stays inside the budget, else at most SCAN_WIDE_CAP (W = 2047) or BUDGET's worth -- the ends of every stretch first,
    then evenly spaced ones"""
    most = min(windows, SCAN_WIDE_CAP if W == 2047 else int(0.8 * BUDGET // pair_cost(L, W, 1)))
    if most >= windows:
        return list(range(windows))
    first = [i for i in (0, g - 2, g - 1, g, g + 1, 2 * g - 1, 2 * g, windows - 1) if 0 <= i < windows]
    rest = [int(i) for i in np.linspace(0, windows - 1, most)]
    out = []
    for i in first + rest:
        if i not in out and len(out) < most:
            out.append(i)
    return sorted(out)
