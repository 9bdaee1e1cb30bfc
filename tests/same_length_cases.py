"""The same-length launches that tests/test_same_length_plan_host.py (CPU: which variant the plan takes) and
tests/test_same_length_sweep_gpu.py (GPU: what that variant computes) share, and the length bands in which a same-length
problem keeps one resident piece per lane (tools/fuzz_parity.py draws from them).

A row of CASES: (L, d, length, n, PK, riders) -- n rows of `length` bases under KERNEL_BITSLICE run k_gram_bitslice's variant
PK (1, 2 several pieces per lane; 4 group records; 5 with riders; 6, 7 the same two with shift records) and carry riders or
not.  The host test recomputes every PK from the packing (bitslice_cpu_probe.so) and the LDS rule of gkm_gram.hip
plan_bitslice; nothing here is taken from a GPU run."""
from collections import namedtuple

from tests.helpers import ALL_LD

W = 10                      # words per lane: a lane holds 32 bit rows of W positions
OWN = 5                     # a piece that does not finish its row owns whole groups of five windows
RIDER_B0 = 30               # riders live in bit rows 30, 31: the resident must end at or below bit row 30
MAXLEN = 2047               # GKM_MAXLEN

Case = namedtuple("Case", "L d length n pk riders")


def lane_capacity(L):
    """l-mer windows a full lane owns (gkm_pack.h same_length_piece_check `cap`; the kernel's BsArgs.cap)"""
    return (32 * W - (L - 1)) // OWN * OWN


def shared_from(L):
    """Free bit rows from which pack_rows starts the next row in the same lane: a first piece of at least 3 W windows"""
    f = 1
    while (f * W - (L - 1)) // OWN * OWN < 3 * W:
        f += 1
    return f


def band(L, lanes):
    """(lo, hi): the lengths at which every row of a same-length problem takes exactly `lanes` lanes, one piece each, and
    no lane is shared: lanes - 1 full pieces, and a last piece that leaves fewer than shared_from(L) bit rows and owns at
    most the lane capacity.  None where the band lies above MAXLEN."""
    cap = lane_capacity(L)
    lo = (lanes - 1) * cap + (32 - shared_from(L)) * W + 1
    hi = lanes * cap + L - 1
    return (lo, min(hi, MAXLEN)) if lo <= MAXLEN else None


def lanes_of(L, length):
    """Lanes per row if `length` lies in a band, else 0 (rows share lanes: the several-pieces variants)"""
    for lanes in range(1, 8):
        b = band(L, lanes)
        if b and b[0] <= length <= b[1]:
            return lanes
    return 0


def rows_for(lanes):
    """The smallest row count with a second tile: n = 70 for one-lane rows (64 residents, 2 riders where they fit, a short
    second tile), 64 // lanes + 3 otherwise"""
    return 70 if lanes <= 1 else 64 // lanes + 3


def _c(L, d, length, pk, riders=False, n=None):
    return Case(L, d, length, n if n is not None else rows_for(lanes_of(L, length)), pk, riders)


# every instantiated pair at 300 bp: riders and shift records for L <= 11 -- but (11, 5), whose six profile rows of 128 slots
# leave the longer hit list no room in four LDS granules: group records with riders -- and PK 6 for L = 12 (no rider variant)
AT_300 = [_c(L, d, 300, 6 if L == 12 else 5 if (L, d) == (11, 5) else 7, riders=L <= 11) for (L, d) in ALL_LD]

EDGES = [
    # one lane: the band's edges, the first length without riders, the first length below (rows share lanes)
    _c(10, 3, 281, 7, True), _c(10, 3, 280, 2, n=70), _c(11, 3, 301, 6), _c(11, 3, 320, 6), _c(10, 3, 319, 6),
    _c(6, 1, 320, 6), _c(5, 2, 281, 7, True), _c(5, 2, 319, 6), _c(5, 4, 301, 6), _c(8, 4, 320, 1, n=70),
    _c(12, 4, 271, 6), _c(12, 4, 316, 6), _c(12, 4, 270, 2, n=70),
    # a last piece that would own more than the lane capacity (one window past the last whole group): several pieces
    _c(10, 3, 320, 1, n=70), _c(12, 4, 320, 1, n=70), _c(10, 3, 630, 1, n=35),
    # two and three lanes
    _c(10, 3, 591, 6), _c(10, 3, 629, 6), _c(11, 3, 630, 6), _c(10, 3, 590, 1, n=35),
    _c(11, 3, 901, 6), _c(11, 3, 940, 6), _c(7, 2, 936, 6), _c(11, 3, 900, 1, n=24),
    # four lanes: d = 4 with both record kinds inside the LDS budget; (12, 6) with group records only
    _c(10, 4, 1249, 6), _c(12, 6, 926, 6), _c(12, 6, 1186, 4),
    # five lanes: at d = 4 the whole band lies where shift records do not fit and group records do
    _c(10, 4, 1521, 4), _c(10, 4, 1559, 4), _c(10, 4, 1520, 1, n=15), _c(11, 5, 1521, 4), _c(9, 2, 1521, 6),
    _c(12, 6, 1491, 4), _c(12, 6, 1536, 6),
    # six lanes, the most a same-length problem reaches below 2 048 bp: the budget crossings lie inside the band
    _c(10, 4, 1831, 4), _c(10, 4, 1853, 4), _c(10, 4, 1854, 6), _c(10, 4, 1869, 6), _c(10, 4, 1830, 1, n=13),
    _c(8, 2, 1855, 6), _c(8, 2, 1856, 4), _c(11, 5, 1831, 6),
    # the longest sequence: six full lanes and a seventh piece of 19 bit rows, whose lane the next row shares
    _c(10, 4, 2047, 1, n=12),
]

CASES = AT_300 + EDGES

# the launches repeated through the column-range launch and the cross kernel
MODE_CASES = [c for c in CASES if (c.L, c.d, c.length) in ((5, 4, 300), (9, 2, 300), (11, 5, 300), (10, 4, 1521))]
# multi-lane and fallback cases run a dense-hit input as well
DENSE_CASES = [c for c in EDGES if c.length > 320] + [c for c in AT_300 if (c.L, c.d) in ((11, 5), (5, 4), (6, 3), (8, 4))]


def case_id(c):
    return "L%d-d%d-%dbp-n%d-pk%d%s" % (c.L, c.d, c.length, c.n, c.pk, "r" if c.riders else "")
