"""The hard inputs of tests/dense_inputs.py and the CPU references they are judged by, without a GPU: the generator holds
what it promises, the three Python references (explain_ref, ism_ref, lmer_ref) agree with closed forms on homopolymers,
and the queue inputs fill k_ism's hit queue to every depth it is designed for (by the CPU model of its push order)."""
import collections

import numpy as np
import pytest

from tests import dense_inputs as D
from tests import explain_ref as E
from tests import hyp_ref as HR
from tests import ism_ref as R
from tests import lmer_ref as LR


def test_generator_is_deterministic_and_covers_its_list():
    L, d = 10, 3
    a, b = D.queries(L, d), D.queries(L, d)
    assert [n for n, _ in a] == [n for n, _ in b] and all(np.array_equal(x, y) for (_, x), (_, y) in zip(a, b))
    assert all(x.dtype == np.uint8 and x.max() <= 3 and L <= len(x) <= D.MAX_LEN for _, x in a)
    assert set(D.lengths(L)) <= {len(x) for _, x in a}
    names = " ".join(n for n, _ in a)
    for kind in ("polyA", "polyC", "polyG", "polyT", "AC_", "AT_", "CG_", "period3", "period7", "period9", "period10",
                 "period11", "spliced", "sv_copy", "sv_rc", "sv_sub1", "sv_sub3", "sv_sub4", "sv_sub5"):
        assert kind in names, kind
    at, cg = D.repeat((D.A, D.T), 40), D.repeat((D.C, D.G), 40)
    assert np.array_equal(D.rc(at), at) and np.array_equal(D.rc(cg), cg)          # self-reverse-complementary
    assert list(D.WEIGHTS) == ["w50", "w254", "w255", "unit"]
    w = E.weights(4, 101, 255, 1e6)
    assert w[50] == 0 and (np.delete(w, 50) == 255).all()                         # the centre byte wraps
    assert (E.weights(4, 101, 254, 1e6) == 254).all()


@pytest.mark.parametrize("n", [1, 3, 4, 5])
def test_substituted_copies_put_exactly_n_mismatches_into_one_lmer(n):
    L = 10
    s = D.spliced(120, L, 7)
    y = D.substituted(s, n, L, n)
    diff = np.nonzero(s != y)[0]
    assert len(diff) == n and diff.max() - diff.min() < L
    m = np.array([(s[p:p + L] != y[p:p + L]).sum() for p in range(len(s) - L + 1)])
    assert m.max() == n and set(range(n + 1)) <= set(m.tolist())


def _cover(T, L):
    """the number of l-mers over each position of a T-base sequence"""
    t = np.arange(T)
    return np.minimum(t, T - L) - np.maximum(0, t - L + 1) + 1


@pytest.mark.parametrize("L,d,T,S", [(10, 3, 64, 37), (5, 3, 5, 9), (12, 11, 30, 12), (5, 5, 23, 17)])
def test_references_on_homopolymers_have_closed_forms(L, d, T, S):
    """unit weights: poly-A against poly-A matches every pair on every base (m = 0); against poly-T's strand and against
    poly-C every pair mismatches on every base (m = L), which only ISM's row B[L] sees, and only if d >= L - 1"""
    x, ns = D.homopolymer(D.A, T), S - L + 1
    cover = _cover(T, L)
    if d < L:
        H = E.tallies(x, D.homopolymer(D.A, S), 0, L, d)
        assert np.array_equal(H[:, 0], cover * ns) and not H[:, 1:].any()
        assert not E.tallies(x, D.homopolymer(D.C, S), 0, L, d).any()
    U, B = R.tallies(x, D.homopolymer(D.A, S), 0, L, d)
    assert np.array_equal(U[:, 0], cover * ns) and not U[:, 1:].any()
    wantB = np.zeros_like(B)
    if d + 1 >= L:
        wantB[:, L, D.T] = cover * ns                     # the reverse strand of poly-A is poly-T
    assert np.array_equal(B, wantB)
    U, B = R.tallies(x, D.homopolymer(D.C, S), 0, L, d)
    wantB = np.zeros_like(B)
    if d + 1 >= L:
        wantB[:, L, D.C] = cover * ns
        wantB[:, L, D.G] = cover * ns
    assert not U.any() and np.array_equal(B, wantB)
    nx = T - L + 1
    P = R.profile(x, D.homopolymer(D.A, S), 0, L, d)
    want = np.zeros(d + 1, dtype=np.int64)
    want[0] = nx * ns
    if d >= L:
        want[L] = nx * ns
    assert np.array_equal(P, want)
    if d < L:
        share = np.linspace(1.0, 2.0, d + 1)
        U, B = R.tallies(x, D.homopolymer(D.A, S), 0, L, d)
        raw = HR.raw_from_tallies(x, U, B, share, d)
        assert np.array_equal(raw[:, D.A], share[0] * cover * ns) and not raw[:, 1:3].any()


def test_weighted_homopolymer_tally_is_the_product_of_the_weight_sums():
    """positional weights: H[0][t] = (sum of w_x over the l-mers over t) x (sum of w_s), here with every weight 254"""
    L, T, S = 12, 100, 40
    H = E.tallies(D.homopolymer(D.G, T), D.homopolymer(D.G, S), 4, L, 4, 254, 1e6)
    assert np.array_equal(H[:, 0], _cover(T, L) * 254 * (S - L + 1) * 254)
    U, _ = R.tallies(D.homopolymer(D.G, T), D.homopolymer(D.G, S), 4, L, 4, 254, 1e6)
    assert np.array_equal(U, H)


@pytest.mark.parametrize("L,d,T", [(10, 3, 40), (5, 3, 12)])
def test_self_profiles_of_a_homopolymer_have_a_closed_form(L, d, T):
    """poly-A with one base set to C or G: the na l-mers over it differ from each other in two bases, from the others in
    one (set to T, the mutant's reverse strand carries an A and meets the forward l-mers at m = L - 2: not this form)"""
    x = D.homopolymer(D.A, T)
    nx = T - L + 1
    got = R.self_profiles(x, 0, L, d)
    cover = _cover(T, L)
    for t in range(T):
        na = int(cover[t])
        own = np.zeros(d + 1, dtype=np.int64)
        own[0] = nx * nx
        mut = np.zeros(d + 1, dtype=np.int64)
        mut[0], mut[1], mut[2] = (nx - na) ** 2 + na, 2 * na * (nx - na), na * (na - 1)
        assert np.array_equal(got[t, D.A], own), t
        for b in (D.C, D.G):
            assert np.array_equal(got[t, b], mut), (t, b)


@pytest.mark.parametrize("L,d", [(8, 3), (5, 5)])
def test_lmer_count_on_homopolymer_classes_has_a_closed_form(L, d):
    """classes A^L (its reverse complement is T^L) and, for even L, the palindrome (AT)^(L/2), which counts twice"""
    polyA, polyT = 0, 4 ** L - 1
    oneC = 1                                                        # A..AC: one substitution from A^L
    v, cv = np.array([polyA]), np.array([3.0])
    for m in range(d + 1):
        c = np.zeros(d + 1)
        c[m] = 1.0
        W = LR.count(np.array([polyA, polyT, oneC]), v, cv, L, d, c)
        want = [3.0 * ((m == 0) + (m == L)), 3.0 * ((m == 0) + (m == L)), 3.0 * ((m == 1) + (m == L))]
        assert W.tolist() == want, (m, W)
    if L % 2 == 0:
        pal = int(E.pack(D.repeat((D.A, D.T), L), L)[0])
        assert LR.rc_codes(np.array([pal]), L)[0] == pal
        c = np.zeros(d + 1)
        c[0] = 1.0
        assert LR.count(np.array([pal]), np.array([pal]), np.array([1.0]), L, d, c)[0] == 2.0


def _queue_histogram():
    t, L, k, d = D.QUEUE_SHAPE
    sv, qs = D.queue_inputs()
    total = collections.Counter()
    for x in qs:
        total += D.queue_depths(x, sv, L, d, D.ism_tile(L, d))
    return total, qs


def test_queue_inputs_reach_every_design_depth():
    """by the CPU model of k_ism's push order, the queue inputs flush at every depth 64 .. 127 at least once: 127 (63
    queued, then a push of 64) is the deepest the design allows, 64 the shallowest that triggers a flush, and every depth
    past 96 shows that a push on top of a part-filled queue is exercised"""
    total, qs = _queue_histogram()
    missing = [k for k in range(D.QUEUE_FLUSH, D.QUEUE_CAP) if k not in total]
    assert not missing, missing
    assert max(total) == D.QUEUE_CAP - 1 and total[D.QUEUE_FLUSH] > 0
    assert all(len(x) == D.MAX_LEN for x in qs)


def test_dense_pairs_overfill_nothing_in_the_model():
    """fully dense pairs (every lane hits on both strands) run the model at its steady state: 64 per push, every flush at
    exactly 64; the model asserts internally that no depth reaches the capacity"""
    L, d = 12, 8
    x = D.repeat((D.A, D.T), 700)
    total = D.queue_depths(x, D.repeat((D.A, D.T), 40), L, d, D.ism_tile(L, d))
    assert total[64] > 0 and max(total) < D.QUEUE_CAP
    total = D.queue_depths(D.spliced(1500, 10, 3), D.spliced(200, 10, 4), 10, 3, D.ism_tile(10, 3))
    assert len([k for k in total if k > 64]) > 10            # spliced input: a spread of depths on top of part-filled queues
