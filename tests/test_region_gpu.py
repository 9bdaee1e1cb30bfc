"""The Gram path over the whole legal parameter region -- 2 <= L <= 12, k <= L, d <= L - k, so k = 0 and d = L too --
against the CPU oracle and the reference-made fixture tests/golden/region_expected.npz.  Outside the 43 bit-sliced (L, d)
pairs k_gram_direct is the only Gram kernel: nothing cross-checks it there but these tests.  Integer profiles and raw
values bit for bit (raw G = sum_m c_m P_m in ascending m from 0.0, the kernels' documented order), K at 1e-12 per element
with NaN in the same cells, sentinels kept in every cell a launch must not write."""
import ctypes

import numpy as np
import pytest

from tests import helpers
from tests import scan_ref as SR

pytestmark = pytest.mark.gpu

K_TOL = 1e-12          # the suite's bound on K (tests/test_gpu_parity.py), per element
SENT = -5.5            # what every output buffer holds before a launch
N_REGION = 80          # tuples of the fixture


@pytest.fixture(scope="module")
def dev(built):
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    from gkmqc_amd import device
    device.load()
    return device


@pytest.fixture(scope="module")
def region_seqs(dev):
    seqs, n_pos, _, _ = dev.read_problem(helpers.REGION_POS, helpers.REGION_NEG)
    return [np.array(s) for s in seqs]


@pytest.fixture(scope="module")
def region_cases():
    cases, lens, npos, _ = helpers.region_expected()
    assert len(cases) == N_REGION
    return cases, lens, npos


def _stream():
    import torch
    return torch.cuda.current_stream().cuda_stream


def _triangle(dev, seqs, params, kernel, want_profiles=True):
    """gkmhip_gram_rows over every row + gkmhip_normalize on sentinel-filled buffers one row and one column larger than
    the matrix -> dict(raw, K [n + 1, n + 1], P [n, n, d + 1] (sentinel -9), sq, kernel)"""
    import torch
    t, L, k, d, M, H, g = params
    ctx = dev.GramContext(t, L, k, d, M, H, g)
    try:
        ctx.set_kernel(kernel)
        ctx.set_sequences(seqs, _stream())
        n = len(seqs)
        G = torch.full((n + 1, n + 1), SENT, dtype=torch.float64, device="cuda")
        P = torch.full((n, n, d + 1), -9, dtype=torch.int32, device="cuda") if want_profiles else None
        sq = torch.full((n + 1,), SENT, dtype=torch.float64, device="cuda")
        ctx.gram_rows(np.arange(n), G.data_ptr(), n + 1, P.data_ptr() if want_profiles else None, n, False, _stream())
        torch.cuda.synchronize()
        name = ctx.last_kernel_name()
        raw = G.clone()
        ctx.normalize(G.data_ptr(), n + 1, sq.data_ptr(), False, _stream())
        torch.cuda.synchronize()
        return dict(raw=raw, K=G, P=P, sq=sq, kernel=name, n=n)
    finally:
        ctx.close()


def _refused_bitslice(dev, seqs, params):
    with pytest.raises(dev.GkmError, match="not instantiated"):
        _triangle(dev, seqs, params, dev.KERNEL_BITSLICE)


def _assert_close(got, want, tol, what):
    same, err = helpers.same_nonfinite_rel_err(got, want)
    print("%s: max rel err %.3g, %d NaN" % (what, err, int(np.isnan(np.asarray(want)).sum())))
    assert same, "%s: NaN / infinity in other cells than the oracle's" % (what,)
    assert err < tol, "%s: %g" % (what, err)


def _check_triangle(res, want_P, want_G, want_K, what, sqnorm=None):
    """P over the lower triangle and raw G bit for bit, unit diagonal, K at the bound, nothing above the diagonal or in
    the padding row and column"""
    n = res["n"]
    il, iu = np.tril_indices(n), np.triu_indices(n, 1)
    ils = np.tril_indices(n, -1)
    if want_P is not None:
        P = res["P"].cpu().numpy()
        assert np.array_equal(P[il], want_P[il]), "%s: integer mismatch profiles differ (%s)" % (what, res["kernel"])
        assert (P[iu] == -9).all(), "%s: profiles written above the diagonal" % (what,)
    raw, K, sq = res["raw"].cpu().numpy(), res["K"].cpu().numpy(), res["sq"].cpu().numpy()
    if want_G is not None:
        assert raw[:n, :n][il].tobytes() == want_G[il].tobytes(), "%s: raw values differ from sum_m c_m P_m" % (what,)
    for M in (raw, K):
        assert (M[:n, :n][iu] == SENT).all(), "%s: cells above the diagonal written" % (what,)
        assert (M[n] == SENT).all() and (M[:, n] == SENT).all(), "%s: padding written" % (what,)
    assert sq[n] == SENT
    assert (np.diag(K)[:n] == 1.0).all()
    if sqnorm is not None:
        _assert_close(sq[:n], sqnorm, K_TOL, what + " self norms")
    _assert_close(K[:n, :n][ils], want_K[ils] if want_K.ndim == 2 else want_K, K_TOL, what + " K")


# ------------------------------------------------------------------ (a), (b): every (L, d), k = L - d
_CASES = {}


def _ld_case(dev, region_seqs, L, d, t):
    """(sequences, oracle, k_gram_direct's result) for one (L, d, type), computed once: the region sequences plus three
    cut to L, L + 1 and 2 L - 1 bases (one, two and L l-mers)"""
    key = (L, d, t)
    if key not in _CASES:
        rng = np.random.default_rng(1000 + L)
        seqs = list(region_seqs) + [rng.integers(0, 4, m).astype(np.uint8) for m in (L, L + 1, 2 * L - 1)]
        params = (t, L, L - d, d, 50, 50.0, 1.0)
        _CASES[key] = (seqs, params, helpers.oracle_problem(seqs, params), _triangle(dev, seqs, params, dev.KERNEL_DIRECT))
    return _CASES[key]


@pytest.mark.parametrize("L", range(2, 13))
def test_direct_kernel_at_every_d(dev, region_seqs, L):
    """k_gram_direct at every d = 0 .. L of one L (k = L - d, so k = 0 at d = L), unweighted and weighted."""
    for d in range(L + 1):
        for t in (0, 4):
            seqs, params, orc, res = _ld_case(dev, region_seqs, L, d, t)
            assert res["kernel"] == "k_gram_direct"
            _check_triangle(res, orc["P"], orc["G"], orc["K"], "L=%d d=%d t=%d" % (L, d, t))


@pytest.mark.parametrize("L", range(2, 13))
def test_auto_equals_direct_at_every_d(dev, region_seqs, L):
    """KERNEL_AUTO gives k_gram_direct's numbers for every (L, d); outside the bit-sliced table it IS k_gram_direct and an
    explicit request for the bit-sliced kernel is refused."""
    import torch
    for d in range(L + 1):
        for t in (0, 4):
            seqs, params, orc, want = _ld_case(dev, region_seqs, L, d, t)
            auto = _triangle(dev, seqs, params, dev.KERNEL_AUTO)
            for key in ("raw", "K", "P", "sq"):
                assert torch.equal(auto[key].view(torch.int64) if auto[key].dtype == torch.float64 else auto[key],
                                   want[key].view(torch.int64) if want[key].dtype == torch.float64 else want[key]), (L, d, t, key)
            if (L, d) not in helpers.ALL_LD:
                assert auto["kernel"] == "k_gram_direct", (L, d, auto["kernel"])
                if t == 4:
                    _refused_bitslice(dev, seqs, params)


# ------------------------------------------------------------------ (c): the reference-made fixture, all six types
@pytest.mark.parametrize("idx", range(N_REGION))
def test_region_fixture(dev, region_seqs, region_cases, idx):
    """Every tuple of region_expected.npz through k_gram_direct, and through the bit-sliced kernel where it is
    instantiated (refused elsewhere): the reference's integer profiles, self norms and K.  At L = 12, k = 0, d = 12 the
    reference's K is undefined (it writes past its own profile array): P against the fixture, K against the oracle."""
    c = region_cases[0][idx]
    params = (c["kernel_type"], c["L"], c["k"], c["d"], c["M"], c["H"], c["gamma"])
    what = "t=%d L=%d k=%d d=%d M=%d" % params[:5]
    want_K, sqnorm = c["K"], c["sqnorm"]
    if want_K is None:
        assert (c["L"], c["k"], c["d"]) == (12, 0, 12)
        orc = helpers.oracle_problem(region_seqs, params)
        want_K, sqnorm = helpers.tril_pack(orc["K"]), np.sqrt(np.diag(orc["G"]))
    kernels = [dev.KERNEL_DIRECT]
    if (c["L"], c["d"]) in helpers.ALL_LD:
        kernels.append(dev.KERNEL_BITSLICE)
    else:
        _refused_bitslice(dev, region_seqs, params)
    for kern in kernels:
        res = _triangle(dev, region_seqs, params, kern)
        assert res["kernel"] == "k_gram_direct" if kern == dev.KERNEL_DIRECT else res["kernel"].startswith("k_gram_bitslice")
        _check_triangle(res, c["P"], None, want_K, what + " " + res["kernel"], sqnorm=sqnorm)


# ------------------------------------------------------------------ (d): the four launch modes of k_gram_direct
def _bits(x):
    return np.ascontiguousarray(x, dtype=np.float64).view(np.int64)


@pytest.mark.parametrize("L,d", [(12, 12), (12, 9), (11, 6), (10, 7), (10, 5), (8, 8), (6, 5), (3, 3), (2, 2), (2, 0)])
def test_launch_modes_of_the_direct_kernel(dev, region_seqs, L, d):
    """gkmhip_gram_rows on a row subset with local rows, gkmhip_gram_rows_full + gkmhip_normalize_rows_full,
    gkmhip_gram_block on a column range away from 0 (rows before, inside and after it) + gkmhip_normalize_block, and
    gkmhip_self_norms (the diagonal band): raw values bit for bit the oracle's, K at the bound, sentinels kept."""
    import torch
    rng = np.random.default_rng(77 + 13 * L + d)
    seqs = list(region_seqs) + [rng.integers(0, 4, int(m)).astype(np.uint8) for m in rng.integers(L, 90, 7)]
    n = len(seqs)
    for t in (0, 4):
        params = (t, L, L - d, d, 50, 50.0, 1.0)
        orc = helpers.oracle_problem(seqs, params)
        Gw, Kw = orc["G"], orc["K"]
        what = "L=%d d=%d t=%d" % (L, d, t)
        ctx = dev.GramContext(*params)
        try:
            ctx.set_kernel(dev.KERNEL_DIRECT)
            ctx.set_sequences(seqs, _stream())

            def buf(r, c):
                return torch.full((r, c), SENT, dtype=torch.float64, device="cuda")

            # the triangle, a row subset, local rows
            rows = np.array([0, 3, 4, 9, 17, n - 1], dtype=np.int32)
            G = buf(len(rows) + 1, n + 2)
            ctx.gram_rows(rows, G.data_ptr(), n + 2, None, 0, True, _stream())
            torch.cuda.synchronize()
            assert ctx.last_kernel_name() == "k_gram_direct"
            got = G.cpu().numpy()
            for i, a in enumerate(rows):
                assert (_bits(got[i, :a + 1]) == _bits(Gw[a, :a + 1])).all(), (what, "gram_rows", a)
                assert (got[i, a + 1:] == SENT).all(), (what, "gram_rows wrote past the diagonal", a)
            assert (got[len(rows)] == SENT).all()
            # the diagonal band
            sq = torch.full((n + 1,), SENT, dtype=torch.float64, device="cuda")
            ctx.self_norms(sq.data_ptr(), _stream())
            torch.cuda.synchronize()
            assert ctx.last_kernel_name() == "k_gram_direct"
            sqh = sq.cpu().numpy()
            with np.errstate(invalid="ignore"):
                assert np.array_equal(_bits(sqh[:n]), _bits(np.sqrt(np.diag(Gw)))), (what, "self norms")
            assert sqh[n] == SENT
            # full rows
            G = buf(len(rows) + 1, n + 2)
            ctx.gram_rows_full(rows, G.data_ptr(), n + 2, True, _stream())
            torch.cuda.synchronize()
            assert ctx.last_kernel_name() == "k_gram_direct"
            got = G.cpu().numpy()
            assert (_bits(got[:len(rows), :n]) == _bits(Gw[rows])).all(), (what, "gram_rows_full")
            assert (got[:, n:] == SENT).all() and (got[len(rows)] == SENT).all()
            ctx.normalize_rows_full(rows, G.data_ptr(), n + 2, sq.data_ptr(), True, _stream())
            torch.cuda.synchronize()
            got = G.cpu().numpy()
            off = np.ones((len(rows), n), dtype=bool)
            off[np.arange(len(rows)), rows] = False
            assert (got[np.arange(len(rows)), rows] == 1.0).all()
            _assert_close(got[:len(rows), :n][off], Kw[rows][off], K_TOL, what + " rows_full K")
            assert (got[:, n:] == SENT).all() and (got[len(rows)] == SENT).all()
            # a column range away from 0
            c0, c1 = 5, n - 4
            rows = np.array([1, 5, 7, c1 - 1, c1, n - 1], dtype=np.int32)
            ld = c1 - c0 + 2
            G = buf(len(rows) + 1, ld)
            ctx.gram_block(rows, c0, c1, G.data_ptr(), ld, _stream())
            torch.cuda.synchronize()
            assert ctx.last_kernel_name() == "k_gram_direct"
            got = G.cpu().numpy()
            assert (_bits(got[:len(rows), :c1 - c0]) == _bits(Gw[rows][:, c0:c1])).all(), (what, "gram_block")
            assert (got[:, c1 - c0:] == SENT).all() and (got[len(rows)] == SENT).all()
            ctx.normalize_block(rows, c0, c1, G.data_ptr(), ld, sq.data_ptr(), _stream())
            torch.cuda.synchronize()
            got = G.cpu().numpy()[:, :c1 - c0]
            want = Kw[rows][:, c0:c1]
            own = rows[:, None] == np.arange(c0, c1)[None, :]
            assert own.sum() == 3 and (got[:len(rows)][own] == 1.0).all()
            _assert_close(got[:len(rows)][~own], want[~own], K_TOL, what + " block K")
            assert (G.cpu().numpy()[:, c1 - c0:] == SENT).all() and (got[len(rows)] == SENT).all()
        finally:
            ctx.close()


# ------------------------------------------------------------------ (e): several columns per workgroup at high d
@pytest.mark.parametrize("L,d", [(8, 8), (6, 5)])
def test_several_columns_per_workgroup_at_high_d(dev, L, d):
    """The 2 600 short ragged sequences of test_general_kernel_with_several_columns_per_workgroup (three columns per
    workgroup, a ragged last chunk per tile) where no bit-sliced kernel can cross-check: 400 sampled cells and 20 diagonal
    ones against the oracle run on the sequences those cells name."""
    rng = np.random.default_rng(29)
    seqs = [rng.integers(0, 4, int(n)).astype(np.uint8) for n in rng.integers(24, 72, 2600)]
    params = (4, L, L - d, d, 50, 50.0, 1.0)
    res = _triangle(dev, seqs, params, dev.KERNEL_DIRECT, want_profiles=False)
    assert res["kernel"] == "k_gram_direct"
    pick = np.random.default_rng(5)
    rows = np.sort(pick.choice(np.arange(1300, 2600), 20, replace=False))
    cols = np.sort(pick.choice(np.arange(0, 1300), 20, replace=False))
    cols[0], rows[-1] = 0, 2599
    import torch
    ri, ci = torch.from_numpy(rows).cuda(), torch.from_numpy(cols).cuda()
    Gw, Kw = helpers.oracle_cells(seqs, rows, cols, params)
    raw = res["raw"][ri][:, ci].cpu().numpy()
    K = res["K"][ri][:, ci].cpu().numpy()
    assert (_bits(raw) == _bits(Gw)).all()
    _assert_close(K, Kw, K_TOL, "L=%d d=%d sampled K" % (L, d))
    Gd, Kd = helpers.oracle_cells(seqs, rows, rows, params)
    assert (_bits(res["raw"][ri, ri].cpu().numpy()) == _bits(np.diag(Gd))).all()
    assert (res["K"][ri, ri].cpu().numpy() == 1.0).all()
    up = res["K"][ci][:, ri].cpu().numpy()          # (the mirror cells lie above the diagonal)
    assert (up == SENT).all()


# ------------------------------------------------------------------ (f): int32 wrap at d = L
def _oracle_profiles(seqs, t, L, k, d, M=50, H=50.0):
    from oracle import oracle as O
    opt = O.make_opt(t, L, k, d, M, H)
    n = len(seqs)
    P = np.zeros((n, n, d + 1), dtype=np.int32)
    prof = np.zeros(d + 1, dtype=np.int32)
    vp = ctypes.c_void_p
    for a in range(n):
        for j in range(a + 1):
            O.lib().gkmo_profile(ctypes.byref(opt), seqs[a].ctypes.data_as(vp), len(seqs[a]),
                                 seqs[j].ctypes.data_as(vp), len(seqs[j]), prof.ctypes.data_as(vp))
            P[a, j] = prof
    return P


def test_int32_wraparound_at_d_equal_L(dev):
    """test_int32_wraparound_matches_wrapping_arithmetic's sequences where every window pair is counted (d = L, k = 0):
    the weighted profiles of the poly-A rows pass 2^31 many times over and must wrap like the oracle's unsigned
    arithmetic.  (The unweighted tuple cannot wrap -- 2 x 2038^2 < 2^31 -- and pins the m = L row at that size.)"""
    seqs = [np.zeros(2047, np.uint8), np.zeros(2000, np.uint8), np.tile(np.array([0, 0, 1], np.uint8), 600)]
    il = np.tril_indices(len(seqs))
    wrapped = {}
    for (t, L) in ((0, 10), (4, 12)):
        want = _oracle_profiles(seqs, t, L, 0, L, M=255, H=2000.0)
        wrapped[t] = bool((want < 0).any() or (np.abs(want.astype(np.int64)) > 2 ** 30).any())
        if t == 4:
            assert wrapped[4], "the oracle's weighted profiles did not wrap: the test checks nothing"
        res = dev.gram_matrix(seqs, t, L, 0, L, 255, 2000.0, want_profiles=True, kernel=dev.KERNEL_DIRECT)
        assert res["kernel"] == "k_gram_direct"
        assert (res["P"].cpu().numpy()[il] == want[il]).all(), (t, L)
        assert want[0, 0, 0] != 0 and want[0, 0, L] != 0         # poly-A: forward pairs at m = 0, reverse ones at m = L


def test_weighted_kernel_at_L2_with_a_2047_base_sequence(dev, tmp_path):
    """L = 2 and a sequence of the longest length the reader keeps: 2 046 l-mers, the first 1 023 away from the centre one,
    so the callers' distance-weight table (max(n) / 2 + 2 entries) has 1 025 -- gkmhip_set_sequences refused more than
    1 024, through the device layer and through gkm_main_pywrapper, for a tuple the reference accepts."""
    rng = np.random.default_rng(2047)
    seqs = [rng.integers(0, 4, m).astype(np.uint8) for m in (2047, 2046, 300, 2)]
    letters = np.frombuffer(b"ACGT", dtype=np.uint8)
    pf, nf = str(tmp_path / "p.fa"), str(tmp_path / "n.fa")
    for path, part in ((pf, seqs[:2]), (nf, seqs[2:])):
        with open(path, "wb") as f:
            for i, x in enumerate(part):
                f.write(b">s%d\n" % i + letters[x].tobytes() + b"\n")
    n = len(seqs)
    for d in (1, 2):
        params = (4, 2, 2 - d, d, 50, 50.0, 1.0)
        orc = helpers.oracle_problem(seqs, params)
        res = _triangle(dev, seqs, params, dev.KERNEL_AUTO)
        assert res["kernel"] == "k_gram_direct"
        _check_triangle(res, orc["P"], orc["G"], orc["K"], "L=2 d=%d, 2047 bases" % d)
        opt = dev.gkmOpt(4, 2, 2 - d, d, 50, 50.0, 1.0, pf.encode(), nf.encode(), 1, 0)
        kmat = np.zeros((n, n))
        rows = (kmat.ctypes.data + np.arange(n) * kmat.strides[0]).astype(np.uintp)
        sizes = np.zeros(2, dtype=np.int32)
        assert dev.load().gkm_main_pywrapper(ctypes.byref(opt), rows.ctypes.data, sizes.ctypes.data) == 0
        assert tuple(sizes) == (2, 2) and (np.diag(kmat) == 1.0).all() and (np.triu(kmat, 1) == 0).all()
        _assert_close(helpers.tril_pack(kmat), helpers.tril_pack(orc["K"]), K_TOL, "L=2 d=%d drop-in K" % d)


# ------------------------------------------------------------------ (g): the drop-in call
# (kernel type, L, k, d, M)
PYWRAPPER_TUPLES = [(2, 2, 1, 1, 50), (4, 3, 1, 2, 50), (4, 12, 1, 11, 50), (3, 10, 3, 7, 50), (5, 8, 1, 7, 50), (1, 9, 2, 7, 50),
                    (0, 11, 0, 11, 50), (4, 12, 4, 8, 255)]


@pytest.mark.parametrize("key", PYWRAPPER_TUPLES)
def test_drop_in_call_over_the_region(dev, region_cases, key):
    """gkm_main_pywrapper on the region FASTA pair against the reference's own K: sizes, unit diagonal, nothing above the
    diagonal or outside the matrix, every finite cell within 1e-15 (test_tiny_and_degenerate_problems (a)'s bound; an RBF
    cell is exp() of a value of at most 1 from the device's exp, a few ulp of 1.1e-16), NaN where the reference has NaN
    ((1, 9, 2, 7): negative c_m; (4, 12, 4, 8) at M = 255: a wrapped self profile)."""
    cases, lens, npos = region_cases
    (c,) = [x for x in cases if (x["kernel_type"], x["L"], x["k"], x["d"], x["M"]) == key]
    n = len(lens)
    opt = dev.gkmOpt(c["kernel_type"], c["L"], c["k"], c["d"], c["M"], c["H"], c["gamma"],
                     helpers.REGION_POS.encode(), helpers.REGION_NEG.encode(), 2, 0)
    kmat = np.zeros((n + 3, n + 3))
    rows = (kmat.ctypes.data + np.arange(kmat.shape[0]) * kmat.strides[0]).astype(np.uintp)
    sizes = np.zeros(2, dtype=np.int32)
    assert dev.load().gkm_main_pywrapper(ctypes.byref(opt), rows.ctypes.data, sizes.ctypes.data) == 0
    assert tuple(sizes) == (npos, n - npos)
    assert (np.diag(kmat)[:n] == 1.0).all()
    assert (np.triu(kmat, 1) == 0).all() and (kmat[n:] == 0).all() and (kmat[:, n:] == 0).all()
    got, want = helpers.tril_pack(kmat[:n, :n]), c["K"]
    assert np.array_equal(np.isnan(got), np.isnan(want))
    fin = np.isfinite(want)
    err = float(np.abs(got[fin] - want[fin]).max())
    print("%s: max abs err %.3g, %d NaN" % (key, err, int((~fin).sum())))
    assert np.isfinite(got[fin]).all() and err < 1e-15


# ------------------------------------------------------------------ (h): exact self profiles below L = 5 and at d = L
@pytest.mark.parametrize("t", [0, 4])
@pytest.mark.parametrize("L,d", [(2, 2), (3, 1), (4, 4), (7, 7), (12, 12)])
def test_exact_self_profiles_outside_the_scan_tests_range(dev, region_seqs, t, L, d):
    """gkmhip_self_profiles on the region sequences and gkmhip_scan_profiles (widths L and 64, strides 1 and 7) on iid
    bases and on a homopolymer: the oracle's P_m(w, w) bit for bit (tests/test_scan_gpu.py starts at L = 5, d <= 4)."""
    import torch
    from tests.test_scan_gpu import _device_profiles, _oracle_profiles as scan_oracle
    k = L - d
    ctx = dev.GramContext(t, L, k, d)
    try:
        ctx.set_sequences(region_seqs, _stream())
        n = len(region_seqs)
        ps = torch.full((n + 1, d + 1), -7, dtype=torch.int64, device="cuda")
        ctx.self_profiles(0, n, ps.data_ptr(), _stream())
        torch.cuda.synchronize()
        got = ps.cpu().numpy()
    finally:
        ctx.close()
    want = np.array([SR.self_profile(s, t, L, k, d) for s in region_seqs], dtype=np.int64)
    assert np.array_equal(got[:n], want) and (got[n] == -7).all()
    rng = np.random.default_rng(100 * L + d)
    for name, x in (("iid", rng.integers(0, 4, size=300, dtype=np.uint8)), ("polyA", np.zeros(150, dtype=np.uint8))):
        for W in (L, 64):
            for s in (1, 7):
                got, _, lm = _device_profiles(dev, t, L, k, d, x, W, s)
                want = scan_oracle(x, W, s, t, L, k, d)
                assert got.shape == want.shape and len(want) == (len(x) - W) // s + 1
                assert np.array_equal(got, want), (name, t, L, d, W, s, np.nonzero((got != want).any(axis=1))[0][:5])
                assert np.array_equal(lm, SR.R.pack(x, L))
