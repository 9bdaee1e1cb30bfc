"""Where the device ABI of include/gkm_hip.h puts its results: leading dimensions larger than n (ld, ldp, lds), the cells a
call must not write, and the calls that must refuse a leading dimension that is too small.  Every output starts filled
with a sentinel bit pattern (tests/abi_cases.py) and every comparison is of bytes: a written cell equals the ld == n
launch (and, where test_same_length_sweep_gpu.py holds that launch against the CPU oracle, the oracle), every other
cell still holds the sentinel.  An `n` typed for an `ld` in one of the kernels that index by hand shows here as a value
in the wrong cell."""
import numpy as np
import pytest

from tests import abi_cases as A
from tests import helpers

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev(built):
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    from gkmqc_amd import device
    device.load()
    return device


def _stream():
    import torch
    return torch.cuda.current_stream().cuda_stream


def _context(dev, launch, t, gamma=1.0):
    seqs = launch.seqs()
    ctx = dev.GramContext(t, launch.L, launch.L - launch.d, launch.d, gamma=gamma)
    ctx.set_kernel(getattr(dev, launch.kernel))
    ctx.set_sequences(seqs, _stream())
    return ctx, seqs


def _family(kernel_name):
    return kernel_name.split("<")[0]


_PLAIN = {}


def _plain(dev, launch, t):
    """(P, G) of the ld == ldp == n launch over all rows, numpy, computed once per (launch, weighting)"""
    from tests.test_shift_records_gpu import _launch
    if (launch.name, t) not in _PLAIN:
        P, G, riders, name, pk = _launch(dev, launch.seqs(), (t, launch.L, launch.L - launch.d, launch.d),
                                         getattr(dev, launch.kernel))
        assert (name, pk, riders > 0) == (launch.kernel_name, launch.variant, launch.riders)
        _PLAIN[(launch.name, t)] = (P, G)
    return _PLAIN[(launch.name, t)]


def _written(nrows_out, width, rows, local):
    """mask [nrows_out, width] of the cells a triangle launch over `rows` writes, and the matrix row each output row is"""
    mask = np.zeros((nrows_out, width), dtype=bool)
    where = {}
    for i, a in enumerate(rows):
        r = i if local else int(a)
        mask[r, :a + 1] = True
        where[r] = int(a)
    return mask, where


# ------------------------------------------------------------------ 1. gram_rows
@pytest.mark.parametrize("t", A.WEIGHTINGS)
@pytest.mark.parametrize("launch", A.LAUNCHES, ids=A.launch_id)
def test_gram_rows_with_padded_rows_and_profiles(dev, launch, t):
    import torch
    ctx, seqs = _context(dev, launch, t)
    try:
        n, d = len(seqs), launch.d
        Pn, Gn = _plain(dev, launch, t)
        Pn, Gn = A.bits(Pn), A.bits(Gn)
        subset = A.subset_with_a_jump(n)
        ldp = n + 5
        for ld in A.leading_dimensions(n):
            for rows, local in ((np.arange(n, dtype=np.int32), False), (subset, False), (subset, True)):
                nr = len(rows) if local else n
                G, P = A.sentinel_f64((nr, ld)), A.sentinel_i32((nr, ldp, d + 1))
                ctx.gram_rows(rows, G.data_ptr(), ld, P.data_ptr(), ldp, local, _stream())
                torch.cuda.synchronize()
                if len(rows) == n:
                    A.assert_path(ctx, launch)
                else:      # (fewer rows may pack into the other several-pieces variant: the family stays)
                    assert _family(ctx.last_kernel_name()) == _family(launch.kernel_name)
                gmask, where = _written(nr, ld, rows, local)
                pmask, _ = _written(nr, ldp, rows, local)
                Gb, Pb = A.bits(G), A.bits(P)
                for r, a in where.items():
                    assert (Gb[r, :a + 1] == Gn[a, :a + 1]).all(), (ld, local, a)
                    assert (Pb[r, :a + 1] == Pn[a, :a + 1]).all(), (ld, local, a)
                # the upper triangle, the padding columns and the rows not listed
                assert A.untouched(G, ~gmask), (ld, local)
                assert A.untouched(P, ~pmask), (ld, local)
                if launch.case is not None and len(rows) == n:
                    from tests.test_same_length_sweep_gpu import _reference
                    orows, Po, Go = _reference(launch.case, seqs, "iid", t)
                    Gf, Pf = G.cpu().numpy(), P.cpu().numpy()
                    for a in orows:
                        assert np.array_equal(Pf[a, :a + 1], Po[a, :a + 1]), (ld, a)
                        assert np.array_equal(Gf[a, :a + 1], Go[a, :a + 1]), (ld, a)
    finally:
        ctx.close()


# ------------------------------------------------------------------ 2. full rows
@pytest.mark.parametrize("t,gamma", [(4, 1.0), (5, 2.0)])
@pytest.mark.parametrize("name", ["pk7", "packed", "direct"])
def test_full_rows_with_padding(dev, name, t, gamma):
    """gkmhip_gram_rows_full + gkmhip_normalize_rows_full into rows of n + 3 doubles, listed rows in both placements:
    every cell of a listed row equals the symmetric completion of gram_matrix's K; padding and unlisted rows keep the
    sentinel."""
    import torch
    launch = A.by_name(name)
    ctx, seqs = _context(dev, launch, t, gamma)
    try:
        n = len(seqs)
        full = dev.gram_matrix(seqs, t, launch.L, launch.L - launch.d, launch.d, gamma=gamma,
                               kernel=getattr(dev, launch.kernel))
        assert full["kernel"] == launch.kernel_name and full["variant"] == launch.variant
        K = full["K"].cpu().numpy()
        Ksym = A.bits(np.tril(K) + np.tril(K, -1).T)
        ld = n + 3
        sq = torch.zeros(n, dtype=torch.float64, device="cuda")
        ctx.self_norms(sq.data_ptr(), _stream())
        assert A.same_bytes(sq, full["sqnorm"])
        rows = A.subset_with_a_jump(n)
        for local in (False, True):
            nr = len(rows) if local else n
            G = A.sentinel_f64((nr, ld))
            ctx.gram_rows_full(rows, G.data_ptr(), ld, local, _stream())
            assert _family(ctx.last_kernel_name()) == _family(launch.kernel_name)
            ctx.normalize_rows_full(rows, G.data_ptr(), ld, sq.data_ptr(), local, _stream())
            torch.cuda.synchronize()
            Gb = A.bits(G)
            mask = np.zeros((nr, ld), dtype=bool)
            for i, a in enumerate(rows):
                r = i if local else int(a)
                mask[r, :n] = True
                assert (Gb[r, :n] == Ksym[a]).all(), (local, a)
            assert A.untouched(G, ~mask), local
    finally:
        ctx.close()


# ------------------------------------------------------------------ 3. normalize
def _raw_matrix(dev, n, t, gamma):
    """(context with n short sequences uploaded, their raw lower triangle as numpy)"""
    import torch
    from tests.test_rider_parity_gpu import _seqs
    ctx = dev.GramContext(t, 8, 6, 2, gamma=gamma)
    ctx.set_sequences(_seqs(n, 40, 4000 + n), _stream())
    G = torch.zeros((n, n), dtype=torch.float64, device="cuda")
    ctx.gram_rows(np.arange(n), G.data_ptr(), n, None, 0, False, _stream())
    torch.cuda.synchronize()
    return ctx, G.cpu().numpy()


def _normalised(raw, rbf, gamma):
    """The header's formula in float64 numpy: product of the norms first, one division, RBF, unit diagonal; lower triangle"""
    sq = np.sqrt(np.diag(raw))
    n = len(sq)
    K = np.zeros((n, n))
    il = np.tril_indices(n, -1)
    K[il] = raw[il] / (sq[il[0]] * sq[il[1]])
    if rbf:
        K[il] = np.exp(gamma * (K[il] - 1))
    np.fill_diagonal(K, 1.0)
    return K, sq


def _padded_lower(raw, ld):
    """device [n, ld]: the lower triangle of `raw`, the sentinel everywhere else"""
    import torch
    n = raw.shape[0]
    host = np.full((n, ld), A.SENTINEL_F64, dtype=np.int64)
    il = np.tril_indices(n)
    host[il] = A.bits(raw)[il]
    return torch.from_numpy(host).cuda().view(torch.float64)


def _check_normalised(K, ld, n, want, symmetric, rbf):
    """K [n, ld] against the lower triangle `want`: values, the mirror or the untouched upper triangle, the padding"""
    Kb = A.bits(K)
    got = K.cpu().numpy()
    il, iu = np.tril_indices(n), np.triu_indices(n, 1)
    if rbf:      # the device's exp() against the host's: the bound test_scoring_against_a_set_matches_the_reference uses
        err = helpers.max_rel_err(got[il], want[il])
        assert err < 1e-12, err
    else:
        assert (Kb[il] == A.bits(want)[il]).all()
    assert (got[np.arange(n), np.arange(n)] == 1.0).all()
    upper = np.zeros((n, ld), dtype=bool)
    upper[iu] = True
    pad = np.zeros((n, ld), dtype=bool)
    pad[:, n:] = True
    if symmetric:
        assert (Kb[:, :n][iu] == Kb[:, :n].T[iu]).all()      # the bitwise mirror of the lower triangle
    else:
        assert A.untouched(K, upper)
    assert A.untouched(K, pad)


@pytest.mark.parametrize("t", [2, 3])
@pytest.mark.parametrize("n", [70, 257, 300])
def test_normalize_with_padded_rows(dev, n, t):
    """gkmhip_normalize on a raw matrix with ld > n: 70 rows (one block of 256 threads, partly idle), 257 (one thread into
    the second block), 300."""
    import torch
    gamma, rbf = 2.0, t == 3
    ctx, raw = _raw_matrix(dev, n, t, gamma)
    try:
        want, sq_want = _normalised(raw, rbf, gamma)
        for ld in A.leading_dimensions(n):
            for symmetric in (False, True):
                for with_sq in (False, True):
                    K = _padded_lower(raw, ld)
                    sq = A.sentinel_f64((n + 2,))
                    ctx.normalize(K.data_ptr(), ld, sq.data_ptr() if with_sq else None, symmetric, _stream())
                    torch.cuda.synchronize()
                    _check_normalised(K, ld, n, want, symmetric, rbf)
                    guard = np.zeros(n + 2, dtype=bool)
                    guard[n:] = True
                    if with_sq:
                        assert (A.bits(sq)[:n] == A.bits(sq_want)).all() and A.untouched(sq, guard)
                    else:
                        assert A.untouched(sq, np.ones(n + 2, dtype=bool))
    finally:
        ctx.close()


# ------------------------------------------------------------------ 4. assemble_normalize
@pytest.mark.parametrize("t,gamma", [(4, 1.0), (5, 2.0)])
@pytest.mark.parametrize("packed", [False, True], ids=["lds=n+5", "packed"])
def test_assemble_normalize_from_padded_and_packed_slabs(dev, packed, t, gamma):
    """The slabs hold the raw rows in a permuted order -- rows of n + 5 doubles, or packed back to back behind five
    doubles of slack (lds == 1) -- with NaN wherever no value of j <= a sits; K has ld = n + 3."""
    import torch
    from gkmqc_amd import sharding
    launch = A.by_name("packed")
    ctx, seqs = _context(dev, launch, t, gamma)
    try:
        n = len(seqs)
        G = torch.zeros((n, n), dtype=torch.float64, device="cuda")
        ctx.gram_rows(np.arange(n), G.data_ptr(), n, None, 0, False, _stream())
        A.assert_path(ctx, launch)
        raw = G.clone()
        sq_want = torch.zeros(n, dtype=torch.float64, device="cuda")
        ctx.normalize(G.data_ptr(), n, sq_want.data_ptr(), False, _stream())
        torch.cuda.synchronize()
        raw, want = raw.cpu().numpy(), G.cpu().numpy()
        order = np.random.default_rng(17).permutation(n)          # slab position -> matrix row
        slot = np.zeros(n, dtype=np.int64)
        if packed:
            off = sharding.packed_row_offsets(order) + 5          # (not at the start of the buffer)
            lds = 1
            slabs = np.full(int(off[-1]) + 7, np.nan)
            for i, a in enumerate(order):
                slabs[off[i]:off[i] + a + 1] = raw[a, :a + 1]
                slot[a] = off[i]
        else:
            lds = n + 5
            slabs = np.full((n, lds), np.nan)
            for i, a in enumerate(order):
                slabs[i, :a + 1] = raw[a, :a + 1]
                slot[a] = i
        d_slabs, d_slot = torch.from_numpy(slabs).cuda(), torch.from_numpy(slot).cuda()
        ld = n + 3
        for symmetric in (False, True):
            K, sq = A.sentinel_f64((n, ld)), A.sentinel_f64((n + 2,))
            ctx.assemble_normalize(d_slabs.data_ptr(), lds, d_slot.data_ptr(), K.data_ptr(), ld, sq.data_ptr(), symmetric,
                                   _stream())
            torch.cuda.synchronize()
            _check_normalised(K, ld, n, want, symmetric, rbf=False)      # (the same device expression: bit for bit, RBF too)
            guard = np.zeros(n + 2, dtype=bool)
            guard[n:] = True
            assert (A.bits(sq)[:n] == A.bits(sq_want)).all() and A.untouched(sq, guard)
    finally:
        ctx.close()


# ------------------------------------------------------------------ 5. all-gather
@pytest.mark.parametrize("devices", [[0, 0], [0, 0, 0]], ids=["0,0", "0,0,0"])
def test_allgather_into_padded_matrices(dev, devices):
    import torch
    seqs, _, _, _ = dev.read_problem(helpers.QUIRK_POS, helpers.QUIRK_NEG)
    n = len(seqs)
    assert n % 64
    ld = n + 3
    pad = np.zeros((n, ld), dtype=bool)
    pad[:, n:] = True
    upper = np.zeros((n, ld), dtype=bool)
    upper[np.triu_indices(n, 1)] = True
    for symmetric in (False, True):
        one = dev.gram_matrix(seqs, 4, 11, 7, 3, symmetric=symmetric)["K"]
        out = [A.sentinel_f64((n, ld)) for _ in devices]
        res = dev.gram_matrix_multi(seqs, 4, 11, 7, 3, devices=devices, symmetric=symmetric, ld=ld, out=out)
        torch.cuda.synchronize()
        assert res["transport"] == "p2p"
        for K in out:
            cells = ~pad if symmetric else ~(pad | upper)
            assert (A.bits(K)[cells] == A.bits(one)[cells[:, :n]]).all()
            assert A.untouched(K, pad if symmetric else pad | upper)
    # the default is unchanged: ld = n, zeroed matrices
    res = dev.gram_matrix_multi(seqs, 4, 11, 7, 3, devices=devices)
    assert all(tuple(K.shape) == (n, n) and torch.equal(K, torch.tril(one)) for K in res["K"])


# ------------------------------------------------------------------ 6. copy-out
STAGING_BYTES = 64 << 20      # gkm_copyout.hip: one pinned staging buffer


def _pieces(n, bytes_=STAGING_BYTES):
    """gkm_copyout.hip cut_pieces: a piece [q0, q1) travels as a rectangle of q1 columns and grows while it fits"""
    out, q0 = [], 0
    while q0 < n:
        q1 = q0 + 1
        while q1 < n and (q1 + 1) * (q1 + 1 - q0) * 8 <= bytes_:
            q1 += 1
        out.append((q0, q1))
        q0 = q1
    return out


@pytest.mark.parametrize("n,pieces", [(300, 1), (4800, 3)])
def test_copy_lower_to_rows(dev, n, pieces):
    """gkmhip_copy_lower_to_rows from a padded device matrix (ld = n + 3) into host rows of n + 2 doubles.  n = 4 800: the
    64-MiB staging rule cuts the rows at 2 896 and 4 686, so the third piece reuses the first piece's staging buffer
    while the second is in flight, and its 114 rows are scattered by the host threads (64 rows or more)."""
    import time
    import torch
    cut = _pieces(n)
    assert len(cut) == pieces and (pieces == 1 or cut[-1][1] - cut[-1][0] >= 64), cut
    ld = n + 3
    g = torch.Generator(device="cuda").manual_seed(n)
    K = torch.full((n, ld), float("nan"), dtype=torch.float64, device="cuda")
    K[:, :n] = torch.randn((n, n), generator=g, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    want = A.bits(K[:, :n])
    lower = np.tri(n, n + 2, dtype=bool)
    ctx = dev.GramContext(4, 11, 7, 3)
    try:
        for nthreads in (1, 3, 16):
            host = np.full((n, n + 2), np.nan)
            t0 = time.perf_counter()
            ctx.copy_lower_to_rows(K.data_ptr(), ld, n, host, nthreads)
            print("copy_lower_to_rows n = %d, %d threads: %.0f ms" % (n, nthreads, 1e3 * (time.perf_counter() - t0)))
            hb = A.bits(host)
            assert (hb[:, :n][lower[:, :n]] == want[lower[:, :n]]).all(), nthreads
            assert np.isnan(host[~lower]).all(), nthreads
        assert not np.isnan(host[lower]).any()
    finally:
        ctx.close()


def test_gram_to_host_rows_with_padded_scratch(dev):
    """gkmhip_gram_to_host_rows and both parts of a two-part gkmhip_gram_part_to_host_rows, device scratch of n + 3
    doubles per row, into host rows of n + 2 doubles: the lower triangle of gram_matrix, nothing above it."""
    seqs = A.ragged_301()
    n = len(seqs)
    assert n == 301
    want = A.bits(dev.gram_matrix(seqs, 4, 11, 7, 3)["K"])
    lower = np.tri(n + 1, n + 2, dtype=bool)
    lower[n:] = False                                       # (a guard row below the matrix)
    ctx = dev.GramContext(4, 11, 7, 3)
    try:
        ctx.set_sequences(seqs, _stream())
        ld = n + 3
        for parts in (1, 2):
            host = np.full((n + 1, n + 2), np.nan)
            G = A.sentinel_f64((n, ld))
            for part in range(parts):
                ctx.gram_to_host_rows(G.data_ptr(), ld, host, 3, part, parts)
                if part + 1 < parts:
                    assert np.isnan(host[lower]).any() and not np.isnan(host[lower]).all()   # each part has rows of its own
            assert (A.bits(host)[:n, :n][lower[:n, :n]] == want[lower[:n, :n]]).all(), parts
            assert np.isnan(host[~lower]).all(), parts
            pad = np.zeros((n, ld), dtype=bool)
            pad[:, n:] = True
            assert A.untouched(G, pad), parts
    finally:
        ctx.close()


# ------------------------------------------------------------------ 7. refusals
def _refused(dev, call):
    with pytest.raises(dev.GkmError) as e:
        call()
    assert "(2)" in str(e.value), str(e.value)


def test_too_small_leading_dimensions_are_refused_and_nothing_is_written(dev):
    import torch
    launch = A.by_name("packed")
    ctx, seqs = _context(dev, launch, 4)
    try:
        n, d = len(seqs), launch.d
        rows = A.subset_with_a_jump(n)
        last = int(rows[-1])
        G, P = A.sentinel_f64((n + 1, n + 3)), A.sentinel_i32((n + 1, n + 5, d + 1))
        sq = torch.ones(n, dtype=torch.float64, device="cuda")
        slot = torch.arange(n, dtype=torch.int64, device="cuda")
        host = np.full((n, n), np.nan)
        s = _stream()
        for local in (False, True):
            for ldp in (0, 1, last):      # P[(r ldp + j)(d + 1) + m] with ldp <= the last row: rows over each other
                _refused(dev, lambda: ctx.gram_rows(rows, G.data_ptr(), n + 3, P.data_ptr(), ldp, local, s))
            _refused(dev, lambda: ctx.gram_rows(rows, G.data_ptr(), last, P.data_ptr(), n + 5, local, s))
            _refused(dev, lambda: ctx.gram_rows_full(rows, G.data_ptr(), n - 1, local, s))
        ctx.gram_rows(rows, G.data_ptr(), last + 1, None, 0, True, s)      # (no profiles asked for: ldp is not looked at)
        torch.cuda.synchronize()
        A.refill(G)
        _refused(dev, lambda: ctx.normalize_block(rows, 3, n, G.data_ptr(), n - 4, sq.data_ptr(), s))
        _refused(dev, lambda: ctx.assemble_normalize(G.data_ptr(), n, slot.data_ptr(), G.data_ptr(), n - 1, sq.data_ptr(),
                                                     False, s))
        _refused(dev, lambda: ctx.assemble_normalize(G.data_ptr(), n - 1, slot.data_ptr(), G.data_ptr(), n, sq.data_ptr(),
                                                     False, s))
        _refused(dev, lambda: ctx.copy_lower_to_rows(G.data_ptr(), n - 1, n, host, 2))
        _refused(dev, lambda: ctx.gram_to_host_rows(G.data_ptr(), n - 1, host, 2))
        out = [A.sentinel_f64((n, n - 1)) for _ in range(2)]
        _refused(dev, lambda: dev.gram_matrix_multi(seqs, 4, launch.L, launch.L - launch.d, launch.d, devices=[0, 0],
                                                    ld=n - 1, out=out))
        torch.cuda.synchronize()
        everything = lambda t: np.ones(tuple(t.shape), dtype=bool)      # noqa: E731
        for t in [G, P] + out:
            assert A.untouched(t, everything(t))
        assert np.isnan(host).all() and bool((sq == 1.0).all())
    finally:
        ctx.close()
