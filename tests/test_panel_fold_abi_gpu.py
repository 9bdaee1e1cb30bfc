"""k_panel_weights through GramContext.panel_weights (gkm_panel_fold.hip).  The contract: column m of the
image is what gkmhip_lmer_weights writes for (v, CV[:, m]), bit for bit, whatever nm, ms, the range or the split into
pieces.  CV mixes exact zeros, both signs and magnitudes from 1e-8 to 1e8, so any reordering of the additions changes
bits.  The single-table reference of the 64 columns is computed once per class list over all codes and shared; a panel of
nm models holds the first nm columns."""
import re

import numpy as np
import pytest

from tests import lmer_ref as LR
from tests import panel_fold_ref as PR

pytestmark = pytest.mark.gpu

FILL = -7.25          # what an output buffer holds before a launch
GUARD = 3             # rows of FILL in front of and behind the image
NVS = (1, 7, 8, 9, 67)
NMS = (1, 7, 8, 9, 64)
RANGES = ((0, 1024), (3, 260), (1023, 1024))


@pytest.fixture(scope="module")
def dv(built):
    from gkmqc_amd import device
    return device


@pytest.fixture(scope="module")
def stride(built):
    from gkmqc_amd import gkmtables
    return gkmtables.panel_row_stride


def _classes(L, nv, seed, lo=0, hi=None):
    """nv distinct canonical codes drawn from [lo, hi) and their reverse complements, ascending"""
    rng = np.random.default_rng(seed)
    hi = 4 ** L if hi is None else hi
    u = rng.integers(lo, hi, size=8 * nv + 8)
    v = np.unique(np.minimum(u, LR.rc_codes(u, L)))
    return np.sort(rng.permutation(v)[:nv]).astype(np.uint32)


def _coefficients(nv, seed, cols=64):
    """(nv, cols): a fifth exact zeros, the rest of either sign with magnitudes from 1e-8 to 1e8"""
    rng = np.random.default_rng(seed)
    CV = rng.standard_normal((nv, cols)) * 10.0 ** rng.integers(-8, 9, size=(nv, cols))
    CV[rng.random((nv, cols)) < 0.2] = 0.0
    return CV


class _Ctx:
    """one context per (L, d), its class list on the device"""

    def __init__(self, dv, L, d, v):
        import torch
        self.torch, self.L, self.d = torch, L, d
        self.ctx = dv.GramContext(0, L, max(0, L - d), d, device=0)
        self.stream = torch.cuda.current_stream().cuda_stream
        self.v = np.ascontiguousarray(v, dtype=np.uint32)
        self.d_v = torch.from_numpy(self.v.view(np.int32)).cuda()

    def close(self):
        self.ctx.close()

    def single(self, c, cv, u0, u1):
        """gkmhip_lmer_weights for one coefficient column"""
        torch = self.torch
        d_cv = torch.from_numpy(np.ascontiguousarray(cv, dtype=np.float64)).cuda()
        W = torch.full((u1 - u0,), FILL, dtype=torch.float64, device="cuda")
        self.ctx.lmer_weights(c, self.d_v.data_ptr(), d_cv.data_ptr(), len(self.v), u0, u1, W.data_ptr(), self.stream)
        torch.cuda.synchronize()
        return W.cpu().numpy()

    def panel(self, c, CV, nm, ms, u0, u1):
        """gkmhip_panel_weights -> the whole buffer, GUARD rows of FILL around the image"""
        torch = self.torch
        rows = np.zeros((len(self.v), ms))
        rows[:, :nm] = CV[:, :nm]
        rows[:, nm:] = 123.0        # (the coefficient columns beyond nm are never read into a result)
        d_CV = torch.from_numpy(rows).cuda()
        buf = torch.full((u1 - u0 + 2 * GUARD, ms), FILL, dtype=torch.float64, device="cuda")
        self.ctx.panel_weights(c, self.d_v.data_ptr(), d_CV.data_ptr(), len(self.v), nm, ms, u0, u1,
                               buf.data_ptr() + 8 * ms * GUARD, self.stream)
        torch.cuda.synchronize()
        assert self.ctx.last_kernel_name() == "k_panel_weights"
        assert self.ctx.last_comparisons() == 2.0 * len(self.v) * (u1 - u0)
        return buf.cpu().numpy()


def _check_image(buf, want, nm):
    """the guard rows untouched, columns nm.. +0.0, columns < nm the reference's bits"""
    assert (buf[:GUARD] == FILL).all() and (buf[-GUARD:] == FILL).all()
    img = buf[GUARD:-GUARD]
    pad = img[:, nm:]
    assert (pad == 0.0).all() and not np.signbit(pad).any()
    assert img[:, :nm].tobytes() == np.ascontiguousarray(want).tobytes()


C52 = np.array([1.0, 0.3, 0.07])      # d + 1 = 3 coefficients that are no powers of two


@pytest.mark.parametrize("nv", NVS)
def test_every_column_is_the_single_table_bit_for_bit(dv, stride, nv):
    """L = 5, d = 2: nv below, at and above the scalar request of eight classes; nm at every lane split"""
    L, d = 5, 2
    v = _classes(L, nv, 10 + nv)
    CV = _coefficients(len(v), 20 + nv)
    x = _Ctx(dv, L, d, v)
    try:
        ref = np.stack([x.single(C52, CV[:, m], 0, 4 ** L) for m in range(64)], axis=1)
        for nm in NMS:
            for u0, u1 in RANGES:
                _check_image(x.panel(C52, CV, nm, stride(nm), u0, u1), ref[u0:u1, :nm], nm)
        # a row stride wider than panel_row_stride gives
        _check_image(x.panel(C52, CV, 8, 8 + 8, 3, 260), ref[3:260, :8], 8)
        _check_image(x.panel(C52, CV, 9, 16 + 8, 3, 260), ref[3:260, :9], 9)
    finally:
        x.close()


def test_unit_coefficients_and_integer_classes_match_the_restatement_exactly(dv, stride):
    """c a unit vector per mismatch class, integer CV: every sum is exact, so the numpy restatement must agree to the bit"""
    L, d = 5, 2
    v = _classes(L, 67, 3)
    rng = np.random.default_rng(4)
    CV = rng.integers(-7, 8, size=(len(v), 64)).astype(np.float64)
    x = _Ctx(dv, L, d, v)
    try:
        for m in range(d + 1):
            c = np.zeros(d + 1)
            c[m] = 1.0
            for nm in (1, 9, 64):
                want = PR.panel_weights(c, v, CV, nm, L, d, 3, 260)
                _check_image(x.panel(c, CV, nm, stride(nm), 3, 260), want, nm)
    finally:
        x.close()


def test_mixed_magnitudes_match_the_restatement(dv, stride):
    """the restatement rounds each product and each sum as the kernel does: the same bits on the order-sensitive CV too"""
    L, d = 5, 2
    v = _classes(L, 67, 5)
    CV = _coefficients(len(v), 6)
    x = _Ctx(dv, L, d, v)
    try:
        for nm in (7, 64):
            want = PR.panel_weights(C52, v, CV, nm, L, d, 0, 4 ** L)
            _check_image(x.panel(C52, CV, nm, stride(nm), 0, 4 ** L), want, nm)
    finally:
        x.close()


def test_dense_hits_fill_the_list_many_times(dv, stride):
    """L = 5, d = 3 with 300 classes: a random pair of 5-mers is within 3 mismatches with probability 1 - 5 (3/4)^4 / 4 -
    (3/4)^5 = 0.37, so on either strand about 0.6 of all (code, class) pairs hit, and a class inside a wave's own block of
    64 codes (the same first two bases) is hit by all 64 lanes: the hit list fills and is resolved every few classes, runs
    of classes arrive that every lane hits, and the tail classes (300 % 8 = 4) come on a list that is not empty"""
    L, d = 5, 3
    c = np.array([1.0, 0.3, 0.07, 0.011])
    v = _classes(L, 300, 7)
    assert len(v) == 300
    CV = _coefficients(len(v), 8)
    x = _Ctx(dv, L, d, v)
    try:
        hits = np.minimum(LR.mismatches(np.arange(4 ** L), v, L), LR.mismatches(np.arange(4 ** L), LR.rc_codes(v, L), L)) <= d
        assert hits.mean() > 0.5 and hits[:64].all(axis=0).sum() >= 8
        ref = np.stack([x.single(c, CV[:, m], 0, 4 ** L) for m in range(64)], axis=1)
        for nm in (1, 9, 33, 64):
            _check_image(x.panel(c, CV, nm, stride(nm), 0, 4 ** L), ref[:, :nm], nm)
            _check_image(x.panel(c, CV, nm, stride(nm), 3, 260), ref[3:260, :nm], nm)
    finally:
        x.close()


def test_the_top_of_the_code_space(dv, stride):
    """L = 12, d = 4: the last 130 codes below 4^12 with 9 classes drawn from among them"""
    L, d = 12, 4
    top = 4 ** L
    c = np.array([1.0, 0.3, 0.07, 0.011, 0.0013])
    u = np.arange(top - 130, top, dtype=np.int64)
    v = np.unique(np.minimum(u, LR.rc_codes(u, L)))[::15][:9].astype(np.uint32)
    assert len(v) == 9
    CV = _coefficients(len(v), 9)
    x = _Ctx(dv, L, d, v)
    try:
        ref = np.stack([x.single(c, CV[:, m], top - 130, top) for m in range(64)], axis=1)
        assert np.count_nonzero(ref) > 0
        for nm in (1, 9, 64):
            _check_image(x.panel(c, CV, nm, stride(nm), top - 130, top), ref[:, :nm], nm)
    finally:
        x.close()


def test_two_runs_and_two_piece_splits_give_the_same_bytes(dv, stride):
    L, d = 5, 2
    v = _classes(L, 67, 11)
    CV = _coefficients(len(v), 12)
    x = _Ctx(dv, L, d, v)
    try:
        for nm in (9, 64):
            ms = stride(nm)
            whole = x.panel(C52, CV, nm, ms, 0, 1024)
            assert x.panel(C52, CV, nm, ms, 0, 1024).tobytes() == whole.tobytes()
            for cuts in ((0, 64, 100, 1024), (0, 1, 513, 1023, 1024)):
                pieces = [x.panel(C52, CV, nm, ms, a, b)[GUARD:-GUARD] for a, b in zip(cuts[:-1], cuts[1:])]
                assert np.concatenate(pieces).tobytes() == whole[GUARD:-GUARD].tobytes()
    finally:
        x.close()


def test_no_classes_give_a_zero_image(dv):
    import torch
    ctx = dv.GramContext(0, 5, 3, 2, device=0)
    try:
        buf = torch.full((100 + 2 * GUARD, 8), FILL, dtype=torch.float64, device="cuda")
        ctx.panel_weights(C52, None, None, 0, 3, 8, 5, 105, buf.data_ptr() + 8 * 8 * GUARD,
                          torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        _check_image(buf.cpu().numpy(), np.zeros((100, 3)), 3)
    finally:
        ctx.close()


def test_every_refusal_writes_nothing(dv):
    import torch
    L, d = 5, 2
    ctx = dv.GramContext(0, L, 3, d, device=0)
    try:
        stream = torch.cuda.current_stream().cuda_stream
        v = torch.from_numpy(_classes(L, 9, 1).view(np.int32)).cuda()
        CV = torch.ones((9, 16), dtype=torch.float64, device="cuda")
        P = torch.full((1024, 16), FILL, dtype=torch.float64, device="cuda")
        good = dict(c=C52, v=v.data_ptr(), CV=CV.data_ptr(), nv=9, nm=9, ms=16, u0=0, u1=1024, P=P.data_ptr())
        for change, word in ((dict(c=C52[:2]), "d + 1"), (dict(u0=5, u1=5), "code range"), (dict(u1=1025), "code range"),
                             (dict(nv=-1), "negative"), (dict(v=None), "bad arguments"), (dict(CV=None), "bad arguments"),
                             (dict(P=None), "bad arguments"), (dict(nm=0), "1..64 models"), (dict(nm=65, ms=72), "1..64 models"),
                             (dict(ms=8), "row stride"), (dict(ms=12), "row stride")):
            a = dict(good, **change)
            with pytest.raises(dv.GkmError, match=re.escape(word)):
                ctx.panel_weights(a["c"], a["v"], a["CV"], a["nv"], a["nm"], a["ms"], a["u0"], a["u1"], a["P"], stream)
            torch.cuda.synchronize()
            assert (P == FILL).all().item(), change
        ctx.panel_weights(*(good[key] for key in ("c", "v", "CV", "nv", "nm", "ms", "u0", "u1", "P")), stream)
        torch.cuda.synchronize()
        assert not (P == FILL).any().item()
    finally:
        ctx.close()
