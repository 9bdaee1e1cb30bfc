"""The launches the window tests share: gkmhip_scan_lmers + gkmhip_scan_profiles over every window of a record, and
gkmhip_wsim_profiles over every window pair of two, each with guard bands behind its outputs; the host count of a tiled
axis; device.cross_kernel on the windows cut out.  Test infrastructure."""
import numpy as np

from tests import scan_ref as SR


def words(ctx, x, guard=64):
    """gkmhip_scan_lmers of a code array (values >= 4 invalid) -> (int32 device tensor with a guard band, nlm)"""
    import torch
    x = np.asarray(x, dtype=np.uint8)
    valid = (x < 4).astype(np.uint8)
    d_x = torch.from_numpy(np.where(x < 4, x, 0).astype(np.uint8)).cuda()
    d_v = torch.from_numpy(valid).cuda()
    nlm = len(x) - ctx.L + 1
    lm = torch.full((nlm + guard,), -1, dtype=torch.int32, device="cuda")
    ctx.scan_lmers(d_x.data_ptr(), d_v.data_ptr(), len(x), lm.data_ptr(), torch.cuda.current_stream().cuda_stream)
    return lm, nlm


def wsim_profiles(ctx, x, y, W, sx, sy):
    """gkmhip_wsim_profiles over every window pair -> ((nA, nB, d + 1) int64 profiles, G, comparisons)"""
    import torch
    stream = torch.cuda.current_stream().cuda_stream
    lmx, nlmx = words(ctx, x)
    lmy, nlmy = words(ctx, y)
    nA, nB = len(SR.starts(len(x), W, sx)), len(SR.starts(len(y), W, sy))
    G = torch.full((nA + 1, nB), -7.0, dtype=torch.float64, device="cuda")
    P = torch.full((nA + 1, nB, ctx.d + 1), -7, dtype=torch.int32, device="cuda")
    ctx.wsim_profiles(lmx.data_ptr(), nlmx, lmy.data_ptr(), nlmy, W, sx, sy, nA, nB, G.data_ptr(), nB, P.data_ptr(), stream)
    torch.cuda.synchronize()
    assert ctx.last_kernel_name() == "k_wsim_profiles"
    assert (G[nA] == -7.0).all() and (P[nA] == -7).all() and (lmx[nlmx:] == -1).all() and (lmy[nlmy:] == -1).all()
    return P[:nA].cpu().numpy().astype(np.int64), G[:nA].cpu().numpy(), ctx.last_comparisons()


def record(x, W, s, windows, cap=1500):
    """the first bases of x that hold `windows` windows (fewer where `cap` bases hold fewer)"""
    T = min(cap, W + (windows - 1) * s)
    assert T >= W
    return x[:T]


def tile_count(n, s, g, nw):
    """sum over the tiles of an axis of their l-mer words n + (windows - 1) s"""
    return sum(n + (min(g, nw - w0) - 1) * s for w0 in range(0, nw, g))


def cross(dv, x, y, W, sx, sy, t, L, k, d, gamma):
    """device.cross_kernel on the windows of x and y cut out -> the (nA, nB) block of windows of x against windows of y"""
    wx, wy = [w for _, w in SR.windows(x, W, sx)], [w for _, w in SR.windows(y, W, sy)]
    r = dv.cross_kernel(wx + wy, list(range(len(wx))), t, L, k, d, gamma=gamma)
    return r["K"][:, len(wx):].cpu().numpy()


def scan_profiles(dv, t, L, k, d, x, W, s, valid=None):
    """gkmhip_scan_lmers + gkmhip_scan_profiles over every window of x -> ((windows, d + 1) int64, comparisons)"""
    import torch
    ctx = dv.GramContext(t, L, k, d, device=0)
    try:
        stream = torch.cuda.current_stream().cuda_stream
        valid = np.ones(len(x), dtype=np.uint8) if valid is None else np.asarray(valid, dtype=np.uint8)
        d_x = torch.from_numpy(np.ascontiguousarray(x, dtype=np.uint8)).cuda()
        d_v = torch.from_numpy(valid).cuda()
        nlm = len(x) - L + 1
        lm = torch.full((nlm + 64,), -1, dtype=torch.int32, device="cuda")          # (a guard band: nothing lands there)
        ctx.scan_lmers(d_x.data_ptr(), d_v.data_ptr(), len(x), lm.data_ptr(), stream)
        nwin = len(SR.starts(len(x), W, s))
        wt = torch.from_numpy(dv.position_weights(t, W - L + 1)).cuda()
        prof = torch.full((nwin + 1, d + 1), -7, dtype=torch.int64, device="cuda")
        ctx.scan_profiles(lm.data_ptr(), nlm, wt.data_ptr(), W, s, nwin, prof.data_ptr(), stream)
        torch.cuda.synchronize()
        assert ctx.last_kernel_name() == "k_scan_profiles"
        assert (lm[nlm:] == -1).all() and (prof[nwin] == -7).all()
        return prof[:nwin].cpu().numpy(), ctx.last_comparisons(), lm[:nlm].cpu().numpy().view(np.uint32)
    finally:
        ctx.close()
