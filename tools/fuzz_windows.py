"""Randomised sweep of the window kernels (gkm_scan.hip, gkm_wsim.hip) over the whole legal
(L, k, d, W, stride) region: per case the l-mer words and the windows' self profiles of the scan, every window pair's
profile and G of k_wsim_profiles -- all exact against the oracle's profile of the windows cut out --, window_kernel byte
for byte against device.cross_kernel on the materialised windows, and window_best against the plain argmax.
    python tools/fuzz_windows.py [--cases 40 | --seconds S] [--seed 1] [--dry]
--cases: a fixed count, so that a run does not depend on the speed of the box (--seconds: until the time is up, for use by
hand).  --dry: the draw alone, without the device: what a seed reaches.

A draw: the kernel type (0..3); L in 2..12, then k in 0..L and d in 0..L - k (a tuple the oracle's parameter check rejects
is never emitted and does not count); W from {L, L + 1, 63 + L, 64 + L, 300, 600, 1035, 2047} or uniform in L..2047; each
stride from {1, 2, n / 8, n - 1, n, n + 1, W + 3}; window counts around the tile's g on each axis; the composition and the
invalid bases of tests/window_cases.py, dense compositions (polyA, y = x) only where n <= 64.  A shape is drawn again until
the reference costs at most window_cases.BUDGET l-mer comparisons.  Every drawn case is checked."""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SCAN_COMPARED = 4                     # self profiles of x held against the oracle's where all of them would pass the budget


def draw(rng):
    """one case, by arithmetic and the oracle's parameter check alone -> dict"""
    from oracle import oracle as O
    from tests import window_cases as WC
    while True:
        t = int(rng.integers(0, 4))
        L = int(rng.integers(2, 13))
        k = int(rng.integers(0, L + 1))
        d = int(rng.integers(0, L - k + 1))
        if O.lib().gkmo_check_params(t, L, k, d) is not None:
            continue
        W = int(rng.choice([L, L + 1, 63 + L, 64 + L, 300, 600, 1035, 2047])) if rng.random() < 0.75 else int(rng.integers(L, 2048))
        n = W - L + 1
        sx, sy = (int(rng.choice([1, 2, max(1, n // 8), max(1, n - 1), n, n + 1, W + 3])) for _ in range(2))
        gx, gy = WC.group(n, sx, WC.WS_GMAX), WC.group(n, sy, WC.WS_GMAX)
        nx, ny = (int(rng.choice([c for c in (1, 2, g - 1, g, g + 1, 2 * g + 1) if c >= 1])) for g in (gx, gy))
        dense = n <= 64 and rng.random() < 0.3
        comp = str(rng.choice(["polyA", "same"])) if dense else str(rng.choice(["iid", "planted"]))
        invalid = int(rng.integers(1, 4)) if rng.random() < 0.25 else 0
        seed = int(rng.integers(0, 2 ** 31))
        sep = int(rng.choice([0, 1, W, 3 * W]))
        if WC.pair_cost(L, W, nx * ny + min(nx, SCAN_COMPARED)) > WC.BUDGET:
            continue
        gs = WC.group(n, sx, WC.SP_GMAX)
        return dict(t=t, L=L, k=k, d=d, W=W, sx=sx, sy=sy, nx=nx, ny=ny, comp=comp, invalid=invalid, seed=seed, sep=sep,
                    lds=WC.wsim_lds_bytes(L, d, W, sx, sy),
                    tile_limited=1 < gx < WC.WS_GMAX or 1 < gy < WC.WS_GMAX, scan_limited=1 < gs < WC.SP_GMAX)


def inputs(case):
    """(x, y) of a case; where the invalid bases leave an axis without a valid window, they are taken out of that record"""
    from tests import scan_ref as SR
    from tests import window_cases as WC
    c = case
    x, y = WC.records(c["seed"], c["comp"], c["L"], c["d"], c["W"], c["sx"], c["sy"], c["nx"], c["ny"], c["invalid"])
    if c["invalid"]:
        cx, cy = WC.records(c["seed"], c["comp"], c["L"], c["d"], c["W"], c["sx"], c["sy"], c["nx"], c["ny"])
        if not any(SR.valid_windows(x, c["W"], c["sx"])):
            x = cx
        if not any(SR.valid_windows(y, c["W"], c["sy"])):
            y = cy
    return x, y


def check(case):
    """every check of one case -> None, or the name of the first that failed"""
    import torch
    from gkmqc_amd import device as dv
    from gkmqc_amd import gkmwindows as gw
    from tests import helpers
    from tests import scan_ref as SR
    from tests import wsim_ref as WR
    c = case
    t, L, k, d, W, sx, sy, nx, ny = (c[key] for key in ("t", "L", "k", "d", "W", "sx", "sy", "nx", "ny"))
    x, y = inputs(c)
    okx, oky = np.array(SR.valid_windows(x, W, sx)), np.array(SR.valid_windows(y, W, sy))
    wx, wy = SR.windows(x, W, sx), SR.windows(y, W, sy)
    if (len(wx), len(wy)) != (nx, ny):
        return "window count"
    n = W - L + 1
    stream = torch.cuda.current_stream().cuda_stream
    ctx = dv.GramContext(t, L, k, d, device=0)
    try:
        words = []
        for rec in (x, y):
            d_x = torch.from_numpy(np.where(rec < 4, rec, 0).astype(np.uint8)).cuda()
            d_v = torch.from_numpy((rec < 4).astype(np.uint8)).cuda()
            nlm = len(rec) - L + 1
            lm = torch.full((nlm + 64,), -1, dtype=torch.int32, device="cuda")
            ctx.scan_lmers(d_x.data_ptr(), d_v.data_ptr(), len(rec), lm.data_ptr(), stream)
            torch.cuda.synchronize()
            host = lm[:nlm].cpu().numpy().view(np.uint32)
            bad = np.array([(rec[p:p + L] >= 4).any() for p in range(nlm)])
            if not ((lm[nlm:] == -1).all() and np.array_equal(host & 0x00FFFFFF, SR.R.pack(np.where(rec < 4, rec, 0), L))
                    and np.array_equal((host >> 31).astype(bool), bad) and not (host & 0x7F000000).any()):
                return "scan words"
            words.append((lm, nlm))
        (lmx, nlmx), (lmy, nlmy) = words
        # the scan's self profiles of the windows of x, all-ones weights (types 0..3)
        wt = torch.from_numpy(dv.position_weights(t, n)).cuda()
        prof = torch.full((nx + 1, d + 1), -7, dtype=torch.int64, device="cuda")
        ctx.scan_profiles(lmx.data_ptr(), nlmx, wt.data_ptr(), W, sx, nx, prof.data_ptr(), stream)
        torch.cuda.synchronize()
        if ctx.last_kernel_name() != "k_scan_profiles" or not (prof[nx] == -7).all():
            return "scan profiles: guard"
        got = prof[:nx].cpu().numpy()
        g = ctx.scan_group(W, sx)
        from tests import window_cases as WC
        if WC.pair_cost(L, W, nx * ny + nx) <= WC.BUDGET:                  # every valid window where the budget allows
            at = [int(i) for i in np.flatnonzero(okx)]
        else:                                                              # else the ends of the first stretch and the last
            at = sorted({i for i in (0, g - 1, g, nx - 1) if 0 <= i < nx and okx[i]})[:SCAN_COMPARED]
        for i in at:
            if not np.array_equal(got[i], SR.self_profile(wx[i][1], t, L, k, d)):
                return "scan profiles: window %d" % i
        # every window pair's profile and G
        G = torch.full((nx + 1, ny + 3), -7.0, dtype=torch.float64, device="cuda")
        P = torch.full((nx + 1, ny, d + 1), -7, dtype=torch.int32, device="cuda")
        ctx.wsim_profiles(lmx.data_ptr(), nlmx, lmy.data_ptr(), nlmy, W, sx, sy, nx, ny, G.data_ptr(), ny + 3, P.data_ptr(), stream)
        torch.cuda.synchronize()
        if ctx.last_kernel_name() != "k_wsim_profiles" or not ((G[nx] == -7.0).all() and (G[:, ny:] == -7.0).all() and (P[nx] == -7).all()):
            return "wsim profiles: guard"
        gotP, gotG = P[:nx].cpu().numpy().astype(np.int64), G[:nx, :ny].cpu().numpy()
        want = np.zeros((nx, ny, d + 1), dtype=np.int64)
        for i in np.flatnonzero(okx):
            for j in np.flatnonzero(oky):
                want[i, j] = WR.pair_profile(wx[i][1], wy[j][1], t, L, k, d)
        live = okx[:, None] & oky[None, :]
        if not np.array_equal(gotP[live], want[live]):
            return "wsim profiles"
        coef = dv.mismatch_weights(t, L, k)[:d + 1]
        if helpers.raw_from_profiles(want, coef)[live].tobytes() != gotG[live].tobytes():
            return "wsim G"
    finally:
        ctx.close()
        WR.forget()
    gamma = 0.7 if t == 3 else 1.0
    r = gw.window_kernel(x, y, W, sx, sy, t, L, k, d, gamma)
    ix, iy = np.flatnonzero(okx), np.flatnonzero(oky)
    seqs = [wx[i][1] for i in ix] + [wy[j][1] for j in iy]
    cross = dv.cross_kernel(seqs, list(range(len(ix))), t, L, k, d, gamma=gamma)["K"][:, len(ix):].cpu().numpy()
    K = r["K"]
    if K.shape != (nx, ny) or not (np.isnan(K[~okx]).all() and np.isnan(K[:, ~oky]).all()):
        return "window_kernel: invalid windows"
    if np.ascontiguousarray(K[np.ix_(ix, iy)]).tobytes() != np.ascontiguousarray(cross).tobytes():
        sub = K[np.ix_(ix, iy)]
        if not (np.array_equal(np.isnan(sub), np.isnan(cross)) and sub[~np.isnan(sub)].tobytes() == cross[~np.isnan(cross)].tobytes()):
            return "window_kernel vs cross_kernel"                          # (a NaN's payload may differ, nothing else)
    best = gw.window_best(x, y, W, sx, sy, t, L, k, d, gamma, min_separation=c["sep"])
    want_j, want_k = WR.best(K, r["x_starts"], r["y_starts"], c["sep"])
    if not (np.array_equal(best["y_start"], want_j) and best["K"].tobytes() == want_k.tobytes()):
        return "window_best"
    return None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", type=int, default=None)
    ap.add_argument("--seconds", type=float, default=None)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--dry", action="store_true")
    a = ap.parse_args()
    if a.cases is None and a.seconds is None:
        a.cases = 40
    from tests import window_cases as WC
    rng = np.random.default_rng(a.seed)
    t_end = None if a.seconds is None else time.time() + a.seconds
    cases = high_d = big_lds = tile_limited = scan_limited = small_l = 0
    while (a.cases is None or cases < a.cases) and (t_end is None or time.time() < t_end):
        case = draw(rng)
        if not a.dry:
            failed = check(case)
            if failed:
                raise SystemExit("WINDOW MISMATCH (%s) seed=%d case=%d %r" % (failed, a.seed, cases, case))
        cases += 1
        high_d += case["d"] >= 9
        big_lds += case["lds"] > WC.LDS_64K
        tile_limited += bool(case["tile_limited"])
        scan_limited += bool(case["scan_limited"])
        small_l += case["L"] <= 3
        if not a.dry and cases % 10 == 0:
            print("%d cases ok" % cases, flush=True)
    print("window fuzz %s: %d cases; %d with d >= 9, %d with more than 64 KiB of LDS, %d with a stretch-limited tile of "
          "k_wsim_profiles, %d with a stretch-limited group of k_scan_profiles, %d with L <= 3"
          % ("draw" if a.dry else "ok", cases, high_d, big_lds, tile_limited, scan_limited, small_l))

if __name__ == "__main__":
    main()
