"""Randomised sweep of the column-range launch (gkmhip_gram_block + gkmhip_normalize_block, the scoring path of
gkmqc_amd/gkmquery.py) against the CPU oracle on the GPU box: the parameter draw and length modes of
tools/fuzz_parity.py, then per case a random ascending row subset (with rows inside the range and just either side of
it), a random column range [c0, c1), a padded leading dimension, a sentinel-filled buffer with spare rows, every kernel
(auto, general, bit-sliced where instantiated) and now and then GKM_FORCE_PACKED / GKM_COL_CHUNK (test infrastructure).
Raw values must equal the oracle's sum_m c_m P_m bit for bit, kernel values the oracle's K within fuzz_parity.py's
tolerance (NaNs where the oracle has them), and every cell outside [:nrows, :c1 - c0] must keep its sentinel.
python tools/fuzz_block.py [--seconds 240] [--seed 1]"""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SENTINEL = -3.125e7


def draw_params(rng, device, ALL_LD):
    """fuzz_parity.py's draw -> (t, L, k, d, M, H, gamma), or None for a combination the device layer refuses"""
    t = int(rng.integers(0, 6))
    if rng.random() < 0.75:
        pairs = [(L, d) for L, d in ALL_LD if d <= 4]
        L, d = pairs[int(rng.integers(len(pairs)))]
        k = int(rng.integers(1, L - d + 1))
    else:
        L = int(rng.integers(3, 13))
        k = int(rng.integers(1, L + 1))
        d = int(rng.integers(0, min(4, L - k) + 1))
    if device.check_parameters(t, L, k, d):
        return None
    M, H = int(rng.integers(1, 256)), float(rng.integers(1, 200))
    gamma = float(rng.choice([0.5, 1.0, 2.0]))
    return t, L, k, d, M, H, gamma


def draw_sequences(rng, L):
    """fuzz_parity.py's length modes 0-5 with a duplicate, a poly-A sequence and a reverse complement -> (codes, mode)"""
    n = int(rng.integers(2, 90))
    mode = int(rng.choice([0, 0, 5, 5, 5, 1, 2, 3, 4]))
    if mode == 0:
        lens = np.full(n, int(rng.integers(L, 700)))
    elif mode == 5:
        lens = np.full(n, int(rng.choice([int(rng.integers(170, 321)), int(rng.integers(500, 641)), 300, 600])))
    elif mode == 1:
        lens = rng.integers(L, 700, n)
    elif mode == 2:
        lens = rng.integers(L, L + 12, n)
    elif mode == 3:
        lens = rng.choice([150, 300, 320, 321, 640, 2047], n)
    else:
        lens = rng.integers(L, 2048, n)
    seqs = [rng.integers(0, 4, int(ln)).astype(np.uint8) for ln in lens]
    if n > 4:
        seqs[1] = seqs[0].copy()                                   # duplicate
        seqs[2] = np.zeros(len(seqs[2]), dtype=np.uint8)           # poly-A
        seqs[3] = (3 - seqs[0][::-1]).astype(np.uint8)             # reverse complement
    return seqs, mode


def draw_range(rng, n):
    """0 <= c0 < c1 <= n; width 1, c0 = 0, c1 = n and c0 % 8 != 0 each come up often"""
    shape = int(rng.integers(0, 5))
    if shape == 0:                                   # width 1
        c0 = int(rng.integers(0, n))
        return c0, c0 + 1
    if shape == 1:                                   # from 0
        return 0, int(rng.integers(1, n + 1))
    if shape == 2:                                   # to n
        return int(rng.integers(0, n)), n
    if shape == 3 and n > 9:                         # off an 8-column boundary
        c0 = int(rng.choice([c for c in range(1, n) if c % 8]))
        return c0, int(rng.integers(c0 + 1, n + 1))
    c0 = int(rng.integers(0, n))
    return c0, int(rng.integers(c0 + 1, n + 1))


def draw_rows(rng, n, c0, c1):
    """a strictly ascending row subset; usually with rows inside [c0, c1) and the rows c0 - 1 and c1"""
    rows = set(int(r) for r in rng.choice(n, int(rng.integers(1, n + 1)), replace=False))
    if rng.random() < 0.7:
        rows.update(int(r) for r in rng.integers(c0, c1, 3))
        rows.update(r for r in (c0 - 1, c1) if 0 <= r < n)
    return np.array(sorted(rows), dtype=np.int32)


def run_block(device, torch, seqs, params, kern, rows, c0, c1, ld, spare):
    """-> (raw block, normalised block, kernel name), both [len(rows) + spare, ld] with sentinels around the range"""
    stream = torch.cuda.current_stream().cuda_stream
    ctx = device.GramContext(*params)
    try:
        ctx.set_kernel(kern)
        ctx.set_sequences(seqs, stream)
        G = torch.full((len(rows) + spare, ld), SENTINEL, dtype=torch.float64, device="cuda")
        ctx.gram_block(rows, c0, c1, G.data_ptr(), ld, stream)
        torch.cuda.synchronize()
        raw = G.cpu().numpy()
        sq = torch.zeros(len(seqs), dtype=torch.float64, device="cuda")
        ctx.self_norms(sq.data_ptr(), stream)
        ctx.normalize_block(rows, c0, c1, G.data_ptr(), ld, sq.data_ptr(), stream)
        torch.cuda.synchronize()
        return raw, G.cpu().numpy(), ctx.last_kernel_name()
    finally:
        ctx.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seconds", type=float, default=240)
    ap.add_argument("--seed", type=int, default=1)
    a = ap.parse_args()
    import torch
    from gkmqc_amd import device
    from tests import helpers
    rng = np.random.default_rng(a.seed)
    t_end = time.time() + a.seconds
    cases = 0
    kernels, envs = {}, {}
    saved = {v: os.environ.get(v) for v in ("GKM_FORCE_PACKED", "GKM_COL_CHUNK")}
    try:
        while time.time() < t_end:
            params = draw_params(rng, device, helpers.ALL_LD)
            if params is None:
                continue
            t, L, k, d = params[:4]
            seqs, mode = draw_sequences(rng, L)
            n = len(seqs)
            c0, c1 = draw_range(rng, n)
            rows = draw_rows(rng, n, c0, c1)
            ld = (c1 - c0) + int(rng.choice([0, 0, 1, 3, 8, 29]))
            spare = int(rng.integers(0, 3))
            env = {}
            if rng.random() < 0.3:
                env["GKM_FORCE_PACKED"] = str(rng.choice(["1", "128"]))
            if rng.random() < 0.3:
                env["GKM_COL_CHUNK"] = str(rng.choice([8, 40, 64]))
            for v in saved:
                os.environ.pop(v, None)
            os.environ.update(env)
            ref = helpers.oracle_problem(seqs, params)
            G_want = ref["G"][np.ix_(rows, np.arange(c0, c1))]
            K_want = ref["K"][np.ix_(rows, np.arange(c0, c1))]
            kerns = [device.KERNEL_AUTO, device.KERNEL_DIRECT] + ([device.KERNEL_BITSLICE] if (L, d) in helpers.ALL_LD else [])
            what = "t=%d L=%d k=%d d=%d M=%d H=%g gamma=%g n=%d mode=%d rows=%d [%d, %d) ld=%d env=%s seed=%d case=%d" % (
                t, L, k, d, params[4], params[5], params[6], n, mode, len(rows), c0, c1, ld, env, a.seed, cases)
            for kern in kerns:
                raw, K, name = run_block(device, torch, seqs, params, kern, rows, c0, c1, ld, spare)
                w, nr = c1 - c0, len(rows)
                outside = np.ones(raw.shape, dtype=bool)
                outside[:nr, :w] = False
                if not ((raw[outside] == SENTINEL).all() and (K[outside] == SENTINEL).all()):
                    raise SystemExit("WRITE OUTSIDE THE BLOCK %s kernel=%s" % (what, name))
                if raw[:nr, :w].tobytes() != G_want.tobytes():
                    bad = np.argwhere(raw[:nr, :w] != G_want)[:3]
                    raise SystemExit("RAW MISMATCH %s kernel=%s first cells %s" % (what, name, bad.tolist()))
                # (a poly-A row with large weights wraps its int32 self profile -- like the reference -- and its square
                #  root is NaN on both sides: NaNs must coincide, the rest must agree)
                kd, kr = K[:nr, :w], K_want
                fin = np.isfinite(kr)
                same_nan = np.array_equal(np.isnan(kd), np.isnan(kr))
                err = (np.abs(kd[fin] - kr[fin]).max() / max(1e-300, np.abs(kr[fin]).max())) if fin.any() else 0.0
                tol = 1e-9 if t in (3, 5) else 1e-12
                if not (same_nan and err < tol):
                    raise SystemExit("K MISMATCH %g %s kernel=%s" % (err, what, name))
                kernels[name] = kernels.get(name, 0) + 1
            for v in env:
                envs[v] = envs.get(v, 0) + 1
            cases += 1
            if cases % 50 == 0:
                print("%d cases ok %s" % (cases, kernels), flush=True)
    finally:
        for v, val in saved.items():
            if val is None:
                os.environ.pop(v, None)
            else:
                os.environ[v] = val
    print("block fuzz ok: %d cases, kernels used: %s, cases with %s" % (cases, kernels, envs))


if __name__ == "__main__":
    main()
