"""Time motif scoring (gkmqc_amd/gkmmotifs.py, gkm_contract.hip) in one process on one GPU:

    L = 10   a random symmetric table, 1 000 seeded motifs of widths 6..20, as a single table and as panels of 8 and 64
    L = 12   one table, the same motifs

against, in the same run,

    (a) the numpy restatement of the definition on the host, on a SAMPLE of windows, extrapolated to all of them
    (b) what a user could write with torch on the same GPU: the chain of batched products over the window axis
        (T <- sum_b T[..., b] P[:, i, b], level by level), on a SAMPLE of windows, extrapolated; it rounds in the same order
        and its values are checked against motif_scores' bit for bit
    (c) for panels, the loop over motif_scores per member, in full

    python tools/motif_throughput.py [--motifs 1000 --models 8,64 --repeats 3 --sample 8 --skip-l12]

One warm-up of every side, then `--repeats` rounds, each round every side once (interleaved).  Reported per side: the median
wall time (a host clock around calls that end with their results on the host) with its spread (max - min over the rounds),
and for the device paths the kernels' milliseconds of the last round (HIP events, summed over the blocks).  The lines say
plainly where (b) or (c) is not beaten beyond the spreads."""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def rc_codes(L):
    u = np.arange(4 ** L, dtype=np.int64)
    r = np.zeros_like(u)
    for i in range(L):
        r = (r << 2) | (3 - ((u >> (2 * i)) & 3))
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--motifs", type=int, default=1000)
    ap.add_argument("--models", default="8,64")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--sample", type=int, default=8, help="windows the host restatement and the torch chain are timed on")
    ap.add_argument("--skip-l12", action="store_true")
    a = ap.parse_args()
    import torch
    from gkmqc_amd import gkmmotifs as gm
    from gkmqc_amd import gkmtables as gt
    sizes = [int(s) for s in a.models.split(",")]
    rng = np.random.default_rng(7)
    motifs = [("m%d" % i, rng.dirichlet(np.ones(4) * 0.5, size=int(rng.integers(6, 21)))) for i in range(a.motifs)]
    print("motif_throughput: %d motifs of widths 6..20; %d timed rounds after one warm-up; host and torch baselines on %d "
          "windows, extrapolated; %s" % (a.motifs, a.repeats, a.sample, torch.cuda.get_device_name(0)))

    def table(L, seed):
        w = np.random.default_rng(100 * L + seed).standard_normal(4 ** L)
        return gt.LmerTable(w[np.minimum(np.arange(4 ** L), rc_codes(L))], 2, L, L - 1, 1, 50, 50.0, 0.0)

    def torch_chain(W, P):
        """W: device (4^L,) or (4^L, nm); P: device (n, L, 4) -> (n,) or (n, nm), the definition's order"""
        T = W.reshape((1,) + tuple(W.shape)).expand((len(P),) + tuple(W.shape))
        tail = tuple(W.shape[1:])
        for i in range(P.shape[1] - 1, -1, -1):
            T = T.reshape((len(P), -1, 4) + tail)
            p = P[:, i].reshape((len(P), 1, 4) + (1,) * len(tail))
            T = ((T[:, :, 0] * p[:, :, 0] + T[:, :, 1] * p[:, :, 1]) + T[:, :, 2] * p[:, :, 2]) + T[:, :, 3] * p[:, :, 3]
        return T.reshape((len(P),) + tail)

    def measure(sides):
        """sides: [(name, fn)], fn() -> kernel ms or None; one warm-up each, then interleaved rounds -> {name: (median,
        spread, kernel ms of the last round)}"""
        for _, fn in sides:
            fn()
        walls, kms = {n: [] for n, _ in sides}, {}
        for _ in range(a.repeats):
            for name, fn in sides:
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                kms[name] = fn()
                torch.cuda.synchronize()
                walls[name].append(time.perf_counter() - t0)
        return {n: (float(np.median(w)), max(w) - min(w), kms[n]) for n, w in walls.items()}

    def verdict(ours, other, what):
        (m0, s0, _), (m1, s1, _) = ours, other
        if m1 - s1 > m0 + s0:
            return "%s / device %.1f, device cheaper" % (what, m1 / m0)
        if m0 - s0 > m1 + s1:
            return "%s / device %.2f, %s cheaper: NOT BEATEN HERE" % (what, m1 / m0, what)
        return "%s / device %.2f, inside the run-to-run spread: NOT BEATEN BEYOND THE SPREADS" % (what, m1 / m0)

    def workload(L, nm):
        tables = [table(L, s) for s in range(max(nm, 1))]
        folded = gt.LmerPanel(tables) if nm else tables[0]
        names, mats, bg = (gm.check_panel_motif_scores if nm else gm.check_motif_scores)(folded, motifs)
        wins = np.concatenate([gm.motif_windows(M, L, bg) for M in mats])
        nwin = len(wins) + 1
        sample = np.ascontiguousarray(wins[:: max(1, len(wins) // a.sample)][:a.sample])
        got = {}

        def device_side():
            ms = []
            got["r"] = (gm.motif_scores_with_panel if nm else gm.motif_scores)(
                folded, motifs, profiles=True, on_block=lambda info: ms.append(info["kernel_ms"]))
            return sum(ms)

        def host_side():
            got["host"] = np.array([[gm.contract_reference(t.W, P) for t in tables[:1]] for P in sample])
            return None

        d_W = torch.from_numpy(folded.W).cuda()
        d_P = torch.from_numpy(sample).cuda()

        def torch_side():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            step = max(1, (1 << 28) // (4 ** L * max(nm, 1)))                # at most 2 GiB per product
            got["torch"] = torch.cat([torch_chain(d_W, d_P[i:i + step]) for i in range(0, len(d_P), step)]).cpu().numpy()
            e1.record()
            torch.cuda.synchronize()
            return e0.elapsed_time(e1)

        def loop_side():
            ms = []
            got["loop0"] = None
            for t in tables:
                r = gm.motif_scores(t, motifs, on_block=lambda info: ms.append(info["kernel_ms"]))
                if got["loop0"] is None:
                    got["loop0"] = r
            return sum(ms)

        sides = [("device", device_side), ("host", host_side), ("torch", torch_side)] + ([("loop", loop_side)] if nm else [])
        res = measure(sides)
        scale = nwin / len(sample)
        flat = np.concatenate(got["r"]["profiles"])[:: max(1, len(wins) // a.sample)][:a.sample]
        same_torch = np.ascontiguousarray(flat).tobytes() == np.ascontiguousarray(got["torch"]).tobytes()
        same_host = np.ascontiguousarray(flat.reshape(len(sample), -1)[:, 0]).tobytes() == got["host"][:, 0].tobytes()
        dev, host, tch = res["device"], res["host"], res["torch"]
        host_x = tuple(v * scale * max(nm, 1) for v in host[:2])
        tch_x = tuple(v * scale for v in tch[:2])
        line = ("L=%2d n_models %2d, %d windows: device %8.4f s (spread %.4f; kernels %.2f ms) | (a) host numpy, %d windows "
                "of one table extrapolated: %.1f s (spread %.1f) | (b) torch chain, %d windows extrapolated: %.4f s (spread "
                "%.4f; device ms of the sample %.2f); %s"
                % (L, nm, nwin, dev[0], dev[1], dev[2], len(sample), host_x[0], host_x[1], len(sample), tch_x[0], tch_x[1],
                   tch[2], verdict(dev, tch_x + (None,), "torch")))
        if nm:
            loop = res["loop"]
            same_loop = all(np.ascontiguousarray(got["r"][key][:, 0]).tobytes() == got["loop0"][key].tobytes()
                            for key in ("affinity", "enrichment", "peak", "peak_offset"))
            line += (" | (c) loop of %d: %.4f s (spread %.4f; kernels %.2f ms); %s; column 0 equals table 0: %s"
                     % (nm, loop[0], loop[1], loop[2], verdict(dev, loop, "loop"), same_loop))
        line += "; sample equals torch: %s, host: %s" % (same_torch, same_host)
        print(line, flush=True)

    workload(10, 0)
    for nm in sizes:
        workload(10, nm)
    if not a.skip_l12:
        workload(12, 0)


if __name__ == "__main__":
    main()
