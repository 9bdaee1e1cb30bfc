"""Time window_kernel (gkmqc_amd/gkmwindows.py) against the route it replaces -- every window of both
records cut out and sent through the Gram path -- at L=11 k=7 d=3, W = 300, kernel types 0 and 3, in one process on one
GPU:

    python tools/wsim_throughput.py [--bases 100000 --width 300 --strides 1,20,300 --types 0,3 --corner 2000
                                     --repeats 3 --json out.json]

The records are synth.random_bases(31, bases) and synth.random_bases(32, bases): iid, so hits are as rare as the kernel
ever sees them.  The materialised side is device.cross_kernel's own sequence of calls (set_sequences on the cut-out
windows of x followed by those of y, self_norms, then gram_block and normalize_block with the windows of x as rows and
the windows of y as the column range -- cross_kernel itself would also compute x against x) and a copy of the block to
the host, as window_kernel ends with one.  At a stride below `--corner-below` BOTH sides take only the first `--corner`
windows of either record (the full matrix of two 100 kb records at stride 1 is 80 GB); the line says so.  Per stride and
type: one warm-up of both sides, then `--repeats` rounds, each round window_kernel and then the materialised route
(alternating the two).  Reported per side: the median wall time with its spread (max - min over the rounds) and the hot
kernel's time by HIP events in the last round (k_wsim_profiles summed over the chunk pairs; the Gram kernel of
gram_block).  Every round checks that the two matrices hold the same bytes.  A line says plainly which side is faster,
or that the difference lies inside the spreads."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def materialised(dv, torch, x, y, width, stride, t, L, k, d, gamma):
    """-> (K as a host array, the Gram kernel's ms, its name, its comparisons)"""
    wx = [x[a:a + width] for a in range(0, len(x) - width + 1, stride)]
    wy = [y[a:a + width] for a in range(0, len(y) - width + 1, stride)]
    ctx = dv.GramContext(t, L, k, d, gamma=gamma, device=0)
    try:
        stream = torch.cuda.current_stream().cuda_stream
        ctx.set_sequences(wx + wy, stream)
        rows = np.arange(len(wx), dtype=np.int32)
        G = torch.empty((len(wx), len(wy)), dtype=torch.float64, device="cuda")
        sq = torch.empty(len(wx) + len(wy), dtype=torch.float64, device="cuda")
        ctx.self_norms(sq.data_ptr(), stream)
        ctx.gram_block(rows, len(wx), len(wx) + len(wy), G.data_ptr(), len(wy), stream)
        name, comparisons = ctx.last_kernel_name(), ctx.last_comparisons()
        ctx.normalize_block(rows, len(wx), len(wx) + len(wy), G.data_ptr(), len(wy), sq.data_ptr(), stream)
        K = G.cpu().numpy()
        return K, ctx.last_kernel_ms(), name, comparisons      # (the events of the Gram kernel: the block calls take none)
    finally:
        ctx.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--bases", type=int, default=100000)
    ap.add_argument("--width", type=int, default=300)
    ap.add_argument("--strides", default="1,20,300")
    ap.add_argument("--types", default="0,3")
    ap.add_argument("--corner", type=int, default=2000, help="windows of either record both sides take at a small stride")
    ap.add_argument("--corner-below", type=int, default=20, help="strides below this take the corner only")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    import torch
    from gkmqc_amd import device as dv
    from gkmqc_amd import gkmwindows as gw
    from gkmqc_amd import synth
    L, k, d, gamma = 11, 7, 3, 1.0
    X, Y = synth.random_bases(31, a.bases), synth.random_bases(32, a.bases)
    out = dict(L=L, k=k, d=d, bases=a.bases, width=a.width, repeats=a.repeats, device=torch.cuda.get_device_name(0), rows=[])
    print("wsim_throughput: L=%d k=%d d=%d; two iid records of %d bases, W=%d; %d timed rounds after one warm-up; %s"
          % (L, k, d, a.bases, a.width, a.repeats, out["device"]), flush=True)
    for stride in [int(s) for s in a.strides.split(",")]:
        corner = stride < a.corner_below
        T = a.width + (a.corner - 1) * stride if corner else a.bases
        x, y = X[:T], Y[:T]
        for t in [int(s) for s in a.types.split(",")]:
            args = (a.width, stride, stride, t, L, k, d, gamma)
            gw.window_kernel(x, y, *args)
            materialised(dv, torch, x, y, a.width, stride, t, L, k, d, gamma)
            torch.cuda.synchronize()
            tw, tm, same = [], [], True
            for _ in range(a.repeats):
                ev = []
                t0 = time.perf_counter()
                got = gw.window_kernel(x, y, *args, on_chunk=ev.append)["K"]
                tw.append(time.perf_counter() - t0)
                t0 = time.perf_counter()
                want, gram_ms, gram_name, gram_cmp = materialised(dv, torch, x, y, a.width, stride, t, L, k, d, gamma)
                tm.append(time.perf_counter() - t0)
                same = same and got.tobytes() == want.tobytes()
            row = dict(stride=stride, kernel_type=t, windows=list(got.shape), corner_only=corner,
                       window_kernel_s=tw, materialised_s=tm, window_kernel_median_s=float(np.median(tw)),
                       window_kernel_spread_s=max(tw) - min(tw), materialised_median_s=float(np.median(tm)),
                       materialised_spread_s=max(tm) - min(tm), chunk_pairs=len(ev),
                       wsim_kernel_ms=float(sum(e["profile_kernel_ms"] for e in ev)),
                       wsim_comparisons=float(sum(e["comparisons"] for e in ev)), gram_kernel=gram_name,
                       gram_kernel_ms=float(gram_ms), gram_comparisons=float(gram_cmp), results_equal=same)
            diff = row["materialised_median_s"] - row["window_kernel_median_s"]
            noise = row["window_kernel_spread_s"] + row["materialised_spread_s"]
            row["verdict"] = ("window_kernel faster" if diff > noise else "the materialised route faster" if -diff > noise
                              else "inside the run-to-run spread")
            out["rows"].append(row)
            print("stride %3d type %d: %d x %d windows%s | window_kernel %8.4f s (spread %.4f) | materialised %8.4f s "
                  "(spread %.4f) | %s; results equal: %s"
                  % (stride, t, got.shape[0], got.shape[1], " (the corner only, both sides)" if corner else "",
                     row["window_kernel_median_s"], row["window_kernel_spread_s"], row["materialised_median_s"],
                     row["materialised_spread_s"], row["verdict"], same), flush=True)
            print("                   kernels by HIP events: k_wsim_profiles %.3f ms over %d chunk pair(s), %.4g comparisons "
                  "(%.3g / s) | %s %.3f ms, %.4g comparisons (%.3g / s)"
                  % (row["wsim_kernel_ms"], len(ev), row["wsim_comparisons"],
                     row["wsim_comparisons"] / max(row["wsim_kernel_ms"], 1e-6) * 1e3, gram_name, row["gram_kernel_ms"],
                     row["gram_comparisons"], row["gram_comparisons"] / max(row["gram_kernel_ms"], 1e-6) * 1e3), flush=True)
    print(json.dumps(out))
    if a.json:
        with open(a.json, "w") as f:
            json.dump(out, f, indent=1)
    dv.release_cached_contexts()


if __name__ == "__main__":
    main()
