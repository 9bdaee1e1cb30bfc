"""Time window_align (gkmqc_amd/gkmwindows.py) against window_kernel alone -- the copy of K to the host that
any host-side consumer pays before its own work starts -- at L=11 k=7 d=3, W = 300, in one process on one GPU:

    python tools/walign_throughput.py [--bases 100000 --width 300 --stride 20 --types 0,3 --repeats 9 --json out.json]

The records are synth.random_bases(31, bases) and synth.random_bases(32, bases) with a diverged segment planted, so that
a path exists: a fifth of x from 0.4 bases on, 10 % of its bases substituted and 200 bases deleted from its middle, put
into y from 0.3 bases on.  The offset is the 0.999 quantile of K (taken from the warm-up's window_kernel) and the gap
penalty a quarter of max(K) - offset; the line says what they came to.  Per type: one warm-up of both sides, then
`--repeats` rounds, each round window_align (forward) and then window_kernel (alternating the two).  Reported: the
median wall time of either side with its spread (max - min over the rounds), and by HIP events in the same runs the
medians of k_wsim_profiles, of k_walign_tiles (all its launches, summed over the chunk pairs) and of k_walign_trace, the
launches of the DP, and the bytes that come back against K's.  Every round checks the score and the path against the
first round's.  A line says plainly which side is faster, or that the difference lies inside the spreads."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def records(synth, bases):
    x, y = synth.random_bases(31, bases).copy(), synth.random_bases(32, bases).copy()
    rng = np.random.default_rng(33)
    a, n, b = bases * 2 // 5, bases // 5, bases * 3 // 10
    seg = x[a:a + n].copy()
    hit = rng.random(n) < 0.10
    seg[hit] = (seg[hit] + rng.integers(1, 4, size=int(hit.sum()))) % 4
    seg = np.concatenate((seg[:n // 2 - 100], seg[n // 2 + 100:])).astype(x.dtype)
    y[b:b + len(seg)] = seg
    return x, y


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--bases", type=int, default=100000)
    ap.add_argument("--width", type=int, default=300)
    ap.add_argument("--stride", type=int, default=20)
    ap.add_argument("--types", default="0,3")
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    import torch
    from gkmqc_amd import device as dv
    from gkmqc_amd import gkmwindows as gw
    from gkmqc_amd import synth
    L, k, d, gamma = 11, 7, 3, 1.0
    x, y = records(synth, a.bases)
    tile_r, tile_c = dv.walign_tile()
    out = dict(L=L, k=k, d=d, bases=a.bases, width=a.width, stride=a.stride, repeats=a.repeats, tile=[tile_r, tile_c],
               device=torch.cuda.get_device_name(0), rows=[])
    print("walign_throughput: L=%d k=%d d=%d; two records of %d bases with a planted diverged segment, W=%d, stride %d; "
          "DP tiles of %d x %d; %d timed rounds after one warm-up; %s"
          % (L, k, d, a.bases, a.width, a.stride, tile_r, tile_c, a.repeats, out["device"]), flush=True)
    for t in [int(s) for s in a.types.split(",")]:
        args = (a.width, a.stride, a.stride, t, L, k, d, gamma)
        K = gw.window_kernel(x, y, *args)["K"]
        offset = float(np.nanquantile(K, 0.999))
        gap = (float(np.nanmax(K)) - offset) / 4
        first = gw.window_align(x, y, *args, offset, gap)
        torch.cuda.synchronize()
        ctx = dv.cached_context(t, L, k, d, gamma=gamma, device=0)
        ta, tk, prof_ms, dp_ms, trace_ms, same = [], [], [], [], [], True
        for _ in range(a.repeats):
            ev = []
            t0 = time.perf_counter()
            got = gw.window_align(x, y, *args, offset, gap, on_chunk=ev.append)
            ta.append(time.perf_counter() - t0)
            assert ctx.last_kernel_name() == "k_walign_trace"
            trace_ms.append(ctx.last_kernel_ms())
            prof_ms.append(sum(e["profile_kernel_ms"] for e in ev))
            dp_ms.append(sum(e["align_kernel_ms"] for e in ev))
            t0 = time.perf_counter()
            K = gw.window_kernel(x, y, *args)["K"]
            tk.append(time.perf_counter() - t0)
            same = same and got["score"] == first["score"] and np.array_equal(got["x_index"], first["x_index"]) \
                and np.array_equal(got["y_index"], first["y_index"])
        launches = sum((e["x_windows"] + tile_r - 1) // tile_r + (e["y_windows"] + tile_c - 1) // tile_c - 1 for e in ev)
        back = 8 * len(got["x_index"]) + 24 + 24 * len(ev)      # the path's pairs, the trace's count, a best cell per block
        med = lambda v: float(np.median(v))                      # noqa: E731
        spread = lambda v: float(max(v) - min(v))                # noqa: E731
        row = dict(kernel_type=t, windows=list(K.shape), offset=offset, gap=gap, score=got["score"], pairs=len(got["x_index"]),
                   span_x=[int(got["x_start"][0]), int(got["x_start"][-1])] if len(got["x_start"]) else None,
                   span_y=[int(got["y_start"][0]), int(got["y_start"][-1])] if len(got["y_start"]) else None,
                   window_align_s=ta, window_kernel_s=tk, window_align_median_s=med(ta), window_align_spread_s=spread(ta),
                   window_kernel_median_s=med(tk), window_kernel_spread_s=spread(tk), chunk_pairs=len(ev),
                   wsim_kernel_ms=prof_ms, walign_tiles_ms=dp_ms, walign_trace_ms=trace_ms, dp_launches=launches,
                   bytes_back=back, bytes_K=int(K.nbytes), results_equal=same)
        diff = row["window_kernel_median_s"] - row["window_align_median_s"]
        noise = row["window_align_spread_s"] + row["window_kernel_spread_s"]
        row["verdict"] = ("window_align faster than window_kernel alone" if diff > noise else
                          "window_kernel alone faster" if -diff > noise else "inside the run-to-run spread")
        out["rows"].append(row)
        print("type %d: %d x %d windows, offset %.6g, gap %.6g -> score %.6g, %d pairs, x %s, y %s; the same every round: %s"
              % (t, K.shape[0], K.shape[1], offset, gap, got["score"], row["pairs"], row["span_x"], row["span_y"], same), flush=True)
        print("        wall: window_align %8.4f s (spread %.4f) | window_kernel alone %8.4f s (spread %.4f) | %s"
              % (row["window_align_median_s"], row["window_align_spread_s"], row["window_kernel_median_s"],
                 row["window_kernel_spread_s"], row["verdict"]), flush=True)
        print("        kernels by HIP events, medians (spreads): k_wsim_profiles %.3f ms (%.3f) | k_walign_tiles %.3f ms (%.3f) "
              "in %d launches over %d chunk pair(s) | k_walign_trace %.3f ms (%.3f)"
              % (med(prof_ms), spread(prof_ms), med(dp_ms), spread(dp_ms), launches, len(ev), med(trace_ms), spread(trace_ms)),
              flush=True)
        print("        bytes back: %d against %d of K" % (back, K.nbytes), flush=True)
    print(json.dumps(out))
    if a.json:
        with open(a.json, "w") as f:
            json.dump(out, f, indent=1)
    dv.release_cached_contexts()


if __name__ == "__main__":
    main()
