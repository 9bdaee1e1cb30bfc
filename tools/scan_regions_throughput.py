"""Time scan_regions (gkmqc_amd/gkmscan.py) against the route it replaces -- `scan`, every window's
score copied back, then the reduction on the host -- at gkmQC's shape (L=10 k=6 d=3, kernel type 4, W = 600) in one
process on one GPU:

    python tools/scan_regions_throughput.py [--bases 1000000 --width 600 --strides 1,10 --quantile 0.99 --gap 0
                                             --repeats 3 --json out.json]

The record is synth.random_bases(21, bases); the table a seeded random one with W[u] = W[rc(u)] (no path's cost depends
on the weights).  The threshold is the `--quantile` of that run's own `scan` scores.  The host side is `scan` followed by
host_regions below, a vectorised numpy restatement of the definition (no Python loop over windows).  Per stride: one
warm-up of both sides, then `--repeats` rounds, each round scan_regions and then the host route (alternating the two).
Reported per side: the median wall time with its spread (max - min over the rounds) and the bytes copied back from the
device; for scan_regions also, by HIP events summed over the chunks of the last round, the region kernels next to
k_scan_profiles + k_scan_score of the same chunks.  Every round checks the two results against each other bit for bit.
A line says plainly which side is faster, or that the difference lies inside the spreads."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def host_regions(scores, width, stride, threshold, gap):
    """the definition on `scan`'s scores of one record, vectorised -> scan_regions' dict"""
    at = np.flatnonzero(scores >= threshold)                               # (False for a NaN)
    if not len(at):
        e = np.empty(0, np.int64)
        return dict(start=e, end=e, peak=np.empty(0), summit=e, windows=e)
    begins = np.ones(len(at), dtype=bool)
    begins[1:] = np.diff(at) > gap + 1
    b = np.flatnonzero(begins)
    group = np.cumsum(begins) - 1
    v = scores[at]
    top = np.flatnonzero(v == np.maximum.reduceat(v, b)[group])
    top = top[np.concatenate(([True], group[top][1:] != group[top][:-1]))]
    return dict(start=at[b] * stride, end=at[np.append(b[1:], len(at)) - 1] * stride + width, peak=v[top],
                summit=at[top] * stride, windows=np.diff(np.append(b, len(at))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--bases", type=int, default=1000000)
    ap.add_argument("--width", type=int, default=600)
    ap.add_argument("--strides", default="1,10")
    ap.add_argument("--quantile", type=float, default=0.99)
    ap.add_argument("--gap", type=int, default=0)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    import torch
    from gkmqc_amd import device as dv
    from gkmqc_amd import gkmpredict as gp
    from gkmqc_amd import synth
    L, k, d = 10, 6, 3
    w = np.random.default_rng(100).standard_normal(4 ** L)
    table = gp.LmerTable(w + w[gp.lmer_rc(np.arange(4 ** L, dtype=np.uint32), L)], 4, L, k, d, 50, 50.0, 0.0)
    record = synth.random_bases(21, a.bases)
    out = dict(L=L, k=k, d=d, kernel_type=4, bases=a.bases, width=a.width, quantile=a.quantile, gap=a.gap, repeats=a.repeats,
               device=torch.cuda.get_device_name(0), rows=[])
    print("scan_regions_throughput: L=%d k=%d d=%d type 4; one record of %d bases, W=%d; threshold = the %g quantile of "
          "the run's scan scores, gap %d; %d timed rounds after one warm-up; %s"
          % (L, k, d, a.bases, a.width, a.quantile, a.gap, a.repeats, out["device"]), flush=True)
    for stride in [int(s) for s in a.strides.split(",")]:
        scores = gp.scan(table, [record], a.width, stride)[0][2]           # (the warm-up of the host side)
        thr = float(np.quantile(scores, a.quantile))
        gp.scan_regions(table, [record], a.width, stride, thr, a.gap)
        torch.cuda.synchronize()
        td, th, same = [], [], True
        for _ in range(a.repeats):
            ev = []
            t0 = time.perf_counter()
            got = gp.scan_regions(table, [record], a.width, stride, thr, a.gap, on_chunk=ev.append)[0][1]
            td.append(time.perf_counter() - t0)
            t0 = time.perf_counter()
            scores = gp.scan(table, [record], a.width, stride)[0][2]
            want = host_regions(scores, a.width, stride, thr, a.gap)
            th.append(time.perf_counter() - t0)
            same = same and all(got[key].tobytes() == want[key].tobytes() for key in gp.REGION_FIELDS)
        row = dict(stride=stride, windows=len(scores), threshold=thr, regions=len(got["start"]),
                   device_s=td, host_s=th, device_median_s=float(np.median(td)), device_spread_s=max(td) - min(td),
                   host_median_s=float(np.median(th)), host_spread_s=max(th) - min(th),
                   device_copied_bytes=int(sum(e["copied_bytes"] for e in ev)), host_copied_bytes=int(scores.nbytes),
                   region_kernels_ms=float(sum(e["region_kernels_ms"] for e in ev)),
                   profile_kernel_ms=float(sum(e["profile_kernel_ms"] for e in ev)),
                   score_kernel_ms=float(sum(e["score_kernel_ms"] for e in ev)), chunks=len(ev), results_equal=same)
        diff = row["host_median_s"] - row["device_median_s"]
        noise = row["device_spread_s"] + row["host_spread_s"]
        row["verdict"] = ("scan_regions faster" if diff > noise else "the host route faster" if -diff > noise
                          else "inside the run-to-run spread")
        scan_ms = row["profile_kernel_ms"] + row["score_kernel_ms"]
        row["kernels"] = ("the region kernels cost less than the scan kernels they follow" if row["region_kernels_ms"] < scan_ms
                          else "THE REGION KERNELS COST MORE THAN THE SCAN KERNELS THEY FOLLOW")
        out["rows"].append(row)
        print("stride %2d: %d windows, %d regions | scan_regions %8.4f s (spread %.4f), %d bytes back | scan + host "
              "reduction %8.4f s (spread %.4f), %d bytes back | %s; results equal: %s"
              % (stride, row["windows"], row["regions"], row["device_median_s"], row["device_spread_s"],
                 row["device_copied_bytes"], row["host_median_s"], row["host_spread_s"], row["host_copied_bytes"],
                 row["verdict"], same), flush=True)
        print("           kernels by HIP events over %d chunk(s): regions %.3f ms | k_scan_profiles %.3f ms + k_scan_score "
              "%.3f ms | %s" % (row["chunks"], row["region_kernels_ms"], row["profile_kernel_ms"], row["score_kernel_ms"],
                                row["kernels"]), flush=True)
    print(json.dumps(out))
    if a.json:
        with open(a.json, "w") as f:
            json.dump(out, f, indent=1)
    dv.release_cached_contexts()


if __name__ == "__main__":
    main()
