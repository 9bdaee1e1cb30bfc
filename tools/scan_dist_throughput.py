"""Time scan_quantiles and scan_tail_counts (gkmqc_amd/gkmscan.py) against the route they replace --
`scan`, every window's score copied back, then numpy on the host -- at gkmQC's shape (L=10 k=6 d=3, kernel type 4,
W = 600) in one process on one GPU:

    python tools/scan_dist_throughput.py [--bases 1000000 --width 600 --strides 1,10 --quantile 0.99 --thresholds 100
                                          --repeats 5 --json out.json]

The record is synth.random_bases(21, bases); the table a seeded random one with W[u] = W[rc(u)] (no path's cost depends
on the weights).  Per stride: one warm-up of every side, then `--repeats` rounds, each round the four sides one after
the other (interleaved):
  (a) scan_quantiles(q = --quantile) | `scan` + np.partition at the same rank on the host;
  (b) scan_tail_counts of `--thresholds` thresholds (evenly spaced order statistics of the warm-up's scores) | `scan` +
      np.searchsorted on the sorted scores.
Reported per side: the median wall time with its spread (max - min over the rounds) and the bytes copied back from the
device; (c) for the device sides also, by HIP events summed over the chunks (and passes) of the last round, the dist
kernels next to k_scan_profiles + k_scan_score of the same chunks.  Every round checks each pair of results against each
other exactly.  A line says plainly which side is faster, or that the difference lies inside the spreads."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def _verdict(device_s, host_s, name):
    diff = np.median(host_s) - np.median(device_s)
    noise = (max(device_s) - min(device_s)) + (max(host_s) - min(host_s))
    return "%s faster" % name if diff > noise else "the host route faster" if -diff > noise else "inside the run-to-run spread"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--bases", type=int, default=1000000)
    ap.add_argument("--width", type=int, default=600)
    ap.add_argument("--strides", default="1,10")
    ap.add_argument("--quantile", type=float, default=0.99)
    ap.add_argument("--thresholds", type=int, default=100)
    ap.add_argument("--repeats", type=int, default=5)
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
    out = dict(L=L, k=k, d=d, kernel_type=4, bases=a.bases, width=a.width, quantile=a.quantile, thresholds=a.thresholds,
               repeats=a.repeats, device=torch.cuda.get_device_name(0), rows=[])
    print("scan_dist_throughput: L=%d k=%d d=%d type 4; one record of %d bases, W=%d; the %g quantile and the tail counts "
          "of %d thresholds; %d timed rounds after one warm-up; %s"
          % (L, k, d, a.bases, a.width, a.quantile, a.thresholds, a.repeats, out["device"]), flush=True)
    for stride in [int(s) for s in a.strides.split(",")]:
        scores = gp.scan(table, [record], a.width, stride)[0][2]           # (the warm-up of the host side)
        n = len(scores)
        rank = gp.quantile_ranks(n, [a.quantile])[0]
        thr = np.sort(scores)[np.linspace(0, n - 1, a.thresholds).astype(np.int64)]
        gp.scan_quantiles(table, [record], a.width, stride, q=[a.quantile])
        gp.scan_tail_counts(table, [record], a.width, stride, thr)
        torch.cuda.synchronize()
        tq, thq, tt, tht, same = [], [], [], [], True
        for _ in range(a.repeats):
            passes, chunks = [], []
            t0 = time.perf_counter()
            quant = gp.scan_quantiles(table, [record], a.width, stride, q=[a.quantile], on_pass=passes.append)
            tq.append(time.perf_counter() - t0)
            t0 = time.perf_counter()
            scores = gp.scan(table, [record], a.width, stride)[0][2]
            want_q = np.partition(scores, rank)[rank]
            thq.append(time.perf_counter() - t0)
            t0 = time.perf_counter()
            tail = gp.scan_tail_counts(table, [record], a.width, stride, thr, on_chunk=chunks.append)
            tt.append(time.perf_counter() - t0)
            t0 = time.perf_counter()
            scores = gp.scan(table, [record], a.width, stride)[0][2]
            want_t = n - np.searchsorted(np.sort(scores), thr, side="left")
            tht.append(time.perf_counter() - t0)
            same = (same and quant["values"][0] == want_q and quant["scored"] == n
                    and np.array_equal(tail["counts"], want_t))
        row = dict(stride=stride, windows=n, rank=rank, value=float(quant["values"][0]),
                   passes=[p["kind"] for p in passes], quantiles_s=tq, quantiles_host_s=thq, tail_s=tt, tail_host_s=tht,
                   quantiles_copied_bytes=int(sum(p["copied_bytes"] for p in passes)),
                   tail_copied_bytes=8 * (a.thresholds + 1), host_copied_bytes=int(scores.nbytes),
                   quantiles_dist_kernels_ms=float(sum(p["dist_kernels_ms"] for p in passes)),
                   quantiles_scan_kernels_ms=float(sum(p["scan_kernels_ms"] for p in passes)),
                   tail_dist_kernels_ms=float(sum(c["dist_kernels_ms"] for c in chunks)),
                   tail_scan_kernels_ms=float(sum(c["profile_kernel_ms"] + c["score_kernel_ms"] for c in chunks)),
                   chunks=len(chunks), results_equal=bool(same))
        row["quantiles_verdict"] = _verdict(tq, thq, "scan_quantiles")
        row["tail_verdict"] = _verdict(tt, tht, "scan_tail_counts")
        out["rows"].append(row)
        print("stride %2d: %d windows; results equal: %s" % (stride, n, same), flush=True)
        print("  (a) scan_quantiles   %8.4f s (spread %.4f), %d passes (%s), %d bytes back | scan + np.partition    %8.4f s "
              "(spread %.4f), %d bytes back | %s"
              % (np.median(tq), max(tq) - min(tq), len(passes), " ".join(row["passes"]), row["quantiles_copied_bytes"],
                 np.median(thq), max(thq) - min(thq), row["host_copied_bytes"], row["quantiles_verdict"]), flush=True)
        print("  (b) scan_tail_counts %8.4f s (spread %.4f), %d thresholds, %d bytes back | scan + np.searchsorted %8.4f s "
              "(spread %.4f), %d bytes back | %s"
              % (np.median(tt), max(tt) - min(tt), a.thresholds, row["tail_copied_bytes"], np.median(tht),
                 max(tht) - min(tht), row["host_copied_bytes"], row["tail_verdict"]), flush=True)
        for name, dist_ms, scan_ms in (("scan_quantiles, all passes", row["quantiles_dist_kernels_ms"],
                                        row["quantiles_scan_kernels_ms"]),
                                       ("scan_tail_counts", row["tail_dist_kernels_ms"], row["tail_scan_kernels_ms"])):
            print("  (c) kernels by HIP events, %s: dist %.3f ms | k_scan_profiles + k_scan_score %.3f ms | %s"
                  % (name, dist_ms, scan_ms, "the dist kernels are %.1f%% of the scan kernels they follow"
                     % (100.0 * dist_ms / scan_ms) if dist_ms < scan_ms else
                     "THE DIST KERNELS COST MORE THAN THE SCAN KERNELS THEY FOLLOW"), flush=True)
    print(json.dumps(out))
    if a.json:
        with open(a.json, "w") as f:
            json.dump(out, f, indent=1)
    dv.release_cached_contexts()


if __name__ == "__main__":
    main()
