"""Time `scan` (gkmqc_amd/gkmscan.py) against the materialised path -- score_with_table on the same
windows, each cut out as a query of its own -- at gkmQC's shape: type 4, L=10 k=6 d=3, windows of 600 bases over a seeded
sequence of 1 Mb, at strides 1, 10, 50 and 600, in one run on one GPU.

    python tools/scan_throughput.py [--bases 1000000 --width 600 --strides 1,10,50,600 --repeats 5 --json out.json]

The table is a seeded random one with W[u] = W[rc(u)]: neither path's cost depends on the weights.  Per stride: one
warm-up of each path, then `--repeats` timed runs of each, interleaved; the median wall time with its spread (max - min),
windows/s, the pair comparisons and k_scan_profiles' milliseconds (HIP events, summed over the chunks) of `scan`, and
whether the two results are bit-identical.  Cutting the windows out on the host is timed apart and NOT charged to the
materialised path.  --sample N: time the materialised path on the first N windows only and extrapolate linearly (labelled
so in the output), for a device whose memory refuses the whole set.  Verdict per stride: `scan` is faster when the
materialised median exceeds its median by more than the two spreads together, not slower when it does not exceed the
materialised median by more than that."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--bases", type=int, default=1000000)
    ap.add_argument("--width", type=int, default=600)
    ap.add_argument("--strides", default="1,10,50,600")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--sample", type=int, default=0, help="materialise only the first N windows and extrapolate")
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    import torch
    from gkmqc_amd import device as dv
    from gkmqc_amd import gkmpredict as gp
    L, k, d, W = 10, 6, 3, a.width
    rng = np.random.default_rng(20)
    tw = rng.standard_normal(4 ** L)
    tw = tw + tw[gp.lmer_rc(np.arange(4 ** L, dtype=np.uint32), L)]
    table = gp.LmerTable(tw, 4, L, k, d, 50, 50.0, -0.5)
    x = rng.integers(0, 4, size=a.bases, dtype=np.uint8)
    out = dict(bases=a.bases, width=W, L=L, k=k, d=d, kernel_type=4, repeats=a.repeats, strides=[])
    for s in [int(v) for v in a.strides.split(",")]:
        nw = gp.scan_window_count(a.bases, W, s)
        nm = min(nw, a.sample) if a.sample else nw
        t0 = time.perf_counter()
        idx = (np.arange(nm, dtype=np.int64) * s)[:, None] + np.arange(W, dtype=np.int64)[None, :]
        wins = dv.FlatSequences(x[idx].reshape(-1), np.arange(nm + 1, dtype=np.int64) * W)
        del idx
        cut_s = time.perf_counter() - t0

        def run_scan():
            chunks = []
            t0 = time.perf_counter()
            res = gp.scan(table, [x], W, s, on_chunk=chunks.append)[0][2]
            return time.perf_counter() - t0, res, chunks

        def run_mat():
            t0 = time.perf_counter()
            _, res = gp.score_with_table(table, wins)
            return time.perf_counter() - t0, res

        run_scan()
        run_mat()
        torch.cuda.synchronize()
        ts, tm = [], []
        for _ in range(a.repeats):
            t, got, chunks = run_scan()
            ts.append(t)
            t, want = run_mat()
            tm.append(t * (nw / nm))
        ms, mm = float(np.median(ts)), float(np.median(tm))
        ss, sm = max(ts) - min(ts), max(tm) - min(tm)
        row = dict(stride=s, windows=nw, materialised_windows=nm, extrapolated=bool(nm < nw), cut_windows_s=cut_s,
                   scan_s=ts, scan_median_s=ms, scan_spread_s=ss, materialised_s=tm, materialised_median_s=mm,
                   materialised_spread_s=sm, scan_windows_per_s=nw / ms, materialised_windows_per_s=nw / mm,
                   scan_comparisons=sum(c["comparisons"] for c in chunks),
                   materialised_comparisons=2.0 * (W - L + 1) ** 2 * nw,
                   profile_kernel_ms=sum(c["profile_kernel_ms"] for c in chunks), chunks=len(chunks),
                   bit_identical=bool(np.array_equal(got[:nm], want)),
                   faster=bool(mm - ms > ss + sm), not_slower=bool(ms - mm <= ss + sm))
        out["strides"].append(row)
        print("stride %(stride)d: %(windows)d windows; scan median %(scan_median_s).4f s (spread %(scan_spread_s).4f) = "
              "%(scan_windows_per_s).0f windows/s, %(scan_comparisons).3g comparisons, k_scan_profiles "
              "%(profile_kernel_ms).2f ms in %(chunks)d chunk(s); materialised%(label)s median %(materialised_median_s).4f "
              "s (spread %(materialised_spread_s).4f) = %(materialised_windows_per_s).0f windows/s, "
              "%(materialised_comparisons).3g comparisons (windows cut in %(cut_windows_s).2f s, not charged); "
              "bit-identical %(bit_identical)s; faster %(faster)s, not slower %(not_slower)s"
              % dict(row, label=" (first %d windows, extrapolated)" % nm if nm < nw else ""), flush=True)
        del wins
    print(json.dumps(out))
    if a.json:
        with open(a.json, "w") as f:
            json.dump(out, f, indent=1)
    dv.release_cached_contexts()


if __name__ == "__main__":
    main()
