"""Time the panel functions (gkmqc_amd/gkmtables.py, gkmscan.py, gkmdelta.py) against the loop
over the single-table function on the same tables, at gkmQC's shape -- L=10 k=6 d=3, kernel type 4 -- in one process on one GPU:

    scan     a seeded locus of 1 Mb at W = 600, strides 1 and 10      scan_with_panel            vs  n x scan
    score    100 000 seeded queries of 600 bp                         score_with_panel           vs  n x score_with_table
    delta    1 000 000 random SNVs over the locus                     delta_with_panel           vs  n x delta

    python tools/panel_throughput.py [--models 1,8,20,64 --only scan,score,delta --repeats 3 --bases 1000000
                                      --queries 100000 --snvs 1000000 --json out.json]

The tables are seeded random ones with W[u] = W[rc(u)]: no path's cost depends on the weights.  Per workload and n_models:
one warm-up of the panel call and of one single-table call, then `--repeats` timed rounds, each round the panel call and
then the whole loop (alternating the two sides).  Reported per side: the median wall time (a host clock around calls that
end with their results on the host) with its spread (max - min over the rounds) and the kernels' milliseconds of the
last round (HIP events, summed over the chunks or blocks; scan_with_panel reports the profile kernel and the score
kernel apart, `scan` the profile kernel only).  The
claim under test is "a panel of n costs less than n single calls": the ratio loop / panel is printed with both spreads,
and a line says plainly where it fails.  Every round also checks column 0 of the panel against the first table's result,
bit for bit."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--models", default="1,8,20,64")
    ap.add_argument("--only", default="scan,score,delta")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--bases", type=int, default=1000000)
    ap.add_argument("--width", type=int, default=600)
    ap.add_argument("--strides", default="1,10")
    ap.add_argument("--queries", type=int, default=100000)
    ap.add_argument("--snvs", type=int, default=1000000)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    import torch
    from gkmqc_amd import device as dv
    from gkmqc_amd import gkmpredict as gp
    L, k, d = 10, 6, 3
    sizes = [int(s) for s in a.models.split(",")]
    only = a.only.split(",")
    rc = gp.lmer_rc(np.arange(4 ** L, dtype=np.uint32), L)
    tables = []
    for m in range(max(sizes)):
        w = np.random.default_rng(100 + m).standard_normal(4 ** L)
        tables.append(gp.LmerTable(w + w[rc], 4, L, k, d, 50, 50.0, 0.01 * m))
    rng = np.random.default_rng(21)
    locus = rng.integers(0, 4, size=a.bases, dtype=np.uint8)
    qcodes = rng.integers(0, 4, size=a.queries * 600, dtype=np.uint8)
    queries = dv.FlatSequences(qcodes, np.arange(a.queries + 1, dtype=np.int64) * 600)
    pos = rng.integers(0, a.bases, size=a.snvs)
    alt = (locus[pos] + rng.integers(1, 4, size=a.snvs)) % 4
    text = gp.codes_to_text(locus)
    variants = [(0, p, text[p], "ACGT"[b]) for p, b in zip(pos.tolist(), alt.tolist())]

    def kernel_ms(events, keys):
        return {key: float(sum(e[key] for e in events)) for key in keys}

    def workload(name):
        """-> (panel call, single call, the kernel-time keys of their measurement dicts); a call -> (result, events)"""
        if name.startswith("scan"):
            stride = int(name[5:])

            def panel_call(panel):
                ev = []
                return gp.scan_with_panel(panel, [locus], a.width, stride, on_chunk=ev.append)[0][2], ev

            def single_call(table):
                ev = []
                return gp.scan(table, [locus], a.width, stride, on_chunk=ev.append)[0][2], ev
            return panel_call, single_call, ("profile_kernel_ms",), ("profile_kernel_ms", "score_kernel_ms")
        if name == "score":
            def panel_call(panel):
                ev = []
                return gp.score_with_panel(panel, queries, on_block=ev.append)[1], ev

            def single_call(table):
                ev = []
                return gp.score_with_table(table, queries, on_block=ev.append)[1], ev
            return panel_call, single_call, ("score_kernel_ms",), ("score_kernel_ms",)

        def panel_call(panel):
            ev = []
            return gp.delta_with_panel(panel, [locus], variants, on_chunk=ev.append), ev

        def single_call(table):
            ev = []
            return gp.delta(table, [locus], variants, on_chunk=ev.append), ev
        return panel_call, single_call, ("kernel_ms",), ("kernel_ms",)

    names = []
    for w in only:
        names += ["scan/%s" % s for s in a.strides.split(",")] if w == "scan" else [w]
    out = dict(L=L, k=k, d=d, kernel_type=4, bases=a.bases, width=a.width, queries=a.queries, snvs=a.snvs,
               repeats=a.repeats, device=torch.cuda.get_device_name(0), rows=[])
    print("panel_throughput: L=%d k=%d d=%d type 4; locus %d bases, W=%d; %d queries of 600 bp; %d SNVs; %d timed rounds "
          "after one warm-up; %s" % (L, k, d, a.bases, a.width, a.queries, a.snvs, a.repeats, out["device"]), flush=True)
    for name in names:
        panel_call, single_call, single_keys, panel_keys = workload(name)
        for n in sizes:
            panel = gp.LmerPanel(tables[:n])
            panel_call(panel)
            single_call(tables[0])
            torch.cuda.synchronize()
            tp, tl, same = [], [], True
            for _ in range(a.repeats):
                t0 = time.perf_counter()
                got, pev = panel_call(panel)
                tp.append(time.perf_counter() - t0)
                t0 = time.perf_counter()
                lev = []
                for m in range(n):
                    one, ev = single_call(tables[m])
                    lev += ev
                    if m == 0:
                        first = one
                tl.append(time.perf_counter() - t0)
                col = got[..., 0]
                keep = ~np.isnan(first)
                same = same and bool(np.array_equal(np.isnan(col), ~keep) and col[keep].tobytes() == first[keep].tobytes())
            row = dict(workload=name, n_models=n, panel_s=tp, loop_s=tl, panel_median_s=float(np.median(tp)),
                       panel_spread_s=max(tp) - min(tp), loop_median_s=float(np.median(tl)), loop_spread_s=max(tl) - min(tl),
                       panel_kernel_ms=kernel_ms(pev, panel_keys), loop_kernel_ms=kernel_ms(lev, single_keys),
                       panel_launches=len(pev), loop_launches=len(lev), column0_equals_table0=same)
            row["ratio"] = row["loop_median_s"] / row["panel_median_s"]
            # the claim holds when the medians differ by more than both spreads
            gap = row["loop_median_s"] - row["panel_median_s"]
            noise = row["panel_spread_s"] + row["loop_spread_s"]
            row["verdict"] = ("panel cheaper" if gap > noise else "loop cheaper: THE CLAIM FAILS HERE" if -gap > noise
                              else "inside the run-to-run spread")
            out["rows"].append(row)
            print("%-8s n_models %2d: panel %8.4f s (spread %.4f; kernels %s) | loop of %2d %8.4f s (spread %.4f; kernels %s)"
                  " | loop / panel %5.2f, %s; column 0 equals table 0: %s"
                  % (name, n, row["panel_median_s"], row["panel_spread_s"],
                     ", ".join("%s %.2f" % kv for kv in row["panel_kernel_ms"].items()), n, row["loop_median_s"],
                     row["loop_spread_s"], ", ".join("%s %.2f" % kv for kv in row["loop_kernel_ms"].items()),
                     row["ratio"], row["verdict"], same), flush=True)
    print(json.dumps(out))
    if a.json:
        with open(a.json, "w") as f:
            json.dump(out, f, indent=1)
    dv.release_cached_contexts()


if __name__ == "__main__":
    main()
