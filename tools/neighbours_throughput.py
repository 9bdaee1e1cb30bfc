"""Time the neighbour reductions (gkmqc_amd/gkmneighbours.py, gkm_knn.hip) in one process on one GPU:

    (a) gkmQC's subset: 5 000 peak-like + 5 000 null sequences of 600 bp against themselves, wgkm L=10 k=6 d=3
    (b) --queries (100 000) more peak-like sequences against those 10 000

each as `nearest` (k_nn = 10) and as `pairs_above` (the threshold: the 99.9th percentile of the kernel values among the
first 512 sequences), against, in the same run, the route that existed before: the SAME Gram blocks (the same block loop,
gram_block + normalize_block) copied to the host and reduced with numpy there -- argpartition and a sort of the k_nn
kept per row, or nonzero.

    python tools/neighbours_throughput.py [--queries 100000 --repeats 3 --skip-b]

One warm-up of every side, then `--repeats` rounds, each round every side once (interleaved).  Reported per side: the
median wall time (a host clock around calls that end with their results on the host) with its spread (max - min over the
rounds), the Gram kernels' and the reduce kernels' milliseconds of the last round (HIP events, summed over the blocks; the
timed runs wait after every kernel, both sides alike), and the bytes that came back to the host.  The lines say plainly
where the host route is not beaten beyond the spreads."""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

PARAMS = dict(kernel_type=4, L=10, k=6, d=3)
K_NN = 10


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--queries", type=int, default=100000)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--skip-b", action="store_true")
    a = ap.parse_args()
    import torch
    from gkmqc_amd import device as dv
    from gkmqc_amd import gkmneighbours as gn
    from gkmqc_amd import synth
    from gkmqc_amd.gkmquery import _as_queries

    def flat(seqs):
        return _as_queries([dv.encode(s) for s in seqs])[0]

    pool = flat(synth.make_peak_sequences(11, 5000, 600, True) + synth.make_peak_sequences(12, 5000, 600, False))
    head = dv.gram_matrix([pool[s] for s in range(512)], 4, 10, 6, 3, symmetric=True)["K"].cpu().numpy()
    threshold = float(np.percentile(head[np.triu_indices(512, 1)], 99.9))
    print("neighbours_throughput: wgkm L=10 k=6 d=3, k_nn %d, threshold %.6f; %d timed rounds after one warm-up; %s"
          % (K_NN, threshold, a.repeats, torch.cuda.get_device_name(0)), flush=True)

    def host_route(rows, cols, self_set, want):
        """The same tiles, each copied to the host whole and reduced there -> (result, gram ms, bytes copied)"""
        tiles = gn._Tiles(rows, cols, 4, 10, 6, 3, 50, 50.0, 1.0, 0, None, timed=True,
                          skip=(lambda r0, r1, c0, c1: c1 <= r0 + 1) if (self_set and want == "pairs") else None)
        nbytes = 0
        if want == "nearest":
            idx = np.full((len(rows), K_NN), -1, dtype=np.int64)
            val = np.full((len(rows), K_NN), -np.inf)
        else:
            parts = []
        for r0, r1, c0, c1 in tiles:
            H = tiles.G[:r1 - r0, :c1 - c0].cpu().numpy()
            nbytes += H.nbytes
            if want == "nearest":
                if self_set:                      # a sequence is not its own neighbour
                    own = np.arange(r0, r1) - c0
                    ok = (own >= 0) & (own < c1 - c0)
                    H[np.nonzero(ok)[0], own[ok]] = -np.inf
                kk = min(K_NN, H.shape[1])
                part = np.argpartition(H, H.shape[1] - kk, axis=1)[:, -kk:]
                cv = np.concatenate((val[r0:r1], np.take_along_axis(H, part, 1)), axis=1)
                ci = np.concatenate((idx[r0:r1], part + c0), axis=1)
                order = np.lexsort((ci, -cv), axis=1)[:, :K_NN]
                val[r0:r1], idx[r0:r1] = np.take_along_axis(cv, order, 1), np.take_along_axis(ci, order, 1)
            else:
                i, j = np.nonzero(H >= threshold)
                if self_set:
                    keep = j + c0 > i + r0
                    i, j = i[keep], j[keep]
                parts.append((i + r0, j + c0, H[i, j]))
        if want == "nearest":
            return (idx, val), tiles.gram_ms, nbytes
        return tuple(np.concatenate([p[n] for p in parts]) for n in range(3)), tiles.gram_ms, nbytes

    def measure(sides):
        for _, fn in sides:
            fn()
        walls, last = {n: [] for n, _ in sides}, {}
        for _ in range(a.repeats):
            for name, fn in sides:
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                last[name] = fn()
                torch.cuda.synchronize()
                walls[name].append(time.perf_counter() - t0)
        return {n: (float(np.median(w)), max(w) - min(w)) + tuple(last[n]) for n, w in walls.items()}

    def verdict(dev, host):
        if host[0] - host[1] > dev[0] + dev[1]:
            return "host / device %.2f, device cheaper" % (host[0] / dev[0])
        if dev[0] - dev[1] > host[0] + host[1]:
            return "host / device %.2f, host cheaper: NOT BEATEN HERE" % (host[0] / dev[0])
        return "host / device %.2f, inside the run-to-run spread: NOT BEATEN BEYOND THE SPREADS" % (host[0] / dev[0])

    def workload(label, rows, cols, self_set):
        got = {}

        def dev_nearest():
            info = {}
            got["dn"] = gn.nearest(rows, None if self_set else cols, K_NN, on_block=info.update, **PARAMS)
            return info["gram_kernel_ms"], info["merge_kernel_ms"], got["dn"][0].nbytes + got["dn"][1].nbytes

        def dev_pairs():
            info = {}
            got["dp"] = gn.pairs_above(rows, threshold, None if self_set else cols, on_block=info.update, **PARAMS)
            return info["gram_kernel_ms"], info["pairs_kernel_ms"], sum(x.nbytes for x in got["dp"])

        def host_nearest():
            got["hn"], gram_ms, nbytes = host_route(rows, cols, self_set, "nearest")
            return gram_ms, 0.0, nbytes

        def host_pairs():
            got["hp"], gram_ms, nbytes = host_route(rows, cols, self_set, "pairs")
            return gram_ms, 0.0, nbytes

        res = measure([("dev_nearest", dev_nearest), ("host_nearest", host_nearest), ("dev_pairs", dev_pairs),
                       ("host_pairs", host_pairs)])
        same_nn = bool(np.array_equal(got["dn"][1], got["hn"][1]) and np.array_equal(got["dn"][0], got["hn"][0]))
        order = np.lexsort((got["hp"][1], got["hp"][0]))
        same_p = all(np.array_equal(g, h[order]) for g, h in zip(got["dp"], got["hp"]))
        cells = len(rows) * len(cols)
        for what, d, h, same in (("nearest k_nn=%d" % K_NN, res["dev_nearest"], res["host_nearest"], same_nn),
                                 ("pairs >= threshold (%d pairs)" % len(got["dp"][0]), res["dev_pairs"], res["host_pairs"],
                                  same_p)):
            print("%s, %d x %d, %s: device %8.3f s (spread %.3f; Gram kernels %.1f ms, reduce kernels %.2f ms; %d bytes "
                  "returned) | host numpy on the same blocks %8.3f s (spread %.3f; Gram kernels %.1f ms; %d bytes returned); "
                  "%s; %.3g cells/s on the device route; results equal: %s"
                  % (label, len(rows), len(cols), what, d[0], d[1], d[2], d[3], d[4], h[0], h[1], h[2], h[4], verdict(d, h),
                     cells / d[0], same), flush=True)

    workload("(a)", pool, pool, True)
    if not a.skip_b:
        workload("(b)", flat(synth.make_peak_sequences(13, a.queries, 600, True)), pool, False)


if __name__ == "__main__":
    main()
