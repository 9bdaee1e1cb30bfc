"""Time the genome window index (gkmqc_amd/nullseq.py build_index) on one seeded synthetic soft-masked
chromosome -- 250 Mb with repeat runs and N gaps, t = 600 -- in one run on one GPU, stage by stage, and the tests' numpy
formulation (tests/nullidx_ref.py index_vectorised: cumulative sums, a stable argsort, bincount) on the same box for the
same input.

    python tools/nullidx_throughput.py [--bases 250000000 --width 600 --repeats 3 --out profiles/r11_nullidx_throughput.txt]

One warm-up build of 1 Mb, then `--repeats` builds of the chromosome: per stage the median of a host clock around work
that ends in a stream synchronise (upload, allocation, keys + planes, cell counts + scan, sort, download), with its spread
(max - min).  File writing (fa, three .bit, pos.npy, ptr.npz) is timed once into a temporary directory, the numpy
formulation once.  The device's arrays are compared with numpy's byte for byte."""
import argparse
import os
import shutil
import sys
import tempfile
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

STAGES = ("upload", "allocate", "keys", "cells", "sort", "download")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--bases", type=int, default=250000000)
    ap.add_argument("--width", type=int, default=600)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    from gkmqc_amd import device as dv
    from gkmqc_amd import nullseq
    from tests import nullidx_ref as NR
    assert torch.cuda.is_available(), "this measurement needs a GPU"
    T, t = a.bases, a.width
    t0 = time.perf_counter()
    raw = NR.soft_masked(T, seed=11, n_gaps=max(3, T // 10000000), gap=200000)
    gen_s = time.perf_counter() - t0
    say = lambda m: print(m, file=sys.stderr, flush=True)
    say("generated")
    dv.nullidx_build(NR.soft_masked(1000000, seed=1), t)        # warm-up: code objects, the allocator
    runs = []
    for _ in range(a.repeats):
        times = {}
        t0 = time.perf_counter()
        ix = dv.nullidx_build(raw, t, times=times)
        times["total"] = time.perf_counter() - t0
        runs.append(times)
        say("build done: %.2f s" % times["total"])
    tmp = tempfile.mkdtemp(prefix="nullidx_")
    try:
        fa = os.path.join(tmp, "chrS.fa")
        nullseq._write_record(fa, "chrS", raw)
        t0 = time.perf_counter()
        recs = list(nullseq.read_genome_fasta(fa))
        read_s = time.perf_counter() - t0
        assert len(recs) == 1 and recs[0][1].tobytes() == raw.tobytes()
        del recs
        wt = {}
        nullseq.build_index(fa, os.path.join(tmp, "idx"), t, times=wt)
        write_s = wt["write"]
        say("files written")
        size = sum(os.path.getsize(os.path.join(dp, f)) for dp, _, fs in os.walk(os.path.join(tmp, "idx")) for f in fs)
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    t0 = time.perf_counter()
    ref = NR.index_vectorised(raw, t)
    numpy_s = time.perf_counter() - t0
    same = ix["len"] == ref["len"] and all(ix[k].tobytes() == ref[k].tobytes() for k in ("key", "pos", "ptr", "na", "cg", "rp"))

    def med(name):
        v = sorted(r[name] for r in runs)
        return v[len(v) // 2], v[-1] - v[0]

    lines = ["nullidx: one synthetic soft-masked chromosome of %d bases (generated in %.1f s), t = %d, %d of %d windows "
             "indexed in %d cells; %d builds after a warm-up" %
             (T, gen_s, t, ix["len"], max(0, T - t), int((np.diff(np.append(ix["ptr"].ravel(), ix["len"])) > 0).sum()),
              a.repeats)]
    for name in STAGES + ("total",):
        m, s = med(name)
        lines.append("  %-9s median %8.4f s (spread %.4f)%s" %
                     (name, m, s, "   = %.0f Mbases/s" % (T / m / 1e6) if name in ("keys", "cells", "sort", "total") else ""))
    dev_s = med("total")[0]
    lines.append("file writing (fa, 3 bit planes, pos.npy, ptr.npz; %.2f GB): %.2f s; reading the FASTA back: %.2f s" %
                 (size / 1e9, write_s, read_s))
    lines.append("numpy formulation (cumulative sums, stable argsort, bincount, packbits) on this box, once: %.2f s" % numpy_s)
    lines.append("device build without file writing vs numpy: %.1f x; end to end with file writing: %.2f s vs %.2f s = %.1f x" %
                 (numpy_s / dev_s, dev_s + write_s, numpy_s + write_s, (numpy_s + write_s) / (dev_s + write_s)))
    lines.append("device arrays equal numpy's byte for byte: %s" % same)
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text)
    return 0 if same else 1


if __name__ == "__main__":
    sys.exit(main())
