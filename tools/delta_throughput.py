"""Time `delta` and `delta_saturation` (gkmqc_amd/gkmdelta.py) at gkmQC's shape table -- L=10 k=6 d=3 --
over a seeded record of 1 Mb: 1 000 000 random SNVs plus 100 000 indels through `delta`, the full saturation map, and
the same variants the way a user could score them before -- score_with_table on the two materialised context strings per
variant (the reference and the alternate allele with L - 1 bases on either side) -- in one run on one GPU.

    python tools/delta_throughput.py [--bases 1000000 --snvs 1000000 --indels 100000 --repeats 5 --json out.json]

The table is a seeded random one with W[u] = W[rc(u)]: no path's cost depends on the weights.  One warm-up of each
path, then `--repeats` timed runs of each, interleaved; per path the median wall time (a host clock around a call that
ends with its results on the host) with its spread (max - min), the kernels' milliseconds (HIP events, summed over the
chunks or blocks) and the gathers made.  `delta`'s wall time includes the host's checks and trimming of the variant list,
which are also timed alone.  The materialised route computes another quantity (two normalised window scores per variant,
whose difference is not the delta): it is timed, not compared; cutting its strings out on the host is timed apart and NOT
charged to it.  --sample N: time the materialised route on the first N variants only and extrapolate linearly (labelled
so in the output)."""
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
    ap.add_argument("--snvs", type=int, default=1000000)
    ap.add_argument("--indels", type=int, default=100000)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--sample", type=int, default=0, help="materialise only the first N variants and extrapolate")
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    import torch
    from gkmqc_amd import device as dv
    from gkmqc_amd import gkmpredict as gp
    from gkmqc_amd.gkmdelta import _resolve_variants
    from gkmqc_amd.gkmscan import _as_scan_records
    L, k, d, T = 10, 6, 3, a.bases
    rng = np.random.default_rng(20)
    tw = rng.standard_normal(4 ** L)
    tw = tw + tw[gp.lmer_rc(np.arange(4 ** L, dtype=np.uint32), L)]
    table = gp.LmerTable(tw, 4, L, k, d, 50, 50.0, -0.5)
    x = rng.integers(0, 4, size=T, dtype=np.uint8)
    text = gp.codes_to_text(x)
    # SNVs and indels (insertions of 1..20 bases, deletions of 1..20) with their whole context inside the record
    pos = rng.integers(L - 1, T - L - 20, size=a.snvs + a.indels).tolist()
    alt_base = ((x[pos[:a.snvs]] + rng.integers(1, 4, size=a.snvs)) % 4).tolist()
    variants = [(0, p, text[p], "ACGT"[b]) for p, b in zip(pos[:a.snvs], alt_base)]
    lens = rng.integers(1, 21, size=a.indels).tolist()
    for i, (p, n) in enumerate(zip(pos[a.snvs:], lens)):
        if i % 2:
            variants.append((0, p, text[p:p + n], ""))
        else:
            variants.append((0, p, "", gp.codes_to_text(rng.integers(0, 4, size=n))))
    nv = len(variants)
    t0 = time.perf_counter()
    _, vpos, vrlen, valts = _resolve_variants(_as_scan_records([x]), variants)
    resolve_s = time.perf_counter() - t0
    # the materialised route's strings: x[a:e] and x[a:pos] + alt + x[pos + r:e] per variant
    nm = min(nv, a.sample) if a.sample else nv
    t0 = time.perf_counter()
    strings = []
    for p, r, alt in zip(vpos[:nm].tolist(), vrlen[:nm].tolist(), valts[:nm]):
        lo, hi = p - (L - 1), p + r + (L - 1)
        strings.append(x[lo:hi])
        strings.append(np.concatenate((x[lo:p], np.frombuffer(alt, dtype=np.uint8), x[p + r:hi])))
    off = np.zeros(len(strings) + 1, dtype=np.int64)
    np.cumsum([len(s) for s in strings], out=off[1:])
    wins = dv.FlatSequences(np.concatenate(strings), off)
    del strings
    cut_s = time.perf_counter() - t0

    def run_delta():
        chunks = []
        t0 = time.perf_counter()
        res = gp.delta(table, [x], variants, on_chunk=chunks.append)
        return time.perf_counter() - t0, res, chunks

    def run_sat():
        chunks = []
        t0 = time.perf_counter()
        res = gp.delta_saturation(table, [x], on_chunk=chunks.append)[0][1]
        return time.perf_counter() - t0, res, chunks

    def run_mat():
        blocks = []
        t0 = time.perf_counter()
        _, res = gp.score_with_table(table, wins, on_block=blocks.append)
        return time.perf_counter() - t0, res, blocks

    run_delta()
    run_sat()
    run_mat()
    torch.cuda.synchronize()
    td, ts, tm = [], [], []
    for _ in range(a.repeats):
        t, got, dchunks = run_delta()
        td.append(t)
        t, sat, schunks = run_sat()
        ts.append(t)
        t, _, blocks = run_mat()
        tm.append(t * (nv / nm))
    snv_rows = np.array(pos[:a.snvs]), np.array(alt_base)
    out = dict(bases=T, L=L, k=k, d=d, snvs=a.snvs, indels=a.indels, repeats=a.repeats,
               resolve_variants_s=resolve_s, cut_strings_s=cut_s, materialised_variants=nm, extrapolated=bool(nm < nv),
               delta_s=td, delta_median_s=float(np.median(td)), delta_spread_s=max(td) - min(td),
               delta_kernel_ms=sum(c["kernel_ms"] for c in dchunks), delta_gathers=sum(c["gathers"] for c in dchunks),
               delta_chunks=len(dchunks), delta_variants_per_s=nv / float(np.median(td)),
               saturation_s=ts, saturation_median_s=float(np.median(ts)), saturation_spread_s=max(ts) - min(ts),
               saturation_kernel_ms=sum(c["kernel_ms"] for c in schunks),
               saturation_gathers=sum(c["gathers"] for c in schunks), saturation_chunks=len(schunks),
               saturation_positions_per_s=T / float(np.median(ts)),
               materialised_s=tm, materialised_median_s=float(np.median(tm)), materialised_spread_s=max(tm) - min(tm),
               materialised_score_kernel_ms=sum(b["score_kernel_ms"] for b in blocks) * (nv / nm),
               materialised_gathers=sum(b["lmers"] for b in blocks) * (nv / nm), materialised_blocks=len(blocks),
               materialised_variants_per_s=nv / float(np.median(tm)),
               snvs_equal_saturation_entries=bool(got[:a.snvs].tobytes() == sat[snv_rows].tobytes()),
               all_finite=bool(np.isfinite(got).all() and np.isfinite(sat).all()))
    print("delta: %(snvs)d SNVs + %(indels)d indels over %(bases)d bases; median %(delta_median_s).4f s (spread "
          "%(delta_spread_s).4f) = %(delta_variants_per_s).0f variants/s, of which the host's checks and trimming take "
          "%(resolve_variants_s).2f s; k_delta_variants %(delta_kernel_ms).3f ms for %(delta_gathers).3g gathers in "
          "%(delta_chunks)d chunk(s)" % out)
    print("delta_saturation: %(bases)d positions; median %(saturation_median_s).4f s (spread %(saturation_spread_s).4f) = "
          "%(saturation_positions_per_s).0f positions/s; k_delta_sat %(saturation_kernel_ms).3f ms for "
          "%(saturation_gathers).3g gathers in %(saturation_chunks)d chunk(s)" % out)
    print("materialised%(label)s: two context strings per variant through score_with_table; median "
          "%(materialised_median_s).4f s (spread %(materialised_spread_s).4f) = %(materialised_variants_per_s).0f "
          "variants/s; k_lmer_score %(materialised_score_kernel_ms).3f ms for %(materialised_gathers).3g gathers in "
          "%(materialised_blocks)d block(s) (strings cut in %(cut_strings_s).2f s, not charged)"
          % dict(out, label=" (first %d variants, extrapolated)" % nm if nm < nv else ""))
    print("SNVs equal the saturation entries bit for bit: %(snvs_equal_saturation_entries)s; all finite: %(all_finite)s" % out,
          flush=True)
    print(json.dumps(out))
    if a.json:
        with open(a.json, "w") as f:
            json.dump(out, f, indent=1)
    dv.release_cached_contexts()


if __name__ == "__main__":
    main()
