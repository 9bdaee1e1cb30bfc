"""Null (negative) sequences for a set of peaks: a genome window index built on the GPU, and a sampler that draws
GC- and repeat-matched windows from it (INTEGRATION.md "Null sequences").

The index of one chromosome and a window width t (device.nullidx_build, include/gkm_hip.h gkmhip_nullidx_*): every
window start i in [0, T - t) without an N is filed under the cell (C/G bytes, soft-masked bytes) of its t bytes.  An
index directory holds, per record <chr> of the genome FASTA,

    fa/<chr>.fa                     the record, case kept
    bit/<chr>.{na,cg,rp}.bit        one bit per base (N, C/G, lower-case acgt), first base in the highest bit of a byte
    nidx_t<t>/<chr>_pos.npy         int32: the indexed starts by cell, ascending inside a cell
    nidx_t<t>/<chr>_ptr.npz         ptr (int32 [t + 1, t + 1]: the indexed windows in smaller cells) and len

-- the names and contents of gkmQC's index directory.  `sample` works on the host from these files alone.

    python -m gkmqc_amd.nullseq build-index [--width 600] genome.fa DIR
    python -m gkmqc_amd.nullseq sample [--width --margin-gc --margin-rp --seed] DIR pos.bed neg.bed [--fasta pos.fa neg.fa]
"""
import argparse
import bisect
import logging
import os
import sys

import numpy as np

from . import device as dv

DEFAULT_WIDTH = 600


class NullseqError(ValueError):
    pass


# ------------------------------------------------------------------ reading the genome
def read_genome_fasta(path):
    """Yield (name, letters) per record: name = the header up to the first blank, letters = the record's bytes as uint8
    with line breaks removed and case kept, of any length."""
    with open(path, "rb") as f:
        data = f.read()
    at = 0 if data.startswith(b">") else data.find(b"\n>") + 1
    if not data.startswith(b">") and at == 0:
        return
    while at < len(data):
        eol = data.find(b"\n", at)
        if eol < 0:
            eol = len(data)
        header = data[at + 1:eol].strip().split()
        nxt = data.find(b"\n>", eol)
        end = len(data) if nxt < 0 else nxt
        body = (np.frombuffer(data, dtype=np.uint8, count=end - eol - 1, offset=eol + 1) if end - eol - 1 > 0
                else np.zeros(0, np.uint8))
        yield (header[0].decode("utf-8", "replace") if header else ""), body[(body != 10) & (body != 13)]
        at = end + 1


def _write_record(path, name, raw, cols=60):
    raw = np.ascontiguousarray(raw, dtype=np.uint8)
    full = len(raw) // cols
    with open(path, "wb") as f:
        f.write(b">" + name.encode() + b"\n")
        if full:
            lines = np.full((full, cols + 1), 10, dtype=np.uint8)
            lines[:, :cols] = raw[:full * cols].reshape(full, cols)
            lines.tofile(f)
        if len(raw) > full * cols:
            f.write(raw[full * cols:].tobytes() + b"\n")


# ------------------------------------------------------------------ the index on disk
def build_index(genome_fa, out_dir, width=DEFAULT_WIDTH, device=0, times=None):
    """Index every record of `genome_fa` on the GPU and write the index directory.  Returns [(name, T, len)].
    times: a dict that receives the seconds spent per stage (device.nullidx_build's, plus "write")."""
    import time
    width = int(width)
    dv.nullidx_check(0, width)
    for sub in ("fa", "bit", "nidx_t%d" % width):
        os.makedirs(os.path.join(out_dir, sub), exist_ok=True)
    done, seen = [], set()
    for name, raw in read_genome_fasta(genome_fa):
        if not name or "/" in name or name in seen:
            raise NullseqError("%s: record name %r is empty, repeated or holds a '/'" % (genome_fa, name))
        seen.add(name)
        dv.nullidx_check(len(raw), width)
        ix = dv.nullidx_build(raw, width, device=device, times=times)
        t0 = time.perf_counter()
        _write_record(os.path.join(out_dir, "fa", name + ".fa"), name, raw)
        for pl in ("na", "cg", "rp"):
            ix[pl].tofile(os.path.join(out_dir, "bit", "%s.%s.bit" % (name, pl)))
        np.save(os.path.join(out_dir, "nidx_t%d" % width, name + "_pos.npy"), ix["pos"])
        np.savez_compressed(os.path.join(out_dir, "nidx_t%d" % width, name + "_ptr.npz"), ptr=ix["ptr"], len=ix["len"])
        if times is not None:
            times["write"] = times.get("write", 0.0) + time.perf_counter() - t0
        logging.info("%s: %d bases, %d of %d windows of %d indexed", name, len(raw), ix["len"], max(0, len(raw) - width),
                     width)
        done.append((name, len(raw), ix["len"]))
    if not done:
        raise NullseqError("%s holds no FASTA record" % genome_fa)
    return done


class ChromIndex:
    """One chromosome of an index directory: pos (memory-mapped), ptr, len, and the text read on first use."""

    def __init__(self, out_dir, width, name):
        self.name, self.width = name, width
        sub = os.path.join(out_dir, "nidx_t%d" % width)
        self.pos = np.load(os.path.join(sub, name + "_pos.npy"), mmap_mode="r")
        with np.load(os.path.join(sub, name + "_ptr.npz")) as z:
            self.ptr = np.ascontiguousarray(z["ptr"], dtype=np.int32)
            self.len = int(z["len"])
        if self.ptr.shape != (width + 1, width + 1) or len(self.pos) != self.len:
            raise NullseqError("%s: the index of %s does not fit the width %d" % (out_dir, name, width))
        self._fa = os.path.join(out_dir, "fa", name + ".fa")
        self._text = None
        self._bounds = np.append(self.ptr.ravel().astype(np.int64), self.len)

    @property
    def text(self):
        if self._text is None:
            recs = list(read_genome_fasta(self._fa))
            if len(recs) != 1:
                raise NullseqError("%s must hold exactly one record" % self._fa)
            self._text = recs[0][1]
        return self._text

    def cell(self, c, r):
        """The indexed starts of cell (c, r), ascending."""
        k = c * (self.width + 1) + r
        return self.pos[self._bounds[k]:self._bounds[k + 1]]

    def cell_of(self, start):
        """(C/G bytes, soft-masked bytes) of the window at `start`, counted on the text."""
        w = self.text[start:start + self.width]
        return int(_IS_CG[w].sum()), int(_IS_RP[w].sum())


class NullIndex:
    def __init__(self, out_dir, width):
        self.out_dir, self.width = out_dir, int(width)
        dv.nullidx_check(0, self.width)
        sub = os.path.join(out_dir, "nidx_t%d" % self.width)
        if not os.path.isdir(sub):
            raise NullseqError("%s holds no index of width %d" % (out_dir, self.width))
        self.names = sorted(f[:-len("_pos.npy")] for f in os.listdir(sub) if f.endswith("_pos.npy"))
        self._chroms = {}

    def chrom(self, name):
        if name not in self._chroms:
            if name not in self.names:
                raise NullseqError("chromosome %r is not in the index %s" % (name, self.out_dir))
            self._chroms[name] = ChromIndex(self.out_dir, self.width, name)
        return self._chroms[name]


def load_index(out_dir, width=DEFAULT_WIDTH):
    """Open an index directory (whoever wrote it): pos stays memory-mapped, texts are read when first needed."""
    return NullIndex(out_dir, width)


def _table(letters):
    t = np.zeros(256, dtype=bool)
    t[list(letters)] = True
    return t


_IS_CG, _IS_RP, _IS_BASE = _table(b"cgCG"), _table(b"acgt"), _table(b"ACGTacgt")


# ------------------------------------------------------------------ sampling
def cell_offsets(mg, mr):
    """The (dc, dr) of the cells a negative may come from, nearest first: by |dc| + |dr|, then |dc|, then dc, then dr."""
    offs = [(dc, dr) for dc in range(-mg, mg + 1) for dr in range(-mr, mr + 1)]
    return sorted(offs, key=lambda o: (abs(o[0]) + abs(o[1]), abs(o[0]), o[0], o[1]))


def _free(occupied, cand, t):
    """Which of the ascending starts `cand` overlap no window whose start is in the sorted list `occupied`."""
    occ = np.asarray(occupied, dtype=np.int64)
    cand = np.asarray(cand, dtype=np.int64)
    return np.searchsorted(occ, cand - t, side="right") == np.searchsorted(occ, cand + t, side="left")


def sample(index, positives, margin_gc=0.02, margin_rp=0.02, seed=1):
    """One matched negative window per positive (module docstring; INTEGRATION.md has the rules).

    positives: a list of subsets, each a list of (chrom, start) of windows of index.width bases.
    Returns, per subset, a list aligned with its positives: (chrom, start) of the negative, or None where no admissible
    window was left when the positive's turn came.  Depends on (index, positives, margins, seed) only."""
    t = index.width
    offs = cell_offsets(int(margin_gc * t), int(margin_rp * t))
    out = []
    for si, subset in enumerate(positives):
        subset = [(str(c), int(s)) for c, s in subset]
        occupied = {}
        for chrom, start in subset:
            ci = index.chrom(chrom)
            if start < 0 or start + t > len(ci.text):
                raise NullseqError("positive %s:%d-%d does not lie inside the %d bases of %s" %
                                   (chrom, start, start + t, len(ci.text), chrom))
            bisect.insort(occupied.setdefault(chrom, []), start)
        chosen, short = [], 0
        for pi, (chrom, start) in enumerate(subset):
            ci = index.chrom(chrom)
            c, r = ci.cell_of(start)
            rng = np.random.default_rng([int(seed), si, pi])
            got = None
            for dc, dr in offs:
                if not (0 <= c + dc <= t and 0 <= r + dr <= t):
                    continue
                cand = ci.cell(c + dc, r + dr)
                if not len(cand):
                    continue
                cand = np.asarray(cand)[_free(occupied[chrom], cand, t)]
                for j in rng.permutation(len(cand)):
                    s = int(cand[j])
                    if _IS_BASE[ci.text[s:s + t]].all():
                        got = s
                        break
                if got is not None:
                    break
            if got is None:
                short += 1
                chosen.append(None)
            else:
                bisect.insort(occupied[chrom], got)
                chosen.append((chrom, got))
        if short:
            logging.warning("subset %d: %d of %d positives are left without a negative: no admissible window remained",
                            si, short, len(subset))
        out.append(chosen)
    return out


# ------------------------------------------------------------------ files
def read_bed(path):
    """[(chrom, start)] of a BED file's records, in file order ('#' lines and blank lines skipped)."""
    sites = []
    with open(path) as f:
        for ln, line in enumerate(f, 1):
            if not line.strip() or line.startswith("#"):
                continue
            cols = line.split()
            try:
                sites.append((cols[0], int(cols[1])))
            except (IndexError, ValueError):
                raise NullseqError("%s:%d: not a BED record" % (path, ln))
    return sites


def write_bed(path, sites, width):
    with open(path, "w") as f:
        for chrom, start in sites:
            f.write("%s\t%d\t%d\n" % (chrom, start, start + width))


def write_fasta(path, index, sites):
    """>chrom:start+1-end and the window's letters, upper-cased, per site."""
    t = index.width
    with open(path, "w") as f:
        for chrom, start in sites:
            text = index.chrom(chrom).text
            if start < 0 or start + t > len(text):
                raise NullseqError("%s:%d-%d does not lie inside %s" % (chrom, start, start + t, chrom))
            f.write(">%s:%d-%d\n%s\n" % (chrom, start + 1, start + t, text[start:start + t].tobytes().decode("ascii").upper()))


# ------------------------------------------------------------------ command line
def main(argv=None):
    ap = argparse.ArgumentParser(prog="python -m gkmqc_amd.nullseq", description=__doc__.split("\n\n")[0])
    sub = ap.add_subparsers(dest="cmd", required=True)
    b = sub.add_parser("build-index", help="index a genome FASTA on the GPU")
    b.add_argument("--width", type=int, default=DEFAULT_WIDTH)
    b.add_argument("--device", type=int, default=0)
    b.add_argument("genome")
    b.add_argument("dir")
    s = sub.add_parser("sample", help="draw one matched negative per positive of a BED file")
    s.add_argument("--width", type=int, default=DEFAULT_WIDTH)
    s.add_argument("--margin-gc", type=float, default=0.02)
    s.add_argument("--margin-rp", type=float, default=0.02)
    s.add_argument("--seed", type=int, default=1)
    s.add_argument("--fasta", nargs=2, metavar=("POS_FA", "NEG_FA"))
    s.add_argument("dir")
    s.add_argument("pos_bed")
    s.add_argument("neg_bed")
    a = ap.parse_args(argv)
    logging.basicConfig(level=logging.INFO, format="%(levelname)s %(message)s")
    try:
        if a.cmd == "build-index":
            for name, T, n in build_index(a.genome, a.dir, a.width, a.device):
                print("%s\t%d\t%d" % (name, T, n))
        else:
            index = load_index(a.dir, a.width)
            pos = read_bed(a.pos_bed)
            neg = [n for n in sample(index, [pos], a.margin_gc, a.margin_rp, a.seed)[0] if n is not None]
            write_bed(a.neg_bed, neg, a.width)
            if a.fasta:
                write_fasta(a.fasta[0], index, pos)
                write_fasta(a.fasta[1], index, neg)
            print("%d positives, %d negatives" % (len(pos), len(neg)))
    except (NullseqError, dv.GkmError, OSError) as e:
        print("error: %s" % e, file=sys.stderr)
        return 1
    return 0


if __name__ == "__main__":
    sys.exit(main())
