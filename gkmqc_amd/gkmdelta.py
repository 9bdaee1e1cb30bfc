"""Variant effects from a weight table or a panel (deltaSVM): a list of variants, or every SNV of every
position.  Each panel form stands right after the single-table form whose result it repeats per member, bit for bit."""
import time

import numpy as np

from . import device as dv
from .gkmmodel import ModelError, codes_to_text
from .gkmquery import BLOCK_BYTES
from .gkmtables import LmerPanel, LmerTable, _check_folded, _models, _panel_row, _per_item
from .gkmscan import _as_scan_records


# ------------------------------------------------------------------ variant effects (deltaSVM)
DELTA_MAX_ALLELE = 255    # bases of an allele after trimming (GKMHIP_DELTA_MAX_ALLELE)
_ALLELE_CODES = {ord(ch): i & 3 for i, ch in enumerate("ACGTacgt")}


def delta_trim(pos, ref, alt):
    """A variant without the bases its alleles share -> (pos, ref, alt): first the common suffix goes, then the common
    prefix, which moves pos.  A VCF-style A -> AT at pos becomes "" -> "T" at pos + 1."""
    pos, ref, alt = int(pos), ref.upper(), alt.upper()
    n = 0
    while n < len(ref) and n < len(alt) and ref[len(ref) - 1 - n] == alt[len(alt) - 1 - n]:
        n += 1
    ref, alt = ref[:len(ref) - n], alt[:len(alt) - n]
    n = 0
    while n < len(ref) and n < len(alt) and ref[n] == alt[n]:
        n += 1
    return pos + n, ref[n:], alt[n:]


def delta_context(T, L, pos, ref_len):
    """The bases [a, e) a trimmed variant's delta reads: L - 1 on either side of the reference allele, inside the record.
    pos, ref_len: integers or arrays."""
    pos, ref_len = np.asarray(pos, dtype=np.int64), np.asarray(ref_len, dtype=np.int64)
    return np.maximum(0, pos - (L - 1)), np.minimum(int(T), pos + ref_len + (L - 1))


def delta_min_chunk(L):
    """The fewest bases a chunk may hold: the context of the longest allele, and a base."""
    return 2 * (int(L) - 1) + DELTA_MAX_ALLELE + 1


def default_delta_chunk(budget=BLOCK_BYTES):
    """Bases per chunk: a base costs its code, mask and l-mer word and, in a saturation map, its four doubles, within
    `budget` bytes of device memory."""
    return int(budget // 48)


def delta_chunk_plan(T, L, pos, ref_len, chunk):
    """The chunks that serve the trimmed variants (pos ascending) of a record of T bases -> [(v0, v1, b0, b1)]: variants
    [v0, v1) from the bases [b0, b1), at most `chunk` of them.  Every variant falls in exactly one chunk and its whole
    context (delta_context) lies inside it; a chunk starts where its first variant's context starts and ends where the
    last context it holds ends, so consecutive chunks overlap by at most L - 1 bases plus an allele."""
    a, e = delta_context(T, L, pos, ref_len)
    pos = np.asarray(pos, dtype=np.int64)
    out, v0 = [], 0
    while v0 < len(pos):
        b0 = int(a[v0])
        hi = int(np.searchsorted(pos, b0 + int(chunk), side="right"))      # (contexts that start beyond the chunk)
        over = np.flatnonzero(e[v0:hi] > b0 + int(chunk))
        v1 = v0 + int(over[0]) if len(over) else hi
        if v1 == v0:
            raise ModelError("delta: a chunk of %d bases cannot hold the context of a variant" % chunk)
        out.append((v0, v1, b0, int(e[v0:v1].max())))
        v0 = v1
    return out


def delta_saturation_chunk_plan(T, L, chunk):
    """The chunks of a saturation map of a record of T >= L bases -> [(t0, t1, b0, b1)]: positions [t0, t1) from the
    bases [b0, b1), at most max(chunk, 2 L - 1) of them: the positions and L - 1 bases of context on either side, where
    the record has them."""
    chunk, out, t0 = max(int(chunk), 2 * L - 1), [], 0
    while t0 < T:
        b0 = max(0, t0 - (L - 1))
        b1 = min(T, b0 + chunk)
        t1 = T if b1 == T else b1 - (L - 1)
        out.append((t0, t1, b0, b1))
        t0 = t1
    return out


def _variant_text(i, v):
    return "variant %d (%s)" % (i, ", ".join(repr(f) for f in tuple(v)[:4]))


def _allele(i, v, text):
    """An allele's base codes as bytes; ModelError if it is no string of A, C, G, T (either case)."""
    if not isinstance(text, str):
        raise ModelError("delta: %s: an allele must be a string of A, C, G, T" % _variant_text(i, v))
    coded = text.translate(_ALLELE_CODES)
    if coded and max(coded) > "\x03":
        raise ModelError("delta: %s: an allele holds a character other than A, C, G, T" % _variant_text(i, v))
    return coded.encode("latin-1")


def _resolve_variants(records, variants, match=True):
    """The checks of a variant list against the records it names, and its trimmed form -> (rec, pos, ref_len, alt): int64
    arrays in the order of `variants` and the alternate alleles' base codes as bytes.  match: also hold the reference
    allele against the record's valid bases.  records None: the alleles alone are checked (rec and pos as given)."""
    by_name = {}
    for j, (name, _, _) in enumerate(records or []):
        by_name.setdefault(name, j)
    rec, pos, rlen, alts = (np.zeros(len(variants), dtype=np.int64), np.zeros(len(variants), dtype=np.int64),
                            np.zeros(len(variants), dtype=np.int64), [])
    for i, v in enumerate(variants):
        if len(v) < 4:
            raise ModelError("delta: %s: a variant is (record, pos, ref, alt)" % _variant_text(i, v))
        r, p, ref, alt = v[0], v[1], v[2], v[3]
        rc, ac = _allele(i, v, ref), _allele(i, v, alt)
        if not isinstance(p, (int, np.integer)) or isinstance(p, bool) or p < 0:
            raise ModelError("delta: %s: the position must be an integer from 0 on" % _variant_text(i, v))
        j, p = 0, int(p)
        if records is not None:
            if isinstance(r, (int, np.integer)) and not isinstance(r, bool):
                j = int(r) if 0 <= int(r) < len(records) else -1
            else:
                j = by_name.get(r, -1)
            if j < 0:
                raise ModelError("delta: %s: no such record" % _variant_text(i, v))
            _, codes, valid = records[j]
            if p + len(rc) > len(codes):
                raise ModelError("delta: %s: the position lies outside the record of %d bases"
                                 % (_variant_text(i, v), len(codes)))
            if match and rc:
                have = codes[p:p + len(rc)]
                if (have[0] != rc[0] and valid[p]) if len(rc) == 1 else \
                        ((have != np.frombuffer(rc, dtype=np.uint8)) & valid[p:p + len(rc)]).any():
                    raise ModelError("delta: %s: the reference allele does not match the record, which reads %s there"
                                     % (_variant_text(i, v), codes_to_text(have)))
        if len(rc) == 1 and len(ac) == 1:                                  # (delta_trim on the codes, SNVs first)
            rc, ac = (b"", b"") if rc == ac else (rc, ac)
        elif rc and ac:
            n = 0
            while n < len(rc) and n < len(ac) and rc[len(rc) - 1 - n] == ac[len(ac) - 1 - n]:
                n += 1
            rc, ac = rc[:len(rc) - n], ac[:len(ac) - n]
            n = 0
            while n < len(rc) and n < len(ac) and rc[n] == ac[n]:
                n += 1
            p, rc, ac = p + n, rc[n:], ac[n:]
        if max(len(rc), len(ac)) > DELTA_MAX_ALLELE:
            raise ModelError("delta: %s: an allele of %d bases after trimming; at most %d"
                             % (_variant_text(i, v), max(len(rc), len(ac)), DELTA_MAX_ALLELE))
        rec[i], pos[i], rlen[i] = j, p, len(rc)
        alts.append(ac)
    return rec, pos, rlen, alts


def check_delta(table, variants=None, records=None, chunk=None):
    """What `delta` and `delta_saturation` refuse before they touch the device: a model in place of a table, a chunk too
    small for a context and, with `variants`, an allele with a character other than A, C, G, T or longer than
    DELTA_MAX_ALLELE after trimming and a negative position; with the `records` they refer to as well ([(name, codes,
    valid)], as read_long_fasta gives them), an unknown record and a position outside its record."""
    _check_delta(LmerTable, "delta", table, variants, records, chunk)


def check_panel_delta(panel, variants=None, records=None, chunk=None):
    """What `delta_with_panel` and `delta_saturation_with_panel` refuse before they touch the device (check_delta's
    refusals)."""
    _check_delta(LmerPanel, "delta-panel", panel, variants, records, chunk)


def _check_delta(want, what, folded, variants, records, chunk):
    """check_delta's and check_panel_delta's refusals; what: the prefix of the messages about the table or panel and the
    chunk (a variant's are `delta:` either way)"""
    _check_folded(want, what, folded)
    if chunk is not None and int(chunk) < delta_min_chunk(folded.L):
        raise ModelError("%s: a chunk must hold a variant's context (at least %d bases for L = %d)"
                         % (what, delta_min_chunk(folded.L), folded.L))
    if variants is not None:
        _resolve_variants(records, list(variants), match=False)


def _delta_upload(ctx, codes, valid, b0, b1, L, dev, stream):
    """The bases [b0, b1) of a record on the device -> (codes, l-mer words or None when there are fewer than L)."""
    import torch
    d_codes = torch.from_numpy(codes[b0:b1]).to(dev)
    if b1 - b0 < L:
        return d_codes, None
    d_valid = torch.from_numpy(valid[b0:b1].view(np.uint8)).to(dev)
    lm = torch.empty(b1 - b0 - L + 1, dtype=torch.int32, device=dev)
    ctx.scan_lmers(d_codes.data_ptr(), d_valid.data_ptr(), b1 - b0, lm.data_ptr(), stream)
    return d_codes, lm


def delta(table, fasta_or_sequences, variants, device=0, chunk=None, on_chunk=None):
    """deltaSVM of a list of variants from an l-mer weight table -> float64 array in the order of
    `variants`.  A variant is (record, pos, ref, alt[, ...]): the record by name or by index into the FASTA file (or the
    list of uint8 code arrays, values >= 4 invalid), pos 0-based, ref and alt strings of A, C, G, T, either possibly
    empty; VCF-style alleles that share bases are trimmed (delta_trim).  With S(z) the plain sum of W over the l-mers of
    z in order, the value is S(alternate context) - S(reference context), the context being the allele and L - 1 bases
    on either side, inside the record.  No positional weights enter: a variant has no window, so w_x = 1 for every
    kernel type.  NaN where the context holds a character other than A, C, G, T; +0.0 where the alleles are the same.
    Every value depends on the table, the record and the variant only: not on `chunk`, the order of the variants or
    the other records.  A reference allele that differs from the record is a ModelError.
    chunk: bases per device chunk (default_delta_chunk).  on_chunk(dict) (measurements): called after every chunk with
    its variants, bases, k_delta_variants' milliseconds (HIP events), its gathers and the chunk's wall time."""
    check_delta(table, chunk=chunk)
    return _delta_values(table, fasta_or_sequences, variants, device, chunk, on_chunk)


def delta_with_panel(panel, fasta_or_sequences, variants, device=0, chunk=None, on_chunk=None):
    """`delta` for every member of a panel -> float64 (len(variants), n_models): column m is delta's result for member m,
    bit for bit (NaN in every column where the context holds a character other than A, C, G, T; +0.0 where the alleles
    are the same).  The variants are resolved, sorted and checked once -- most of delta's time -- and each chunk is one
    k_panel_delta_variants launch.  on_chunk(dict) (measurements): delta's keys and `models`."""
    check_panel_delta(panel, chunk=chunk)
    return _delta_values(panel, fasta_or_sequences, variants, device, chunk, on_chunk)


def _delta_values(folded, fasta_or_sequences, variants, device, chunk, on_chunk):
    """The body `delta` and `delta_with_panel` share: the variants resolved, sorted and checked once, then one launch per
    chunk -> float64 (len(variants),) + folded.cols.  folded: the table or panel (checked)."""
    variants = list(variants)
    records = _as_scan_records(fasta_or_sequences)
    rec, pos, rlen, alts = _resolve_variants(records, variants)
    cols = folded.cols
    out = np.empty((len(variants),) + cols)
    if not len(variants):
        return out
    import torch
    L = folded.L
    chunk = int(chunk) if chunk else default_delta_chunk()
    alen = np.fromiter((len(a) for a in alts), dtype=np.int64, count=len(alts))
    ctx = dv.cached_context(*folded.kernel_params(), device=device)
    dev = torch.device("cuda", device)
    with torch.cuda.device(dev):
        stream = torch.cuda.current_stream().cuda_stream
        W = torch.from_numpy(folded.device_weights()).to(dev)
        launch = folded.launcher(ctx, "delta_variants")
        for j in np.unique(rec).tolist():
            _, codes, valid = records[j]
            T = len(codes)
            idx = np.flatnonzero(rec == j)
            idx = idx[np.argsort(pos[idx], kind="stable")]
            bad = np.zeros(T + 1, dtype=np.int64)
            np.cumsum(~valid, out=bad[1:])
            a, e = delta_context(T, L, pos[idx], rlen[idx])
            ok = bad[e] == bad[a]
            for v0, v1, b0, b1 in delta_chunk_plan(T, L, pos[idx], rlen[idx], chunk):
                t0 = time.perf_counter()
                mine = idx[v0:v1]
                d_codes, lm = _delta_upload(ctx, codes, valid, b0, b1, L, dev, stream)
                var = np.empty((len(mine), 4), dtype=np.int32)
                var[:, 0], var[:, 1], var[:, 3] = pos[mine] - b0, rlen[mine], alen[mine]
                var[:, 2] = np.cumsum(alen[mine]) - alen[mine]
                alt = np.frombuffer(b"".join([alts[i] for i in mine.tolist()]), dtype=np.uint8)
                d_out = torch.empty((len(mine),) + cols, dtype=torch.float64, device=dev)
                launch(lm.data_ptr() if lm is not None else None, d_codes.data_ptr(), b1 - b0, var, alt, W.data_ptr(),
                       d_out.data_ptr(), stream)
                out[mine] = np.where(_per_item(ok[v0:v1], cols), d_out.cpu().numpy(), np.nan)
                if on_chunk is not None:
                    on_chunk(dict(variants=len(mine), bases=b1 - b0, kernel_ms=ctx.last_kernel_ms(),
                                  gathers=ctx.last_comparisons(), kernel=ctx.last_kernel_name(),
                                  wall_ms=(time.perf_counter() - t0) * 1e3, **_models(cols)))
    return out


def delta_saturation(table, fasta_or_sequences, device=0, chunk=None, on_chunk=None):
    """The saturation map of every record of a FASTA file (or of each of a list of uint8 code arrays, values >= 4
    invalid) from an l-mer weight table -> [(name, (T, 4) float64)]: row t, column b (A, C, G, T) is `delta` of the SNV
    that puts b at position t, bit for bit; +0.0 in the column of the base that is there; a row of NaN where the context
    of t (L - 1 bases on either side) holds a character other than A, C, G, T.  Independent of `chunk` and of the other
    records.  A record shorter than L is an error.
    chunk: bases per device chunk (default_delta_chunk).  on_chunk(dict) (measurements): called after every chunk with
    its positions, bases, k_delta_sat's milliseconds (HIP events), its gathers and the chunk's wall time."""
    check_delta(table, chunk=chunk)
    return _saturation_folded(table, fasta_or_sequences, device, chunk or default_delta_chunk(), on_chunk)


def delta_saturation_with_panel(panel, fasta_or_sequences, device=0, chunk=None, on_chunk=None):
    """`delta_saturation` for every member of a panel -> [(name, (T, 4, n_models) float64)]: [:, :, m] is
    delta_saturation's map for member m, bit for bit, and D[t, b, m] is delta_with_panel's value of that SNV.
    on_chunk(dict) (measurements): delta_saturation's keys and `models`."""
    check_panel_delta(panel, chunk=chunk)
    return _saturation_folded(panel, fasta_or_sequences, device, chunk or
                              max(delta_min_chunk(panel.L), int(BLOCK_BYTES // (16 + 32 * panel.n_models))), on_chunk)


def _saturation_folded(folded, fasta_or_sequences, device, chunk, on_chunk):
    """The body `delta_saturation` and `delta_saturation_with_panel` share -> [(name, (T, 4) + folded.cols)].  folded: the
    table or panel (checked with chunk); chunk: bases per chunk."""
    records = _as_scan_records(fasta_or_sequences)
    L, cols, chunk = folded.L, folded.cols, int(chunk)
    for name, codes, _ in records:
        if len(codes) < L:
            raise ModelError("delta-saturation: record %r has %d bases, fewer than L = %d" % (name, len(codes), L))
    import torch
    ctx = dv.cached_context(*folded.kernel_params(), device=device)
    dev = torch.device("cuda", device)
    out = []
    with torch.cuda.device(dev):
        stream = torch.cuda.current_stream().cuda_stream
        W = torch.from_numpy(folded.device_weights()).to(dev)
        launch = folded.launcher(ctx, "delta_sat")
        for name, codes, valid in records:
            T = len(codes)
            D = np.empty((T, 4) + cols)
            for t0, t1, b0, b1 in delta_saturation_chunk_plan(T, L, chunk):
                w0 = time.perf_counter()
                _, lm = _delta_upload(ctx, codes, valid, b0, b1, L, dev, stream)
                d_out = torch.empty((t1 - t0, 4) + cols, dtype=torch.float64, device=dev)
                launch(lm.data_ptr(), len(lm), t0 - b0, t1 - b0, W.data_ptr(), d_out.data_ptr(), stream)
                D[t0:t1] = d_out.cpu().numpy()
                if on_chunk is not None:
                    on_chunk(dict(positions=t1 - t0, bases=b1 - b0, **_models(cols), kernel_ms=ctx.last_kernel_ms(),
                                  gathers=ctx.last_comparisons(), kernel=ctx.last_kernel_name(),
                                  wall_ms=(time.perf_counter() - w0) * 1e3))
            out.append((name, D))
    return out


def _variant_fields(path, no, fields):
    """name, pos (1-based in the file), ref, alt[, id] -> (name, pos 0-based, ref, alt[, id]); "." or "-" is the empty
    allele"""
    if len(fields) not in (4, 5):
        raise ModelError("%s:%d: expected name<TAB>pos<TAB>ref<TAB>alt[<TAB>id]" % (path, no))
    try:
        pos = int(fields[1])
    except ValueError:
        pos = 0
    if pos < 1:
        raise ModelError("%s:%d: the position must be an integer from 1 on: %r" % (path, no, fields[1]))
    ref, alt = ("" if f in (".", "-") else f for f in fields[2:4])
    return (fields[0], pos - 1, ref, alt) + tuple(fields[4:])


def read_variants(path):
    """A variant file -> [(name, pos, ref, alt[, id])] with pos 0-based: tab-separated name, pos (1-based), ref, alt and
    an optional id per line; "." or "-" stands for an empty allele; lines that start with '#' and empty lines are
    ignored."""
    out = []
    with open(path) as f:
        for no, line in enumerate(f.read().split("\n"), 1):
            line = line.rstrip("\r")
            if line and not line.startswith("#"):
                out.append(_variant_fields(path, no, line.split("\t")))
    return out


def write_delta(path, variants, values):
    """The `delta` output: the columns of the variant file (name, 1-based pos, ref, alt[, id]; "." for an empty allele)
    plus the delta at %.17g, which reads back to the same double; a variant without a value keeps its row, with nan."""
    with open(path, "w") as f:
        for v, x in zip(variants, np.asarray(values, dtype=np.float64).tolist()):
            f.write("\t".join([str(v[0]), "%d" % (int(v[1]) + 1), v[2] or ".", v[3] or "."] + [str(c) for c in v[4:5]]
                              + ["nan" if x != x else "%.17g" % x]) + "\n")


def read_delta(path):
    """-> (variants as read_variants gives them, float64 array) from a file written by write_delta."""
    variants, values = [], []
    with open(path) as f:
        for no, line in enumerate(f.read().split("\n")[:-1], 1):
            fields = line.split("\t")
            variants.append(_variant_fields(path, no, fields[:-1]))
            values.append(float(fields[-1]))
    return variants, np.array(values, dtype=np.float64)


def write_panel_delta(path, panel_names, variants, values):
    """The `delta-panel` output: the header #name<TAB>pos<TAB>ref<TAB>alt[<TAB>id]<TAB>member names (id when the first
    variant carries one), then write_delta's leading columns and one delta per member at %.17g, nan where there is none."""
    with open(path, "w") as f:
        lead = ["name", "pos", "ref", "alt"] + (["id"] if len(variants) and len(variants[0]) > 4 else [])
        f.write("#" + "\t".join(lead + list(panel_names)) + "\n")
        for v, row in zip(variants, np.asarray(values, dtype=np.float64).tolist()):
            f.write(_panel_row([str(v[0]), "%d" % (int(v[1]) + 1), v[2] or ".", v[3] or "."] + [str(c) for c in v[4:5]],
                               row))


def write_saturation(path, results, fasta_or_sequences):
    """The `delta-saturation` output: name<TAB>pos<TAB>ref<TAB>dA<TAB>dC<TAB>dG<TAB>dT per position, pos 1-based, ref the
    base of the record there, values at %.17g; positions without a value (NaN) are left out.  results: what
    delta_saturation returned for the same records.  -> how many were left out."""
    omitted = 0
    with open(path, "w") as f:
        for (name, D), (_, codes, _) in zip(results, _as_scan_records(fasta_or_sequences)):
            keep = np.flatnonzero(~np.isnan(D).any(axis=1))
            omitted += len(D) - len(keep)
            text = codes_to_text(codes)
            for i in range(0, len(keep), 1 << 16):
                k = keep[i:i + (1 << 16)]
                f.write("".join("%s\t%d\t%s\t%.17g\t%.17g\t%.17g\t%.17g\n" % ((name, t + 1, text[t]) + tuple(row))
                                for t, row in zip(k.tolist(), D[k].tolist())))
    return omitted


def read_saturation(path):
    """-> [(name, pos 0-based, ref, (4,) float64)] from a file written by write_saturation."""
    out = []
    with open(path) as f:
        for line in f.read().split("\n")[:-1]:
            name, t, ref, a, c, g, tt = line.rsplit("\t", 6)
            out.append((name, int(t) - 1, ref, np.array([float(a), float(c), float(g), float(tt)])))
    return out
