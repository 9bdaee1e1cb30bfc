"""PWM motifs scored against an l-mer weight table or panel on the device.

    read_motifs(path)                        minimal MEME text -> [(name, M)]
    motif_windows(M, L, background)          the m + L - 1 windows of a motif embedded in background
    motif_scores(table, motifs, ...)         affinity, enrichment, peak of every motif against a table
    motif_scores_with_panel(panel, ...)      the same with a trailing n_models axis
    position_marginals(table)                the table's own base preference per l-mer position
    contract_windows(table_or_panel, P)      the launch under all of them: any (n, L, 4) windows -> their values

A window is an (L, 4) array of float64, P[i][b] for l-mer position i (0: the first base) and base b (A, C, G, T).  Its value
is the expected table weight of an l-mer drawn from its columns,

    a(P) = sum over all 4^L codes u of W(u) prod_i P[i][u_i]

evaluated on the device in one fixed order of rounded operations (contract_reference restates it), so a value depends on the
table and the window alone: not on the block size, the order of the motifs or the run.  A motif M (m rows, 1 <= m <=
MOTIF_MAX_WIDTH) is padded with L - 1 background rows on either side; window o holds rows o .. o + L - 1 of that.  Per
motif: profile[o] = a(window o); affinity = their sum in ascending o; background = a(the all-background window); enrichment
= affinity - (m + L - 1) background; peak = the largest profile value, the lowest o on a tie; peak_offset = o - (L - 1), the
motif column at which the peak window begins.  No orientation is reported: a table satisfies W[u] == W[rc(u)], so the
reverse-complement motif has the same profile reversed, up to rounding.

Command line:
    python -m gkmqc_amd.gkmmotifs score       [--background a,c,g,t --profiles FILE --block N --device D] weights motifs out.tsv
    python -m gkmqc_amd.gkmmotifs score-panel [... --field enrichment]                                     panel   motifs out.tsv
    python -m gkmqc_amd.gkmmotifs marginals   [--device D]                                                 weights out.tsv
"""
import argparse
import os
import sys
import time

import numpy as np

from . import device as dv
from .gkmmodel import ModelError
from .gkmquery import BLOCK_BYTES
from .gkmtables import (LmerPanel, LmerTable, _check_folded, _panel_row, load_lmer_panel, load_lmer_table, panel_row_stride,
                        read_panel_output)

MOTIF_MAX_WIDTH = 64
ROW_SUM_TOLERANCE = 0.01            # MEME files are rounded to six digits; a row further from 1 is no distribution
FIELDS = ("affinity", "background", "enrichment", "peak", "peak_offset")
PANEL_FIELDS = ("affinity", "enrichment", "peak", "peak_offset")   # what score-panel's --field takes
_SCORE_HEADER = "#name\twidth\t" + "\t".join(FIELDS)
_MARGINAL_HEADER = "#position\tA\tC\tG\tT"


class MotifError(ModelError):
    pass


# ------------------------------------------------------------------ motifs and windows
def _row_sums(M):
    return ((M[:, 0] + M[:, 1]) + M[:, 2]) + M[:, 3]


def normalise_motif(name, M):
    """The input rules of a motif -> float64 (m, 4), every row divided by its sum ((a + c) + g) + t.  Refused with the
    motif's name and the row: a shape other than (1..MOTIF_MAX_WIDTH, 4), a value that is not finite or is negative, a row
    whose sum lies further than ROW_SUM_TOLERANCE from 1."""
    try:
        M = np.array(M, dtype=np.float64)
    except (TypeError, ValueError):
        raise MotifError("motif %s: not an array of numbers" % name)
    if M.ndim != 2 or M.shape[1] != 4 or not 1 <= M.shape[0] <= MOTIF_MAX_WIDTH:
        raise MotifError("motif %s: needs 1..%d rows of four probabilities, not the shape %r"
                         % (name, MOTIF_MAX_WIDTH, M.shape))
    bad = ~np.isfinite(M) | (M < 0)
    if bad.any():
        raise MotifError("motif %s: row %d holds a value that is not finite or is negative"
                         % (name, int(np.nonzero(bad.any(axis=1))[0][0])))
    s = _row_sums(M)
    off = np.abs(s - 1.0) > ROW_SUM_TOLERANCE
    if off.any():
        r = int(np.nonzero(off)[0][0])
        raise MotifError("motif %s: row %d sums to %r, further than %g from 1" % (name, r, float(s[r]), ROW_SUM_TOLERANCE))
    return M / s[:, None]


def check_background(background, what="motif_scores"):
    """None (uniform 0.25) or four probabilities under the rules of a motif row -> float64 (4,)."""
    if background is None:
        return np.full(4, 0.25)
    try:
        b = np.array(background, dtype=np.float64)
    except (TypeError, ValueError):
        raise MotifError("%s: the background must be four numbers" % what)
    if b.shape != (4,):
        raise MotifError("%s: the background must be four numbers (A, C, G, T)" % what)
    if not np.isfinite(b).all() or (b < 0).any():
        raise MotifError("%s: the background holds a value that is not finite or is negative" % what)
    s = ((b[0] + b[1]) + b[2]) + b[3]
    if abs(s - 1.0) > ROW_SUM_TOLERANCE:
        raise MotifError("%s: the background sums to %r, further than %g from 1" % (what, float(s), ROW_SUM_TOLERANCE))
    return b / s


def motif_windows(M, L, background=None):
    """The windows of a motif -> float64 (m + L - 1, L, 4): M as given (normalise_motif is the caller's) between L - 1
    background rows on either side, window o = rows o .. o + L - 1."""
    M = np.asarray(M, dtype=np.float64)
    L = int(L)
    if M.ndim != 2 or M.shape[1] != 4 or len(M) < 1:
        raise MotifError("motif_windows: a motif is (m, 4) with m >= 1")
    if L < 1:
        raise MotifError("motif_windows: L must be at least 1")
    pad = np.broadcast_to(check_background(background, "motif_windows"), (L - 1, 4))
    padded = np.concatenate((pad, M, pad))
    return np.ascontiguousarray(np.lib.stride_tricks.sliding_window_view(padded, (L, 4))[:, 0])


def reverse_complement_motif(M):
    """The motif read on the other strand: rows reversed, A <-> T and C <-> G."""
    return np.ascontiguousarray(np.asarray(M, dtype=np.float64)[::-1, ::-1])


def contract_reference(W, P):
    """a(P) of one window (L, 4) against the 4^L weights W in the device's order, with numpy's elementwise operations only
    (each product and sum rounded on its own).  The host statement of the definition: milliseconds per window."""
    T = np.asarray(W, dtype=np.float64)
    P = np.asarray(P, dtype=np.float64)
    for i in range(len(P) - 1, -1, -1):
        T = T.reshape(-1, 4)
        T = ((T[:, 0] * P[i, 0] + T[:, 1] * P[i, 1]) + T[:, 2] * P[i, 2]) + T[:, 3] * P[i, 3]
    return float(T[0])


def read_motifs(path):
    """Minimal MEME text -> [(name, M float64 (m, 4))], rows normalised (normalise_motif).  `MOTIF <name> [alt]`, then
    `letter-probability matrix: ... w= <m> ...` and m rows of four numbers; what precedes the first MOTIF is ignored, except
    an ALPHABET= other than ACGT.  Refused with path:line: a duplicate name, a row count that disagrees with w=, a width
    outside 1..MOTIF_MAX_WIDTH, a row that is not four numbers, a row that breaks the input rules, a file without a
    motif."""
    with open(path) as f:
        lines = f.read().split("\n")
    out, names = [], set()
    name = name_line = None     # the motif whose matrix has not begun
    rows = want = None          # the matrix being read

    def fail(no, text):
        raise MotifError("%s:%d: %s" % (path, no, text))

    def numbers(fields):
        try:
            return [float(x) for x in fields]
        except ValueError:
            return None

    def finish(no):
        nonlocal name, rows, want
        if len(rows) != want:
            fail(no, "motif %s: %d rows where w= announces %d" % (name, len(rows), want))
        try:
            out.append((name, normalise_motif(name, rows)))
        except MotifError as e:
            fail(first, "%s (rows counted from this line)" % e)
        name = rows = want = None

    first = 0                   # the line of the matrix's first row
    for no, line in enumerate(lines, 1):
        fields = line.split()
        if rows is not None:
            vals = numbers(fields) if len(fields) == 4 else None
            if vals is not None:
                if len(rows) == want:
                    fail(no, "motif %s: a row beyond the %d that w= announces" % (name, want))
                if not rows:
                    first = no
                rows.append(vals)
                continue
            if len(rows) < want and fields and numbers(fields[:1]) is not None:     # begins like a row
                fail(no, "motif %s: row %d is not four numbers" % (name, len(rows)))
            finish(no)                                                              # anything else ends the matrix
        if not fields:
            continue
        if fields[0] == "MOTIF":
            if name is not None:
                fail(name_line, "motif %s has no letter-probability matrix" % name)
            if len(fields) < 2:
                fail(no, "MOTIF without a name")
            if fields[1] in names:
                fail(no, "the motif name %s is given twice" % fields[1])
            name, name_line = fields[1], no
            names.add(name)
        elif line.startswith("letter-probability matrix"):
            if name is None:
                fail(no, "a letter-probability matrix without a MOTIF line")
            keys = line.split(":", 1)[1].replace("=", "= ").split()
            vals = dict(zip(keys[::2], keys[1::2]))
            if "alength=" in vals and vals["alength="] != "4":
                fail(no, "motif %s: alength= %s; only the four-letter alphabet ACGT is served" % (name, vals["alength="]))
            try:
                want = int(vals["w="])
            except (KeyError, ValueError):
                fail(no, "motif %s: the matrix line carries no integer w=" % name)
            if not 1 <= want <= MOTIF_MAX_WIDTH:
                fail(no, "motif %s: the width %d lies outside 1..%d" % (name, want, MOTIF_MAX_WIDTH))
            rows = []
        elif not names and line.startswith("ALPHABET"):
            if line.replace(" ", "") != "ALPHABET=ACGT":
                fail(no, "the alphabet must be ACGT: %s" % line.strip())
    if rows is not None:
        finish(len(lines))
    if name is not None:
        fail(name_line, "motif %s has no letter-probability matrix" % name)
    if not out:
        raise MotifError("%s: holds no motif" % path)
    return out


# ------------------------------------------------------------------ checks without a device
def default_motif_block(L, n_models=0, budget=BLOCK_BYTES):
    """Windows per device block: a window's L x 4 doubles, its max(1, n_models) results and its share of the tiles' partial
    values (device.contract_scratch_bytes) within `budget` bytes, at most device.contract_max_windows."""
    per = 32 * int(L) + 8 * max(1, int(n_models)) + dv.contract_scratch_bytes(L, n_models, 1)
    return int(max(1, min(dv.contract_max_windows(L, n_models), int(budget) // per)))


def _check_scores(want, what, folded, motifs, background, block):
    """-> (names, [normalised M], background (4,)).  Refuses a model, or a table where a panel is needed and the reverse, a
    bad background, a block outside 1..contract_max_windows, an empty motif list, a duplicate or empty name and whatever
    normalise_motif refuses."""
    _check_folded(want, what, folded)
    bg = check_background(background, what)
    if block is not None:
        most = dv.contract_max_windows(folded.L, folded.cols[0] if folded.cols else 0)
        if int(block) < 1 or int(block) > most:
            raise MotifError("%s: a block holds 1..%d windows, not %d" % (what, most, int(block)))
    motifs = list(motifs)
    if not motifs:
        raise MotifError("%s: no motifs" % what)
    names, mats = [], []
    for i, item in enumerate(motifs):
        try:
            name, M = item
        except (TypeError, ValueError):
            raise MotifError("%s: motif %d is no (name, matrix) pair" % (what, i))
        if not isinstance(name, str) or not name or "\t" in name or "\n" in name:
            raise MotifError("%s: the name of motif %d must be a non-empty string without tab or newline: %r" % (what, i, name))
        if name in names:
            raise MotifError("%s: the motif name %s is given twice" % (what, name))
        names.append(name)
        mats.append(normalise_motif(name, M))
    return names, mats, bg


def check_motif_scores(table, motifs, background=None, block=None):
    """What motif_scores refuses before the device is touched -> (names, normalised matrices, background)."""
    return _check_scores(LmerTable, "motif_scores", table, motifs, background, block)


def check_panel_motif_scores(panel, motifs, background=None, block=None):
    """What motif_scores_with_panel refuses before the device is touched."""
    return _check_scores(LmerPanel, "motif_scores_with_panel", panel, motifs, background, block)


# ------------------------------------------------------------------ the device loop
def contract_windows(folded, P, device=0, block=None, on_block=None):
    """a(P) of the windows P (n, L, 4), n >= 1, against a table -> (n,) or a panel -> (n, n_models), in blocks of `block`
    windows: per block the windows go up, one launch, n (x n_models) doubles come back.  What motif_scores and
    position_marginals run on; the windows' rows are taken as they are."""
    import torch
    L, cols = folded.L, folded.cols
    nm = cols[0] if cols else 0
    P = np.ascontiguousarray(P, dtype=np.float64)
    if P.ndim != 3 or P.shape[1:] != (L, 4) or len(P) < 1:
        raise MotifError("contract_windows: the windows must be (n, L, 4) = (n, %d, 4) with n >= 1, not %r" % (L, P.shape))
    block = default_motif_block(L, nm) if block is None else int(block)
    ctx = dv.cached_context(*folded.kernel_params(), device=device)
    dev = torch.device("cuda", device)
    out = np.empty((len(P),) + cols)
    with torch.cuda.device(dev):
        stream = torch.cuda.current_stream().cuda_stream
        W = torch.from_numpy(folded.device_weights()).to(dev)
        d_out = torch.empty((min(block, len(P)),) + cols, dtype=torch.float64, device=dev)
        for w0 in range(0, len(P), block):
            t0 = time.perf_counter()
            w1 = min(len(P), w0 + block)
            d_P = torch.from_numpy(P[w0:w1]).to(dev)
            if cols:
                ctx.panel_contract(W.data_ptr(), nm, panel_row_stride(nm), d_P.data_ptr(), w1 - w0, d_out.data_ptr(), nm, stream)
            else:
                ctx.lmer_contract(W.data_ptr(), d_P.data_ptr(), w1 - w0, d_out.data_ptr(), stream)
            out[w0:w1] = d_out[:w1 - w0].cpu().numpy()
            if on_block is not None:
                on_block(dict(windows=w1 - w0, **(dict(models=nm) if cols else {}), kernel_ms=ctx.last_kernel_ms(),
                              terms=ctx.last_comparisons(), kernel=ctx.last_kernel_name(),
                              wall_ms=(time.perf_counter() - t0) * 1e3))
    return out


def summarise_profile(profile, m, L, b0):
    """The per-motif values from a profile (m + L - 1,) or (m + L - 1, n_models) and the background level b0, by the stated
    host arithmetic -> (affinity, enrichment, peak, peak_offset): the sum by sequential additions in ascending o, one
    rounded product and one rounded subtraction, the first largest value."""
    profile = np.asarray(profile, dtype=np.float64)
    affinity = np.cumsum(profile, axis=0)[-1]
    enrichment = affinity - np.float64(m + L - 1) * b0
    o = np.argmax(profile, axis=0)
    peak = np.take_along_axis(profile, np.expand_dims(o, 0), axis=0)[0] if profile.ndim > 1 else profile[o]
    return affinity, enrichment, peak, o - (L - 1)


def _scores(folded, checked, profiles, device, block, on_block):
    names, mats, bg = checked
    L = folded.L
    wins = [motif_windows(M, L, bg) for M in mats]
    wins.append(np.broadcast_to(bg, (1, L, 4)))                            # the all-background window, once per call
    values = contract_windows(folded, np.ascontiguousarray(np.concatenate(wins)), device, block, on_block)
    b0 = values[-1]
    res = dict(names=names, width=np.array([len(M) for M in mats], dtype=np.int64), background=b0 if folded.cols else float(b0))
    per, at = [], 0
    for M in mats:
        n = len(M) + L - 1
        per.append(values[at:at + n])
        at += n
    parts = [summarise_profile(p, len(M), L, b0) for p, M in zip(per, mats)]
    for i, key in enumerate(("affinity", "enrichment", "peak", "peak_offset")):
        res[key] = np.array([p[i] for p in parts], dtype=np.int64 if key == "peak_offset" else np.float64)
    if profiles:
        res["profiles"] = [p.copy() for p in per]
    return res


def motif_scores(table, motifs, background=None, profiles=False, device=0, block=None, on_block=None):
    """Every motif of [(name, M)] against an l-mer weight table -> dict(names, width int64 (n,), affinity, enrichment, peak
    float64 (n,), peak_offset int64 (n,), background float, and with profiles=True profiles: [float64 (m + L - 1,)]).  The
    windows of all motifs are pooled and sent in blocks of `block` windows (default_motif_block); only one double per
    window comes back.  The same bytes for every block and every order of the motifs.  on_block(dict) (measurements):
    called after every block with its windows, the kernels' milliseconds (HIP events), the 4^L terms per window summed
    and the block's wall time."""
    return _scores(table, check_motif_scores(table, motifs, background, block), profiles, device, block, on_block)


def motif_scores_with_panel(panel, motifs, background=None, profiles=False, device=0, block=None, on_block=None):
    """motif_scores for every member of a panel: the same fields with a trailing n_models axis (background: (n_models,)),
    column m bit for bit motif_scores' result on panel.table(m).  One row read per l-mer serves every member."""
    return _scores(panel, check_panel_motif_scores(panel, motifs, background, block), profiles, device, block, on_block)


def marginal_windows(L):
    """The 4 L windows of position_marginals -> (L, 4, L, 4): window (i, b) is one-hot b at position i, uniform elsewhere."""
    P = np.full((L, 4, L, 4), 0.25)
    for i in range(L):
        P[i, :, i, :] = np.eye(4)
    return P


def _marginals(want, what, folded, device):
    _check_folded(want, what, folded)
    L = folded.L
    values = contract_windows(folded, marginal_windows(L).reshape(4 * L, L, 4), device, None, None)
    return values.reshape((L, 4) + folded.cols)


def position_marginals(table, device=0):
    """The table's own base preference per l-mer position -> float64 (L, 4): a(P) of the window that is one-hot b at
    position i and uniform elsewhere, 4 L windows through motif_scores' launch."""
    return _marginals(LmerTable, "position_marginals", table, device)


def position_marginals_with_panel(panel, device=0):
    """position_marginals for every member of a panel -> float64 (L, 4, n_models)."""
    return _marginals(LmerPanel, "position_marginals_with_panel", panel, device)


# ------------------------------------------------------------------ files
def _atomically(path, text):
    tmp = path + ".tmp"
    with open(tmp, "w") as f:
        f.write(text)
    os.replace(tmp, path)


def write_motif_scores(path, result):
    """The `score` output: the header #name, width and FIELDS, then one line per motif with repr() floats (which read back
    to the same doubles)."""
    rows = zip(result["names"], result["width"].tolist(), result["affinity"].tolist(), result["enrichment"].tolist(),
               result["peak"].tolist(), result["peak_offset"].tolist())
    b0 = float(result["background"])
    _atomically(path, _SCORE_HEADER + "\n" + "".join("%s\t%d\t%r\t%r\t%r\t%r\t%d\n" % (n, w, a, b0, e, p, o)
                                                      for n, w, a, e, p, o in rows))


def read_motif_scores(path):
    """-> dict(names, width, affinity, background, enrichment, peak, peak_offset) from a file written by
    write_motif_scores."""
    with open(path) as f:
        lines = f.read().split("\n")[:-1]
    if not lines or lines[0] != _SCORE_HEADER:
        raise MotifError("%s: no motif score header" % path)
    rows = []
    for no, line in enumerate(lines[1:], 2):
        f = line.split("\t")
        try:
            if len(f) != 7:
                raise ValueError
            rows.append((f[0], int(f[1]), float(f[2]), float(f[3]), float(f[4]), float(f[5]), int(f[6])))
        except ValueError:
            raise MotifError("%s:%d: expected a name, a width, four numbers and an offset" % (path, no))
    if len({r[3] for r in rows}) > 1:
        raise MotifError("%s: the background column holds more than one value" % path)

    def col(i, dt):
        return np.array([r[i] for r in rows], dtype=dt)

    return dict(names=[r[0] for r in rows], width=col(1, np.int64), affinity=col(2, np.float64),
                background=rows[0][3] if rows else float("nan"), enrichment=col(4, np.float64), peak=col(5, np.float64),
                peak_offset=col(6, np.int64))


def write_panel_motif_scores(path, panel_names, result, field="enrichment"):
    """The `score-panel` output: the header #name<TAB>member names, then per motif its name and one value of `field` per
    member at %.17g (read_panel_motif_scores)."""
    if field not in PANEL_FIELDS:
        raise MotifError("score-panel: the field must be one of %s" % ", ".join(PANEL_FIELDS))
    values = np.asarray(result[field], dtype=np.float64)
    _atomically(path, "#" + "\t".join(["name"] + list(panel_names)) + "\n"
                + "".join(_panel_row([name], row) for name, row in zip(result["names"], values.tolist())))


def read_panel_motif_scores(path):
    """-> (member names, motif names, float64 (motifs, n_models)) from a file written by write_panel_motif_scores."""
    members, leads, values = read_panel_output(path, 1)
    return members, [lead[0] for lead in leads], values


def write_motif_profiles(path, result, L):
    """The --profiles output: name<TAB>offset<TAB>value per window, offset = o - (L - 1) the motif column at which the window
    begins; repr() floats for a table, one %.17g column per member for a panel."""
    text = []
    for name, prof in zip(result["names"], result["profiles"]):
        for o, v in enumerate(prof.tolist()):
            lead = [name, "%d" % (o - (int(L) - 1))]
            text.append(_panel_row(lead, v) if isinstance(v, list) else "\t".join(lead + [repr(v)]) + "\n")
    _atomically(path, "".join(text))


def read_motif_profiles(path):
    """-> (names, [int64 offsets], [float64 (windows,) or (windows, n_models)]) from a file written by
    write_motif_profiles."""
    names, offs, vals = [], [], []
    with open(path) as f:
        for no, line in enumerate(f.read().split("\n")[:-1], 1):
            fields = line.split("\t")
            try:
                if len(fields) < 3:
                    raise ValueError
                o, v = int(fields[1]), [float(x) for x in fields[2:]]
            except ValueError:
                raise MotifError("%s:%d: expected a name, an offset and values" % (path, no))
            if not names or names[-1] != fields[0]:
                names.append(fields[0])
                offs.append([])
                vals.append([])
            offs[-1].append(o)
            vals[-1].append(v[0] if len(v) == 1 else v)
    return names, [np.array(o, dtype=np.int64) for o in offs], [np.array(v, dtype=np.float64) for v in vals]


def write_marginals(path, marg):
    """The `marginals` output: the header #position A C G T, then per l-mer position its index and four repr() floats."""
    marg = np.asarray(marg, dtype=np.float64)
    if marg.ndim != 2 or marg.shape[1] != 4:
        raise MotifError("write_marginals: needs (L, 4) values")
    _atomically(path, _MARGINAL_HEADER + "\n" + "".join("%d\t%r\t%r\t%r\t%r\n" % ((i,) + tuple(row))
                                                         for i, row in enumerate(marg.tolist())))


def read_marginals(path):
    """-> float64 (L, 4) from a file written by write_marginals."""
    with open(path) as f:
        lines = f.read().split("\n")[:-1]
    if not lines or lines[0] != _MARGINAL_HEADER:
        raise MotifError("%s: no marginals header" % path)
    try:
        rows = [[float(x) for x in line.split("\t")] for line in lines[1:]]
        if any(len(r) != 5 or r[0] != i for i, r in enumerate(rows)):
            raise ValueError
    except ValueError:
        raise MotifError("%s: expected a position and four numbers per line" % path)
    return np.array([r[1:] for r in rows], dtype=np.float64).reshape(len(rows), 4)


# ------------------------------------------------------------------ command line
def parse_background(text):
    """--background a,c,g,t -> four floats (check_background judges them)."""
    try:
        return [float(x) for x in text.split(",")]
    except ValueError:
        raise MotifError("--background takes four comma-separated numbers, not %r" % text)


def build_parser():
    p = argparse.ArgumentParser(prog="gkmmotifs", description=__doc__.split("\n\n")[0])
    sub = p.add_subparsers(dest="cmd", required=True)
    for name, text in (("score", "every motif of a MEME file against a weights file -> TSV"),
                       ("score-panel", "the same against a panel: one field, one column per member -> TSV"),
                       ("marginals", "the table's base preference per l-mer position -> TSV")):
        q = sub.add_parser(name, help=text)
        if name != "marginals":
            q.add_argument("--background", default=None, help="a,c,g,t: the order-0 background (default: uniform)")
            q.add_argument("--profiles", default=None, help="also write every window's value to this file")
            q.add_argument("--block", type=int, default=None, help="windows per device block (default: from device memory)")
        if name == "score-panel":
            q.add_argument("--field", default="enrichment", help="one of %s (default enrichment)" % ", ".join(PANEL_FIELDS))
        q.add_argument("--device", type=int, default=0)
        q.add_argument("source", metavar="panel" if name == "score-panel" else "weights")
        if name != "marginals":
            q.add_argument("motifs")
        q.add_argument("output")
    return p


def main(argv=None):
    a = build_parser().parse_args(argv)
    try:
        for path in [a.source] + ([a.motifs] if a.cmd != "marginals" else []):
            if not os.path.isfile(path):
                raise MotifError("cannot read %s" % path)
        if a.cmd == "marginals":
            write_marginals(a.output, position_marginals(load_lmer_table(a.source), device=a.device))
            print("%s -> %s" % (a.source, a.output), file=sys.stderr)
            return 0
        if a.cmd == "score-panel" and a.field not in PANEL_FIELDS:
            raise MotifError("score-panel: the field must be one of %s" % ", ".join(PANEL_FIELDS))
        bg = None if a.background is None else parse_background(a.background)
        motifs = read_motifs(a.motifs)
        kw = dict(background=bg, profiles=a.profiles is not None, device=a.device, block=a.block)
        if a.cmd == "score":
            folded = load_lmer_table(a.source)
            r = motif_scores(folded, motifs, **kw)
            write_motif_scores(a.output, r)
        else:
            folded = load_lmer_panel(a.source)
            r = motif_scores_with_panel(folded, motifs, **kw)
            write_panel_motif_scores(a.output, folded.names, r, a.field)
        if a.profiles is not None:
            write_motif_profiles(a.profiles, r, folded.L)
        print("%d motifs, %d windows -> %s" % (len(motifs), int(r["width"].sum()) + len(motifs) * (folded.L - 1), a.output),
              file=sys.stderr)
    except (ModelError, dv.GkmError, OSError) as e:
        print("gkmmotifs: error: %s" % e, file=sys.stderr)
        return 1
    return 0


if __name__ == "__main__":
    sys.exit(main())
