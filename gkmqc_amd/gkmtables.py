"""A model folded over its support vectors: l-mer weight tables, per-base importance tables and panels of weight tables
(DESIGN.md §5g, §5j, §5n), their files, and the query operations served from them."""
import os
import time

import numpy as np

from . import device as dv
from .gkmmodel import _ACGT, ModelError
from .gkmquery import (BLOCK_BYTES, _as_queries, _Blocks, _exact_norms, _fit_block, _hyp_finish, _longest,
                       check_explainable, check_queries, explain_shares)


# ------------------------------------------------------------------ l-mer weight tables
TABLE_FORMAT = "gkmqc-lmer-weights-1"
_TABLE_KEYS = ("format", "kernel_type", "L", "k", "d", "M", "H", "rho")
TABLE_PIECE = 1 << 20     # codes per k_lmer_weights launch


def check_table_model(model, what="weights"):
    """The models an l-mer table serves: every model `score` serves except the RBF types, whose score is not linear in
    the query's l-mers."""
    if model.kernel_type in (3, 5):
        raise ModelError("%s: RBF kernels (types 3 and 5) have no l-mer weight table (their score is not linear in the "
                         "query's l-mers)" % what)


def pack_lmers(codes, L):
    """Codes of the l-mers of a base-code array, first base in the highest pair (as the device tables pack them)."""
    codes = np.asarray(codes, dtype=np.uint32)
    n = len(codes) - L + 1
    v = np.zeros(max(n, 0), dtype=np.uint32)
    for i in range(L):
        v = (v << np.uint32(2)) | codes[i:i + n]
    return v


def lmer_rc(u, L):
    """Reverse complements of l-mer codes."""
    u = np.asarray(u, dtype=np.uint32)
    r = np.zeros_like(u)
    for i in range(L):
        r = (r << np.uint32(2)) | (np.uint32(3) - ((u >> np.uint32(2 * i)) & np.uint32(3)))
    return r


def lmer_classes(model, sq):
    """(v, cv): the canonical classes min(f, rc(f)) of the support vectors' forward l-mers f, ascending, and for each the
    sum of dual_coef_s / sq_s * w_s[q] over its occurrences (s, q) in support-vector order, then position order.  sq: the
    support vectors' self norms."""
    L = model.L
    coef = model.dual_coef() / np.asarray(sq, dtype=np.float64)
    lens = np.array([len(s) for s in model.seqs], dtype=np.int64)
    n = lens - L + 1
    codes = np.concatenate(model.seqs)
    starts = np.concatenate(([0], np.cumsum(lens)[:-1]))
    owner = np.repeat(np.arange(model.n_sv), n)
    pos = np.arange(int(n.sum()), dtype=np.int64) - np.repeat(np.cumsum(n) - n, n)
    f = pack_lmers(codes, L)[np.repeat(starts, n) + pos]
    if model.kernel_type in (4, 5):
        wd = dv.distance_weights(model.kernel_type, int(n.max()), model.M, model.H).astype(np.float64)
        w = wd[np.abs(np.repeat(n // 2, n) - pos)]
    else:
        w = np.ones(len(f))
    v, inv = np.unique(np.minimum(f, lmer_rc(f, L)), return_inverse=True)
    cv = np.bincount(inv.reshape(-1), weights=coef[owner] * w, minlength=len(v))
    return v.astype(np.uint32), cv


class _FoldedModel:
    """What the tables a trained model folds into share: the kernel parameters and rho, checked; no support vectors."""

    def _set_params(self, what, kernel_type, L, k, d, M, H, rho, explainable=False):
        self.kernel_type, self.L, self.k, self.d, self.M = int(kernel_type), int(L), int(k), int(d), int(M)
        self.H, self.rho = float(H), float(rho)
        bad = dv.check_parameters(self.kernel_type, self.L, self.k, self.d)
        if bad:
            raise ModelError("kernel parameters rejected: %s" % bad)
        check_table_model(self, what)
        if explainable:
            check_explainable(self, what)
        if not 0 <= self.M <= 255 or not (np.isfinite(self.H) and np.isfinite(self.rho)):
            raise ModelError("M must lie in 0..255, H and rho must be finite")

    def kernel_params(self):
        return (self.kernel_type, self.L, self.k, self.d, self.M, self.H, 1.0)


class LmerTable(_FoldedModel):
    """A trained model folded into one weight per l-mer: W (float64, 4^L, indexed by code, W[u] ==
    W[rc(u)]) plus what scoring needs -- the kernel parameters and rho; no support vectors."""

    def __init__(self, W, kernel_type, L, k, d, M, H, rho):
        self.W = np.ascontiguousarray(W, dtype=np.float64)
        self._set_params("table", kernel_type, L, k, d, M, H, rho)
        if self.W.shape != (4 ** self.L,):
            raise ModelError("a table for L = %d needs 4^L = %d weights" % (self.L, 4 ** self.L))

    # what the drivers that serve a table and a panel alike ask of either (_score_folded, _scan_folded,
    # _saturation_folded, _delta_values)
    cols = ()                                                              # the trailing shape of a result

    def device_weights(self):
        """The host array the launches read."""
        return self.W

    def launcher(self, ctx, name):
        """The context's launch `name` (lmer_score, scan_score, delta_sat or delta_variants) from this table: that method
        itself, called as (..., weights pointer, out pointer, stream)."""
        return getattr(ctx, name)

    def save(self, path):
        """Write the weights file (format: INTEGRATION.md §5b): `# key value` header lines, then LMER<TAB>weight for
        every canonical l-mer in lexicographic ACGT order, with repr() floats."""
        u = canonical_codes(self.L)
        head = [("format", TABLE_FORMAT), ("kernel_type", self.kernel_type), ("L", self.L), ("k", self.k), ("d", self.d),
                ("M", self.M), ("H", repr(self.H)), ("rho", repr(self.rho))]
        tmp = path + ".tmp"
        with open(tmp, "w") as f:
            for key, val in head:
                f.write("# %s %s\n" % (key, val))
            text, weights = lmer_text(u, self.L), self.W[u].tolist()
            for i in range(0, len(u), 1 << 16):
                f.write("".join("%s\t%r\n" % tw for tw in zip(text[i:i + (1 << 16)], weights[i:i + (1 << 16)])))
        os.replace(tmp, path)


def canonical_codes(L):
    """The canonical l-mer codes (u <= rc(u)) in ascending order = lexicographic ACGT order:
    (4^L + 4^(L/2) [L even]) / 2 of them."""
    u = np.arange(4 ** L, dtype=np.uint32)
    return u[u <= lmer_rc(u, L)]


def lmer_text(u, L):
    """l-mer codes -> their ACGT strings"""
    u = np.asarray(u, dtype=np.uint32)
    digits = np.stack([(u >> np.uint32(2 * (L - 1 - i))) & np.uint32(3) for i in range(L)], axis=1).astype(np.uint8)
    return _ACGT[digits].view("S%d" % L).reshape(-1).astype(str).tolist() if len(u) else []


def load_lmer_table(path):
    """Read a weights file written by LmerTable.save; anything malformed raises ModelError with the reason."""
    with open(path) as f:
        lines = f.read().split("\n")
    if lines and lines[-1] == "":
        lines.pop()
    head, i = {}, 0
    while i < len(lines) and lines[i].startswith("#"):
        parts = lines[i].split(" ")
        if len(parts) != 3 or parts[0] != "#" or parts[1] not in _TABLE_KEYS:
            raise ModelError("%s:%d: not a `# key value` line of the header: %r" % (path, i + 1, lines[i]))
        if parts[1] in head:
            raise ModelError("%s:%d: key %s given twice" % (path, i + 1, parts[1]))
        head[parts[1]] = parts[2]
        i += 1
    missing = [key for key in _TABLE_KEYS if key not in head]
    if missing:
        raise ModelError("%s: missing key(s): %s" % (path, ", ".join(missing)))
    if head["format"] != TABLE_FORMAT:
        raise ModelError("%s: format %r, expected %r" % (path, head["format"], TABLE_FORMAT))
    try:
        val = {key: int(head[key]) for key in ("kernel_type", "L", "k", "d", "M")}
        val.update({key: float(head[key]) for key in ("H", "rho")})
    except ValueError as e:
        raise ModelError("%s: %s" % (path, e))
    L = val["L"]
    bad = dv.check_parameters(val["kernel_type"], L, val["k"], val["d"])
    if bad:
        raise ModelError("%s: kernel parameters rejected: %s" % (path, bad))
    body = lines[i:]
    want = len(canonical_codes(L))
    if len(body) != want:
        raise ModelError("%s: %d l-mer lines, expected %d for L = %d" % (path, len(body), want, L))
    pairs = [line.split("\t") for line in body]
    for j, p in enumerate(pairs):
        if len(p) != 2 or len(p[0]) != L:
            raise ModelError("%s:%d: expected an l-mer of %d bases<TAB>weight" % (path, i + 1 + j, L))
    raw = np.frombuffer("".join(p[0] for p in pairs).encode("latin-1", "replace"), dtype=np.uint8).reshape(-1, L)
    lut = np.full(256, 255, dtype=np.uint8)
    lut[_ACGT] = np.arange(4, dtype=np.uint8)
    digits = lut[raw]
    if (digits == 255).any():
        j = int(np.nonzero((digits == 255).any(axis=1))[0][0])
        raise ModelError("%s:%d: an l-mer holds a character other than A, C, G, T" % (path, i + 1 + j))
    u = np.zeros(len(body), dtype=np.uint32)
    for b in range(L):
        u = (u << np.uint32(2)) | digits[:, b].astype(np.uint32)
    rc = lmer_rc(u, L)
    if (u > rc).any():
        j = int(np.nonzero(u > rc)[0][0])
        raise ModelError("%s:%d: %s is not canonical (its reverse complement comes first)" % (path, i + 1 + j, pairs[j][0]))
    order = np.argsort(u, kind="stable")
    rep = np.nonzero(u[order][1:] == u[order][:-1])[0]
    if len(rep):
        j = int(order[rep[0] + 1])
        raise ModelError("%s:%d: l-mer %s given twice" % (path, i + 1 + j, pairs[j][0]))
    try:
        w = np.array([float(p[1]) for p in pairs], dtype=np.float64)
    except ValueError as e:
        raise ModelError("%s: %s" % (path, e))
    W = np.empty(4 ** L, dtype=np.float64)
    W[u] = w
    W[rc] = w
    return LmerTable(W, val["kernel_type"], L, val["k"], val["d"], val["M"], val["H"], val["rho"])


def _fold_table(model, device, on_piece, width, method, coef=None):
    """The support-vector side of `model` folded over all 4^L codes -> float64 host array (4^L, width): the support
    vectors uploaded, their exact self norms, the classes (v, cv) of lmer_classes on the device, then the context's
    `method` (lmer_weights or lmer_importance; coef: its d + 1 coefficients, default c) per piece of TABLE_PIECE codes,
    on_piece after each."""
    import torch
    S, L, d = model.n_sv, model.L, model.d
    ctx = dv.cached_context(*model.kernel_params(), device=device)
    dev = torch.device("cuda", device)
    c = dv.mismatch_weights(model.kernel_type, L, model.k)[:d + 1]
    with torch.cuda.device(dev):
        stream = torch.cuda.current_stream().cuda_stream
        ctx.set_sequences(model.flat_seqs(), stream)
        sq = torch.empty(S, dtype=torch.float64, device=dev)
        _exact_norms(ctx, S, c, sq, stream)
        v, cv = lmer_classes(model, sq.cpu().numpy())
        d_v = torch.from_numpy(v.view(np.int32)).to(dev)
        d_cv = torch.from_numpy(cv).to(dev)
        out = torch.empty((4 ** L, width), dtype=torch.float64, device=dev)
        for u0 in range(0, 4 ** L, TABLE_PIECE):
            u1 = min(4 ** L, u0 + TABLE_PIECE)
            getattr(ctx, method)(c if coef is None else coef, d_v.data_ptr(), d_cv.data_ptr(), len(v), u0, u1,
                                 out.data_ptr() + 8 * width * u0, stream)
            if on_piece is not None:
                on_piece(dict(codes=u1 - u0, classes=len(v), kernel_ms=ctx.last_kernel_ms(),
                              comparisons=ctx.last_comparisons(), kernel=ctx.last_kernel_name()))
        return out.cpu().numpy()


def lmer_weights(model, device=0, on_piece=None):
    """The l-mer weight table of `model` -> LmerTable:

        W(u) = sum_s (dual_coef_s / sq_s) sum_q w_s[q] (c[m(u, f_q)] + c[m(u, rc(f_q))])      (c[m] = 0 for m > d)

    so that score(x) = sum_p w_x[p] W(u_p) / sq_x + rho on the no-wrap domain (sq_s from exact 64-bit
    self profiles, so beyond it the table holds the exact model where `score` follows the reference's wrap).  Every model `score` serves except RBF (types 3 and 5), k = 0
    included.  The support vectors' self norms come from one gkmhip_self_profiles launch, the classes (v, cv) from the host
    (lmer_classes), W from k_lmer_weights over all 4^L codes in pieces of TABLE_PIECE.  on_piece(dict) (measurements):
    called after every piece with its codes, kernel milliseconds (HIP events) and l-mer comparisons."""
    check_table_model(model)
    Wh = _fold_table(model, device, on_piece, 1, "lmer_weights").reshape(-1)
    return LmerTable(Wh, model.kernel_type, model.L, model.k, model.d, model.M, model.H, model.rho)


def default_table_block(max_len, budget=BLOCK_BYTES):
    """Queries per block: the upload's per-sequence device tables (sized by the longest query, a few words per base)
    within `budget` bytes, and at most 32 768 (about `score`'s blocks of support vectors and queries together)."""
    return _fit_block(max_len, 32, budget, cap=1 << 15)


def score_with_table(table, fasta_or_sequences, device=0, block=None, on_block=None):
    """Decision values from an l-mer weight table for a FASTA file (or a list / FlatSequences of base codes) -> (names,
    scores): sum_p w_x[p] W(u_p) / sq_x + rho, `score`'s value up to rounding on the no-wrap domain (INTEGRATION.md §5b;
    beyond it the exact score).  Only the queries are uploaded: per block the exact self norms (gkmhip_self_profiles) and one gather per l-mer (k_lmer_score); bit-identical for every block size.
    on_block(dict) (measurements): called after every block with its size, k_lmer_score's milliseconds and the block's
    wall time."""
    return _score_folded(table, fasta_or_sequences, device, block, on_block)


def _models(cols):
    """what a panel's measurement dicts hold beside the table's"""
    return dict(models=cols[0]) if cols else {}


def _per_item(v, cols):
    """a vector of one value per item (numpy or torch), broadcastable against (items,) + cols"""
    return v.reshape((-1,) + (1,) * len(cols))


def _rho_operand(folded, dev):
    """rho as the epilogues add it: a table's float as it is, a panel's (n_models,) on the device"""
    import torch
    return torch.from_numpy(folded.rho).to(dev) if folded.cols else folded.rho


def _score_folded(folded, fasta_or_sequences, device, block, on_block):
    """The body `score_with_table` and `score_with_panel` share -> (names, scores (Q,) + folded.cols).  folded: the table
    or panel (checked)."""
    import torch
    seqs, names = _as_queries(fasta_or_sequences)
    check_queries(folded, seqs)
    blocks = _Blocks(folded, seqs, device, block, default_table_block(_longest(seqs)), exact=True)
    ctx, sq, dev, cols = blocks.ctx, blocks.sq, blocks.dev, folded.cols
    out = np.empty((len(seqs),) + cols)
    with torch.cuda.device(dev):
        W = torch.from_numpy(folded.device_weights()).to(dev)
        rho = _rho_operand(folded, dev)
        T = torch.empty((blocks.qb_max,) + cols, dtype=torch.float64, device=dev)
        launch = folded.launcher(ctx, "lmer_score")
        for b in blocks:
            launch(0, b.qb, W.data_ptr(), T.data_ptr(), blocks.stream)
            out[b.q0:b.q1] = (T[:b.qb] / _per_item(sq[:b.qb], cols) + rho).cpu().numpy()
            if on_block is not None:
                on_block(dict(queries=b.qb, **_models(cols), score_kernel_ms=ctx.last_kernel_ms(),
                              lmers=ctx.last_comparisons(), kernel=ctx.last_kernel_name(),
                              wall_ms=(time.perf_counter() - b.t0) * 1e3))
    return names, out


# ------------------------------------------------------------------ per-base importance tables
IMPORTANCE_FORMAT = "gkmqc-lmer-importance-1"
_IMPORTANCE_INTS = ("kernel_type", "L", "k", "d", "M")
_IMPORTANCE_FLOATS = ("H", "rho")
_IMPORTANCE_KEYS = ("format",) + _IMPORTANCE_INTS + _IMPORTANCE_FLOATS + ("V",)


class LmerImportanceTable(_FoldedModel):
    """A trained model folded into one value per (l-mer, offset): V (float64, (4^L, L), indexed by code
    and by the offset from the l-mer's first base; V[rc(u), L-1-i] == V[u, i] and V.sum(1) is the weight table's W) plus
    what explaining needs -- the kernel parameters and rho; no support vectors."""

    def __init__(self, V, kernel_type, L, k, d, M, H, rho):
        self._set_params("importance table", kernel_type, L, k, d, M, H, rho, explainable=True)
        self.V = np.ascontiguousarray(V, dtype=np.float64)
        if self.V.shape != (4 ** self.L, self.L):
            raise ModelError("an importance table for L = %d needs (4^L, L) = (%d, %d) values"
                             % (self.L, 4 ** self.L, self.L))

    def save(self, path):
        """Write the table file (format: INTEGRATION.md §5b) to exactly `path`: an uncompressed .npz with the format
        tag, the scalar parameters and the rows of the canonical l-mers in ascending order (the other half follows from
        V[rc(u), L-1-i] == V[u, i])."""
        head = {key: np.int64(getattr(self, key)) for key in _IMPORTANCE_INTS}
        head.update({key: np.float64(getattr(self, key)) for key in _IMPORTANCE_FLOATS})
        tmp = path + ".tmp"
        with open(tmp, "wb") as f:
            np.savez(f, format=np.array(IMPORTANCE_FORMAT), V=self.V[canonical_codes(self.L)], **head)
        os.replace(tmp, path)


def load_importance_table(path):
    """Read a table file written by LmerImportanceTable.save; anything malformed raises ModelError with the reason."""
    with open(path, "rb") as f:
        try:
            with np.load(f, allow_pickle=False) as z:
                got = {key: z[key] for key in z.files}
        except Exception as e:   # (not a zip archive, a truncated member, a pickled object, ...)
            raise ModelError("%s: not an importance table file: %s" % (path, e))
    missing = [key for key in _IMPORTANCE_KEYS if key not in got]
    if missing:
        raise ModelError("%s: missing key(s): %s" % (path, ", ".join(missing)))
    extra = [key for key in got if key not in _IMPORTANCE_KEYS]
    if extra:
        raise ModelError("%s: key(s) %s do not belong to format %s" % (path, ", ".join(extra), IMPORTANCE_FORMAT))
    fmt = got["format"]
    if fmt.shape != () or fmt.dtype.kind != "U" or str(fmt) != IMPORTANCE_FORMAT:
        raise ModelError("%s: format %r, expected %r" % (path, fmt.tolist(), IMPORTANCE_FORMAT))
    val = {}
    for key, kinds in [(key, "iu") for key in _IMPORTANCE_INTS] + [(key, "f") for key in _IMPORTANCE_FLOATS]:
        if got[key].shape != () or got[key].dtype.kind not in kinds:
            raise ModelError("%s: %s must be one %s" % (path, key, "integer" if kinds == "iu" else "float"))
        val[key] = got[key].item()
    L = val["L"]
    bad = dv.check_parameters(val["kernel_type"], L, val["k"], val["d"])
    if bad:
        raise ModelError("%s: kernel parameters rejected: %s" % (path, bad))
    can = canonical_codes(L)
    Vc = got["V"]
    if Vc.dtype != np.float64 or Vc.shape != (len(can), L):
        raise ModelError("%s: V is %s %r, expected float64 (%d, %d): one row per canonical l-mer of L = %d"
                         % (path, Vc.dtype, Vc.shape, len(can), L, L))
    rc = lmer_rc(can, L)
    pal = can == rc
    if Vc[pal].tobytes() != Vc[pal][:, ::-1].tobytes():
        raise ModelError("%s: the row of a palindromic l-mer is not its own mirror image" % path)
    V = np.empty((4 ** L, L), dtype=np.float64)
    V[rc] = Vc[:, ::-1]
    V[can] = Vc
    try:
        return LmerImportanceTable(V, val["kernel_type"], L, val["k"], val["d"], val["M"], val["H"], val["rho"])
    except ModelError as e:
        raise ModelError("%s: %s" % (path, e))


def lmer_importance(model, device=0, on_piece=None):
    """The per-base importance table of `model` -> LmerImportanceTable:

        V(u, i) = sum over classes (v, cv) of cv (share[m(u, v)] [u[i] == v[i]] + share[m(u, rc v)] [u[i] == rc(v)[i]])

    with lmer_weights' classes and self norms and explain's shares, so that explain(x)[t] = sum_i w_x[t-i] V(u_{t-i}, i)
    / sq_x up to rounding.  The models `explain` serves (no RBF, no k = 0), checked before the device is touched.  V comes
    from k_lmer_importance over all 4^L codes in pieces of TABLE_PIECE.  on_piece(dict) (measurements): called after
    every piece with its codes, kernel milliseconds (HIP events) and l-mer comparisons."""
    check_explainable(model, "lmer_importance")
    Vh = _fold_table(model, device, on_piece, model.L, "lmer_importance", explain_shares(model))
    return LmerImportanceTable(Vh, model.kernel_type, model.L, model.k, model.d, model.M, model.H, model.rho)


def default_imptable_block(max_len, d=None, budget=BLOCK_BYTES):
    """Queries per block of explain_with_table (d None) or hypothetical_with_table: the upload's per-sequence device
    tables and the per-base output -- for the hypothetical table also the mutants' self profiles (4 (d + 1) int64 per
    base) and the finishing temporaries -- within `budget` bytes, and at most 32 768 (as default_table_block)."""
    per_base = 40 if d is None else 8 * (4 * (int(d) + 1) + 28)
    return _fit_block(max_len, per_base, budget, cap=1 << 15)


def explain_with_table(itable, fasta_or_sequences, device=0, block=None, on_block=None):
    """Per-base importance from an importance table for a FASTA file (or a list / FlatSequences of base codes) ->
    (names, [float64 array of one value per base, per query]): sum_i w_x[t-i] V(u_{t-i}, i) / sq_x, `explain`'s value up
    to rounding.  Only the queries are uploaded: per block the exact self norms (gkmhip_self_profiles) and L gathers per
    base (k_lmer_explain); bit-identical for every block size.  on_block(dict) (measurements): called after every block
    with its size, k_lmer_explain's milliseconds and the block's wall time."""
    import torch
    seqs, names = _as_queries(fasta_or_sequences)
    check_queries(itable, seqs)
    blocks = _Blocks(itable, seqs, device, block, default_imptable_block(_longest(seqs)), exact=True)
    ctx, sq, dev = blocks.ctx, blocks.sq, blocks.dev
    out = []
    with torch.cuda.device(dev):
        V = torch.from_numpy(itable.V).to(dev)
        E = torch.empty(blocks.most_bases(), dtype=torch.float64, device=dev)
        for b in blocks:
            xscale = 1.0 / sq[:b.qb]
            ctx.lmer_explain(0, b.qb, V.data_ptr(), xscale.data_ptr(), E.data_ptr(), blocks.stream)
            out.extend(b.split(E[:b.nb].cpu().numpy()))
            if on_block is not None:
                on_block(dict(queries=b.qb, explain_kernel_ms=ctx.last_kernel_ms(), gathers=ctx.last_comparisons(),
                              kernel=ctx.last_kernel_name(), wall_ms=(time.perf_counter() - b.t0) * 1e3))
    return names, out


def hypothetical_with_table(itable, fasta_or_sequences, device=0, block=None, on_block=None):
    """Hypothetical importance from an importance table for a FASTA file (or a list / FlatSequences of base codes) ->
    (names, [float64 array (T, 4) per query], columns A, C, G, T): hyp[t, b] = explain_with_table(y)[t] for y = x with
    base t set to b, bit for bit (hyp[t, x[t]] = explain_with_table(x)[t]), and `hypothetical`'s value up to rounding.
    Only the queries are uploaded: per block their exact self norms, every mutant's self profile
    (gkmhip_ism_self_profiles) and 4 L gathers per base (k_lmer_hyp); bit-identical for every block size.
    on_block(dict) (measurements): called after every block with its size, k_lmer_hyp's milliseconds, the self-profile
    kernels' milliseconds and the block's wall time."""
    import torch
    seqs, names = _as_queries(fasta_or_sequences)
    check_queries(itable, seqs)
    d = itable.d
    blocks = _Blocks(itable, seqs, device, block, default_imptable_block(_longest(seqs), d), exact=True)
    ctx, sq, dev, stream = blocks.ctx, blocks.sq, blocks.dev, blocks.stream
    c = blocks.c
    out = []
    with torch.cuda.device(dev):
        V = torch.from_numpy(itable.V).to(dev)
        most = blocks.most_bases()
        R = torch.empty((most, 4), dtype=torch.float64, device=dev)
        prof = torch.empty((most, 4, d + 1), dtype=torch.int64, device=dev)
        for b in blocks:
            qb = b.qb
            ctx.ism_self_profiles(0, qb, prof.data_ptr(), stream)
            self_ms = ctx.last_kernel_ms() if on_block is not None else None
            xscale = 1.0 / sq[:qb]
            ctx.lmer_hyp(0, qb, V.data_ptr(), R.data_ptr(), stream)
            out.extend(_hyp_finish(b, R, prof, c, xscale, dev))
            if on_block is not None:
                on_block(dict(queries=qb, hyp_kernel_ms=ctx.last_kernel_ms(), gathers=ctx.last_comparisons(),
                              kernel=ctx.last_kernel_name(), self_kernels_ms=self_ms,
                              wall_ms=(time.perf_counter() - b.t0) * 1e3))
    return names, out


# ------------------------------------------------------------------ l-mer weight panels
PANEL_FORMAT = "gkmqc-lmer-panel-1"
PANEL_MAX_MODELS = 64           # models of a panel (GKMHIP_PANEL_MAX): one wave's lanes across the models of a row
PANEL_MAX_BYTES = 8 << 30       # the device image 4^L * ms * 8 of a panel, at most: 64 models at L = 12 just fit
_PANEL_SHARED = ("kernel_type", "L", "k", "d", "M", "H")
_PANEL_INTS = ("kernel_type", "L", "k", "d", "M")
_PANEL_KEYS = ("format",) + _PANEL_SHARED + ("names", "rho", "W")
_PANEL_LAUNCH = dict(lmer_score="panel_score", scan_score="panel_scan_score", delta_sat="panel_delta_sat",
                     delta_variants="panel_delta_variants")    # a table's launch -> the panel's (LmerPanel.launcher)


def panel_row_stride(n_models):
    """Doubles per row of a panel's device image: n_models rounded up to a multiple of 8 (rows of whole 64-byte lines)."""
    return (int(n_models) + 7) // 8 * 8


def _check_panel_names(names, n_models):
    names = list(names)
    if len(names) != n_models:
        raise ModelError("panel: %d names for %d members" % (len(names), n_models))
    for i, name in enumerate(names):
        if not isinstance(name, str) or not name or "\t" in name or "\n" in name:
            raise ModelError("panel: the name of member %d must be a non-empty string without tab or newline: %r"
                             % (i, name))
        if name in names[:i]:
            raise ModelError("panel: the name %r is given to members %d and %d" % (name, names.index(name), i))
    return names


def _check_panel_size(L, n_models):
    """The refusals that precede every allocation of a panel: the number of members and the bytes of the device image."""
    if not 1 <= n_models <= PANEL_MAX_MODELS:
        raise ModelError("panel: %d members; a panel holds 1..%d tables" % (n_models, PANEL_MAX_MODELS))
    size = 4 ** int(L) * panel_row_stride(n_models) * 8
    if size > PANEL_MAX_BYTES:
        raise ModelError("panel: %d tables of L = %d take %d bytes on the device, above PANEL_MAX_BYTES = %d"
                         % (n_models, L, size, PANEL_MAX_BYTES))


class LmerPanel(_FoldedModel):
    """1..64 l-mer weight tables that share (kernel_type, L, k, d, M, H), served together: W (float64,
    (4^L, n_models), C-contiguous: column m is table m's W), rho (n_models,), names (unique).  n_models is the panel
    size; M stays the wgkm distance parameter."""

    def __init__(self, tables, names=None):
        tables = list(tables)
        for i, t in enumerate(tables):
            if not isinstance(t, LmerTable):
                raise ModelError("panel: member %d is no l-mer weight table (gkmpredict weights)" % i)
        if not tables:
            raise ModelError("panel: 0 members; a panel holds 1..%d tables" % PANEL_MAX_MODELS)
        names = _check_panel_names(["table%d" % i for i in range(len(tables))] if names is None else names, len(tables))
        for i, t in enumerate(tables):
            check_table_model(t, "panel: member %d (%s)" % (i, names[i]))
            for key in _PANEL_SHARED:
                if getattr(t, key) != getattr(tables[0], key):
                    raise ModelError("panel: member %d (%s) has %s = %r where member 0 (%s) has %r; the members must share %s"
                                     % (i, names[i], key, getattr(t, key), names[0], getattr(tables[0], key),
                                        ", ".join(_PANEL_SHARED)))
        _check_panel_size(tables[0].L, len(tables))
        self._fill(np.stack([t.W for t in tables], axis=1), names, [t.rho for t in tables],
                   *(getattr(tables[0], key) for key in _PANEL_SHARED))

    def _fill(self, W, names, rho, kernel_type, L, k, d, M, H):
        self._set_params("panel", kernel_type, L, k, d, M, H, 0.0)
        self.names, self.n_models = list(names), len(names)
        self.rho = np.ascontiguousarray(rho, dtype=np.float64)
        self.W = np.ascontiguousarray(W, dtype=np.float64)
        if self.rho.shape != (self.n_models,) or not np.isfinite(self.rho).all():
            raise ModelError("panel: rho must be %d finite values" % self.n_models)
        if self.W.shape != (4 ** self.L, self.n_models):
            raise ModelError("panel: W must be (4^L, n_models) = (%d, %d)" % (4 ** self.L, self.n_models))

    def table(self, m):
        """Member m as an LmerTable of its own (a copy of its column)."""
        return LmerTable(self.W[:, m], self.kernel_type, self.L, self.k, self.d, self.M, self.H, float(self.rho[m]))

    def device_rows(self):
        """The device image: float64 (4^L, ms), ms = panel_row_stride(n_models); columns n_models.. are zero.  W itself
        (no copy; read only) where n_models is a multiple of 8."""
        if panel_row_stride(self.n_models) == self.n_models:
            return self.W
        P = np.zeros((4 ** self.L, panel_row_stride(self.n_models)), dtype=np.float64)
        P[:, :self.n_models] = self.W
        return P

    # LmerTable's members for the shared drivers: the model index is the last axis of every result
    cols = property(lambda self: (self.n_models,))
    device_weights = device_rows

    def launcher(self, ctx, name):
        """LmerTable.launcher's counterpart, called the same way: the context's panel launch with n_models and the row
        stride bound behind the weights pointer."""
        method, nm, ms = getattr(ctx, _PANEL_LAUNCH[name]), self.n_models, panel_row_stride(self.n_models)
        return lambda *args: method(*args[:-2], nm, ms, *args[-2:])

    def save(self, path):
        """Write the panel file (format: INTEGRATION.md §5b) to exactly `path`: an uncompressed .npz with the format tag,
        the six shared parameters, names, rho and the rows of the canonical l-mers in ascending order (W[rc(u)] ==
        W[u] gives the other half)."""
        head = {key: np.int64(getattr(self, key)) for key in _PANEL_INTS}
        tmp = path + ".tmp"
        with open(tmp, "wb") as f:
            np.savez(f, format=np.array(PANEL_FORMAT), H=np.float64(self.H), names=np.array(self.names, dtype=np.str_),
                     rho=self.rho, W=self.W[canonical_codes(self.L)], **head)
        os.replace(tmp, path)


def load_lmer_panel(path):
    """Read a panel file written by LmerPanel.save; anything malformed raises ModelError with the reason."""
    with open(path, "rb") as f:
        try:
            with np.load(f, allow_pickle=False) as z:
                got = {key: z[key] for key in z.files}
        except Exception as e:   # (not a zip archive, a truncated member, a pickled object, ...)
            raise ModelError("%s: not a panel file: %s" % (path, e))
    missing = [key for key in _PANEL_KEYS if key not in got]
    if missing:
        raise ModelError("%s: missing key(s): %s" % (path, ", ".join(missing)))
    extra = [key for key in got if key not in _PANEL_KEYS]
    if extra:
        raise ModelError("%s: key(s) %s do not belong to format %s" % (path, ", ".join(extra), PANEL_FORMAT))
    fmt = got["format"]
    if fmt.shape != () or fmt.dtype.kind != "U" or str(fmt) != PANEL_FORMAT:
        raise ModelError("%s: format %r, expected %r" % (path, fmt.tolist(), PANEL_FORMAT))
    val = {}
    for key, kinds in [(key, "iu") for key in _PANEL_INTS] + [("H", "f")]:
        if got[key].shape != () or got[key].dtype.kind not in kinds:
            raise ModelError("%s: %s must be one %s" % (path, key, "integer" if kinds == "iu" else "float"))
        val[key] = got[key].item()
    L = val["L"]
    bad = dv.check_parameters(val["kernel_type"], L, val["k"], val["d"])
    if bad:
        raise ModelError("%s: kernel parameters rejected: %s" % (path, bad))
    names, rho, Wc = got["names"], got["rho"], got["W"]
    if names.ndim != 1 or names.dtype.kind != "U":
        raise ModelError("%s: names is %s %r, expected one string per member" % (path, names.dtype, names.shape))
    n = len(names)
    try:
        _check_panel_size(L, n)
        if rho.dtype != np.float64 or rho.shape != (n,):
            raise ModelError("rho is %s %r, expected float64 (%d,): one per member" % (rho.dtype, rho.shape, n))
        if not np.isfinite(rho).all():
            raise ModelError("rho of member %d is not finite" % int(np.flatnonzero(~np.isfinite(rho))[0]))
        can = canonical_codes(L)
        if Wc.dtype != np.float64 or Wc.shape != (len(can), n):
            raise ModelError("W is %s %r, expected float64 (%d, %d): one row per canonical l-mer of L = %d, one column per "
                             "member" % (Wc.dtype, Wc.shape, len(can), n, L))
        names = _check_panel_names(names.tolist(), n)
        W = np.empty((4 ** L, n), dtype=np.float64)
        W[lmer_rc(can, L)] = Wc
        W[can] = Wc
        panel = LmerPanel.__new__(LmerPanel)
        panel._fill(W, names, rho, val["kernel_type"], L, val["k"], val["d"], val["M"], val["H"])
    except ModelError as e:
        raise ModelError("%s: %s" % (path, e))
    return panel


def _check_folded(want, what, folded):
    """What every function that takes a table (want: LmerTable) or a panel (LmerPanel) refuses first: anything else."""
    if not isinstance(folded, want):
        raise ModelError("%s: needs an l-mer weight table (gkmpredict weights), not a model" % what if want is LmerTable else
                         "%s: needs an l-mer weight panel (gkmpredict panel), not a table or a model" % what)
    check_table_model(folded, what)


def check_panel(panel, what):
    """What every panel function refuses first: a table or a model where a panel is needed."""
    _check_folded(LmerPanel, what, panel)


def score_with_panel(panel, fasta_or_sequences, device=0, block=None, on_block=None):
    """score_with_table for every member of a panel -> (names, scores (Q, n_models)): column m is score_with_table's
    result for member m, bit for bit, whatever the block size.  Per block the exact self norms once (they depend on the
    shared parameters only) and one k_panel_score launch: one row read per l-mer for all models.
    on_block(dict) (measurements): score_with_table's keys and `models`."""
    check_panel(panel, "predict-panel")
    return _score_folded(panel, fasta_or_sequences, device, block, on_block)


def _panel_row(lead, values):
    return "\t".join(lead + ["nan" if x != x else "%.17g" % x for x in values]) + "\n"


def write_panel_scores(path, panel_names, names, scores):
    """The `predict-panel` output: the header #name<TAB>member names, then name<TAB>one score per member at %.17g."""
    with open(path, "w") as f:
        f.write("#" + "\t".join(["name"] + list(panel_names)) + "\n")
        for name, row in zip(names, np.asarray(scores, dtype=np.float64).tolist()):
            f.write(_panel_row([str(name)], row))


def read_panel_output(path, nlead):
    """-> (member names, [the nlead leading columns of each row], float64 (rows, n_models)) from a file written by
    write_panel_scores (nlead = 1), write_panel_scan (3) or write_panel_delta (4, or 5 with ids)."""
    with open(path) as f:
        lines = f.read().split("\n")[:-1]
    if not lines or not lines[0].startswith("#"):
        raise ModelError("%s: no header line" % path)
    head = lines[0][1:].split("\t")
    leads, values = [], []
    nm = len(head) - int(nlead)
    for line in lines[1:]:
        fields = line.split("\t")
        leads.append(tuple(fields[:-nm]))
        values.append([float(x) for x in fields[-nm:]])
    return head[nlead:], leads, np.array(values, dtype=np.float64).reshape(len(values), nm)
