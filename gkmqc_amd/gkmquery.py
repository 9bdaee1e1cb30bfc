"""What a model answers about a file of queries, one block loop for all of it: score, explain, ism, mutant_scores and
hypothetical, with their default blocks, readers and writers."""
import os
import time

import numpy as np

from . import device as dv
from . import svmcv
from .gkmmodel import Model, ModelError

BLOCK_BYTES = 2 << 30     # device memory one block of queries may take: S x Qb kernel values + the kernel's own output


# ------------------------------------------------------------------ scoring
def _fit_block(unit, unit_bytes, budget, cap=1 << 20):
    """Queries per block when one query takes `unit_bytes` of device memory per unit of `unit` (support vectors, or bases
    of the longest query; counted as at least 64): what fits in `budget` bytes, at least 1 and at most `cap`."""
    return int(max(1, min(cap, budget // (unit_bytes * max(int(unit), 64)))))


def default_block(n_sv, budget=BLOCK_BYTES):
    """Queries per block: the S x Qb kernel values and the Gram kernel's tile-transposed output (about as big) within
    `budget` bytes of device memory, whatever the number of queries."""
    return _fit_block(n_sv, 16, budget)


def _as_queries(fasta_or_sequences):
    if isinstance(fasta_or_sequences, (str, bytes, os.PathLike)):
        seqs, names, _, _ = dv.read_fasta(fasta_or_sequences)
        return seqs, names
    seqs = fasta_or_sequences
    if not isinstance(seqs, dv.FlatSequences):
        seqs = [np.asarray(s, dtype=np.uint8) for s in seqs]
        lens = np.array([len(s) for s in seqs], dtype=np.int64)
        off = np.zeros(len(seqs) + 1, dtype=np.int64)
        np.cumsum(lens, out=off[1:])
        seqs = dv.FlatSequences(np.concatenate(seqs) if seqs else np.zeros(0, np.uint8), off)
    return seqs, ["seq%d" % i for i in range(len(seqs))]


def check_queries(model, seqs):
    if len(seqs) == 0:
        raise ModelError("no query sequences")
    short = np.nonzero(np.diff(seqs.off) < model.L)[0]
    if len(short):
        raise ModelError("query %d is shorter than L = %d" % (int(short[0]), model.L))


class _Block:
    """Queries [q0, q1) of a _Blocks run: qb of them with nb bases, `codes`; qoff their qb + 1 offsets into seqs.codes.
    t0 / t1: the clock before / after the block's upload."""

    def __init__(self, seqs, q0, q1):
        self.q0, self.q1, self.qb = q0, q1, q1 - q0
        self.qoff = seqs.off[q0:q1 + 1]
        self.codes = seqs.codes[self.qoff[0]:self.qoff[-1]]
        self.nb = len(self.codes)

    def split(self, host):
        """One value (or row) per base of the block -> one array per query."""
        return np.split(host, (self.qoff[1:-1] - self.qoff[0]).astype(np.int64))


class _Blocks:
    """`model` serving the queries `seqs` (checked) in blocks of at most qb_max = `block`, or `default`, queries.  Iterating
    uploads, per block, [the S support vectors; the block's queries] into the model's cached context `ctx` (an LmerTable
    has no support vectors: S = 0), takes that set's self norms into `sq` (S + qb_max doubles on `dev`) and yields the
    _Block.  `rows`: the support vectors' sequence indices; `stream`: the current stream of `dev`, which every call takes.
    exact: the norms come from the exact 64-bit self profiles (_exact_norms) instead of gkmhip_self_norms, whose 32-bit
    profiles wrap like the reference's; the same doubles wherever no profile reaches 2^31."""

    def __init__(self, model, seqs, device, block, default, exact=False):
        import torch
        self.seqs = seqs
        self.qb_max = min(len(seqs), int(block) if block else default)
        if self.qb_max < 1:
            raise ModelError("block must be at least 1")
        self.ctx = dv.cached_context(*model.kernel_params(), device=device)
        self.sv = model.flat_seqs() if isinstance(model, Model) else None
        self.S = len(self.sv) if self.sv else 0
        self.rows = np.arange(self.S, dtype=np.int32)
        self.dev = torch.device("cuda", device)
        self.stream = torch.cuda.current_stream(self.dev).cuda_stream
        self.sq = torch.empty(self.S + self.qb_max, dtype=torch.float64, device=self.dev)
        self.c = dv.mismatch_weights(model.kernel_type, model.L, model.k)[:model.d + 1] if exact else None

    def most_bases(self):
        """The bases of the largest block: what a per-base output buffer must hold."""
        off, Q = self.seqs.off, len(self.seqs)
        return max(int(off[min(Q, q0 + self.qb_max)] - off[q0]) for q0 in range(0, Q, self.qb_max))

    def __iter__(self):
        for q0 in range(0, len(self.seqs), self.qb_max):
            t0 = time.perf_counter()
            b = _Block(self.seqs, q0, min(len(self.seqs), q0 + self.qb_max))
            b.t0 = t0
            codes, off = b.codes, b.qoff - b.qoff[0]
            if self.S:
                codes = np.concatenate((self.sv.codes, codes))
                off = np.concatenate((self.sv.off, self.sv.off[-1] + off[1:]))
            self.ctx.set_sequences(dv.FlatSequences(codes, off), self.stream)     # (complete on return)
            b.t1 = time.perf_counter()
            if self.c is None:
                self.ctx.self_norms(self.sq.data_ptr(), self.stream)
            else:
                _exact_norms(self.ctx, self.S + b.qb, self.c, self.sq, self.stream)
            yield b


def _exact_norms(ctx, n, c, sq, stream):
    """sq[:n] = sqrt(sum_m c_m P_m(x, x)) of the first n uploaded sequences from their exact int64 self profiles
    (gkmhip_self_profiles), in ascending m from 0.0 as the oracle forms it: bit for bit gkmhip_self_norms' value while
    every P_m is below 2^31, and the true norm beyond, where the 32-bit profiles of gkmhip_self_norms wrap."""
    import torch
    pself = torch.empty((n, len(c)), dtype=torch.int64, device=sq.device)
    ctx.self_profiles(0, n, pself.data_ptr(), stream)
    sq[:n] = _norms_from_profiles(pself, c)


def _norms_from_profiles(pself, c):
    """sqrt(sum_m c_m P_m) of every row of the (rows, d + 1) int64 device profiles `pself`, in ascending m from 0.0: the
    one epilogue of _exact_norms and `scan`, so that both form the same double from the same profile."""
    import torch
    g = torch.zeros(pself.shape[0], dtype=torch.float64, device=pself.device)
    for m in range(len(c)):
        g.add_(pself[:, m].double().mul_(float(c[m])))
    return g.sqrt_()


def score(model, fasta_or_sequences, device=0, block=None, kernel=dv.KERNEL_AUTO, on_block=None):
    """Decision values of `model` for a FASTA file (or a list / FlatSequences of base codes) -> (names, scores):
    scikit-learn's `decision_function` sign, positive = like the positive set.  block: queries per device block
    (default_block).  on_block(dict) (measurements): called after every block with its size and timings."""
    import torch
    seqs, names = _as_queries(fasta_or_sequences)
    check_queries(model, seqs)
    lib = svmcv._lib()
    blocks = _Blocks(model, seqs, device, block, default_block(model.n_sv))
    ctx, S, rows, qb_max, sq, dev, stream = (blocks.ctx, blocks.S, blocks.rows, blocks.qb_max, blocks.sq, blocks.dev,
                                             blocks.stream)
    ctx.set_kernel(kernel)
    out = np.empty(len(seqs))
    with torch.cuda.device(dev):
        G = torch.empty((S, qb_max), dtype=torch.float64, device=dev)
        d_idx = torch.from_numpy(rows).to(dev)
        d_alpha = torch.from_numpy(model.alpha).to(dev)
        # (SVR: LIBSVM's rho, which scikit-learn's predict takes as -intercept_)
        d_rho = torch.tensor([-model.rho if model.is_svr else model.rho], dtype=torch.float64, device=dev)
        d_test = torch.arange(qb_max, dtype=torch.int32, device=dev)
        d_dec = torch.empty(qb_max, dtype=torch.float64, device=dev)
        off_sv = np.array([0, S], dtype=np.int64)
        n0 = np.array([model.n0], dtype=np.int32)
        for b in blocks:
            qb = b.qb
            ctx.gram_block(rows, S, S + qb, G.data_ptr(), qb_max, stream)
            if on_block is not None:
                torch.cuda.current_stream().synchronize()
            t2 = time.perf_counter()
            gram_ms = ctx.last_kernel_ms() if on_block is not None else None
            ctx.normalize_block(rows, S, S + qb, G.data_ptr(), qb_max, sq.data_ptr(), stream)
            if on_block is not None:
                torch.cuda.current_stream().synchronize()
            t3 = time.perf_counter()
            if model.is_svr:   # scikit-learn's SVR.predict: the signed sum in support-vector order, minus rho
                rc = lib.gkmsvm_decision_signed_batch(device, G.data_ptr(), qb_max, 1, d_idx.data_ptr(),
                                                      off_sv.ctypes.data, d_alpha.data_ptr(), d_rho.data_ptr(),
                                                      d_test.data_ptr(), np.array([0, qb], dtype=np.int64).ctypes.data,
                                                      d_dec.data_ptr(), stream)
                if rc:
                    raise svmcv.SvmError("gkmsvm_decision_signed_batch: %s" % lib.gkmsvm_last_error().decode())
                out[b.q0:b.q1] = d_dec[:qb].cpu().numpy()
            else:
                rc = lib.gkmsvm_decision_batch(device, G.data_ptr(), qb_max, 1, d_idx.data_ptr(), off_sv.ctypes.data,
                                               n0.ctypes.data, d_alpha.data_ptr(), d_rho.data_ptr(), d_test.data_ptr(),
                                               np.array([0, qb], dtype=np.int64).ctypes.data, d_dec.data_ptr(), stream)
                if rc:
                    raise svmcv.SvmError("gkmsvm_decision_batch: %s" % lib.gkmsvm_last_error().decode())
                # LIBSVM's decision value for labels (0, 1) has the opposite sign of scikit-learn's
                out[b.q0:b.q1] = -d_dec[:qb].cpu().numpy()
            t4 = time.perf_counter()
            if on_block is not None:
                on_block(dict(queries=qb, upload_ms=(b.t1 - b.t0) * 1e3, norms_gram_ms=(t2 - b.t1) * 1e3,
                              gram_kernel_ms=gram_ms, normalize_ms=(t3 - t2) * 1e3, decision_ms=(t4 - t3) * 1e3,
                              wall_ms=(t4 - b.t0) * 1e3, comparisons=ctx.last_comparisons(),
                              kernel=ctx.last_kernel_name()))
    return names, out


def _longest(seqs):
    return int(np.diff(seqs.off).max())


def write_scores(path, names, scores):
    """The `predict` (and `predict-table`) output: one line per query, name<TAB>score with a repr() float."""
    with open(path, "w") as f:
        for name, s in zip(names, scores):
            f.write("%s\t%r\n" % (name, float(s)))


# ------------------------------------------------------------------ per-base importance
EXPLAIN_CHUNKS = 16       # the most partial rows gkmhip_explain_block keeps per base (one per chunk of support vectors)


def check_explainable(model, what="explain"):
    """The models `explain` (and `hypothetical`) serves: not the RBF types (exp() breaks completeness) and not k = 0
    (d = L is allowed there, and a pair with L mismatches has no matched base to credit).  what: the error's prefix."""
    if model.kernel_type in (3, 5):
        raise ModelError("%s: RBF kernels (types 3 and 5) have no per-base decomposition" % what)
    if model.k == 0:
        raise ModelError("%s: models with k = 0 have no per-base decomposition (a pair may match on no base)" % what)


def explain_shares(model):
    """share[m] = c_m / (L - m), m = 0..d: what one matched base of a pair with m mismatches is credited."""
    c = dv.mismatch_weights(model.kernel_type, model.L, model.k)[:model.d + 1]
    return c / (model.L - np.arange(model.d + 1))


def default_explain_block(max_len, budget=BLOCK_BYTES):
    """Queries per block: the launch's partial rows (up to EXPLAIN_CHUNKS doubles per base) and the output within `budget`
    bytes of device memory."""
    return _fit_block(max_len, 8 * (EXPLAIN_CHUNKS + 1), budget)


def explain(model, fasta_or_sequences, device=0, block=None, on_block=None):
    """Per-base importance of `model` for a FASTA file (or a list / FlatSequences of base codes) -> (names, [float64 array
    of one value per base, per query]):

        E(x)[t] = sum_s dual_coef_s A_s(x)[t] / (sq_s sq_x)

    where A_s(x)[t] credits every l-mer pair of x (forward) and s (forward or reverse complement) with m <= d mismatches
    with c_m / (L - m) times the pair's positional weights on each of the L - m query bases it matched on.
    sum_t E(x)[t] = score(x) - model.rho on the no-wrap domain (every mismatch profile involved below 2^31: INTEGRATION.md
    §5b); beyond it `score` follows the reference's 32-bit wrap, while sq_s and sq_x here come from exact 64-bit self
    profiles and the sum is the exact score less rho.  For kernel type 0 this is GkmExplain's rule (each shared gapped k-mer split
    evenly over its k bases); for types 1, 2 and 4 the same rule on this project's c_m.  RBF and k = 0 models are refused.
    block: queries per device block (default_explain_block).  on_block(dict) (measurements): called after every block
    with its size, the explain kernel's milliseconds (HIP events), its l-mer comparisons and the block's wall time."""
    import torch
    check_explainable(model)
    seqs, names = _as_queries(fasta_or_sequences)
    check_queries(model, seqs)
    blocks = _Blocks(model, seqs, device, block, default_explain_block(_longest(seqs)), exact=True)
    ctx, S, sq, dev = blocks.ctx, blocks.S, blocks.sq, blocks.dev
    share = explain_shares(model)
    out = []
    with torch.cuda.device(dev):
        dual = torch.from_numpy(model.dual_coef()).to(dev)
        E = torch.empty(blocks.most_bases(), dtype=torch.float64, device=dev)
        for b in blocks:
            coef = dual / sq[:S]
            xscale = 1.0 / sq[S:S + b.qb]
            ctx.explain_block(blocks.rows, S, S + b.qb, share, coef.data_ptr(), xscale.data_ptr(), E.data_ptr(),
                              blocks.stream)
            out.extend(b.split(E[:b.nb].cpu().numpy()))
            if on_block is not None:
                on_block(dict(queries=b.qb, explain_kernel_ms=ctx.last_kernel_ms(), comparisons=ctx.last_comparisons(),
                              kernel=ctx.last_kernel_name(), wall_ms=(time.perf_counter() - b.t0) * 1e3))
    return names, out


def _write_values(path, names, values):
    with open(path, "w") as f:
        for name, v in zip(names, values):
            f.write("%s\t%s\n" % (name, ",".join(repr(float(e)) for e in np.asarray(v).reshape(-1))))


def _read_values(path, shape):
    names, values = [], []
    with open(path) as f:
        for line in f.read().split("\n")[:-1]:
            name, vals = line.rsplit("\t", 1)
            names.append(name)
            values.append(np.array([float(e) for e in vals.split(",")], dtype=np.float64).reshape(shape))
    return names, values


def write_explanation(path, names, values):
    """The `explain` output: one line per query, name<TAB>v0,v1,... with repr() floats (they read back to the same
    doubles)."""
    _write_values(path, names, values)


def read_explanation(path):
    """-> (names, [float64 array per query]) from a file written by write_explanation."""
    return _read_values(path, (-1,))


# ------------------------------------------------------------------ in-silico mutagenesis
ISM_CHUNKS = 16           # the most partial rows gkmhip_ism_block keeps per base (3 doubles per chunk of support vectors)


def check_ism(model):
    """The models `ism` serves: every model `score` serves except the RBF types, whose score is not linear in G."""
    if model.kernel_type in (3, 5):
        raise ModelError("ism: RBF kernels (types 3 and 5) are not served (their score is not linear in the raw kernel)")


def ism_coefficients(model):
    """(fold_u, fold_b, c), d + 1 doubles each: c[m] = c_m for m = 0..d; with c_{d+1} = 0, fold_u[m] = c_{m+1} - c_m
    (a matched base of a pair with m mismatches moves it to m + 1) and fold_b[m - 1] = c_{m-1} - c_m for m = 1..d + 1 (a
    mismatched base set to the support vector's base moves it to m - 1).  c_m beyond d is taken as 0 whatever
    dv.mismatch_weights returns there."""
    c = dv.mismatch_weights(model.kernel_type, model.L, model.k)[:model.d + 1].copy()
    ce = np.append(c, 0.0)
    return ce[1:] - ce[:-1], ce[:-1] - ce[1:], c


def default_ism_block(max_len, d, budget=BLOCK_BYTES):
    """Queries per block: the launch's partial rows (up to 3 x ISM_CHUNKS doubles per base), the (T, 4) output, the
    mutants' self profiles (4 (d + 1) int64 per base) and the finishing temporaries within `budget` bytes of device
    memory."""
    return _fit_block(max_len, 8 * (3 * ISM_CHUNKS + 4 * (int(d) + 1) + 24), budget)


def _mutant_norms_sq(prof, c):
    """G(y, y) = sum_m c_m P_m(y, y) of every single-base mutant y, in ascending m from 0.0 as the oracle forms it.
    prof: the (bases, 4, d + 1) int64 profiles of gkmhip_ism_self_profiles -> (bases, 4) float64."""
    import torch
    g = torch.zeros(prof.shape[:2], dtype=torch.float64, device=prof.device)
    for m in range(prof.shape[2]):
        g.add_(prof[:, :, m].double().mul_(float(c[m])))
    return g


def ism(model, fasta_or_sequences, device=0, block=None, on_block=None):
    """In-silico mutagenesis of `model` for a FASTA file (or a list / FlatSequences of base codes) -> (names, [float64
    array (T, 4) per query], columns A, C, G, T):

        ism(x)[t, b] = score(y) - score(x),   y = x with base t set to b   (0.0 where b == x[t])

    with score as `score` computes it, sum_s dual_coef_s G(y, s) / (sq_s sqrt(G(y, y))) - rho, on the
    no-wrap domain (every mismatch profile involved below 2^31: INTEGRATION.md §5b); beyond it `score` follows the
    reference's 32-bit wrap and this is the difference of the exact scores, every norm from 64-bit profiles.  Every
    model `score` serves except RBF (types 3 and 5), k = 0 included; every query length `score` accepts.  (An RBF model's
    mutagenesis is `mutant_scores` less its own-base column.)
    block: queries per device block (default_ism_block).  on_block(dict) (measurements): called after every block with
    its size, k_ism's milliseconds (HIP events), its l-mer comparisons, the self-profile kernels' milliseconds and the
    block's wall time."""
    import torch
    check_ism(model)
    seqs, names = _as_queries(fasta_or_sequences)
    check_queries(model, seqs)
    d = model.d
    blocks = _Blocks(model, seqs, device, block, default_ism_block(_longest(seqs), d), exact=True)
    ctx, S, sq, dev, stream = blocks.ctx, blocks.S, blocks.sq, blocks.dev, blocks.stream
    fold_u, fold_b, c = ism_coefficients(model)
    out = []
    with torch.cuda.device(dev):
        dual = torch.from_numpy(model.dual_coef()).to(dev)
        most = blocks.most_bases()
        D = torch.empty((most, 4), dtype=torch.float64, device=dev)
        prof = torch.empty((most, 4, d + 1), dtype=torch.int64, device=dev)
        base = torch.empty(blocks.qb_max, dtype=torch.float64, device=dev)
        for b in blocks:
            qb, nb = b.qb, b.nb
            ctx.ism_self_profiles(S, S + qb, prof.data_ptr(), stream)
            self_ms = ctx.last_kernel_ms() if on_block is not None else None
            coef = dual / sq[:S]
            ctx.ism_block(blocks.rows, S, S + qb, fold_u, fold_b, c, coef.data_ptr(), D.data_ptr(), base.data_ptr(),
                          stream)
            # score(y) - score(x) = (base + D) / sqrt(G(y, y)) - base / sq_x
            g = _mutant_norms_sq(prof[:nb], c)
            per = torch.from_numpy(np.diff(b.qoff)).to(dev)
            bx = torch.repeat_interleave(base[:qb], per)
            sx = torch.repeat_interleave(sq[S:S + qb], per)
            res = (bx[:, None] + D[:nb]).div_(g.sqrt_()).sub_((bx / sx)[:, None])
            host = res.cpu().numpy()
            host[np.arange(nb), b.codes] = 0.0
            out.extend(b.split(host))
            if on_block is not None:
                on_block(dict(queries=qb, ism_kernel_ms=ctx.last_kernel_ms(), comparisons=ctx.last_comparisons(),
                              kernel=ctx.last_kernel_name(), self_kernels_ms=self_ms,
                              wall_ms=(time.perf_counter() - b.t0) * 1e3))
    return names, out


def write_ism(path, names, values):
    """The `ism` (and `hypothetical`) output: one line per query, name<TAB>v(0,A),v(0,C),v(0,G),v(0,T),v(1,A),... (4T
    values, position-major) with repr() floats (they read back to the same doubles)."""
    _write_values(path, names, values)


def read_ism(path):
    """-> (names, [float64 array (T, 4) per query]) from a file written by write_ism."""
    return _read_values(path, (-1, 4))


# ------------------------------------------------------------------ the score of every single-base mutant
def default_mutscores_block(max_len, d, n_sv, budget=BLOCK_BYTES):
    """Queries per block: per query, what `ism` takes per base (default_ism_block) plus the mutants' (bases, 4) norms, and
    the n_sv raw kernel values of an RBF model's Gram launch with that launch's tile-transposed output (about as big),
    within `budget` bytes of device memory.  n_sv: 0 for a linear model, which runs no Gram launch."""
    per_query = 8 * (3 * ISM_CHUNKS + 4 * (int(d) + 1) + 28) * max(int(max_len), 64) + 16 * max(int(n_sv), 0)
    return int(max(1, min(1 << 20, budget // per_query)))


def mutant_scores(model, fasta_or_sequences, device=0, block=None, on_block=None):
    """The score of every single-base mutant of each query of a FASTA file (or a list / FlatSequences of base codes) ->
    (names, [float64 array (T, 4) per query], columns A, C, G, T):

        ms(x)[t, b] = score(y),   y = x with base t set to b   (so ms(x)[t, x[t]] = score(x), one double at every t)

    with score as `score` computes it, rho included, on the no-wrap domain `ism` documents.
    In-silico mutagenesis of any model is ms - ms[t, x[t]]; the effect of one SNV (deltaSVM) is one entry of that.  Every
    model `score` serves, the RBF types 3 and 5 and k = 0 included; every query length `score` accepts.

    Types 0, 1, 2 and 4 take `ism`'s launches and finish: (base + D) / sqrt(G(y, y)) + rho.  Types 3 and 5 (DESIGN.md
    §5m) take the raw G(x, s) from `score`'s Gram launch and fold every support vector's tallies through
    dual_s exp(gamma (G(y, s) / (sq_s sqrt(G(y, y))) - 1)) in gkmhip_ism_rbf_block.
    block: queries per device block (default_mutscores_block).  on_block(dict) (measurements): called after every block
    with its size, the fold kernel's milliseconds (HIP events), its l-mer comparisons, the self-profile kernels' and (RBF)
    the Gram kernel's milliseconds and the block's wall time."""
    import torch
    seqs, names = _as_queries(fasta_or_sequences)
    check_queries(model, seqs)
    d = model.d
    rbf = model.kernel_type in (3, 5)
    blocks = _Blocks(model, seqs, device, block,
                     default_mutscores_block(_longest(seqs), d, model.n_sv if rbf else 0), exact=True)
    ctx, S, sq, dev, stream = blocks.ctx, blocks.S, blocks.sq, blocks.dev, blocks.stream
    fold_u, fold_b, c = ism_coefficients(model)
    # score = sum_s dual_coef_s K(y, s) + rho for both SVM types (Model): what `score` makes of k_decision's sum - rho
    # with the C-SVC sign, and of the signed sum less LIBSVM's rho = -model.rho for SVR
    rho = model.rho
    out = []
    with torch.cuda.device(dev):
        dual = torch.from_numpy(model.dual_coef()).to(dev)
        most = blocks.most_bases()
        D = torch.empty((most, 4), dtype=torch.float64, device=dev)
        prof = torch.empty((most, 4, d + 1), dtype=torch.int64, device=dev)
        base = torch.empty(blocks.qb_max, dtype=torch.float64, device=dev)
        if rbf:
            ctx.set_kernel(dv.KERNEL_AUTO)
            gx = torch.empty((S, blocks.qb_max), dtype=torch.float64, device=dev)
        for b in blocks:
            qb, nb = b.qb, b.nb
            gram_ms = None
            if rbf:
                ctx.gram_block(blocks.rows, S, S + qb, gx.data_ptr(), blocks.qb_max, stream)      # raw: not normalised
                gram_ms = ctx.last_kernel_ms() if on_block is not None else None
            ctx.ism_self_profiles(S, S + qb, prof.data_ptr(), stream)
            self_ms = ctx.last_kernel_ms() if on_block is not None else None
            ysq = _mutant_norms_sq(prof[:nb], c).sqrt_()
            if rbf:
                ctx.ism_rbf_block(blocks.rows, S, S + qb, fold_u, fold_b, dual.data_ptr(), sq.data_ptr(), gx.data_ptr(),
                                  blocks.qb_max, ysq.data_ptr(), D.data_ptr(), base.data_ptr(), stream)
                res = D[:nb] + rho
                own = base[:qb] + rho
            else:
                coef = dual / sq[:S]
                ctx.ism_block(blocks.rows, S, S + qb, fold_u, fold_b, c, coef.data_ptr(), D.data_ptr(), base.data_ptr(),
                              stream)
                per = torch.from_numpy(np.diff(b.qoff)).to(dev)
                bx = torch.repeat_interleave(base[:qb], per)
                res = (bx[:, None] + D[:nb]).div_(ysq).add_(rho)
                own = base[:qb] / sq[S:S + qb] + rho
            host = res.cpu().numpy()
            host[np.arange(nb), b.codes] = np.repeat(own.cpu().numpy(), np.diff(b.qoff))
            out.extend(b.split(host))
            if on_block is not None:
                on_block(dict(queries=qb, ism_kernel_ms=ctx.last_kernel_ms(), comparisons=ctx.last_comparisons(),
                              kernel=ctx.last_kernel_name(), self_kernels_ms=self_ms, gram_kernel_ms=gram_ms,
                              wall_ms=(time.perf_counter() - b.t0) * 1e3))
    return names, out


# ------------------------------------------------------------------ hypothetical importance
def default_hyp_block(max_len, d, budget=BLOCK_BYTES):
    """Queries per block: the launch's partial rows (up to 4 x ISM_CHUNKS doubles per base), the raw (T, 4) values, the
    mutants' self profiles (4 (d + 1) int64 per base) and the finishing temporaries within `budget` bytes of device
    memory."""
    return _fit_block(max_len, 8 * (4 * ISM_CHUNKS + 4 * (int(d) + 1) + 28), budget)


def _hyp_finish(b, R, prof, c, xscale, dev):
    """The raw (bases, 4) values R of a block -> its queries' tables: the mutant columns times 1 / sqrt(G(y, y)) (prof:
    the mutants' self profiles), the own column times explain's xscale."""
    import torch
    scale = 1.0 / _mutant_norms_sq(prof[:b.nb], c).sqrt_()
    own = torch.from_numpy(b.codes.astype(np.int64)).to(dev)
    per = torch.from_numpy(np.diff(b.qoff)).to(dev)
    scale.scatter_(1, own[:, None], torch.repeat_interleave(xscale, per)[:, None])
    return b.split((R[:b.nb] * scale).cpu().numpy())


def hypothetical(model, fasta_or_sequences, device=0, block=None, on_block=None):
    """Hypothetical importance of `model` for a FASTA file (or a list / FlatSequences of base codes) -> (names, [float64
    array (T, 4) per query], columns A, C, G, T):

        hyp(x)[t, b] = E(y)[t],   y = x with base t set to b   (so hyp(x)[t, x[t]] = E(x)[t])

    with E the per-base importance `explain` computes, y's own norm sqrt(G(y, y)) included.  Times the
    one-hot of x it is explain(x), bit for bit; each mutant column is explain of that mutant at t, bit for bit, inside
    and beyond the no-wrap domain (all norms from exact 64-bit self profiles, as explain's: INTEGRATION.md §5b).  The
    models `explain` serves (no RBF, no k = 0); every query length `score` accepts.  block: queries per device block
    (default_hyp_block).  on_block(dict) (measurements): called after every block with its size, k_ism<true>'s
    milliseconds (HIP events), its l-mer comparisons, the self-profile kernels' milliseconds and the block's wall time."""
    import torch
    check_explainable(model, "hypothetical")
    seqs, names = _as_queries(fasta_or_sequences)
    check_queries(model, seqs)
    d = model.d
    blocks = _Blocks(model, seqs, device, block, default_hyp_block(_longest(seqs), d), exact=True)
    ctx, S, sq, dev, stream = blocks.ctx, blocks.S, blocks.sq, blocks.dev, blocks.stream
    share = explain_shares(model)
    c = dv.mismatch_weights(model.kernel_type, model.L, model.k)[:d + 1]
    out = []
    with torch.cuda.device(dev):
        dual = torch.from_numpy(model.dual_coef()).to(dev)
        most = blocks.most_bases()
        R = torch.empty((most, 4), dtype=torch.float64, device=dev)
        prof = torch.empty((most, 4, d + 1), dtype=torch.int64, device=dev)
        for b in blocks:
            qb = b.qb
            ctx.ism_self_profiles(S, S + qb, prof.data_ptr(), stream)
            self_ms = ctx.last_kernel_ms() if on_block is not None else None
            coef = dual / sq[:S]
            xscale = 1.0 / sq[S:S + qb]
            ctx.hyp_block(blocks.rows, S, S + qb, share, coef.data_ptr(), R.data_ptr(), stream)
            out.extend(_hyp_finish(b, R, prof, c, xscale, dev))
            if on_block is not None:
                on_block(dict(queries=qb, hyp_kernel_ms=ctx.last_kernel_ms(), comparisons=ctx.last_comparisons(),
                              kernel=ctx.last_kernel_name(), self_kernels_ms=self_ms,
                              wall_ms=(time.perf_counter() - b.t0) * 1e3))
    return names, out
