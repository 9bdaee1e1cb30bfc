"""Train a gkm-SVM on all sequences, keep it in a model file, and score new sequences with it on the GPU.

The other half of a gkm-SVM next to the cross-validation of `gkmsvm.py` (the counterparts of LS-GKM's `gkmtrain` and
`gkmpredict`; the model file is this project's own):

  * `train` builds the Gram matrix of pos + neg on the device (device.gram_matrix, the resident path), solves ONE C-SVC on
    every sample with the GPU solver (svmcv.train_folds; scikit-learn if the solver stops at its iteration cap) and
    keeps the support vectors in LIBSVM's internal order;
  * `score` uploads [support vectors; a block of queries] into one cached context, takes the self norms of that set,
    computes the S x Qb block of kernel values (gkmhip_gram_block: SVs as rows, queries as columns) and its
    normalisation (gkmhip_normalize_block), and sums the decision values with k_decision (gkmsvm_decision_batch) --
    scikit-learn's `decision_function` of the trained SVC, bit for bit, for every block size;
  * `explain` splits each query's score over its bases (gkmhip_explain_block): per block the same upload
    as `score` and the self norms from exact 64-bit profiles (gkmhip_self_profiles: the same doubles as `score`'s while
    no profile reaches 2^31, the no-wrap domain of INTEGRATION.md §5b, and the true norms beyond), then one launch that credits every matching l-mer pair to the query bases it matched on;
  * `ism` scores every single-base substitution of each query (gkmhip_ism_block and
    gkmhip_ism_self_profiles): per block the same upload and exact self norms, one launch that tallies how each l-mer pair's
    mismatch count moves under a substitution, and one that counts every mutant's profile against itself;
  * `mutant_scores` gives the score of every single-base mutant itself, for every model `score` serves, the RBF types
    included: a linear model through `ism`'s launches, an RBF model through gkmhip_ism_rbf_block, which
    takes the raw kernel values of `score`'s Gram launch and folds each support vector's tallies through exp();
  * `hypothetical` gives, for every position and each of the four bases, the importance that base would get there
    (gkmhip_hyp_block): ism's upload, self norms, mutant self profiles and tallies, folded the way
    `explain` folds its own;
  * `weights` folds a model (not RBF) into one weight per l-mer (gkmhip_lmer_weights) and writes that
    table; `predict-table` scores from it with only the queries uploaded: their self norms, then one gather per l-mer
    (gkmhip_lmer_score) -- `predict`'s values up to rounding, for a fraction of the work;
  * `train_svr` fits an epsilon-SVR to one real target per sequence: the same Gram matrix, LIBSVM's
    2l-variable problem solved by the GPU solver with a linear term per position (svmcv.train_svr_folds); its model
    scores through the signed decision (gkmsvm_decision_signed_batch) -- scikit-learn's `SVR.predict`, bit for bit --
    and serves `explain`, `ism`, `hypothetical` and `weights` like a C-SVC model;
  * `scan` takes a weight table along sequences of any length and scores every window of W bases at a stride (DESIGN.md
    §5i, gkmhip_scan_profiles and gkmhip_scan_score): `predict-table`'s value for each window cut out, bit for bit, with
    the self norms of overlapping windows counted together; windows over a non-ACGT character have no score;
  * `importance-table` folds a model (not RBF, not k = 0) into one value per (l-mer, offset) (DESIGN.md §5j,
    gkmhip_lmer_importance); `explain-table` and `hypothetical-table` serve `explain`'s and `hypothetical`'s values from
    it, up to rounding, with only the queries uploaded: their self norms, then L gathers per base (gkmhip_lmer_explain)
    or 4 L (gkmhip_lmer_hyp);
  * `delta` gives the effect of sequence variants -- SNVs, MNVs, insertions, deletions -- from a weight table (deltaSVM,
    DESIGN.md §5k, gkmhip_delta_variants): the change in the summed weights of the l-mers a variant touches, for a list
    of variants against records of any length; `delta-saturation` gives every possible SNV of every position
    (gkmhip_delta_sat), the table-based counterpart of `ism`.

    python -m gkmqc_amd.gkmpredict train [-t -L -k -d -M -H -G -C -e -u] pos.fa neg.fa model.txt
    python -m gkmqc_amd.gkmpredict train-svr [-t -L -k -d -M -H -G -C -p -e -u] seqs.fa targets.txt model.txt
    python -m gkmqc_amd.gkmpredict predict query.fa model.txt out.txt
    python -m gkmqc_amd.gkmpredict explain [--block Qb] query.fa model.txt out.txt
    python -m gkmqc_amd.gkmpredict ism [--block Qb] query.fa model.txt out.txt
    python -m gkmqc_amd.gkmpredict mutant-scores [--block Qb] query.fa model.txt out.txt
    python -m gkmqc_amd.gkmpredict hypothetical [--block Qb] query.fa model.txt out.txt
    python -m gkmqc_amd.gkmpredict weights model.txt weights.txt
    python -m gkmqc_amd.gkmpredict predict-table [--block Qb] query.fa weights.txt out.txt
    python -m gkmqc_amd.gkmpredict scan --width W [--stride s] [--chunk B] seqs.fa weights.txt out.bedgraph
    python -m gkmqc_amd.gkmpredict importance-table model.txt table.npz
    python -m gkmqc_amd.gkmpredict explain-table [--block Qb] query.fa table.npz out.txt
    python -m gkmqc_amd.gkmpredict hypothetical-table [--block Qb] query.fa table.npz out.txt
    python -m gkmqc_amd.gkmpredict delta [--chunk B] weights.txt seqs.fa variants.tsv out.tsv
    python -m gkmqc_amd.gkmpredict delta-saturation [--chunk B] weights.txt seqs.fa out.tsv
"""
import argparse
import logging
import math
import os
import sys
import time

import numpy as np

from . import device as dv
from . import svmcv

FORMAT = "gkmqc-model-1"
SVR_FORMAT = "gkmqc-svr-1"
C_SVC, EPSILON_SVR = "c_svc", "epsilon_svr"
_INT_KEYS = ("kernel_type", "L", "k", "d", "M", "shrinking", "n0", "n_sv")
_FLOAT_KEYS = ("H", "gamma", "C", "tol", "rho", "epsilon")
_KEYS = ("format", "kernel_type", "L", "k", "d", "M", "H", "gamma", "C", "tol", "shrinking", "rho", "n0", "n_sv")
_SVR_KEYS = ("format", "kernel_type", "L", "k", "d", "M", "H", "gamma", "C", "tol", "shrinking", "epsilon", "rho", "n_sv")
MAX_SVR_SAMPLES = svmcv.MAX_FOLD_SAMPLES // 2   # LIBSVM's epsilon-SVR solves 2l variables
BLOCK_BYTES = 2 << 30     # device memory one block of queries may take: S x Qb kernel values + the kernel's own output
_ACGT = np.frombuffer(b"ACGT", dtype=np.uint8)


class ModelError(ValueError):
    pass


def codes_to_text(codes):
    return _ACGT[np.asarray(codes, dtype=np.uint8)].tobytes().decode()


def text_to_codes(text):
    raw = np.frombuffer(text.encode(), dtype=np.uint8)
    lut = np.full(256, 255, dtype=np.uint8)
    lut[_ACGT] = np.arange(4, dtype=np.uint8)
    codes = lut[raw]
    if (codes == 255).any():
        raise ModelError("a stored sequence holds a character other than A, C, G, T")
    return codes


class Model:
    """A trained gkm-SVM: kernel and SVM parameters, rho, and the support vectors, each with its FASTA name and base codes.

    C-SVC (svm_type C_SVC): the support vectors in LIBSVM's internal order (class 0 -- the negatives -- first, n0 of
    them), `alpha` their dual variables (> 0).  epsilon-SVR (svm_type EPSILON_SVR, `epsilon` set, n0 = 0): the support
    vectors in training order, `alpha` their signed coefficients alpha_k - alpha*_k (nonzero).  For both,
    score = sum dual_coef() K + rho: rho is scikit-learn's intercept_ (for SVR that is LIBSVM's rho negated)."""

    def __init__(self, kernel_type, L, k, d, M, H, gamma, C, tol, shrinking, rho, n0, alpha, names, seqs, svm_type=C_SVC,
                 epsilon=None):
        self.kernel_type, self.L, self.k, self.d, self.M = int(kernel_type), int(L), int(k), int(d), int(M)
        self.H, self.gamma, self.C, self.tol = float(H), float(gamma), float(C), float(tol)
        self.shrinking = bool(shrinking)
        self.rho, self.n0 = float(rho), int(n0)
        self.alpha = np.ascontiguousarray(alpha, dtype=np.float64)
        self.names = list(names)
        self.seqs = [np.ascontiguousarray(s, dtype=np.uint8) for s in seqs]
        self.svm_type = svm_type
        self.epsilon = None if epsilon is None else float(epsilon)
        _validate(self)

    @property
    def is_svr(self):
        return self.svm_type == EPSILON_SVR

    @property
    def n_sv(self):
        return len(self.alpha)

    def kernel_params(self):
        return (self.kernel_type, self.L, self.k, self.d, self.M, self.H, self.gamma)

    def dual_coef(self):
        """scikit-learn's `dual_coef_[0]` (C-SVC, labels 0 / 1: class 0 first with a negative sign; SVR: the signed
        coefficients as stored)."""
        if self.is_svr:
            return self.alpha.copy()
        return np.where(np.arange(self.n_sv) < self.n0, -self.alpha, self.alpha)

    def flat_seqs(self):
        """The support vectors back to back, as the device takes them."""
        off = np.zeros(self.n_sv + 1, dtype=np.int64)
        np.cumsum([len(s) for s in self.seqs], out=off[1:])
        return dv.FlatSequences(np.concatenate(self.seqs), off)

    def save(self, path):
        """Write the model file (format: INTEGRATION.md).  Floats as repr(), which reads back to the same double."""
        head = [("format", SVR_FORMAT if self.is_svr else FORMAT), ("kernel_type", self.kernel_type), ("L", self.L),
                ("k", self.k), ("d", self.d), ("M", self.M), ("H", repr(self.H)), ("gamma", repr(self.gamma)),
                ("C", repr(self.C)), ("tol", repr(self.tol)), ("shrinking", int(self.shrinking))]
        if self.is_svr:
            head += [("epsilon", repr(self.epsilon)), ("rho", repr(self.rho)), ("n_sv", self.n_sv)]
        else:
            head += [("rho", repr(self.rho)), ("n0", self.n0), ("n_sv", self.n_sv)]
        tmp = path + ".tmp"
        with open(tmp, "w") as f:
            for key, val in head:
                f.write("%s %s\n" % (key, val))
            f.write("SV\n")
            for a, name, s in zip(self.alpha, self.names, self.seqs):
                f.write("%r\t%s\t%s\n" % (float(a), name, codes_to_text(s)))
        os.replace(tmp, path)


def _validate(m):
    bad = dv.check_parameters(m.kernel_type, m.L, m.k, m.d)
    if bad:
        raise ModelError("kernel parameters rejected: %s" % bad)
    if not 0 <= m.M <= 255:
        raise ModelError("M must lie in 0..255")
    if not (np.isfinite(m.H) and np.isfinite(m.gamma) and np.isfinite(m.rho) and m.C > 0 and m.tol > 0):
        raise ModelError("H, gamma and rho must be finite, C and tol positive")
    if not (len(m.alpha) == len(m.names) == len(m.seqs)) or len(m.alpha) == 0:
        raise ModelError("a model needs at least one support vector, each with alpha, name and sequence")
    if m.svm_type == EPSILON_SVR:
        if m.epsilon is None or not (np.isfinite(m.epsilon) and m.epsilon >= 0):
            raise ModelError("an SVR model needs a finite epsilon >= 0")
        if m.n0 != 0:
            raise ModelError("an SVR model has no classes (n0 = 0)")
        if not (np.isfinite(m.alpha).all() and (m.alpha != 0).all()):
            raise ModelError("every SVR coefficient must be nonzero and finite")
    elif m.svm_type == C_SVC:
        if m.epsilon is not None:
            raise ModelError("a C-SVC model has no epsilon")
        if not 0 <= m.n0 <= len(m.alpha):
            raise ModelError("n0 must lie in 0..n_sv")
        if not (np.isfinite(m.alpha).all() and (m.alpha > 0).all()):
            raise ModelError("every alpha must be positive and finite")
    else:
        raise ModelError("unknown SVM type %r" % (m.svm_type,))
    if any(len(s) < m.L for s in m.seqs):
        raise ModelError("a stored sequence is shorter than L")
    if any("\n" in nm or "\r" in nm for nm in m.names):
        raise ModelError("a name holds a line break")


def load(path):
    """Read a model file written by Model.save (either format tag); anything malformed raises ModelError with the
    reason."""
    with open(path) as f:
        lines = f.read().split("\n")
    if lines and lines[-1] == "":
        lines.pop()
    head, i = {}, 0
    while i < len(lines) and lines[i] != "SV":
        parts = lines[i].split(" ", 1)
        if len(parts) != 2 or parts[0] not in _KEYS + _SVR_KEYS:
            raise ModelError("%s:%d: not a `key value` line of the header: %r" % (path, i + 1, lines[i]))
        if parts[0] in head:
            raise ModelError("%s:%d: key %s given twice" % (path, i + 1, parts[0]))
        head[parts[0]] = parts[1]
        i += 1
    if i == len(lines):
        raise ModelError("%s: no SV line" % path)
    svr = head.get("format") == SVR_FORMAT
    keys = _SVR_KEYS if svr else _KEYS
    missing = [key for key in keys if key not in head]
    if missing:
        raise ModelError("%s: missing key(s): %s" % (path, ", ".join(missing)))
    if head["format"] not in (FORMAT, SVR_FORMAT):
        raise ModelError("%s: format %r, expected %r or %r" % (path, head["format"], FORMAT, SVR_FORMAT))
    extra = [key for key in head if key not in keys]
    if extra:
        raise ModelError("%s: key(s) %s do not belong to format %s" % (path, ", ".join(extra), head["format"]))
    try:
        val = {key: int(head[key]) for key in _INT_KEYS if key in keys}
        val.update({key: float(head[key]) for key in _FLOAT_KEYS if key in keys})
    except ValueError as e:
        raise ModelError("%s: %s" % (path, e))
    body = lines[i + 1:]
    if len(body) != val["n_sv"]:
        raise ModelError("%s: n_sv is %d but %d support vector lines follow" % (path, val["n_sv"], len(body)))
    alpha, names, seqs = np.zeros(len(body)), [], []
    for j, line in enumerate(body):
        parts = line.split("\t", 1)
        rest = parts[1].rsplit("\t", 1) if len(parts) == 2 else []
        if len(rest) != 2:
            raise ModelError("%s:%d: expected %s<TAB>name<TAB>sequence" % (path, i + 2 + j, "coef" if svr else "alpha"))
        try:
            alpha[j] = float(parts[0])
            seqs.append(text_to_codes(rest[1]))
        except ValueError as e:
            raise ModelError("%s:%d: %s" % (path, i + 2 + j, e))
        names.append(rest[0])
    if svr:
        return Model(val["kernel_type"], val["L"], val["k"], val["d"], val["M"], val["H"], val["gamma"], val["C"],
                     val["tol"], val["shrinking"], val["rho"], 0, alpha, names, seqs, EPSILON_SVR, val["epsilon"])
    return Model(val["kernel_type"], val["L"], val["k"], val["d"], val["M"], val["H"], val["gamma"], val["C"], val["tol"],
                 val["shrinking"], val["rho"], val["n0"], alpha, names, seqs)


# ------------------------------------------------------------------ training
def train(pos_fa, neg_fa, kernel_type=4, L=10, k=6, d=3, M=50, H=50, gamma=1.0, C=1.0, tol=1e-3, shrinking=False,
          device=0, kernel=dv.KERNEL_AUTO):
    """One C-SVC on every sequence of pos_fa (label 1) and neg_fa (label 0) -> Model."""
    import torch
    bad = dv.check_parameters(kernel_type, L, k, d)
    if bad:
        raise ModelError("kernel parameters rejected: %s" % bad)
    pos, pos_names, _, _ = dv.read_fasta(pos_fa)
    neg, neg_names, _, _ = dv.read_fasta(neg_fa)
    if len(pos) == 0 or len(neg) == 0:
        raise ModelError("training needs at least one positive and one negative sequence")
    seqs = dv.FlatSequences(np.concatenate((pos.codes, neg.codes)),
                            np.concatenate((pos.off, pos.off[-1] + neg.off[1:])))
    names = pos_names + neg_names
    y = np.concatenate((np.repeat(1, len(pos)), np.repeat(0, len(neg))))
    res = dv.gram_matrix(seqs, kernel_type, L, k, d, M, H, gamma, device, kernel=kernel, symmetric=True,
                         keep_context=True)
    K = res["K"]
    sol, _ = svmcv.train_folds(K, [np.arange(len(y))], y, C, tol, shrinking)
    if sol.iters[0] >= 0:
        a, order = sol.alpha[0], sol.idx[0]
        sv = np.nonzero(a > 0)[0]
        idx, alpha, rho = order[sv], a[sv], float(sol.rho[0])
    else:   # the GPU solver's iteration cap: the reference's solver has none (as svmcv.crossValidate)
        from sklearn.svm import SVC
        logging.warning("training re-solved with scikit-learn (iteration cap of the GPU solver)")
        m = SVC(kernel="precomputed", C=C, tol=tol, shrinking=bool(shrinking)).fit(K.cpu().numpy(), y)
        # (for two classes scikit-learn negates LIBSVM's coefficients and decision value, so intercept_ is LIBSVM's rho)
        idx, alpha, rho = m.support_, np.abs(m.dual_coef_[0]), float(m.intercept_[0])
    del K, res
    torch.cuda.empty_cache()
    return Model(kernel_type, L, k, d, M, H, gamma, C, tol, shrinking, rho, int((y[idx] == 0).sum()), alpha,
                 [names[i] for i in idx], [seqs[i] for i in idx])


def read_targets(path, names):
    """The targets file of `train_svr`: one name<TAB>value line per FASTA record, in FASTA order (split at the LAST tab:
    names may hold tabs).  names: the headers the FASTA reader returned.  -> float64 array; a count or name mismatch, a
    value that is not a finite float, raises ModelError with the line number."""
    with open(path) as f:
        lines = f.read().split("\n")
    if lines and lines[-1] == "":
        lines.pop()
    z = np.empty(len(names))
    for j, line in enumerate(lines):
        if j >= len(names):
            raise ModelError("%s:%d: more target lines than FASTA records (%d)" % (path, j + 1, len(names)))
        parts = line.rsplit("\t", 1)
        if len(parts) != 2:
            raise ModelError("%s:%d: expected name<TAB>value" % (path, j + 1))
        if parts[0] != names[j]:
            raise ModelError("%s:%d: name %r, but FASTA record %d is %r" % (path, j + 1, parts[0], j + 1, names[j]))
        try:
            z[j] = float(parts[1])
        except ValueError:
            raise ModelError("%s:%d: %r is not a number" % (path, j + 1, parts[1]))
        if not np.isfinite(z[j]):
            raise ModelError("%s:%d: the value must be finite, not %r" % (path, j + 1, parts[1]))
    if len(lines) < len(names):
        raise ModelError("%s:%d: no target for FASTA record %d (%r): %d lines for %d records"
                         % (path, len(lines) + 1, len(lines) + 1, names[len(lines)], len(lines), len(names)))
    return z


def train_svr(fasta, targets, kernel_type=4, L=10, k=6, d=3, M=50, H=50, gamma=1.0, C=1.0, epsilon=0.1, tol=1e-3,
              shrinking=False, device=0, kernel=dv.KERNEL_AUTO):
    """One epsilon-SVR on every sequence of `fasta` with `targets` (a targets file, see read_targets, or a sequence of
    floats in FASTA order) -> Model (svm_type EPSILON_SVR): scikit-learn's SVR(kernel="precomputed") on the same matrix,
    bit for bit (the GPU solver; scikit-learn if it stops at its iteration cap).  At most MAX_SVR_SAMPLES sequences.
    The model's `n_iter` holds the solver's iteration count (not stored in the file)."""
    import torch
    bad = dv.check_parameters(kernel_type, L, k, d)
    if bad:
        raise ModelError("kernel parameters rejected: %s" % bad)
    if not (np.isfinite(epsilon) and epsilon >= 0):
        raise ModelError("epsilon must be finite and at least 0")
    if not (C > 0 and tol > 0):
        raise ModelError("C and tol must be positive")
    seqs, names, _, _ = dv.read_fasta(fasta)
    n = len(seqs)
    if n == 0:
        raise ModelError("training needs at least one sequence")
    if n > MAX_SVR_SAMPLES:
        raise ModelError("epsilon-SVR takes at most %d sequences (2l solver variables), not %d" % (MAX_SVR_SAMPLES, n))
    if isinstance(targets, (str, bytes, os.PathLike)):
        z = read_targets(targets, names)
    else:
        z = np.asarray(targets, dtype=np.float64).reshape(-1)
        if len(z) != n:
            raise ModelError("%d targets for %d sequences" % (len(z), n))
        if not np.isfinite(z).all():
            raise ModelError("every target must be finite")
    res = dv.gram_matrix(seqs, kernel_type, L, k, d, M, H, gamma, device, kernel=kernel, symmetric=True,
                         keep_context=True)
    K = res["K"]
    sol = svmcv.train_svr_folds(K, [np.arange(n)], z, C, epsilon, tol, shrinking)
    del K, res
    torch.cuda.empty_cache()
    sv = sol.support[0]
    if len(sv) == 0:
        raise ModelError("no support vectors: every target lies within epsilon = %r of the intercept %r; use a smaller "
                         "epsilon (-p)" % (float(epsilon), float(sol.intercept[0])))
    m = Model(kernel_type, L, k, d, M, H, gamma, C, tol, shrinking, sol.intercept[0], 0, sol.dual_coef[0],
              [names[i] for i in sv], [seqs[i] for i in sv], EPSILON_SVR, epsilon)
    m.n_iter = int(sol.iters[0])
    return m


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


# ------------------------------------------------------------------ scanning long sequences
SCAN_MAX_WIDTH = 2047     # a window is a query of its own: the longest sequence the kernels' norms are defined for
_WHITESPACE = np.array([9, 10, 11, 12, 13, 32], dtype=np.uint8)


def read_long_fasta(path):
    """A FASTA file -> [(name, codes, valid)] with records of any length, uncut: name is the header after '>', codes
    the uint8 base codes (A, C, G, T = 0..3 in either case; 0 at any other character) and valid the bool mask of the
    bases that are A, C, G or T.  Lines before the first header are ignored, as is white space inside a record."""
    with open(path, "rb") as f:
        data = np.frombuffer(f.read(), dtype=np.uint8)
    lut = np.full(256, 255, dtype=np.uint8)
    lut[_ACGT] = np.arange(4, dtype=np.uint8)
    lut[np.frombuffer(b"acgt", dtype=np.uint8)] = np.arange(4, dtype=np.uint8)
    nls = np.flatnonzero(data == 10)
    starts = np.concatenate(([0], nls + 1))                                # where lines begin
    starts = starts[starts < len(data)]
    heads = starts[data[starts] == ord(">")]
    ends = np.append(nls, len(data))[np.searchsorted(nls, heads)]          # where the header lines end
    out = []
    for i, (h, end) in enumerate(zip(heads.tolist(), ends.tolist())):
        name = data[h + 1:end].tobytes().decode("utf-8", "replace").rstrip("\r")
        body = data[end + 1:heads[i + 1] if i + 1 < len(heads) else len(data)]
        body = body[~np.isin(body, _WHITESPACE)]
        codes = lut[body]
        valid = codes != 255
        codes[~valid] = 0
        out.append((name, codes, valid))
    return out


def _as_scan_records(fasta_or_sequences):
    if isinstance(fasta_or_sequences, (str, bytes, os.PathLike)):
        return read_long_fasta(fasta_or_sequences)
    out = []
    for i, x in enumerate(fasta_or_sequences):
        x = np.asarray(x, dtype=np.uint8)
        valid = x < 4
        out.append(("seq%d" % i, np.where(valid, x, 0).astype(np.uint8), valid))
    return out


def scan_window_count(T, width, stride):
    """Windows of `width` bases at starts 0, stride, 2 stride, ... that lie inside T bases."""
    return 0 if T < width else (int(T) - int(width)) // int(stride) + 1


def window_validity(valid, width, stride):
    """-> bool per window: the window covers no invalid base."""
    bad = np.zeros(len(valid) + 1, dtype=np.int64)
    np.cumsum(~np.asarray(valid, dtype=bool), out=bad[1:])
    a = np.arange(scan_window_count(len(valid), width, stride), dtype=np.int64) * int(stride)
    return bad[a + int(width)] == bad[a]


def scan_chunk_plan(T, width, stride, chunk):
    """The chunks of a record of T bases -> [(w0, w1, b0, b1)]: windows [w0, w1) from the bases [b0, b1), at most
    max(chunk, width) of them; every window in exactly one chunk.  Consecutive chunks share the bases between the next
    window's start and the last window's end (width - 1 of them at stride 1)."""
    nw = scan_window_count(T, width, stride)
    per = (max(int(chunk), int(width)) - int(width)) // int(stride) + 1
    return [(w0, min(nw, w0 + per), w0 * stride, (min(nw, w0 + per) - 1) * stride + width) for w0 in range(0, nw, per)]


def default_scan_chunk(d, budget=BLOCK_BYTES):
    """Bases per chunk: at stride 1 a base costs its code, mask and l-mer word, a window's d + 1 int64 profile counts and
    the doubles of the epilogue, within `budget` bytes of device memory."""
    return int(budget // (8 * (int(d) + 1) + 64))


def check_scan(table, width, stride, chunk=None):
    """What `scan` refuses before it reads anything or touches the device."""
    _check_scan(LmerTable, "scan", table, width, stride, chunk)


def _check_folded(want, what, folded):
    """What every function that takes a table (want: LmerTable) or a panel (LmerPanel) refuses first: anything else."""
    if not isinstance(folded, want):
        raise ModelError("%s: needs an l-mer weight table (gkmpredict weights), not a model" % what if want is LmerTable else
                         "%s: needs an l-mer weight panel (gkmpredict panel), not a table or a model" % what)
    check_table_model(folded, what)


def _check_scan(want, what, folded, width, stride, chunk):
    """check_scan's and check_panel_scan's refusals; what: the prefix of every message"""
    _check_folded(want, what, folded)
    if int(width) < folded.L:
        raise ModelError("%s: the width %d is below L = %d" % (what, width, folded.L))
    if int(width) > SCAN_MAX_WIDTH:
        raise ModelError("%s: the width %d is above %d, the longest sequence a score is defined for"
                         % (what, width, SCAN_MAX_WIDTH))
    if int(stride) < 1:
        raise ModelError("%s: the stride must be at least 1" % what)
    if chunk is not None and int(chunk) < int(width):
        raise ModelError("%s: a chunk must hold at least one window (%d bases)" % (what, width))


def scan(table, fasta_or_sequences, width, stride=1, device=0, chunk=None, on_chunk=None):
    """The score of every window of `width` bases at starts 0, stride, 2 stride, ... of each record of a FASTA file (or of
    each of a list of uint8 code arrays, values >= 4 invalid), records of any length -> [(name, starts, scores)], starts
    int64 and scores float64 per record.  A window's score is score_with_table's for the window cut out as a sequence,
    bit for bit, whatever `chunk` and whatever precedes the record; NaN where the window covers a character other than
    A, C, G, T (either case).  A record shorter than `width` has no windows; it is an error if none has any.
    chunk: bases per device chunk (default_scan_chunk).  on_chunk(dict) (measurements): called after every chunk with
    its windows, k_scan_profiles' milliseconds (HIP events), its l-mer comparisons and the chunk's wall time."""
    check_scan(table, width, stride, chunk)
    return _scan_folded(table, "scan", fasta_or_sequences, width, stride, device, chunk or default_scan_chunk(table.d),
                        on_chunk)


def _scan_folded(folded, what, fasta_or_sequences, width, stride, device, chunk, on_chunk):
    """The body `scan` and `scan_with_panel` share -> [(name, starts, scores (windows,) + folded.cols)].  folded: the
    table or panel (checked with width, stride and chunk); what: the prefix of the messages; chunk: bases per chunk."""
    width, stride = int(width), int(stride)
    records = _scan_records(what, fasta_or_sequences, width)
    out = []
    for name, codes, valid in records:
        nw = scan_window_count(len(codes), width, stride)
        out.append((name, np.arange(nw, dtype=np.int64) * stride, np.empty((nw,) + folded.cols)))
    for ch in _scan_chunks(folded, records, width, stride, device, chunk, on_chunk is not None):
        out[ch.record][2][ch.w0:ch.w1] = ch.scores.cpu().numpy()
        if on_chunk is not None:
            ch.info["wall_ms"] = (time.perf_counter() - ch.t0) * 1e3
            on_chunk(ch.info)
    for (_, _, valid), (_, _, scores) in zip(records, out):
        scores[~window_validity(valid, width, stride)] = np.nan
    return out


def _scan_records(what, fasta_or_sequences, width):
    """The records of a scan, or the refusal every scan shares: none of them holds a window."""
    records = _as_scan_records(fasta_or_sequences)
    if not any(len(codes) >= width for _, codes, _ in records):
        raise ModelError("%s: no record holds a window of %d bases" % (what, width))
    return records


class _ScanChunk:
    """What the chunk loop hands over per chunk, all of it on the device: the windows [w0, w1) of records[record], the
    chunk's nlm l-mer words (int32 tensor lm) and the windows' finished scores ((windows,) + folded.cols, rho included;
    whatever stands at a window over an invalid base is not a score).  ctx, stream: for further launches on the chunk;
    info: the measurements so far (None unless asked for); t0: when the chunk began."""
    __slots__ = ("record", "w0", "w1", "lm", "nlm", "scores", "ctx", "stream", "info", "t0")


def _scan_chunks(folded, records, width, stride, device, chunk, measure, score_ms=False):
    """The chunk loop of every scan, a generator of _ScanChunk: per chunk of each record the upload, the l-mer words, the
    windows' self profiles (k_scan_profiles), the table's or panel's score launch and the epilogue T / sq + rho.  The
    consumer runs between two chunks, on the loop's device and stream.  measure: fill info with scan's on_chunk keys;
    score_ms: a table reports its score kernel too."""
    import torch
    chunk = int(chunk)
    L, d, cols = folded.L, folded.d, folded.cols
    ctx = dv.cached_context(*folded.kernel_params(), device=device)
    dev = torch.device("cuda", device)
    c = dv.mismatch_weights(folded.kernel_type, L, folded.k)[:d + 1]
    wt = dv.position_weights(folded.kernel_type, width - L + 1, folded.M, folded.H)
    with torch.cuda.device(dev):
        stream = torch.cuda.current_stream().cuda_stream
        W = torch.from_numpy(folded.device_weights()).to(dev)
        rho = _rho_operand(folded, dev)
        d_wt = torch.from_numpy(wt).to(dev)
        launch = folded.launcher(ctx, "scan_score")
        for r, (name, codes, valid) in enumerate(records):
            for w0, w1, b0, b1 in scan_chunk_plan(len(codes), width, stride, chunk):
                ch = _ScanChunk()
                ch.record, ch.w0, ch.w1, ch.ctx, ch.stream, ch.info = r, w0, w1, ctx, stream, None
                ch.t0 = time.perf_counter()
                d_codes = torch.from_numpy(codes[b0:b1]).to(dev)
                d_valid = torch.from_numpy(valid[b0:b1].view(np.uint8)).to(dev)
                nlm, nwin = b1 - b0 - L + 1, w1 - w0
                lm = torch.empty(nlm, dtype=torch.int32, device=dev)
                ctx.scan_lmers(d_codes.data_ptr(), d_valid.data_ptr(), b1 - b0, lm.data_ptr(), stream)
                prof = torch.empty((nwin, d + 1), dtype=torch.int64, device=dev)
                ctx.scan_profiles(lm.data_ptr(), nlm, d_wt.data_ptr(), width, stride, nwin, prof.data_ptr(), stream)
                if measure:
                    ch.info = dict(windows=nwin, bases=b1 - b0, **_models(cols), profile_kernel_ms=ctx.last_kernel_ms(),
                                   comparisons=ctx.last_comparisons(), kernel=ctx.last_kernel_name())
                T = torch.empty((nwin,) + cols, dtype=torch.float64, device=dev)
                launch(lm.data_ptr(), nlm, d_wt.data_ptr(), width, stride, nwin, W.data_ptr(), T.data_ptr(), stream)
                if measure and (cols or score_ms):                         # (a panel reports its score kernel too)
                    ch.info.update(score_kernel=ctx.last_kernel_name(), score_kernel_ms=ctx.last_kernel_ms())
                sq = _norms_from_profiles(prof, c)
                ch.lm, ch.nlm, ch.scores = lm, nlm, T / _per_item(sq, cols) + rho
                yield ch


def write_scan(path, results, width):
    """The `scan` output: one line per scored window, name<TAB>start<TAB>end<TAB>score (0-based start, end = start +
    width, the score at %.17g, which reads back to the same double); windows without a score (NaN) are left out.
    -> how many were left out."""
    omitted = 0
    with open(path, "w") as f:
        for name, starts, scores in results:
            keep = ~np.isnan(scores)
            omitted += int((~keep).sum())
            for i in range(0, len(starts), 1 << 16):
                k = keep[i:i + (1 << 16)]
                f.write("".join("%s\t%d\t%d\t%.17g\n" % (name, a, a + width, v) for a, v in
                                zip(starts[i:i + (1 << 16)][k].tolist(), scores[i:i + (1 << 16)][k].tolist())))
    return omitted


def read_scan(path):
    """-> [(name, start, end, score)] from a file written by write_scan."""
    out = []
    with open(path) as f:
        for line in f.read().split("\n")[:-1]:
            name, a, b, v = line.rsplit("\t", 3)
            out.append((name, int(a), int(b), float(v)))
    return out


# ------------------------------------------------------------------ regions of a scan
REGION_FIELDS = ("start", "end", "peak", "summit", "windows")   # the arrays of a `regions` dict, in file order
_REGION_KEYS = ("first", "last", "summit", "windows", "peak")   # of a region in window indices, as the device reports it
REGION_MAX_GAP = 1 << 40  # the largest gap the device layer takes (gkmhip_regions_count)


def _check_regions(what, threshold, gap, n_models=None):
    """The refusals `scan_regions` adds to `scan`'s -> the thresholds, one float per member (one in all for a table)."""
    if isinstance(gap, bool) or not isinstance(gap, (int, np.integer)):
        raise ModelError("%s: the gap must be an integer, not %r" % (what, gap))
    if gap < 0:
        raise ModelError("%s: the gap must be at least 0" % what)
    if gap > REGION_MAX_GAP:
        raise ModelError("%s: the gap must be at most 2^40 windows" % what)
    if n_models is None or np.ndim(threshold) == 0:
        values = [threshold] * (n_models or 1)
    else:
        values = list(threshold)
        if len(values) != n_models:
            raise ModelError("%s: %d thresholds for the panel's %d members" % (what, len(values), n_models))
    try:
        values = [float(v) for v in values]
    except (TypeError, ValueError):
        raise ModelError("%s: the threshold must be a number%s" % (what, "" if n_models is None else " or one per member"))
    if any(v != v for v in values):
        raise ModelError("%s: the threshold is NaN" % what)
    return values


def check_scan_regions(table, width, stride, threshold=0.0, gap=0, chunk=None):
    """What `scan_regions` refuses before it reads anything or touches the device: check_scan's refusals, a gap that is
    negative, above 2^40 or no integer, a NaN threshold.  -> the threshold as a float."""
    _check_scan(LmerTable, "scan-regions", table, width, stride, chunk)
    return _check_regions("scan-regions", threshold, gap)[0]


def check_panel_scan_regions(panel, width, stride, threshold=0.0, gap=0, chunk=None):
    """check_scan_regions for `scan_regions_with_panel`: check_panel_scan's refusals, the gap, and the thresholds -- one
    for all members or one per member, none of them NaN.  -> the thresholds, one float per member."""
    _check_scan(LmerPanel, "scan-regions-panel", panel, width, stride, chunk)
    return _check_regions("scan-regions-panel", threshold, gap, panel.n_models)


def _no_regions():
    return dict(first=np.empty(0, np.int64), last=np.empty(0, np.int64), summit=np.empty(0, np.int64),
                windows=np.empty(0, np.int64), peak=np.empty(0, np.float64))


def stitch_regions(per_chunk, gap):
    """The regions of a record's chunks, each found as if its chunk stood alone -> the record's.  per_chunk: one dict per
    chunk, in order, of the arrays first, last, summit, windows (integers) and peak (float64) in the RECORD's window
    indices, ascending.  A region merges with the one before it when its first window lies within gap + 1 of that one's
    last (inside a chunk none does; across chunk boundaries a merge may cascade): the merged region runs from the first
    one's `first` to the last one's `last`, its windows add up, and its peak and summit are those of the part with the
    largest peak, the earliest such part on a tie.  Only the order of the regions enters, not how they are divided among
    the dicts.  -> a dict of the same five arrays (int64, float64)."""
    parts = [c for c in per_chunk if len(c["first"])]
    if not parts:
        return _no_regions()
    first, last, summit, windows = (np.concatenate([np.asarray(c[key], dtype=np.int64) for c in parts])
                                    for key in _REGION_KEYS[:4])
    peak = np.concatenate([np.asarray(c["peak"], dtype=np.float64) for c in parts])
    begins = np.ones(len(first), dtype=bool)
    begins[1:] = first[1:] - last[:-1] > int(gap) + 1
    at = np.flatnonzero(begins)
    group = np.cumsum(begins) - 1
    top = np.flatnonzero(peak == np.maximum.reduceat(peak, at)[group])     # the parts that attain their region's peak
    top = top[np.concatenate(([True], group[top][1:] != group[top][:-1]))]  # the earliest of each region
    return dict(first=first[at], last=last[np.append(at[1:], len(first)) - 1], summit=summit[top],
                windows=np.add.reduceat(windows, at), peak=peak[top])


def _regions_in_bases(r, width, stride):
    """a region dict in window indices -> the `regions` dict of scan_regions, in bases"""
    return dict(start=r["first"] * stride, end=r["last"] * stride + width, peak=r["peak"], summit=r["summit"] * stride,
                windows=r["windows"])


def _chunk_regions(ch, col, ld, width, stride, threshold, gap, scratch):
    """The regions of column `col` of a chunk's scores, in the record's window indices -> (dict, bytes copied back,
    the region kernels' milliseconds).  Only the count and the regions themselves leave the device."""
    import torch
    ctx, nwin = ch.ctx, ch.w1 - ch.w0
    args = (ch.scores.data_ptr() + 8 * col, ld, ch.lm.data_ptr(), ch.nlm, width, stride, nwin, threshold, gap,
            scratch.data_ptr(), scratch.numel())
    n = ctx.regions_count(*args, ch.stream)
    ms = ctx.last_kernel_ms() if ch.info is not None else 0.0
    if n == 0:
        return _no_regions(), 8, ms
    ints = torch.empty((4, n), dtype=torch.int32, device=scratch.device)
    peak = torch.empty(n, dtype=torch.float64, device=scratch.device)
    ctx.regions_fill(*args, n, *(ints[k].data_ptr() for k in range(4)), peak.data_ptr(), ch.stream)
    if ch.info is not None:
        ms += ctx.last_kernel_ms()
    h = ints.cpu().numpy().astype(np.int64)
    out = dict(first=h[0] + ch.w0, last=h[1] + ch.w0, summit=h[2] + ch.w0, windows=h[3], peak=peak.cpu().numpy())
    return out, 8 + 64 + 24 * n, ms                                        # the count; fill's header; 4 int32 + 1 double


def _scan_regions_folded(folded, what, fasta_or_sequences, width, stride, thresholds, gap, device, chunk, on_chunk):
    """The body `scan_regions` and `scan_regions_with_panel` share -> [(name, [regions per member])]: the chunk loop of
    `scan`, then per chunk and member one count and one fill call on the member's column of the device scores."""
    import torch
    width, stride, gap = int(width), int(stride), int(gap)
    records = _scan_records(what, fasta_or_sequences, width)
    nm = len(thresholds)
    found = [[[] for _ in range(nm)] for _ in records]
    for ch in _scan_chunks(folded, records, width, stride, device, chunk, on_chunk is not None, score_ms=True):
        scratch = torch.empty(ch.ctx.regions_scratch_bytes(ch.nlm, ch.w1 - ch.w0), dtype=torch.uint8,
                              device=ch.scores.device)
        got = [_chunk_regions(ch, m, nm, width, stride, thresholds[m], gap, scratch) for m in range(nm)]
        for m, (r, _, _) in enumerate(got):
            found[ch.record][m].append(r)
        if on_chunk is not None:
            counts = [len(r["first"]) for r, _, _ in got]
            ch.info.update(regions=counts if folded.cols else counts[0], copied_bytes=sum(b for _, b, _ in got),
                           region_kernels_ms=sum(ms for _, _, ms in got))
            ch.info["wall_ms"] = (time.perf_counter() - ch.t0) * 1e3
            on_chunk(ch.info)
    return [(name, [_regions_in_bases(stitch_regions(per_chunk, gap), width, stride) for per_chunk in members])
            for (name, _, _), members in zip(records, found)]


def scan_regions(table, fasta_or_sequences, width, stride=1, threshold=0.0, gap=0, device=0, chunk=None, on_chunk=None):
    """The regions of a scan -> [(name, regions)] per record, in file order.  A window passes when it has a score (it
    covers only A, C, G, T) and the score `scan` returns for it, rho included, is >= threshold (a NaN never passes;
    -inf passes every scored window).  Consecutive passing windows belong to one region when at most `gap` windows lie
    between them.  regions: a dict of arrays, one element per region in ascending order: start (the first passing
    window's start), end (the last one's start + width), summit (the start of the first passing window that attains the
    peak) and windows (how many passed), int64, and peak (the largest score among them), float64.  A record shorter than
    `width` or without a passing window has empty arrays.  Whatever `chunk` and whatever precedes the record, the result
    is bit for bit this definition applied to `scan`'s output.
    The reduction runs on the device (k_regions_summaries, k_regions_fill): per chunk only the region count and the
    regions are copied back, and no per-window array exists on the host.  on_chunk(dict) (measurements): scan's keys,
    `score_kernel` and `score_kernel_ms`, `regions`, `copied_bytes` (what the chunk brought back from the device) and
    `region_kernels_ms` (HIP events)."""
    threshold = check_scan_regions(table, width, stride, threshold, gap, chunk)
    res = _scan_regions_folded(table, "scan-regions", fasta_or_sequences, width, stride, [threshold], gap, device,
                               chunk or default_scan_chunk(table.d), on_chunk)
    return [(name, members[0]) for name, members in res]


def write_regions(path, results):
    """The `scan-regions` output: one line per region, name<TAB>start<TAB>end<TAB>peak<TAB>summit<TAB>windows (0-based
    start, end exclusive, the peak at %.17g, which reads back to the same double); a record without regions writes
    nothing.  -> the regions written."""
    n = 0
    with open(path, "w") as f:
        for name, r in results:
            f.write("".join("%s\t%d\t%d\t%.17g\t%d\t%d\n" % ((name,) + row)
                            for row in zip(*(r[key].tolist() for key in REGION_FIELDS))))
            n += len(r["start"])
    return n


def read_regions(path):
    """-> [(name, start, end, peak, summit, windows)] from a file written by write_regions."""
    out = []
    with open(path) as f:
        for line in f.read().split("\n")[:-1]:
            name, a, b, v, s, n = line.rsplit("\t", 5)
            out.append((name, int(a), int(b), float(v), int(s), int(n)))
    return out


# ------------------------------------------------------------------ score distributions of a scan
DIST_MAX_THRESHOLDS = 4096  # edges one gkmhip_dist_edges launch takes
DIST_MAX_RANKS = 64         # prefixes one gkmhip_dist_digits launch carries: one target per requested rank at most
DIST_DIGIT_BITS = 13        # gkmhip_dist_digit_bits of this build (the device's own value is what a scan uses)
_KEY_SIGN, _KEY_ALL = np.uint64(1 << 63), np.uint64(0xFFFFFFFFFFFFFFFF)


def score_keys(values):
    """float64 -> uint64 keys: b ^ (b >> 63 ? ~0 : 1 << 63) of the bits b.  Ascending keys are ascending non-NaN
    doubles, -0.0 just below +0.0; the map is a bijection of the 64-bit words."""
    b = np.ascontiguousarray(values, dtype=np.float64).view(np.uint64)
    return b ^ np.where(b >> np.uint64(63), _KEY_ALL, _KEY_SIGN)


def keys_to_scores(keys):
    """The inverse of score_keys: the same bits back."""
    k = np.ascontiguousarray(keys, dtype=np.uint64)
    return (k ^ np.where(k >> np.uint64(63), _KEY_SIGN, _KEY_ALL)).view(np.float64)


def dist_level_bits(digit_bits=DIST_DIGIT_BITS):
    """The key bits each refinement level resolves for B = digit_bits: ceil(64 / B) levels, the first of
    64 - B (levels - 1) bits, every later one of B."""
    B = int(digit_bits)
    if not 1 <= B <= 64:
        raise ModelError("a level resolves 1..64 bits, not %d" % B)
    levels = -(-64 // B)
    return [64 - B * (levels - 1)] + [B] * (levels - 1)


def dist_boundaries(digit_bits=DIST_DIGIT_BITS):
    """The bits resolved after each level; the last is 64."""
    return np.cumsum(dist_level_bits(digit_bits)).tolist()


def quantile_ranks(n, q):
    """The order statistic a quantile q in [0, 1] of n values names: min(n - 1, floor(q (n - 1))) in Python floats."""
    return [min(int(n) - 1, int(math.floor(float(x) * (int(n) - 1)))) for x in q]


class _RankSearch:
    """Radix selection of order statistics from histograms of a multiset of keys that is never held: a state machine.
    `request` is what it needs next -- ("hist", prefixes, prefix_bits) or ("collect", prefixes, prefix_bits, total), or
    None when `values` holds the answer -- and feed(result) hands it over: for "hist" the counts (len(prefixes) or 1,
    2^bits of the level) of the keys that begin with each prefix by their next digit, for "collect" the `total` values
    whose keys begin with one of the prefixes, in any order.  want(n) -> the ranks, once the first histogram has given
    n.  All targets (the distinct prefixes the ranks fall under, each with the count of keys below it) descend one level
    per pass in lockstep; they are collected as soon as they hold at most collect_cap keys together, and decoded when
    all 64 bits are resolved, which ends the search whatever the values are."""

    def __init__(self, want, collect_cap, digit_bits):
        self.want, self.cap, self.bits = want, int(collect_cap), dist_level_bits(digit_bits)
        self.level, self.prefix_bits = 0, 0
        self.prefixes = np.empty(0, dtype=np.uint64)
        self.request = ("hist", self.prefixes, 0)
        self.n = self.ranks = self.values = None

    def feed(self, result):
        if self.request[0] == "collect":
            self.values, self.request = self._read_off(result), None
            return
        bits = self.bits[self.level]
        counts = np.asarray(result, dtype=np.int64).reshape(max(len(self.prefixes), 1), 1 << bits)
        if self.level == 0:
            self.n = int(counts.sum())
            self.ranks = np.asarray(self.want(self.n), dtype=np.int64).reshape(-1)
            self.target = np.zeros(len(self.ranks), dtype=np.int64)       # the row of each rank's target
            self.below = np.zeros(1, dtype=np.int64)                      # per target: the keys below it
            self.prefixes = np.zeros(1, dtype=np.uint64)
        cum = np.cumsum(counts, axis=1)
        local = self.ranks - self.below[self.target]
        digit = np.array([np.searchsorted(cum[t], r, side="right") for t, r in zip(self.target, local)], dtype=np.int64)
        if (digit >> bits).any():
            raise ModelError("the histogram of a refinement pass does not hold the windows of the pass before it")
        count = counts[self.target, digit]
        below = self.below[self.target] + cum[self.target, digit] - count
        prefix = (self.prefixes[self.target] << np.uint64(bits)) | digit.astype(np.uint64)
        self.level, self.prefix_bits = self.level + 1, self.prefix_bits + bits
        self.prefixes, first, self.target = np.unique(prefix, return_index=True, return_inverse=True)
        self.target = self.target.reshape(-1)
        self.below, self.count = below[first], count[first]
        if self.prefix_bits == 64:                                         # the prefix is the key
            self.values, self.request = keys_to_scores(self.prefixes)[self.target], None
        elif int(self.count.sum()) <= self.cap:
            self.request = ("collect", self.prefixes, self.prefix_bits, int(self.count.sum()))
        else:
            self.request = ("hist", self.prefixes, self.prefix_bits)

    def _read_off(self, values):
        keys = np.sort(score_keys(np.asarray(values, dtype=np.float64).reshape(-1)))
        run = np.repeat(self.prefixes, self.count)
        if len(keys) != len(run) or not np.array_equal(keys >> np.uint64(64 - self.prefix_bits), run):
            raise ModelError("the collected values are not the ones the histograms counted")
        start = np.cumsum(self.count) - self.count
        return keys_to_scores(keys[start[self.target] + self.ranks - self.below[self.target]])


def select_order_statistics(hist_pass, collect_pass, want, collect_cap=1 << 20, digit_bits=DIST_DIGIT_BITS, on_pass=None):
    """Order statistics of a multiset of doubles that only two callables can see -> (n, ranks, values, passes).
    hist_pass(prefixes, prefix_bits) -> counts and collect_pass(prefixes, prefix_bits, total) -> values as _RankSearch
    describes them (prefix_bits 0 and no prefix: the first level over everything); want(n) -> the ranks in 0..n-1.
    values[i] is the ranks[i]-th smallest by key, the very bits.  passes: one dict per call made, in order -- kind
    ("hist" or "collect"), prefix_bits and targets -- at most levels + 1 of them; on_pass(dict) sees each after its
    call."""
    search, passes = _RankSearch(want, collect_cap, digit_bits), []
    while search.request is not None:
        kind, prefixes, prefix_bits = search.request[:3]
        passes.append(dict(kind=kind, prefix_bits=prefix_bits, targets=len(prefixes)))
        search.feed(hist_pass(prefixes, prefix_bits) if kind == "hist" else collect_pass(*search.request[1:]))
        if on_pass is not None:
            on_pass(passes[-1])
    return search.n, search.ranks, search.values, passes


def _check_quantiles(what, q, ranks, collect_cap):
    """The refusals `scan_quantiles` adds to `scan`'s -> (q as floats or None, want): want(n) -> the ranks of a call with
    n scored windows, or the refusals that need n."""
    if (q is None) == (ranks is None):
        raise ModelError("%s: give either q or ranks" % what)
    if isinstance(collect_cap, bool) or not isinstance(collect_cap, (int, np.integer)) or collect_cap < 1:
        raise ModelError("%s: collect_cap must be an integer of at least 1" % what)
    given = np.atleast_1d(np.asarray(q if ranks is None else ranks)).reshape(-1).tolist()
    if not 1 <= len(given) <= DIST_MAX_RANKS:
        raise ModelError("%s: 1..%d %s per call, not %d" % (what, DIST_MAX_RANKS, "quantiles" if ranks is None else "ranks",
                                                           len(given)))
    if ranks is None:
        try:
            qs = [float(x) for x in given]
        except (TypeError, ValueError):
            raise ModelError("%s: a quantile must be a number" % what)
        if any(not 0.0 <= x <= 1.0 for x in qs):                           # (a NaN fails both comparisons)
            raise ModelError("%s: a quantile must lie in 0..1 (and be no NaN)" % what)
    else:
        qs = None
        if any(isinstance(r, bool) or not isinstance(r, (int, np.integer)) for r in given):
            raise ModelError("%s: a rank must be an integer" % what)
        if any(r < 0 for r in given):
            raise ModelError("%s: a rank must lie in 0..n-1" % what)

    def want(n):
        if n == 0:
            raise ModelError("%s: no window has a score" % what)
        if qs is not None:
            return quantile_ranks(n, qs)
        if any(r >= n for r in given):
            raise ModelError("%s: a rank must lie in 0..n-1; %d windows have a score" % (what, n))
        return given
    return qs, want


def _check_thresholds(what, thresholds):
    """The refusals `scan_tail_counts` adds to `scan`'s -> the thresholds as a float64 array, in the caller's order."""
    try:
        values = np.atleast_1d(np.asarray(thresholds, dtype=np.float64)).reshape(-1)
    except (TypeError, ValueError):
        raise ModelError("%s: a threshold must be a number" % what)
    if not 1 <= len(values) <= DIST_MAX_THRESHOLDS:
        raise ModelError("%s: 1..%d thresholds per call, not %d" % (what, DIST_MAX_THRESHOLDS, len(values)))
    if np.isnan(values).any():
        raise ModelError("%s: a threshold is NaN" % what)
    return values


def check_scan_tail_counts(table, width, stride, thresholds=(), chunk=None):
    """What `scan_tail_counts` refuses before it reads anything or touches the device: check_scan's refusals, no
    threshold, more than 4096 of them, a NaN among them.  -> the thresholds, float64."""
    _check_scan(LmerTable, "scan-tail", table, width, stride, chunk)
    return _check_thresholds("scan-tail", thresholds)


def check_scan_quantiles(table, width, stride, q=None, ranks=None, chunk=None, collect_cap=1 << 20):
    """What `scan_quantiles` refuses before it reads anything or touches the device: check_scan's refusals, both or
    neither of q and ranks, none or more than 64 of them, a q that is NaN or outside 0..1, a rank that is negative or no
    integer, a collect_cap below 1.  (A rank of n or more is refused once the first pass has counted n.)
    -> (q as floats, or None where ranks were given; want: n -> the ranks of a call with n scored windows)."""
    _check_scan(LmerTable, "scan-quantiles", table, width, stride, chunk)
    return _check_quantiles("scan-quantiles", q, ranks, collect_cap)


def _dist_windows(records, width, stride):
    return sum(scan_window_count(len(codes), width, stride) for _, codes, _ in records)


def _chunk_dist_args(ch, col, ld, width, stride):
    return (ch.scores.data_ptr() + 8 * col, ld, ch.lm.data_ptr(), ch.nlm, width, stride, ch.w1 - ch.w0)


def _scan_tail_folded(folded, what, fasta_or_sequences, width, stride, thresholds, device, chunk, on_chunk):
    """The body `scan_tail_counts` and `scan_tail_counts_with_panel` share -> (windows, scored (members,), counts
    (members, thresholds)): one scan, per chunk and member one k_dist_edges launch on the member's column; the
    histograms come back once, after the last chunk."""
    import torch
    width, stride = int(width), int(stride)
    records = _scan_records(what, fasta_or_sequences, width)
    nm, order = folded.cols[0] if folded.cols else 1, np.argsort(thresholds, kind="stable")
    dev = torch.device("cuda", device)
    edges = torch.from_numpy(thresholds[order]).to(dev)
    hist = torch.zeros((nm, len(thresholds) + 1), dtype=torch.int64, device=dev)
    for ch in _scan_chunks(folded, records, width, stride, device, chunk, on_chunk is not None, score_ms=True):
        nbytes = ch.ctx.dist_scratch_bytes(ch.nlm, ch.w1 - ch.w0)
        scratch = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        ms = 0.0
        for m in range(nm):
            ch.ctx.dist_edges(*_chunk_dist_args(ch, m, nm, width, stride), edges.data_ptr(), len(thresholds),
                              hist[m].data_ptr(), scratch.data_ptr(), nbytes, ch.stream)
            if on_chunk is not None:
                ms += ch.ctx.last_kernel_ms()
        if on_chunk is not None:
            ch.info.update(dist_kernels_ms=ms, copied_bytes=0)
            ch.info["wall_ms"] = (time.perf_counter() - ch.t0) * 1e3
            on_chunk(ch.info)
    suffix = np.cumsum(hist.cpu().numpy()[:, ::-1], axis=1)[:, ::-1]       # [m, b]: scores with at least b edges <= them
    counts = np.empty((nm, len(thresholds)), dtype=np.int64)
    counts[:, order] = suffix[:, 1:]
    return _dist_windows(records, width, stride), suffix[:, 0].copy(), counts


def scan_tail_counts(table, fasta_or_sequences, width, stride=1, thresholds=(), device=0, chunk=None, on_chunk=None):
    """How many scored windows of a scan reach each threshold, all records pooled -> dict(scored, unscored, thresholds,
    counts).  A window is scored when it covers only A, C, G, T and `scan`'s score for it is no NaN; counts[i] (int64, the
    caller's order) is the number of scored windows with score >= thresholds[i], `scan_regions`' own pass rule: the sum
    of `windows` over scan_regions(threshold=thresholds[i], gap=0).  -inf counts every scored window, +inf only +inf
    scores.  One scan: the host sorts the thresholds, k_dist_edges bins every chunk's scores by them on the device, and
    only the histogram of len(thresholds) + 1 counters comes back, once.  on_chunk(dict) (measurements): scan's keys,
    `score_kernel`, `score_kernel_ms`, `dist_kernels_ms` (HIP events) and `copied_bytes` (0: nothing per chunk)."""
    thresholds = check_scan_tail_counts(table, width, stride, thresholds, chunk)
    windows, scored, counts = _scan_tail_folded(table, "scan-tail", fasta_or_sequences, width, stride, thresholds, device,
                                                chunk or default_scan_chunk(table.d), on_chunk)
    return dict(scored=int(scored[0]), unscored=windows - int(scored[0]), thresholds=thresholds, counts=counts[0])


def _scan_quantiles_folded(folded, what, fasta_or_sequences, width, stride, wants, collect_cap, device, chunk, on_pass):
    """The body `scan_quantiles` and `scan_quantiles_with_panel` share -> (windows, [the finished _RankSearch of each
    member], passes).  Every pass is one chunk loop of `scan` that serves all members still searching, each with its
    own request: per chunk and member one k_dist_digits or k_dist_collect launch on the member's column."""
    import torch
    width, stride = int(width), int(stride)
    records = _scan_records(what, fasta_or_sequences, width)
    nm = len(wants)
    dev = torch.device("cuda", device)
    ctx = dv.cached_context(*folded.kernel_params(), device=device)
    searches = [_RankSearch(want, collect_cap, ctx.dist_digit_bits()) for want in wants]
    passes = []
    while any(s.request is not None for s in searches):
        active = [(m, s) for m, s in enumerate(searches) if s.request is not None]
        bufs = {}
        for m, s in active:
            if s.request[0] == "hist":
                bufs[m] = (torch.zeros(max(len(s.prefixes), 1) << s.bits[s.level], dtype=torch.int64, device=dev),)
            else:
                bufs[m] = (torch.empty(s.request[3], dtype=torch.float64, device=dev),
                           torch.zeros(1, dtype=torch.int64, device=dev))
        ms = scan_ms = 0.0
        for ch in _scan_chunks(folded, records, width, stride, device, chunk, on_pass is not None, score_ms=True):
            nbytes = ctx.dist_scratch_bytes(ch.nlm, ch.w1 - ch.w0)
            scratch = torch.empty(nbytes, dtype=torch.uint8, device=dev)
            if on_pass is not None:
                scan_ms += ch.info["profile_kernel_ms"] + ch.info["score_kernel_ms"]
            for m, s in active:
                args = _chunk_dist_args(ch, m, nm, width, stride) + (s.request[1], s.request[2])
                if s.request[0] == "hist":
                    ctx.dist_digits(*args, bufs[m][0].data_ptr(), scratch.data_ptr(), nbytes, ch.stream)
                else:
                    ctx.dist_collect(*args, bufs[m][0].data_ptr(), s.request[3], bufs[m][1].data_ptr(), scratch.data_ptr(),
                                     nbytes, ch.stream)
                if on_pass is not None:
                    ms += ctx.last_kernel_ms()
        info = dict(kind=[s.request[0] for _, s in active], prefix_bits=[s.request[2] for _, s in active],
                    targets=[len(s.request[1]) for _, s in active], copied_bytes=0)
        if on_pass is not None:
            info.update(dist_kernels_ms=ms, scan_kernels_ms=scan_ms)
        for m, s in active:
            if s.request[0] == "collect":
                found = int(bufs[m][1].item())
                if found != s.request[3]:
                    raise dv.GkmError("%s: k_dist_collect found %d values where the histograms counted %d"
                                      % (what, found, s.request[3]))
                info["copied_bytes"] += 8
            info["copied_bytes"] += 8 * bufs[m][0].numel()
            s.feed(bufs[m][0].cpu().numpy())
        if not folded.cols:
            info.update(kind=info["kind"][0], prefix_bits=info["prefix_bits"][0], targets=info["targets"][0])
        passes.append(info)
        if on_pass is not None:
            on_pass(info)
    return _dist_windows(records, width, stride), searches, passes


def scan_quantiles(table, fasta_or_sequences, width, stride=1, q=None, ranks=None, device=0, chunk=None,
                   collect_cap=1 << 20, on_pass=None):
    """Exact order statistics of a scan's scores, all records pooled -> dict(scored, unscored, q, ranks, values, passes).
    Give either q (quantiles in 0..1) or ranks (0..n-1), at most 64, in any order, duplicates allowed.  With n the scored
    windows of the call (see scan_tail_counts), order statistic r is the r-th smallest score by key (score_keys:
    numerical order, -0.0 below +0.0) and a quantile q is order statistic min(n - 1, floor(q (n - 1))) -- not
    np.quantile, which interpolates.  values[i] is bit for bit that element of `scan`'s own output, whatever `chunk`,
    `collect_cap` and the order of the requests.  It is an error if no window has a score.
    The scores are never kept: radix selection over the keys re-scans instead.  Pass 0 counts every scored window by its
    key's first digit (k_dist_digits), which gives n and places each rank in a bin; the distinct bins are the targets,
    refined in lockstep one level per pass until they hold at most collect_cap windows together -- then one more pass
    gathers exactly those scores (k_dist_collect) and the host sorts them -- or until all 64 bits are resolved and the
    prefix is the value.  At most levels + 1 passes, each a full scan; only histograms and the collected values leave the
    device.  passes / on_pass(dict): per pass its kind ("hist" or "collect"), prefix_bits, targets, and what it brought
    back (copied_bytes); with on_pass also dist_kernels_ms and scan_kernels_ms (k_scan_profiles + k_scan_score), HIP
    events summed over the pass's chunks."""
    qs, want = check_scan_quantiles(table, width, stride, q, ranks, chunk, collect_cap)
    windows, (s,), passes = _scan_quantiles_folded(table, "scan-quantiles", fasta_or_sequences, width, stride, [want],
                                                   int(collect_cap), device, chunk or default_scan_chunk(table.d), on_pass)
    return dict(scored=s.n, unscored=windows - s.n, q=qs, ranks=s.ranks, values=s.values, passes=passes)


def write_tail_counts(path, result):
    """The `scan-tail` output: #scored<TAB>n<TAB>unscored<TAB>m, then threshold<TAB>count per threshold in the caller's
    order, the threshold at %.17g, which reads back to the same double."""
    with open(path, "w") as f:
        f.write("#scored\t%d\tunscored\t%d\n" % (result["scored"], result["unscored"]))
        f.write("".join("%.17g\t%d\n" % row for row in zip(result["thresholds"].tolist(), result["counts"].tolist())))


def _read_dist(path, nlead, convert):
    """-> ([the fields of the #scored lines], [the converted fields of the other lines]); nlead: names in front"""
    heads, rows = [], []
    with open(path) as f:
        for line in f.read().split("\n")[:-1]:
            fields = line.split("\t")
            if fields[nlead] == "#scored":
                heads.append(tuple(fields[:nlead]) + (int(fields[nlead + 1]), int(fields[nlead + 3])))
            else:
                rows.append(tuple(fields[:nlead]) + tuple(c(x) for c, x in zip(convert, fields[nlead:])))
    return heads, rows


def read_tail_counts(path):
    """-> dict(scored, unscored, thresholds, counts) from a file written by write_tail_counts."""
    (head,), rows = _read_dist(path, 0, (float, int))
    return dict(scored=head[0], unscored=head[1], thresholds=np.array([r[0] for r in rows], dtype=np.float64),
                counts=np.array([r[1] for r in rows], dtype=np.int64))


def _q_text(q, i):
    return "-" if q is None else "%.17g" % q[i]


def _q_value(text):
    return None if text == "-" else float(text)


def write_quantiles(path, result):
    """The `scan-quantiles` output: #scored<TAB>n<TAB>unscored<TAB>m, then q<TAB>rank<TAB>value per request in the
    caller's order, q ("-" when ranks were asked for) and the value at %.17g."""
    with open(path, "w") as f:
        f.write("#scored\t%d\tunscored\t%d\n" % (result["scored"], result["unscored"]))
        for i, (r, v) in enumerate(zip(result["ranks"].tolist(), result["values"].tolist())):
            f.write("%s\t%d\t%.17g\n" % (_q_text(result["q"], i), r, v))


def read_quantiles(path):
    """-> dict(scored, unscored, q, ranks, values) from a file written by write_quantiles (q: None where "-")."""
    (head,), rows = _read_dist(path, 0, (_q_value, int, float))
    q = [r[0] for r in rows]
    return dict(scored=head[0], unscored=head[1], q=None if None in q else q,
                ranks=np.array([r[1] for r in rows], dtype=np.int64), values=np.array([r[2] for r in rows], dtype=np.float64))


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


def default_panel_scan_chunk(d, n_models, budget=BLOCK_BYTES):
    """Bases per chunk of scan_with_panel: default_scan_chunk's bytes per base and the window's n_models doubles."""
    return int(budget // (8 * (int(d) + 1) + 64 + 8 * int(n_models)))


def check_panel_scan(panel, width, stride, chunk=None):
    """What `scan_with_panel` refuses before it reads anything or touches the device (check_scan's refusals)."""
    _check_scan(LmerPanel, "scan-panel", panel, width, stride, chunk)


def scan_with_panel(panel, fasta_or_sequences, width, stride=1, device=0, chunk=None, on_chunk=None):
    """`scan` for every member of a panel -> [(name, starts, scores (windows, n_models))]: column m is scan's result for
    member m, bit for bit, whatever `chunk` and whatever precedes the record; a window over a character other than A, C,
    G, T is NaN in every column.  Per chunk the l-mer words and the windows' self profiles once (k_scan_profiles, the
    hot kernel of a scan, depends on the shared parameters only), then one k_panel_scan_score launch.
    chunk: bases per device chunk (default_panel_scan_chunk).  on_chunk(dict) (measurements): scan's keys, `models`,
    `score_kernel` and `score_kernel_ms`."""
    check_panel_scan(panel, width, stride, chunk)
    return _scan_folded(panel, "scan-panel", fasta_or_sequences, width, stride, device,
                        chunk or default_panel_scan_chunk(panel.d, panel.n_models), on_chunk)


def scan_regions_with_panel(panel, fasta_or_sequences, width, stride=1, threshold=0.0, gap=0, device=0, chunk=None,
                            on_chunk=None):
    """`scan_regions` for every member of a panel -> [(name, [regions of member 0, of member 1, ...])]: member m's regions
    are scan_regions' for panel.table(m), bit for bit.  threshold: one for all members or one per member.  Per chunk the
    profiles and k_panel_scan_score run once; the region calls run once per member on its column of the device result
    (leading dimension n_models, no copy).  on_chunk(dict): scan_with_panel's keys, `regions` (one count per member),
    `copied_bytes` and `region_kernels_ms` (both summed over the members)."""
    thresholds = check_panel_scan_regions(panel, width, stride, threshold, gap, chunk)
    return _scan_regions_folded(panel, "scan-regions-panel", fasta_or_sequences, width, stride, thresholds, gap, device,
                                chunk or default_panel_scan_chunk(panel.d, panel.n_models), on_chunk)


def write_panel_regions(path, panel_names, results):
    """The `scan-regions-panel` output: write_regions' line with the member's name in front,
    member<TAB>name<TAB>start<TAB>end<TAB>peak<TAB>summit<TAB>windows; records in file order, the members of a record in
    panel order.  -> the regions written."""
    n = 0
    with open(path, "w") as f:
        for name, members in results:
            for member, r in zip(panel_names, members):
                f.write("".join("%s\t%s\t%d\t%d\t%.17g\t%d\t%d\n" % ((member, name) + row)
                                for row in zip(*(r[key].tolist() for key in REGION_FIELDS))))
                n += len(r["start"])
    return n


def read_panel_regions(path):
    """-> [(member, name, start, end, peak, summit, windows)] from a file written by write_panel_regions."""
    out = []
    for lead, a, b, v, s, n in read_regions(path):
        out.append(tuple(lead.split("\t", 1)) + (a, b, v, s, n))
    return out


def check_panel_scan_tail_counts(panel, width, stride, thresholds=(), chunk=None):
    """check_scan_tail_counts for `scan_tail_counts_with_panel` -> the thresholds, float64."""
    _check_scan(LmerPanel, "scan-tail-panel", panel, width, stride, chunk)
    return _check_thresholds("scan-tail-panel", thresholds)


def check_panel_scan_quantiles(panel, width, stride, q=None, ranks=None, chunk=None, collect_cap=1 << 20):
    """check_scan_quantiles for `scan_quantiles_with_panel`."""
    _check_scan(LmerPanel, "scan-quantiles-panel", panel, width, stride, chunk)
    return _check_quantiles("scan-quantiles-panel", q, ranks, collect_cap)


def scan_tail_counts_with_panel(panel, fasta_or_sequences, width, stride=1, thresholds=(), device=0, chunk=None,
                                on_chunk=None):
    """`scan_tail_counts` for every member of a panel, the same thresholds for all -> dict(scored, unscored (int64, one
    per member), thresholds, counts (n_models, thresholds)): row m is scan_tail_counts' result for panel.table(m), bit
    for bit.  One scan serves all members: k_panel_scan_score once per chunk, then one k_dist_edges launch per member on
    its column of the device result.  on_chunk(dict): scan_with_panel's keys, `dist_kernels_ms` and `copied_bytes`."""
    thresholds = check_panel_scan_tail_counts(panel, width, stride, thresholds, chunk)
    windows, scored, counts = _scan_tail_folded(panel, "scan-tail-panel", fasta_or_sequences, width, stride, thresholds,
                                                device, chunk or default_panel_scan_chunk(panel.d, panel.n_models), on_chunk)
    return dict(scored=scored, unscored=windows - scored, thresholds=thresholds, counts=counts)


def scan_quantiles_with_panel(panel, fasta_or_sequences, width, stride=1, q=None, ranks=None, device=0, chunk=None,
                              collect_cap=1 << 20, on_pass=None):
    """`scan_quantiles` for every member of a panel, the same requests for all -> dict(scored, unscored (int64, one per
    member), q, ranks, values (both (n_models, requests)), passes): row m is scan_quantiles' result for panel.table(m), bit
    for bit.  One chunk loop per pass serves all members; each carries its own targets and collects when ITS targets fit
    collect_cap, so a pass may count for one member and collect for another.  passes / on_pass(dict): kind, prefix_bits
    and targets are lists, one entry per member still searching; the other keys are summed over them."""
    qs, want = check_panel_scan_quantiles(panel, width, stride, q, ranks, chunk, collect_cap)
    windows, found, passes = _scan_quantiles_folded(panel, "scan-quantiles-panel", fasta_or_sequences, width, stride,
                                                    [want] * panel.n_models, int(collect_cap), device,
                                                    chunk or default_panel_scan_chunk(panel.d, panel.n_models), on_pass)
    scored = np.array([s.n for s in found], dtype=np.int64)
    return dict(scored=scored, unscored=windows - scored, q=qs, ranks=np.stack([s.ranks for s in found]),
                values=np.stack([s.values for s in found]), passes=passes)


def write_panel_tail_counts(path, panel_names, result):
    """The `scan-tail-panel` output: write_tail_counts' lines per member in panel order, the member's name in front."""
    with open(path, "w") as f:
        for m, member in enumerate(panel_names):
            f.write("%s\t#scored\t%d\tunscored\t%d\n" % (member, result["scored"][m], result["unscored"][m]))
            f.write("".join("%s\t%.17g\t%d\n" % ((member,) + row)
                            for row in zip(result["thresholds"].tolist(), result["counts"][m].tolist())))


def read_panel_tail_counts(path):
    """-> ([(member, scored, unscored)], [(member, threshold, count)]) from a file written by write_panel_tail_counts."""
    return _read_dist(path, 1, (float, int))


def write_panel_quantiles(path, panel_names, result):
    """The `scan-quantiles-panel` output: write_quantiles' lines per member in panel order, the member's name in front."""
    with open(path, "w") as f:
        for m, member in enumerate(panel_names):
            f.write("%s\t#scored\t%d\tunscored\t%d\n" % (member, result["scored"][m], result["unscored"][m]))
            for i, (r, v) in enumerate(zip(result["ranks"][m].tolist(), result["values"][m].tolist())):
                f.write("%s\t%s\t%d\t%.17g\n" % (member, _q_text(result["q"], i), r, v))


def read_panel_quantiles(path):
    """-> ([(member, scored, unscored)], [(member, q or None, rank, value)]) from a file written by
    write_panel_quantiles."""
    return _read_dist(path, 1, (_q_value, int, float))


def check_panel_delta(panel, variants=None, records=None, chunk=None):
    """What `delta_with_panel` and `delta_saturation_with_panel` refuse before they touch the device (check_delta's
    refusals)."""
    _check_delta(LmerPanel, "delta-panel", panel, variants, records, chunk)


def delta_with_panel(panel, fasta_or_sequences, variants, device=0, chunk=None, on_chunk=None):
    """`delta` for every member of a panel -> float64 (len(variants), n_models): column m is delta's result for member m,
    bit for bit (NaN in every column where the context holds a character other than A, C, G, T; +0.0 where the alleles
    are the same).  The variants are resolved, sorted and checked once -- most of delta's time -- and each chunk is one
    k_panel_delta_variants launch.  on_chunk(dict) (measurements): delta's keys and `models`."""
    check_panel_delta(panel, chunk=chunk)
    return _delta_values(panel, fasta_or_sequences, variants, device, chunk, on_chunk)


def delta_saturation_with_panel(panel, fasta_or_sequences, device=0, chunk=None, on_chunk=None):
    """`delta_saturation` for every member of a panel -> [(name, (T, 4, n_models) float64)]: [:, :, m] is
    delta_saturation's map for member m, bit for bit, and D[t, b, m] is delta_with_panel's value of that SNV.
    on_chunk(dict) (measurements): delta_saturation's keys and `models`."""
    check_panel_delta(panel, chunk=chunk)
    return _saturation_folded(panel, fasta_or_sequences, device, chunk or
                              max(delta_min_chunk(panel.L), int(BLOCK_BYTES // (16 + 32 * panel.n_models))), on_chunk)


def _panel_row(lead, values):
    return "\t".join(lead + ["nan" if x != x else "%.17g" % x for x in values]) + "\n"


def write_panel_scores(path, panel_names, names, scores):
    """The `predict-panel` output: the header #name<TAB>member names, then name<TAB>one score per member at %.17g."""
    with open(path, "w") as f:
        f.write("#" + "\t".join(["name"] + list(panel_names)) + "\n")
        for name, row in zip(names, np.asarray(scores, dtype=np.float64).tolist()):
            f.write(_panel_row([str(name)], row))


def write_panel_scan(path, panel_names, results, width):
    """The `scan-panel` output: the header #name<TAB>start<TAB>end<TAB>member names, then `scan`'s leading columns and
    one score per member at %.17g; windows without a score (NaN) are left out.  -> how many were left out."""
    omitted = 0
    with open(path, "w") as f:
        f.write("#" + "\t".join(["name", "start", "end"] + list(panel_names)) + "\n")
        for name, starts, scores in results:
            keep = ~np.isnan(scores).any(axis=1)
            omitted += int((~keep).sum())
            for i in range(0, len(starts), 1 << 14):
                k = keep[i:i + (1 << 14)]
                f.write("".join(_panel_row([name, "%d" % a, "%d" % (a + width)], row) for a, row in
                                zip(starts[i:i + (1 << 14)][k].tolist(), scores[i:i + (1 << 14)][k].tolist())))
    return omitted


def write_panel_delta(path, panel_names, variants, values):
    """The `delta-panel` output: the header #name<TAB>pos<TAB>ref<TAB>alt[<TAB>id]<TAB>member names (id when the first
    variant carries one), then write_delta's leading columns and one delta per member at %.17g, nan where there is none."""
    with open(path, "w") as f:
        lead = ["name", "pos", "ref", "alt"] + (["id"] if len(variants) and len(variants[0]) > 4 else [])
        f.write("#" + "\t".join(lead + list(panel_names)) + "\n")
        for v, row in zip(variants, np.asarray(values, dtype=np.float64).tolist()):
            f.write(_panel_row([str(v[0]), "%d" % (int(v[1]) + 1), v[2] or ".", v[3] or "."] + [str(c) for c in v[4:5]],
                               row))


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


# ------------------------------------------------------------------ command line
def _add_train_options(p, svr):
    p.add_argument("-t", "--kernel-type", type=int, default=4, help="kernel type 0..5 (default: 4)")
    p.add_argument("-L", "--full-word-length", type=int, default=10, help="full word length (default: 10)")
    p.add_argument("-k", "--non-gap-length", type=int, default=6, help="non-gap positions (default: 6)")
    p.add_argument("-d", "--max-num-gaps", type=int, default=3, help="max gaps (default: 3)")
    p.add_argument("-M", "--init-decay", type=int, default=50, help="initial value of the decay, -t 4/5 (default: 50)")
    p.add_argument("-H", "--half-life-decay", type=float, default=50, help="half life of the decay, -t 4/5 (default: 50)")
    p.add_argument("-G", "--rbf-gamma", type=float, default=1.0, help="gamma for RBF kernels, -t 3/5 (default: 1.0)")
    p.add_argument("-C", "--regularization", type=float, default=1.0, help="regularization parameter C (default: 1.0)")
    if svr:
        p.add_argument("-p", "--epsilon", type=float, default=0.1, help="epsilon of the insensitive loss (default: 0.1)")
    p.add_argument("-e", "--precision", type=float, default=0.001, help="precision parameter epsilon (default: 0.001)")
    p.add_argument("-u", "--shrinking", type=int, choices=(0, 1), default=0, help="shrinking heuristics (default: 0)")


def _add_arguments(p, *positionals, block=True):
    p.add_argument("--device", type=int, default=0, help="GPU (default: 0)")
    if block:
        p.add_argument("--block", type=int, default=None, help="queries per device block (default: from device memory)")
    for name in positionals:
        p.add_argument(name)


def _add_region_options(p, threshold_help):
    p.add_argument("--width", type=int, required=True, help="bases per window (L..2047)")
    p.add_argument("--stride", type=int, default=1, help="bases between window starts (default: 1)")
    p.add_argument("--threshold", default="0", help=threshold_help)
    p.add_argument("--gap", type=int, default=0, help="windows below the threshold a region may bridge (default: 0)")
    p.add_argument("--chunk", type=int, default=None, help="bases per device chunk (default: from device memory)")


def region_thresholds(text, panel=False):
    """--threshold -> a float, or for a panel a list of them when commas separate several."""
    try:
        values = [float(x) for x in text.split(",")] if panel else [float(text)]
    except ValueError:
        raise ModelError("--threshold: %r is no number%s" % (text, " (or comma-separated numbers)" if panel else ""))
    return values[0] if len(values) == 1 else values


def _add_dist_options(p, quantiles):
    p.add_argument("--width", type=int, required=True, help="bases per window (L..2047)")
    p.add_argument("--stride", type=int, default=1, help="bases between window starts (default: 1)")
    p.add_argument("--chunk", type=int, default=None, help="bases per device chunk (default: from device memory)")
    if quantiles:
        p.add_argument("--q", default=None, help="comma-separated quantiles in 0..1, at most 64")
        p.add_argument("--ranks", default=None, help="comma-separated order statistics 0..n-1 instead of --q")
        p.add_argument("--collect-cap", type=int, default=1 << 20,
                       help="scores the last pass may gather on the device (default: 2^20)")
    else:
        p.add_argument("--thresholds", default="", help="comma-separated scores, at most 4096")


def dist_list(option, text, convert):
    """A comma-separated option -> its values, or None where it was not given."""
    if text is None:
        return None
    try:
        return [convert(x) for x in text.split(",")] if text else []
    except ValueError:
        raise ModelError("%s: %r is no comma-separated list of %s" % (option, text,
                                                                     "integers" if convert is int else "numbers"))


def build_parser():
    p = argparse.ArgumentParser(prog="python -m gkmqc_amd.gkmpredict",
                                description="train a gkm-SVM on all sequences / score FASTA sequences with it (MI355X)")
    sub = p.add_subparsers(dest="cmd", required=True)
    t = sub.add_parser("train", help="train on pos.fa + neg.fa and write a model file")
    _add_train_options(t, svr=False)
    _add_arguments(t, "pos_fa", "neg_fa", "model", block=False)
    v = sub.add_parser("train-svr", help="fit an epsilon-SVR to seqs.fa and targets.txt (name<TAB>value per record) "
                                         "and write a model file")
    _add_train_options(v, svr=True)
    _add_arguments(v, "seqs_fa", "targets", "model", block=False)
    q = sub.add_parser("predict", help="score the sequences of query.fa: name<TAB>score per line, in file order")
    _add_arguments(q, "query_fa", "model", "output")
    x = sub.add_parser("explain", help="per-base importance of the sequences of query.fa: name<TAB>v0,v1,... per line")
    _add_arguments(x, "query_fa", "model", "output")
    z = sub.add_parser("ism", help="in-silico mutagenesis of the sequences of query.fa: name<TAB>4T values per line, "
                                   "position-major, columns A, C, G, T")
    _add_arguments(z, "query_fa", "model", "output")
    u = sub.add_parser("mutant-scores", help="the score of every single-base mutant of the sequences of query.fa, RBF "
                                             "models included: name<TAB>4T values per line, position-major, columns "
                                             "A, C, G, T (the ism format)")
    _add_arguments(u, "query_fa", "model", "output")
    h = sub.add_parser("hypothetical", help="hypothetical importance of the sequences of query.fa: name<TAB>4T values per "
                                            "line, position-major, columns A, C, G, T (the ism format)")
    _add_arguments(h, "query_fa", "model", "output")
    w = sub.add_parser("weights", help="fold a model into its l-mer weight table: a `# key value` header, then "
                                       "LMER<TAB>weight per canonical l-mer")
    _add_arguments(w, "model", "output", block=False)
    r = sub.add_parser("predict-table", help="score the sequences of query.fa from an l-mer weight table: name<TAB>score "
                                             "per line, in file order (the predict format)")
    _add_arguments(r, "query_fa", "weights", "output")
    n = sub.add_parser("scan", help="score every window of --width bases of the sequences of seqs.fa (any length) from an "
                                    "l-mer weight table: name<TAB>start<TAB>end<TAB>score per window, windows over a "
                                    "non-ACGT character left out")
    n.add_argument("--width", type=int, required=True, help="bases per window (L..2047)")
    n.add_argument("--stride", type=int, default=1, help="bases between window starts (default: 1)")
    n.add_argument("--chunk", type=int, default=None, help="bases per device chunk (default: from device memory)")
    _add_arguments(n, "seqs_fa", "weights", "output", block=False)
    nr = sub.add_parser("scan-regions", help="scan the sequences of seqs.fa with an l-mer weight table and report the "
                                             "regions whose windows score at least --threshold: name<TAB>start<TAB>end"
                                             "<TAB>peak<TAB>summit<TAB>windows per region")
    _add_region_options(nr, "the score a window must reach (default: 0, the decision boundary)")
    _add_arguments(nr, "weights", "seqs_fa", "output", block=False)
    i = sub.add_parser("importance-table", help="fold a model into its per-base importance table: one value per (l-mer, "
                                                "offset), a binary .npz file")
    _add_arguments(i, "model", "output", block=False)
    e = sub.add_parser("explain-table", help="per-base importance of the sequences of query.fa from an importance "
                                             "table: name<TAB>v0,v1,... per line (the explain format)")
    _add_arguments(e, "query_fa", "table", "output")
    y = sub.add_parser("hypothetical-table", help="hypothetical importance of the sequences of query.fa from an "
                                                  "importance table: name<TAB>4T values per line (the ism format)")
    _add_arguments(y, "query_fa", "table", "output")
    g = sub.add_parser("delta", help="the effect of the variants of variants.tsv (name<TAB>pos<TAB>ref<TAB>alt[<TAB>id], "
                                     "pos 1-based) on the sequences of seqs.fa (any length) from an l-mer weight table "
                                     "(deltaSVM): the same columns plus the delta, nan over a non-ACGT character")
    g.add_argument("--chunk", type=int, default=None, help="bases per device chunk (default: from device memory)")
    _add_arguments(g, "weights", "seqs_fa", "variants", "output", block=False)
    s = sub.add_parser("delta-saturation", help="the effect of every single-base substitution of the sequences of seqs.fa "
                                                "from an l-mer weight table: name<TAB>pos<TAB>ref<TAB>dA<TAB>dC<TAB>dG"
                                                "<TAB>dT per position, positions near a non-ACGT character left out")
    s.add_argument("--chunk", type=int, default=None, help="bases per device chunk (default: from device memory)")
    _add_arguments(s, "weights", "seqs_fa", "output", block=False)
    pn = sub.add_parser("panel", help="join 1..64 l-mer weight tables that share their kernel parameters into a panel, a "
                                      "binary .npz file; the members are named after the files")
    pn.add_argument("--names", default=None, help="comma-separated member names (default: the files' basenames)")
    pn.add_argument("output")
    pn.add_argument("weights", nargs="+")
    pp = sub.add_parser("predict-panel", help="score the sequences of query.fa with every member of a panel: a header, "
                                              "then name<TAB>one score per member")
    _add_arguments(pp, "query_fa", "panel", "output")
    ps = sub.add_parser("scan-panel", help="scan the sequences of seqs.fa with every member of a panel: a header, then "
                                           "name<TAB>start<TAB>end<TAB>one score per member")
    ps.add_argument("--width", type=int, required=True, help="bases per window (L..2047)")
    ps.add_argument("--stride", type=int, default=1, help="bases between window starts (default: 1)")
    ps.add_argument("--chunk", type=int, default=None, help="bases per device chunk (default: from device memory)")
    _add_arguments(ps, "seqs_fa", "panel", "output", block=False)
    pr = sub.add_parser("scan-regions-panel", help="scan-regions for every member of a panel: the member's name, then "
                                                   "scan-regions' columns")
    _add_region_options(pr, "one value for all members or one per member, comma-separated (default: 0)")
    _add_arguments(pr, "panel", "seqs_fa", "output", block=False)
    for name, panel, quantiles, what in (
            ("scan-tail", False, False, "how many scored windows of a scan reach each of --thresholds, all records "
                                        "pooled: #scored<TAB>n<TAB>unscored<TAB>m, then threshold<TAB>count"),
            ("scan-quantiles", False, True, "exact quantiles (--q) or order statistics (--ranks) of a scan's scores, all "
                                            "records pooled: #scored<TAB>n<TAB>unscored<TAB>m, then q<TAB>rank<TAB>value"),
            ("scan-tail-panel", True, False, "scan-tail for every member of a panel: the member's name in front"),
            ("scan-quantiles-panel", True, True, "scan-quantiles for every member of a panel: the member's name in front")):
        ds = sub.add_parser(name, help=what)
        _add_dist_options(ds, quantiles)
        _add_arguments(ds, "panel" if panel else "weights", "seqs_fa", "output", block=False)
    pd = sub.add_parser("delta-panel", help="the effect of the variants of variants.tsv on the sequences of seqs.fa for "
                                            "every member of a panel: a header, then the variant's columns and one delta "
                                            "per member")
    pd.add_argument("--chunk", type=int, default=None, help="bases per device chunk (default: from device memory)")
    _add_arguments(pd, "seqs_fa", "variants", "panel", "output", block=False)
    return p


def panel_member_names(paths, names=None):
    """The member names of `panel`: --names split at commas, or the weight files' basenames."""
    if names is None:
        return [os.path.basename(path) for path in paths]
    return names.split(",")


def check_train_args(a):
    """The argument checks `train` makes before it reads anything; an error message or None."""
    bad = dv.check_parameters(a.kernel_type, a.full_word_length, a.non_gap_length, a.max_num_gaps)
    if bad:
        return bad
    if not 0 <= a.init_decay <= 255:
        return "-M must lie in 0..255"
    if not (a.regularization > 0 and a.precision > 0):
        return "-C and -e must be positive"
    if a.cmd == "train-svr" and not (np.isfinite(a.epsilon) and a.epsilon >= 0):
        return "-p must be finite and at least 0"
    return None


def write_scores(path, names, scores):
    """The `predict` (and `predict-table`) output: one line per query, name<TAB>score with a repr() float."""
    with open(path, "w") as f:
        for name, s in zip(names, scores):
            f.write("%s\t%r\n" % (name, float(s)))


# the commands that serve a query file: command -> (compute, writer).  compute checks that it serves the model before it
# parses the query file, and touches the GPU only after both.
_QUERY_COMMANDS = {
    "predict": (score, write_scores),
    "explain": (explain, write_explanation),
    "ism": (ism, write_ism),
    "mutant-scores": (mutant_scores, write_ism),
    "hypothetical": (hypothetical, write_ism),
    "predict-table": (score_with_table, write_scores),
    "explain-table": (explain_with_table, write_explanation),
    "hypothetical-table": (hypothetical_with_table, write_ism),
}


def main(argv=None):
    a = build_parser().parse_args(argv)
    try:
        if a.cmd in ("train", "train-svr"):
            svr = a.cmd == "train-svr"
            bad = check_train_args(a)
            if bad:
                raise ModelError(bad)
            inputs = (a.seqs_fa, a.targets) if svr else (a.pos_fa, a.neg_fa)
            for path in inputs:
                if not os.path.isfile(path):
                    raise ModelError("cannot read %s" % path)
            kernel_args = (a.kernel_type, a.full_word_length, a.non_gap_length, a.max_num_gaps, a.init_decay,
                           a.half_life_decay, a.rbf_gamma, a.regularization)
            if svr:
                m = train_svr(*inputs, *kernel_args, a.epsilon, a.precision, bool(a.shrinking), a.device)
            else:
                m = train(*inputs, *kernel_args, a.precision, bool(a.shrinking), a.device)
            m.save(a.model)
            if svr:
                print("%d support vectors, rho %r (LIBSVM's: %r), %d iterations -> %s"
                      % (m.n_sv, m.rho, -m.rho, m.n_iter, a.model), file=sys.stderr)
            else:
                print("%d support vectors (%d negative, %d positive), rho %r -> %s"
                      % (m.n_sv, m.n0, m.n_sv - m.n0, m.rho, a.model), file=sys.stderr)
        elif a.cmd == "weights":
            m = load(a.model)
            check_table_model(m)
            lmer_weights(m, a.device).save(a.output)
        elif a.cmd == "importance-table":
            m = load(a.model)
            check_explainable(m, "importance-table")
            lmer_importance(m, a.device).save(a.output)
        elif a.cmd == "scan":
            if not os.path.isfile(a.seqs_fa):
                raise ModelError("cannot read %s" % a.seqs_fa)
            tab = load_lmer_table(a.weights)
            check_scan(tab, a.width, a.stride, a.chunk)
            results = scan(tab, a.seqs_fa, a.width, a.stride, a.device, a.chunk)
            tmp = a.output + ".tmp"
            omitted = write_scan(tmp, results, a.width)
            os.replace(tmp, a.output)
            print("%d windows scored, %d over a non-ACGT character left out -> %s"
                  % (sum(len(r[1]) for r in results) - omitted, omitted, a.output), file=sys.stderr)
        elif a.cmd in ("scan-regions", "scan-regions-panel"):
            if not os.path.isfile(a.seqs_fa):
                raise ModelError("cannot read %s" % a.seqs_fa)
            panel = a.cmd == "scan-regions-panel"
            threshold = region_thresholds(a.threshold, panel)
            tmp = a.output + ".tmp"
            if panel:
                folded = load_lmer_panel(a.panel)
                check_panel_scan_regions(folded, a.width, a.stride, threshold, a.gap, a.chunk)
                results = scan_regions_with_panel(folded, a.seqs_fa, a.width, a.stride, threshold, a.gap, a.device, a.chunk)
                n = write_panel_regions(tmp, folded.names, results)
            else:
                folded = load_lmer_table(a.weights)
                check_scan_regions(folded, a.width, a.stride, threshold, a.gap, a.chunk)
                results = scan_regions(folded, a.seqs_fa, a.width, a.stride, threshold, a.gap, a.device, a.chunk)
                n = write_regions(tmp, results)
            os.replace(tmp, a.output)
            print("%d regions at a threshold of %s, gap %d -> %s" % (n, a.threshold, a.gap, a.output), file=sys.stderr)
        elif a.cmd in ("scan-tail", "scan-tail-panel", "scan-quantiles", "scan-quantiles-panel"):
            if not os.path.isfile(a.seqs_fa):
                raise ModelError("cannot read %s" % a.seqs_fa)
            panel = a.cmd.endswith("-panel")
            folded = load_lmer_panel(a.panel) if panel else load_lmer_table(a.weights)
            tmp = a.output + ".tmp"
            if a.cmd.startswith("scan-tail"):
                thresholds = dist_list("--thresholds", a.thresholds, float)
                check, compute = ((check_panel_scan_tail_counts, scan_tail_counts_with_panel) if panel else
                                  (check_scan_tail_counts, scan_tail_counts))
                check(folded, a.width, a.stride, thresholds, a.chunk)
                result = compute(folded, a.seqs_fa, a.width, a.stride, thresholds, a.device, a.chunk)
                (write_panel_tail_counts(tmp, folded.names, result) if panel else write_tail_counts(tmp, result))
                what = "%d thresholds" % len(thresholds)
            else:
                q, ranks = dist_list("--q", a.q, float), dist_list("--ranks", a.ranks, int)
                check, compute = ((check_panel_scan_quantiles, scan_quantiles_with_panel) if panel else
                                  (check_scan_quantiles, scan_quantiles))
                check(folded, a.width, a.stride, q, ranks, a.chunk, a.collect_cap)
                result = compute(folded, a.seqs_fa, a.width, a.stride, q, ranks, a.device, a.chunk, a.collect_cap)
                (write_panel_quantiles(tmp, folded.names, result) if panel else write_quantiles(tmp, result))
                what = "%d order statistics in %d scans" % (len(q if ranks is None else ranks), len(result["passes"]))
            os.replace(tmp, a.output)
            print("%s of %s scored windows -> %s" % (what, np.max(result["scored"]), a.output), file=sys.stderr)
        elif a.cmd in ("delta", "delta-saturation"):
            for path in (a.seqs_fa,) + ((a.variants,) if a.cmd == "delta" else ()):
                if not os.path.isfile(path):
                    raise ModelError("cannot read %s" % path)
            tab = load_lmer_table(a.weights)
            check_delta(tab, chunk=a.chunk)
            tmp = a.output + ".tmp"
            if a.cmd == "delta":
                variants = read_variants(a.variants)
                values = delta(tab, a.seqs_fa, variants, a.device, a.chunk)
                write_delta(tmp, variants, values)
                os.replace(tmp, a.output)
                print("%d variants scored, %d over a non-ACGT character (nan) -> %s"
                      % (len(values) - int(np.isnan(values).sum()), int(np.isnan(values).sum()), a.output), file=sys.stderr)
            else:
                results = delta_saturation(tab, a.seqs_fa, a.device, a.chunk)
                omitted = write_saturation(tmp, results, a.seqs_fa)
                os.replace(tmp, a.output)
                print("%d positions scored, %d near a non-ACGT character left out -> %s"
                      % (sum(len(r[1]) for r in results) - omitted, omitted, a.output), file=sys.stderr)
        elif a.cmd == "panel":
            names = panel_member_names(a.weights, a.names)
            if len(names) != len(a.weights):
                raise ModelError("panel: %d names for %d weight files" % (len(names), len(a.weights)))
            if len(a.weights) > PANEL_MAX_MODELS:
                raise ModelError("panel: %d weight files; a panel holds 1..%d tables" % (len(a.weights), PANEL_MAX_MODELS))
            LmerPanel([load_lmer_table(path) for path in a.weights], names).save(a.output)
        elif a.cmd in ("predict-panel", "scan-panel", "delta-panel"):
            if a.cmd == "predict-panel" and a.block is not None and a.block < 1:
                raise ModelError("--block must be at least 1")
            for path in [getattr(a, key) for key in ("query_fa", "seqs_fa", "variants") if hasattr(a, key)]:
                if not os.path.isfile(path):
                    raise ModelError("cannot read %s" % path)
            panel = load_lmer_panel(a.panel)
            tmp = a.output + ".tmp"
            if a.cmd == "predict-panel":
                names, values = score_with_panel(panel, a.query_fa, a.device, a.block)
                write_panel_scores(tmp, panel.names, names, values)
                os.replace(tmp, a.output)
            elif a.cmd == "scan-panel":
                check_panel_scan(panel, a.width, a.stride, a.chunk)
                results = scan_with_panel(panel, a.seqs_fa, a.width, a.stride, a.device, a.chunk)
                omitted = write_panel_scan(tmp, panel.names, results, a.width)
                os.replace(tmp, a.output)
                print("%d windows scored for %d models, %d over a non-ACGT character left out -> %s"
                      % (sum(len(r[1]) for r in results) - omitted, panel.n_models, omitted, a.output), file=sys.stderr)
            else:
                check_panel_delta(panel, chunk=a.chunk)
                variants = read_variants(a.variants)
                values = delta_with_panel(panel, a.seqs_fa, variants, a.device, a.chunk)
                write_panel_delta(tmp, panel.names, variants, values)
                os.replace(tmp, a.output)
                bad = int(np.isnan(values).any(axis=1).sum()) if len(values) else 0
                print("%d variants scored for %d models, %d over a non-ACGT character (nan) -> %s"
                      % (len(values) - bad, panel.n_models, bad, a.output), file=sys.stderr)
        else:
            compute, write = _QUERY_COMMANDS[a.cmd]
            if a.block is not None and a.block < 1:
                raise ModelError("--block must be at least 1")
            if not os.path.isfile(a.query_fa):
                raise ModelError("cannot read %s" % a.query_fa)
            if a.cmd == "predict-table":
                m = load_lmer_table(a.weights)
            elif a.cmd in ("explain-table", "hypothetical-table"):
                m = load_importance_table(a.table)
            else:
                m = load(a.model)
            names, values = compute(m, a.query_fa, a.device, a.block)
            tmp = a.output + ".tmp"
            write(tmp, names, values)
            os.replace(tmp, a.output)
    except (ModelError, dv.GkmError, svmcv.SvmError, OSError) as e:
        print("gkmpredict: error: %s" % e, file=sys.stderr)
        return 1
    return 0


if __name__ == "__main__":
    sys.exit(main())
