"""The gkm-SVM model: its file format, and training a C-SVC or an epsilon-SVR on all sequences.

The bottom of the gkmpredict family: gkmmodel <- gkmquery <- gkmtables <- gkmscan <- gkmdelta <- gkmpredict (the command
line, which also re-exports every public name)."""
import logging
import os

import numpy as np

from . import device as dv
from . import svmcv

FORMAT = "gkmqc-model-1"
WEIGHTED_FORMAT = "gkmqc-model-2"      # a C-SVC trained with class weights: weight0, weight1 after C
SVR_FORMAT = "gkmqc-svr-1"
C_SVC, EPSILON_SVR = "c_svc", "epsilon_svr"
_INT_KEYS = ("kernel_type", "L", "k", "d", "M", "shrinking", "n0", "n_sv")
_FLOAT_KEYS = ("H", "gamma", "C", "weight0", "weight1", "tol", "rho", "epsilon")
_KEYS = ("format", "kernel_type", "L", "k", "d", "M", "H", "gamma", "C", "tol", "shrinking", "rho", "n0", "n_sv")
_WEIGHTED_KEYS = ("format", "kernel_type", "L", "k", "d", "M", "H", "gamma", "C", "weight0", "weight1", "tol", "shrinking",
                  "rho", "n0", "n_sv")
_SVR_KEYS = ("format", "kernel_type", "L", "k", "d", "M", "H", "gamma", "C", "tol", "shrinking", "epsilon", "rho", "n_sv")
MAX_SVR_SAMPLES = svmcv.MAX_FOLD_SAMPLES // 2   # LIBSVM's epsilon-SVR solves 2l variables
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
    score = sum dual_coef() K + rho: rho is scikit-learn's intercept_ (for SVR that is LIBSVM's rho negated).
    `class_weight` (C-SVC only): None, or the pair (w0, w1) the model was trained with -- the weights of label 0 (the
    negatives) and label 1 as numbers ("balanced" resolved), alpha of a class bounded by C times its weight."""

    def __init__(self, kernel_type, L, k, d, M, H, gamma, C, tol, shrinking, rho, n0, alpha, names, seqs, svm_type=C_SVC,
                 epsilon=None, class_weight=None):
        self.kernel_type, self.L, self.k, self.d, self.M = int(kernel_type), int(L), int(k), int(d), int(M)
        self.H, self.gamma, self.C, self.tol = float(H), float(gamma), float(C), float(tol)
        self.shrinking = bool(shrinking)
        self.rho, self.n0 = float(rho), int(n0)
        self.alpha = np.ascontiguousarray(alpha, dtype=np.float64)
        self.names = list(names)
        self.seqs = [np.ascontiguousarray(s, dtype=np.uint8) for s in seqs]
        self.svm_type = svm_type
        self.epsilon = None if epsilon is None else float(epsilon)
        try:
            self.class_weight = None if class_weight is None else (float(class_weight[0]), float(class_weight[1]))
        except (TypeError, ValueError, IndexError):
            raise ModelError("class_weight must be None or a pair of numbers")
        if class_weight is not None and len(class_weight) != 2:
            raise ModelError("class_weight must be None or a pair of numbers")
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
        weighted = self.class_weight is not None
        head = [("format", SVR_FORMAT if self.is_svr else WEIGHTED_FORMAT if weighted else FORMAT),
                ("kernel_type", self.kernel_type), ("L", self.L),
                ("k", self.k), ("d", self.d), ("M", self.M), ("H", repr(self.H)), ("gamma", repr(self.gamma)),
                ("C", repr(self.C))]
        if weighted:
            head += [("weight0", repr(self.class_weight[0])), ("weight1", repr(self.class_weight[1]))]
        head += [("tol", repr(self.tol)), ("shrinking", int(self.shrinking))]
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
    if m.class_weight is not None:
        if m.svm_type != C_SVC:
            raise ModelError("only a C-SVC model has class weights")
        if not all(np.isfinite(w) and w > 0 for w in m.class_weight):
            raise ModelError("class weights must be finite and > 0")
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
    """Read a model file written by Model.save (any of the three format tags); anything malformed raises ModelError with the
    reason."""
    with open(path) as f:
        lines = f.read().split("\n")
    if lines and lines[-1] == "":
        lines.pop()
    head, i = {}, 0
    while i < len(lines) and lines[i] != "SV":
        parts = lines[i].split(" ", 1)
        if len(parts) != 2 or parts[0] not in _KEYS + _SVR_KEYS + _WEIGHTED_KEYS:
            raise ModelError("%s:%d: not a `key value` line of the header: %r" % (path, i + 1, lines[i]))
        if parts[0] in head:
            raise ModelError("%s:%d: key %s given twice" % (path, i + 1, parts[0]))
        head[parts[0]] = parts[1]
        i += 1
    if i == len(lines):
        raise ModelError("%s: no SV line" % path)
    svr = head.get("format") == SVR_FORMAT
    weighted = head.get("format") == WEIGHTED_FORMAT
    keys = _SVR_KEYS if svr else _WEIGHTED_KEYS if weighted else _KEYS
    missing = [key for key in keys if key not in head]
    if missing:
        raise ModelError("%s: missing key(s): %s" % (path, ", ".join(missing)))
    if head["format"] not in (FORMAT, WEIGHTED_FORMAT, SVR_FORMAT):
        raise ModelError("%s: format %r, expected %r, %r or %r" % (path, head["format"], FORMAT, WEIGHTED_FORMAT, SVR_FORMAT))
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
                 val["shrinking"], val["rho"], val["n0"], alpha, names, seqs,
                 class_weight=(val["weight0"], val["weight1"]) if weighted else None)


# ------------------------------------------------------------------ training
def resolve_class_weight(class_weight, y):
    """`class_weight` of train / train_panel as numbers for the labels y: None stays None; "balanced" and a pair (w0, w1)
    -- the weights of label 0 and label 1 -- become a pair of floats (svmcv.problem_weights)."""
    if class_weight is None:
        return None
    try:
        w = svmcv.problem_weights([np.asarray(y)], class_weight)[0]
    except svmcv.SvmError as e:
        raise ModelError(str(e))
    return (float(w[0]), float(w[1]))


def train(pos_fa, neg_fa, kernel_type=4, L=10, k=6, d=3, M=50, H=50, gamma=1.0, C=1.0, tol=1e-3, shrinking=False,
          device=0, kernel=dv.KERNEL_AUTO, class_weight=None):
    """One C-SVC on every sequence of pos_fa (label 1) and neg_fa (label 0) -> Model.
    class_weight: None, "balanced" (l / (2 * count) per class, as scikit-learn) or a pair (w0, w1), the weights of label 0
    and label 1: alpha of a class is bounded by C times its weight (scikit-learn's `class_weight`, LIBSVM's -wi)."""
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
    weights = resolve_class_weight(class_weight, y)
    res = dv.gram_matrix(seqs, kernel_type, L, k, d, M, H, gamma, device, kernel=kernel, symmetric=True,
                         keep_context=True)
    K = res["K"]
    sol, _ = svmcv.train_folds(K, [np.arange(len(y))], y, C, tol, shrinking, class_weight=weights)
    if sol.iters[0] >= 0:
        a, order = sol.alpha[0], sol.idx[0]
        sv = np.nonzero(a > 0)[0]
        idx, alpha, rho = order[sv], a[sv], float(sol.rho[0])
    else:   # the GPU solver's iteration cap: the reference's solver has none (as svmcv.crossValidate)
        from sklearn.svm import SVC
        logging.warning("training re-solved with scikit-learn (iteration cap of the GPU solver)")
        m = SVC(kernel="precomputed", C=C, tol=tol, shrinking=bool(shrinking),
                class_weight=None if weights is None else {0: weights[0], 1: weights[1]}).fit(K.cpu().numpy(), y)
        # (for two classes scikit-learn negates LIBSVM's coefficients and decision value, so intercept_ is LIBSVM's rho)
        idx, alpha, rho = m.support_, np.abs(m.dual_coef_[0]), float(m.intercept_[0])
    del K, res
    torch.cuda.empty_cache()
    return Model(kernel_type, L, k, d, M, H, gamma, C, tol, shrinking, rho, int((y[idx] == 0).sum()), alpha,
                 [names[i] for i in idx], [seqs[i] for i in idx], class_weight=weights)


def select(pos_fa, neg_fa, Cs, class_weights=(None,), ncv=5, repeats=1, seed=1, kernel_type=4, L=10, k=6, d=3, M=50, H=50,
           gamma=1.0, tol=1e-3, shrinking=False, device=0, kernel=dv.KERNEL_AUTO):
    """Cross-validate every setting of the grid `Cs` x `class_weights` on ONE Gram matrix of pos_fa (label 1) and neg_fa
    (label 0) and one solver launch (svmcv.cross_validate_grid) -> (records, index of the best one).  Best: the highest
    mean AUC; on a tie the smaller C, then the earlier entry of class_weights."""
    import torch
    bad = dv.check_parameters(kernel_type, L, k, d)
    if bad:
        raise ModelError("kernel parameters rejected: %s" % bad)
    pos, _, _, _ = dv.read_fasta(pos_fa)
    neg, _, _, _ = dv.read_fasta(neg_fa)
    if len(pos) < ncv or len(neg) < ncv:
        raise ModelError("cross-validation needs at least ncv = %d sequences of each class" % ncv)
    seqs = dv.FlatSequences(np.concatenate((pos.codes, neg.codes)),
                            np.concatenate((pos.off, pos.off[-1] + neg.off[1:])))
    res = dv.gram_matrix(seqs, kernel_type, L, k, d, M, H, gamma, device, kernel=kernel, symmetric=True,
                         keep_context=True)
    K = res["K"]
    try:
        records = svmcv.cross_validate_grid(K, len(pos), len(neg), Cs, class_weights, ncv, repeats, seed, tol, shrinking)
    except svmcv.SvmError as e:
        raise ModelError(str(e))
    finally:
        del K, res
        torch.cuda.empty_cache()
    return records, svmcv.best_record(records)


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
