"""The host side of panel training and folding (gkmqc_amd/gkmpanels.py, svmcv.train_tasks), no GPU: the
label file and its refusals, fold_panel's refusals (before any device is touched), the union and scatter of the members'
classes against lmer_classes, the per-problem orders of train_tasks against libsvm_order, and the command line with the
compute replaced by host stand-ins."""
import os

import numpy as np
import pytest


@pytest.fixture(scope="module")
def pn(built):
    from gkmqc_amd import gkmpanels
    return gkmpanels


@pytest.fixture(scope="module")
def gp(built):
    from gkmqc_amd import gkmpredict
    return gkmpredict


NAMES = ["s0", "s1", "with\ttab", "s3"]


def _labels(tmp_path, text):
    path = str(tmp_path / "labels.tsv")
    with open(path, "w") as f:
        f.write(text)
    return path


GOOD = "name\tliver\theart\ns0\t1\t0\ns1\t0\t.\nwith\ttab\t.\t1\ns3\t1\t0\n"


def test_read_labels_reads_a_well_formed_file(pn, tmp_path):
    tasks, Y = pn.read_labels(_labels(tmp_path, GOOD), NAMES)
    assert tasks == ["liver", "heart"]
    assert Y.dtype == np.int8 and Y.tolist() == [[1, 0], [0, -1], [-1, 1], [1, 0]]
    assert pn.NOT_IN_TASK == -1
    # (a missing final newline is the same file)
    assert pn.read_labels(_labels(tmp_path, GOOD[:-1]), NAMES)[1].tolist() == Y.tolist()
    trains, labs = pn.task_problems(Y)
    assert [t.tolist() for t in trains] == [[0, 1, 3], [0, 2, 3]]
    assert [x.tolist() for x in labs] == [[1, 0, 1], [0, 1, 0]]


@pytest.mark.parametrize("text,message", [
    ("", r":1: no header line"),
    ("s0\t1\t0\n", r":1: the header must be name<TAB>task"),
    ("name\n", r":1: the header must be name<TAB>task"),
    ("name\ta\ta\n", r":1: panel: the name 'a' is given to members 0 and 1"),
    ("name\ta\t\n", r":1: panel: the name of member 1 must be a non-empty string"),
    (GOOD.replace("s1\t0\t.", "s1\t0"), r":3: expected name<TAB>2 label"),
    (GOOD.replace("s1\t0\t.", "s1"), r":3: expected name<TAB>2 label"),
    (GOOD.replace("s1\t0\t.", "sX\t0\t."), r":3: name 'sX', but FASTA record 2 is 's1'"),
    (GOOD.replace("s1\t0\t.", "s1\t0\t2"), r":3: the label of task heart must be 1, 0 or \., not '2'"),
    (GOOD.replace("s1\t0\t.", "s1\t\t."), r":3: the label of task liver must be 1, 0 or \., not ''"),
    (GOOD + "s4\t1\t1\n", r":6: more label lines than FASTA records \(4\)"),
    (GOOD.replace("s3\t1\t0\n", ""), r":5: no labels for FASTA record 4 \('s3'\): 3 lines for 4 records"),
    (GOOD.replace("s1\t0\t.", "s1\t1\t."), r"task liver has no negative \(0\) record"),
    (GOOD.replace("with\ttab\t.\t1", "with\ttab\t.\t."), r"task heart has no positive \(1\) record"),
])
def test_read_labels_refuses_by_line(pn, gp, tmp_path, text, message):
    with pytest.raises(gp.ModelError, match=message):
        pn.read_labels(_labels(tmp_path, text), NAMES)


# ------------------------------------------------------------------ models made by hand
def _pool(n=12, length=30, seed=5):
    rng = np.random.default_rng(seed)
    return [rng.integers(0, 4, size=length, dtype=np.uint8) for _ in range(n)]


def _model(gp, pool, members, kernel_type=4, L=6, k=4, d=2, seed=0, **kw):
    """a model whose support vectors are pool[members]: the first third negatives"""
    rng = np.random.default_rng(seed)
    alpha = rng.random(len(members)) + 0.01
    args = dict(kernel_type=kernel_type, L=L, k=k, d=d, M=50, H=50.0, gamma=1.0, C=1.0, tol=1e-3, shrinking=False,
                rho=0.125 * seed - 0.5, n0=len(members) // 3)
    args.update(kw)
    return gp.Model(alpha=alpha, names=["s%d" % i for i in members], seqs=[pool[i] for i in members], **args)


def _no_device(monkeypatch, pn):
    def touched(*a, **k):
        raise AssertionError("the device was touched")
    monkeypatch.setattr(pn.dv, "cached_context", touched)


def test_fold_panel_refuses_before_the_device(pn, gp, monkeypatch):
    _no_device(monkeypatch, pn)
    pool = _pool()
    good = [_model(gp, pool, [0, 1, 2, 3], seed=s) for s in range(3)]
    with pytest.raises(gp.ModelError, match=r"panel: 0 members; a panel holds 1\.\.64 tables"):
        pn.fold_panel([])
    with pytest.raises(gp.ModelError, match=r"panel: 65 members; a panel holds 1\.\.64 tables"):
        pn.fold_panel([good[0]] * 65)
    with pytest.raises(gp.ModelError, match=r"panel: the name 'a' is given to members 0 and 2"):
        pn.fold_panel(good, names=["a", "b", "a"])
    with pytest.raises(gp.ModelError, match=r"panel: 2 names for 3 members"):
        pn.fold_panel(good, names=["a", "b"])
    with pytest.raises(gp.ModelError, match=r"panel: member 1 is no trained model"):
        pn.fold_panel([good[0], "model.txt"])
    for t in (3, 5):
        rbf = _model(gp, pool, [0, 1, 2], kernel_type=t)
        with pytest.raises(gp.ModelError, match=r"panel: member 1 \(table1\): RBF kernels \(types 3 and 5\) have no l-mer weight"):
            pn.fold_panel([good[0], rbf])
    for key, kw in (("kernel_type", dict(kernel_type=2)), ("L", dict(L=7, k=5)), ("k", dict(k=3)), ("d", dict(d=1)),
                    ("M", dict(M=40)), ("H", dict(H=25.0))):
        other = _model(gp, pool, [0, 1, 2], **kw)
        with pytest.raises(gp.ModelError, match=r"panel: member 2 \(c\) has %s = .* where member 0 \(a\) has .*; the members "
                                                r"must share kernel_type, L, k, d, M, H" % key):
            pn.fold_panel([good[0], good[1], other], names=["a", "b", "c"])
    # what the members need not share
    assert pn.check_fold([good[0], _model(gp, pool, [4, 5], C=3.0, tol=0.01, gamma=2.0, shrinking=True)]) == ["table0", "table1"]


def test_the_union_and_scatter_of_the_members_classes(pn, gp):
    """12 sequences; three members with overlapping, disjoint and single support vectors.  v is ascending and distinct,
    every member's (v_m, cv_m) of lmer_classes sits in its column at searchsorted(v, v_m) with its own bits, and every
    other cell of the column is +0.0"""
    pool = _pool()
    members = ([0, 1, 2, 3, 4, 5], [4, 5, 6, 7, 8], [11], list(range(12)))
    models = [_model(gp, pool, mem, seed=s) for s, mem in enumerate(members)]
    rng = np.random.default_rng(9)
    sqs = [rng.random(m.n_sv) + 0.5 for m in models]
    v, CV = pn.panel_classes(models, sqs)
    assert v.dtype == np.uint32 and CV.dtype == np.float64 and CV.shape == (len(v), 8)
    assert (np.diff(v.astype(np.int64)) > 0).all()
    seen = np.zeros(len(v), dtype=bool)
    for m, (model, sq) in enumerate(zip(models, sqs)):
        vm, cvm = gp.lmer_classes(model, sq)
        at = np.searchsorted(v, vm)
        assert (v[at] == vm).all()
        assert CV[at, m].tobytes() == cvm.tobytes()
        rest = np.delete(CV[:, m], at)
        assert (rest == 0.0).all() and not np.signbit(rest).any()
        seen[at] = True
    assert seen.all()
    assert (CV[:, len(models):] == 0.0).all()
    assert len(v) > max(len(gp.lmer_classes(m, sq)[0]) for m, sq in zip(models[:3], sqs))
    assert pn.panel_classes(models, sqs, ms=16)[1].shape == (len(v), 16)


def test_train_tasks_orders_are_libsvm_order_per_problem(pn, built):
    from gkmqc_amd import svmcv
    rng = np.random.default_rng(2)
    Y = rng.integers(-1, 2, size=(40, 5)).astype(np.int8)
    trains, labs = pn.task_problems(Y)
    got = svmcv.task_orders(trains, labs)
    for t in range(Y.shape[1]):
        idx, n0 = svmcv.libsvm_order(trains[t], Y[:, t])
        assert got[t][0].dtype == np.int32 and got[t][0].tolist() == idx.tolist() and got[t][1] == n0
        # LIBSVM's order: the label-0 records in pool order, then the label-1 records in pool order
        assert idx.tolist() == np.flatnonzero(Y[:, t] == 0).tolist() + np.flatnonzero(Y[:, t] == 1).tolist()
        assert n0 == int((Y[:, t] == 0).sum())
    with pytest.raises(svmcv.SvmError, match="exactly two classes"):
        svmcv.task_orders([np.arange(3)], [np.ones(3)])
    with pytest.raises(svmcv.SvmError, match="one label per training sample"):
        svmcv.task_orders([np.arange(3)], [np.array([0, 1])])
    with pytest.raises(svmcv.SvmError, match="2 label vectors for 1 problems"):
        svmcv.task_orders([np.arange(3)], [np.array([0, 1, 1])] * 2)


# ------------------------------------------------------------------ the command line
def test_command_line_shape(pn):
    assert list(pn.COMMANDS) == ["train", "fold"]
    p = pn.build_parser()
    a = p.parse_args(["train", "-t", "0", "-L", "6", "-k", "4", "-d", "2", "--panel", "p.npz", "s.fa", "l.tsv", "out"])
    assert (a.kernel_type, a.full_word_length, a.non_gap_length, a.max_num_gaps) == (0, 6, 4, 2)
    assert (a.seqs_fa, a.labels, a.out_prefix, a.panel, a.device) == ("s.fa", "l.tsv", "out", "p.npz", 0)
    a = p.parse_args(["train", "s.fa", "l.tsv", "out"])
    assert (a.kernel_type, a.full_word_length, a.non_gap_length, a.max_num_gaps, a.panel) == (4, 10, 6, 3, None)
    a = p.parse_args(["fold", "--names", "a,b", "out.npz", "m0.txt", "m1.txt"])
    assert (a.output, a.models, a.names) == ("out.npz", ["m0.txt", "m1.txt"], "a,b")
    with pytest.raises(SystemExit):
        p.parse_args(["fold", "out.npz"])
    assert pn.model_path("out/x", "liver") == "out/x.liver.model.txt"


@pytest.fixture
def cli(pn, gp, tmp_path, monkeypatch):
    """a pool and its label file on disk; train_panel and fold_panel replaced by host stand-ins"""
    pool = _pool(4)
    fa = str(tmp_path / "s.fa")
    with open(fa, "w") as f:
        for i, s in enumerate(pool):
            f.write(">s%d\n%s\n" % (i, gp.codes_to_text(s)))
    tsv = _labels(tmp_path, "name\tliver\theart\ns0\t1\t0\ns1\t0\t.\ns2\t.\t1\ns3\t1\t0\n")
    models = [_model(gp, pool, [0, 1, 3], seed=0), _model(gp, pool, [0, 2, 3], seed=1)]
    calls = []

    def train_panel(fasta, labels, *args):
        calls.append(("train", fasta, labels[0], args))
        return labels[0], models

    def fold_panel(ms, names=None, device=0, on_piece=None):
        calls.append(("fold", len(ms), names))
        rc = gp.lmer_rc(np.arange(4 ** 5, dtype=np.uint32), 5)
        W = np.arange(4 ** 5, dtype=np.float64)
        return gp.LmerPanel([gp.LmerTable(W + W[rc] + m, 0, 5, 4, 1, 50, 50.0, 0.5 * m) for m in range(len(ms))], names)

    monkeypatch.setattr(pn, "train_panel", train_panel)
    monkeypatch.setattr(pn, "fold_panel", fold_panel)
    return dict(fa=fa, tsv=tsv, models=models, calls=calls, dir=str(tmp_path))


def test_train_writes_one_model_per_task_and_the_panel(pn, gp, cli, capsys):
    prefix, panel = os.path.join(cli["dir"], "out"), os.path.join(cli["dir"], "p.npz")
    assert pn.main(["train", "-t", "4", "-L", "6", "-k", "4", "-d", "2", "--panel", panel, cli["fa"], cli["tsv"], prefix]) == 0
    assert cli["calls"][0][:3] == ("train", cli["fa"], ["liver", "heart"])
    assert cli["calls"][0][3] == (4, 6, 4, 2, 50, 50, 1.0, 1.0, 0.001, False, 0)
    assert cli["calls"][1] == ("fold", 2, ["liver", "heart"])
    for task, m in zip(("liver", "heart"), cli["models"]):
        got = gp.load(pn.model_path(prefix, task))
        assert got.alpha.tobytes() == m.alpha.tobytes() and got.names == m.names
    assert gp.load_lmer_panel(panel).names == ["liver", "heart"]
    assert sorted(os.listdir(cli["dir"])) == ["labels.tsv", "out.heart.model.txt", "out.liver.model.txt", "p.npz", "s.fa"]
    assert "2 tasks, 4 records" in capsys.readouterr().err
    # without --panel nothing is folded
    del cli["calls"][:]
    assert pn.main(["train", cli["fa"], cli["tsv"], prefix]) == 0
    assert [c[0] for c in cli["calls"]] == ["train"]


def test_fold_reads_model_files(pn, gp, cli, capsys):
    paths = []
    for i, m in enumerate(cli["models"]):
        paths.append(os.path.join(cli["dir"], "m%d.txt" % i))
        m.save(paths[-1])
    out = os.path.join(cli["dir"], "p.npz")
    assert pn.main(["fold", out] + paths) == 0
    assert cli["calls"] == [("fold", 2, ["m0.txt", "m1.txt"])]
    assert gp.load_lmer_panel(out).names == ["m0.txt", "m1.txt"]
    assert pn.main(["fold", "--names", "a,b", out] + paths) == 0 and gp.load_lmer_panel(out).names == ["a", "b"]
    assert pn.main(["fold", "--names", "a", out] + paths) == 1
    assert "fold: 1 names for 2 model files" in capsys.readouterr().err


def test_a_missing_input_is_refused_by_name(pn, cli, capsys):
    prefix = os.path.join(cli["dir"], "out")
    gone = os.path.join(cli["dir"], "gone")
    for argv in (["train", gone, cli["tsv"], prefix], ["train", cli["fa"], gone, prefix],
                 ["fold", os.path.join(cli["dir"], "p.npz"), gone]):
        assert pn.main(argv) == 1
        assert "gkmpanels: error: cannot read %s" % gone in capsys.readouterr().err
    assert cli["calls"] == []
    assert sorted(os.listdir(cli["dir"])) == ["labels.tsv", "s.fa"]


def test_bad_arguments_and_task_names_are_refused_before_the_compute(pn, cli, capsys, tmp_path):
    prefix = os.path.join(cli["dir"], "out")
    assert pn.main(["train", "-L", "13", cli["fa"], cli["tsv"], prefix]) == 1
    slash = _labels(tmp_path, "name\ta/b\ns0\t1\ns1\t0\ns2\t.\ns3\t1\n")
    assert pn.main(["train", cli["fa"], slash, prefix]) == 1
    assert "cannot be part of a file name" in capsys.readouterr().err
    assert cli["calls"] == []


def test_outputs_appear_only_complete(pn, gp, cli, monkeypatch, capsys):
    """a fold that fails leaves no model file; a writer that fails halfway leaves no file under the output's name"""
    prefix, panel = os.path.join(cli["dir"], "out"), os.path.join(cli["dir"], "p.npz")

    def refuses(*a, **k):
        raise gp.ModelError("stand-in: refused")
    monkeypatch.setattr(pn, "fold_panel", refuses)
    assert pn.main(["train", "--panel", panel, cli["fa"], cli["tsv"], prefix]) == 1
    assert "stand-in: refused" in capsys.readouterr().err
    assert sorted(os.listdir(cli["dir"])) == ["labels.tsv", "s.fa"]
    monkeypatch.undo()

    from gkmqc_amd import gkmmodel, gkmtables
    real = gkmmodel.codes_to_text
    seen = []

    def halfway(codes):
        seen.append(1)
        if len(seen) == 2:
            raise OSError("stand-in: the disk is full")
        return real(codes)
    monkeypatch.setattr(gkmmodel, "codes_to_text", halfway)
    path = os.path.join(cli["dir"], "m.txt")
    with pytest.raises(OSError):
        cli["models"][0].save(path)
    assert not os.path.exists(path)
    monkeypatch.undo()

    def savez_halfway(f, **k):
        f.write(b"PK half")
        raise OSError("stand-in: the disk is full")
    monkeypatch.setattr(gkmtables.np, "savez", savez_halfway)
    rc = gp.lmer_rc(np.arange(4 ** 5, dtype=np.uint32), 5)
    W = np.arange(4 ** 5, dtype=np.float64)
    monkeypatch.setattr(pn, "fold_panel", lambda ms, names=None, device=0: gp.LmerPanel(
        [gp.LmerTable(W + W[rc], 0, 5, 4, 1, 50, 50.0, 0.0) for _ in ms], names))
    cli["models"][0].save(path)
    assert pn.main(["fold", panel, path]) == 1
    assert "the disk is full" in capsys.readouterr().err
    assert not os.path.exists(panel)
