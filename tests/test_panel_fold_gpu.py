"""train_panel and fold_panel on the GPU (gkmqc_amd/gkmpanels.py).  Two contracts, both exact: a task's
model file is the file `train` writes on the task's own positives and negatives, byte for byte; column m of a folded
panel is lmer_weights of member m, bit for bit.  The pool: 40 sequences of 60 bp from the explain tests' planted-motif
generator, three tasks with different labelings (one with records that take no part), L = 6, k = 4, d = 2, a weighted and
an unweighted kernel type.  Everything trained or folded is computed once per kernel type and shared."""
import os

import numpy as np
import pytest

from tests.test_explain_gpu import _planted

pytestmark = pytest.mark.gpu

KP = dict(L=6, k=4, d=2)
TYPES = (4, 0)
MOTIF = np.array([0, 3, 2, 0, 1, 2, 3, 1], np.uint8)
TASKS = ["planted", "halves", "sparse"]


@pytest.fixture(scope="module")
def gp(built):
    from gkmqc_amd import gkmpredict
    return gkmpredict


@pytest.fixture(scope="module")
def pn(built):
    from gkmqc_amd import gkmpanels
    return gkmpanels


def _write_fasta(gp, path, seqs, names):
    with open(path, "w") as f:
        for name, s in zip(names, seqs):
            f.write(">%s\n%s\n" % (name, gp.codes_to_text(s)))


def _pool_labels():
    """the pool in mixed order and Y (40, 3): the planted motif; the pool's halves; a labeling that leaves records out"""
    with_motif, _ = _planted(21, 20, 60, MOTIF)
    without, _ = _planted(22, 20, 60, None)
    rng = np.random.default_rng(23)
    order = rng.permutation(40)
    seqs = [(with_motif + without)[i] for i in order]
    Y = np.empty((40, 3), dtype=np.int8)
    Y[:, 0] = order < 20
    Y[:, 1] = np.arange(40) % 2
    Y[:, 2] = rng.integers(-1, 2, size=40)
    return seqs, Y


class _Shared:
    """per kernel type: the pool's files, train_panel's models, `train`'s models on the split files, both panels"""

    def __init__(self, gp, pn, tmp):
        self.gp, self.pn, self.tmp, self.by_type = gp, pn, tmp, {}
        self.seqs, self.Y = _pool_labels()
        self.names = ["rec%d" % i for i in range(40)]
        self.fa = os.path.join(tmp, "pool.fa")
        _write_fasta(gp, self.fa, self.seqs, self.names)
        self.tsv = os.path.join(tmp, "labels.tsv")
        sym = {1: "1", 0: "0", -1: "."}
        with open(self.tsv, "w") as f:
            f.write("\t".join(["name"] + TASKS) + "\n")
            for name, row in zip(self.names, self.Y.tolist()):
                f.write("\t".join([name] + [sym[x] for x in row]) + "\n")
        self.split = []
        for t, task in enumerate(TASKS):
            files = []
            for lab, word in ((1, "pos"), (0, "neg")):
                keep = np.flatnonzero(self.Y[:, t] == lab)
                files.append(os.path.join(tmp, "%s_%s.fa" % (task, word)))
                _write_fasta(gp, files[-1], [self.seqs[i] for i in keep], [self.names[i] for i in keep])
            self.split.append(files)

    def get(self, ktype):
        if ktype not in self.by_type:
            gp, pn = self.gp, self.pn
            tasks, models = pn.train_panel(self.fa, self.tsv, kernel_type=ktype, **KP)
            assert tasks == TASKS
            single = [gp.train(p, n, kernel_type=ktype, **KP) for p, n in self.split]
            loop = gp.LmerPanel([gp.lmer_weights(m) for m in models], tasks)
            self.by_type[ktype] = dict(models=models, single=single, loop=loop, folded=pn.fold_panel(models, tasks))
        return self.by_type[ktype]


@pytest.fixture(scope="module")
def shared(gp, pn, tmp_path_factory):
    return _Shared(gp, pn, str(tmp_path_factory.mktemp("panel_fold")))


def _file(model, path):
    model.save(path)
    with open(path, "rb") as f:
        return f.read()


def _same_panel(got, want):
    assert got.names == want.names and got.n_models == want.n_models
    assert got.kernel_params() == want.kernel_params()
    assert got.rho.tobytes() == want.rho.tobytes()
    assert got.W.shape == want.W.shape and got.W.tobytes() == want.W.tobytes()


@pytest.mark.parametrize("ktype", TYPES)
def test_a_tasks_model_file_is_trains_byte_for_byte(shared, ktype, tmp_path):
    s = shared.get(ktype)
    for t, task in enumerate(TASKS):
        a, b = s["models"][t], s["single"][t]
        if _file(a, str(tmp_path / "a.txt")) != _file(b, str(tmp_path / "b.txt")):      # say which entry differs
            assert a.names == b.names, task
            assert a.n0 == b.n0 and a.rho == b.rho, (task, a.rho, b.rho)
            diff = np.flatnonzero(a.alpha != b.alpha)
            assert not len(diff), (task, diff[:5], a.alpha[diff[:5]], b.alpha[diff[:5]])
            raise AssertionError("task %s: the files differ outside names, n0, rho and alpha" % task)
    assert len({tuple(m.names) for m in s["models"]}) == 3      # (three different problems)
    assert any(len(m.names) < 40 for m in s["models"])


@pytest.mark.parametrize("ktype", TYPES)
def test_the_folded_panel_is_the_loop_of_single_tables(shared, ktype):
    s = shared.get(ktype)
    _same_panel(s["folded"], s["loop"])
    assert s["folded"].rho.tolist() == [m.rho for m in s["models"]]
    assert np.count_nonzero(s["folded"].W) > 0


def test_on_piece_reports_the_launch(shared, pn, monkeypatch):
    s = shared.get(4)
    monkeypatch.setattr(pn, "TABLE_PIECE", 1000)       # 4^6 = 4096 codes in five pieces
    seen = []
    _same_panel(pn.fold_panel(s["models"], TASKS, on_piece=seen.append), s["loop"])
    assert [p["codes"] for p in seen] == [1000, 1000, 1000, 1000, 96]
    for p in seen:
        assert p["kernel"] == "k_panel_weights" and p["n_models"] == 3 and p["kernel_ms"] > 0
        assert p["comparisons"] == 2.0 * p["classes"] * p["codes"] and p["classes_ms"] >= 0


def test_models_of_unrelated_pools_fold_together(shared, gp, pn, tmp_path):
    """three models trained on three pools that share no sequence: disjoint support vectors, one union of classes"""
    models = []
    for j in range(3):
        pos, _ = _planted(100 + j, 12, 60, MOTIF[::-1].copy() if j == 1 else MOTIF)
        neg, _ = _planted(200 + j, 12, 60, None)
        pf, nf = str(tmp_path / ("p%d.fa" % j)), str(tmp_path / ("n%d.fa" % j))
        _write_fasta(gp, pf, pos, ["p%d_%d" % (j, i) for i in range(12)])
        _write_fasta(gp, nf, neg, ["n%d_%d" % (j, i) for i in range(12)])
        models.append(gp.train(pf, nf, kernel_type=4, **KP))
    names = ["a", "b", "c"]
    _same_panel(pn.fold_panel(models, names), gp.LmerPanel([gp.lmer_weights(m) for m in models], names))


def test_a_panel_of_one(shared, gp, pn):
    m = shared.get(4)["models"][2]
    got = pn.fold_panel([m])
    _same_panel(got, gp.LmerPanel([gp.lmer_weights(m)]))
    assert got.names == ["table0"] and got.W.shape == (4 ** 6, 1)


@pytest.mark.parametrize("ktype", TYPES)
def test_scores_from_the_folded_panel_are_the_tables_scores(shared, gp, ktype):
    s = shared.get(ktype)
    names, got = gp.score_with_panel(s["folded"], shared.fa)
    assert names == shared.names and got.shape == (40, 3)
    for m, model in enumerate(s["models"]):
        _, want = gp.score_with_table(gp.lmer_weights(model), shared.fa)
        assert got[:, m].tobytes() == np.asarray(want, dtype=np.float64).tobytes()


def test_the_command_line_trains_folds_and_round_trips(shared, gp, pn, tmp_path, capsys):
    s = shared.get(4)
    prefix, panel = str(tmp_path / "out"), str(tmp_path / "panel.npz")
    argv = ["train", "-t", "4", "-L", "6", "-k", "4", "-d", "2", "--panel", panel, shared.fa, shared.tsv, prefix]
    assert pn.main(argv) == 0, capsys.readouterr().err
    for t, task in enumerate(TASKS):
        with open(pn.model_path(prefix, task), "rb") as f:
            assert f.read() == _file(s["single"][t], str(tmp_path / "single.txt"))
    _same_panel(gp.load_lmer_panel(panel), s["loop"])
    again = str(tmp_path / "again.npz")
    assert pn.main(["fold", "--names", ",".join(TASKS), again] + [pn.model_path(prefix, task) for task in TASKS]) == 0
    _same_panel(gp.load_lmer_panel(again), s["loop"])
    assert not [name for name in os.listdir(str(tmp_path)) if name.endswith(".tmp")]
