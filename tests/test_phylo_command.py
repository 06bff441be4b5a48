"""``phylo-run`` on the host twins: an external-alignment-hip run of nine tiny genomes (made with the numpy stand-in of the
engine's MSA calls, as ``tests/test_bootstrap_command.py`` makes its own), the files and their names per option, the
distance table and the tree against the restated pipeline of ``tests/subst_cases.py``, the support against the
restatement that draws with ``bootstrap_cases``' draws, the messages and their order, what ``main`` prints and ``--help``."""

from __future__ import annotations

import hashlib
import logging
import shutil
import sqlite3

import numpy as np
import pytest

from pyani_plus_amd import rundb
from pyani_plus_amd import tree as tree_mod
from tests import bootstrap_cases
from tests import subst_cases as cases
from tests import tree_cases
from tests.fake_engine import OracleEngine
from tests.helpers import FIXTURE_SETS, GOLDEN
from tests.msa_checker import NumpyMsaEngine
from tests.test_bootstrap_command import NAMES, order_under, shown_labels, stem

HELP = GOLDEN / "phylo" / "help.txt"
LOGGER = logging.getLogger("test")
N, COLUMNS, SEED = 9, 64, 13
METHOD = "external-alignment-hip"


def names_of(model: str, replicates: bool = False, keep: bool = False) -> list[str]:
    out = [f"{METHOD}_{model}_distances.tsv", f"{METHOD}_{model}_nj.nwk"]
    if replicates:
        out += [f"{METHOD}_{model}_nj_bootstrap.nwk", f"{METHOD}_{model}_nj_bootstrap.tsv"]
    if replicates and keep:
        out.append(f"{METHOD}_{model}_nj_replicates.nwk")
    return out


def write_run(tmp, rows, names, db=None):
    """An external-alignment-hip run of ``rows`` under ``names``: ``(database, alignment file)``."""
    fasta = tmp / "genomes"
    fasta.mkdir()
    for name, row in zip(names, rows):
        (fasta / name).write_bytes(b">" + stem(name).encode() + b" some words\n" + bytes(row[row != ord("-")]) + b"\n")
    aln = tmp / "rows.aln.fasta"
    aln.write_bytes(b"".join(b">" + stem(name).encode() + b"\n" + bytes(row) + b"\n" for name, row in zip(names, rows)))
    db = db or tmp / "runs.sqlite"
    assert rundb.run_external_alignment_hip(fasta, db, alignment=aln, temp=tmp / "t", logger=LOGGER, engine=NumpyMsaEngine()).status == "Done"
    return db, aln


@pytest.fixture(scope="module")
def made(tmp_path_factory):
    """``(database, alignment file, the alignment's rows, file name of each row)``: run 1 is the alignment's."""
    tmp = tmp_path_factory.mktemp("phylo_command")
    rows = cases.alignment(N, COLUMNS, SEED)
    db, aln = write_run(tmp, rows, NAMES)
    return db, aln, rows, NAMES


def read_table(path) -> tuple[list[str], np.ndarray]:
    lines = path.read_text().split("\n")
    assert lines[-1] == ""
    header = lines[0].split("\t")
    assert header[0] == ""
    cells = [line.split("\t") for line in lines[1:-1]]
    assert [c[0] for c in cells] == header[1:]
    values = np.array([[float(x) for x in c[1:]] for c in cells])
    assert all(repr(float(x)) == x for c in cells for x in c[1:])  # written as repr
    return header[1:], values


def as_table(joins: tree_cases.Joins, n: int) -> tree_mod.JoinTable:
    return tree_mod.JoinTable(n, np.asarray(joins.child, dtype=np.uint32), np.asarray(joins.length, dtype=np.float64), tuple(joins.last), joins.last_len, False)


@pytest.mark.parametrize(("model", "label"), [("k80", "stem"), ("jc69", "filename"), ("p", "md5")])
def test_the_table_and_the_tree_are_the_restated_pipelines(made, tmp_path, model, label, caplog):
    caplog.set_level(logging.INFO)
    db, _aln, rows, names = made
    written = rundb.phylo_run(db, tmp_path / "out", label=label, model=model)
    assert [p.name for p in written] == names_of(model) and sorted(p.name for p in (tmp_path / "out").iterdir()) == sorted(names_of(model))
    order = order_under(label, db, names)
    if label == "stem":
        assert order != list(range(N))  # the alignment's rows are not in label order
    labels = shown_labels(label, db, names)
    want = cases.pipeline(rows[order], model, 3.0)
    got_labels, D = read_table(written[0])
    assert got_labels == labels
    cases.assert_distances(D, want.D.undefined, want.D, model)
    assert (D > 0).sum() == N * (N - 1)
    # the tree of the table itself, byte for byte; of the restatement's table, the same tree
    own = tree_cases.neighbour_joining(D)
    assert written[1].read_text() == tree_mod.newick(as_table(own, N), labels) + "\n"
    cases.assert_same_tree(N, own, want.reference, model)
    assert f"{model} distances of 9 genomes: 0 pairs without a shared nucleotide column, 0 saturated pairs (distance 3.0)" in caplog.messages


def test_undefined_pairs_get_the_missing_distance_and_are_logged(tmp_path, caplog):
    caplog.set_level(logging.INFO)
    rows = np.array(cases.alignment(5, 40, 3))
    rows[1, :20], rows[2, 20:] = ord("-"), ord("-")  # rows 1 and 2 share no column
    rows[3] = np.frombuffer(b"ACGT" * 10, dtype=np.uint8)
    rows[4] = np.frombuffer(b"CATG" * 10, dtype=np.uint8)  # every column a transversion: saturated under both models
    names = [f"u{i}.fasta" for i in range(5)]
    db, _aln = write_run(tmp_path, rows, names)
    for model, saturated in (("p", 0), ("jc69", None), ("k80", None)):
        written = rundb.phylo_run(db, tmp_path / model, model=model, missing=0.5)
        want = cases.pipeline(rows, model, 0.5)
        _labels, D = read_table(written[0])
        cases.assert_distances(D, want.D.undefined, want.D, model)
        assert want.D.undefined[0] == 1 and (saturated is None or want.D.undefined[1] == saturated) and D[1, 2] == 0.5  # noqa: PLR2004
        assert model == "p" or (want.D.undefined[1] >= 1 and D[3, 4] == 0.5)  # noqa: PLR2004
        assert (f"{model} distances of 5 genomes: 1 pairs without a shared nucleotide column, {want.D.undefined[1]} saturated pairs (distance 0.5)"
                in caplog.messages)  # fmt: skip


def restated_support_files(want: cases.Restated, labels: list[str], replicates: int) -> tuple[str, str, str]:
    """The three bootstrap files' texts from the restated pipeline, the Newick text written here on its own."""
    n, reference, support = len(labels), want.reference, want.support
    below = {i: 1 for i in range(n)}
    above = {}
    for t in range(n - 2):
        lo, hi = int(reference.child[t][0]), int(reference.child[t][1])
        below[n + t] = below[lo] + below[hi]
        above[lo], above[hi] = float(reference.length[t][0]), float(reference.length[t][1])
    a, b = reference.last
    above[a] = float(reference.last_len)

    def text(node: int) -> str:
        if node < n:
            return f"{labels[node]}:{above[node]!r}"
        t = node - n
        return f"({text(int(reference.child[t][0]))},{text(int(reference.child[t][1]))}){support[t]}:{above[node]!r}"

    t = b - n
    nwk = f"({text(int(reference.child[t][0]))},{text(int(reference.child[t][1]))},{text(a)});\n"
    tsv = "#node\tn_leaves\tlength\tsupport\treplicates\n" + "".join(
        f"{n + t}\t{below[n + t]}\t{above[n + t]!r}\t{support[t]}\t{replicates}\n" for t in range(n - 3))
    kept = "".join(tree_mod.newick(as_table(x, n), labels) + "\n" for x in want.trees)
    return nwk, tsv, kept


def test_the_support_is_the_restatements(made, tmp_path):
    db, _aln, rows, names = made
    order, labels = order_under("stem", db, names), shown_labels("stem", db, names)
    # p takes no logarithm: every byte of every file is the restatement's
    written = rundb.phylo_run(db, tmp_path / "p", model="p", replicates=30, seed=4, keep_trees=True)
    assert [p.name for p in written] == names_of("p", True, True)
    want = cases.pipeline(rows[order], "p", 3.0, replicates=30, seed=4)
    nwk, tsv, kept = restated_support_files(want, labels, 30)
    assert written[2].read_text() == nwk and written[3].read_text() == tsv
    assert written[4].read_text() == kept and kept.count("\n") == 30  # noqa: PLR2004
    assert written[1].read_text() == tree_mod.newick(as_table(want.reference, N), labels) + "\n"
    labelled = want.support[:-1]
    assert len(labelled) == N - 3 and min(labelled) < 30 and all(0 <= s <= 30 for s in labelled)  # noqa: PLR2004
    # k80: the same draws.  The rule's logarithm and math.log differ in last bits, which may number a tree's joins another
    # way but give the same edges: the support of the written tree's nodes among the restatement's replicate trees
    written = rundb.phylo_run(db, tmp_path / "k80", replicates=30, seed=4)
    assert [p.name for p in written] == names_of("k80", True)
    want = cases.pipeline(rows[order], "k80", 3.0, replicates=30, seed=4)
    own = tree_cases.neighbour_joining(read_table(written[0])[1])  # the written tree's joins (the test above)
    support = bootstrap_cases.support(N, own.child, [bootstrap_cases.clades(N, t) for t in want.trees])
    lines = [line.split("\t") for line in written[3].read_text().split("\n")[1:-1]]
    assert [int(c[3]) for c in lines] == support[:-1] and {c[4] for c in lines} == {"30"} and min(support[:-1]) < 30  # noqa: PLR2004
    assert [int(c[0]) for c in lines] == list(range(N, 2 * N - 3))
    # another seed draws other columns; the seed is bootstrap-run's
    assert written[3].read_text() != rundb.phylo_run(db, tmp_path / "other", replicates=30, seed=5)[3].read_text()


def test_alignment_elsewhere_and_its_checks(made, tmp_path):
    db, aln, _rows, _names = made
    moved = tmp_path / "db"
    moved.mkdir()
    shutil.copy(db, moved / "runs.sqlite")
    with pytest.raises(SystemExit) as exit_:
        rundb.phylo_run(moved / "runs.sqlite", tmp_path / "out")
    assert str(exit_.value) == f"Missing alignment file {moved / aln.name}"
    elsewhere = tmp_path / "copy.fasta"
    shutil.copy(aln, elsewhere)
    written = rundb.phylo_run(moved / "runs.sqlite", tmp_path / "out", alignment=elsewhere)
    assert written[0].read_text() == rundb.phylo_run(db, tmp_path / "out2")[0].read_text()
    elsewhere.write_bytes(aln.read_bytes() + b"\n")
    assert hashlib.md5(elsewhere.read_bytes()).hexdigest() != hashlib.md5(aln.read_bytes()).hexdigest()
    with pytest.raises(SystemExit) as exit_:
        rundb.phylo_run(db, tmp_path / "out3", alignment=elsewhere)
    assert str(exit_.value) == f"MD5 checksum of {elsewhere} didn't match."
    assert not list((tmp_path / "out3").iterdir())


@pytest.fixture(scope="module")
def other_runs(tmp_path_factory):
    """A database with a sourmash-hip run (run 1) and an external-alignment-hip run of three genomes (run 2)."""
    tmp = tmp_path_factory.mktemp("phylo_other")
    db = tmp / "runs.sqlite"
    scaled, _genomes = FIXTURE_SETS["bacterial_example"]
    assert rundb.run_sourmash_hip(GOLDEN / "bacterial_example", db, cache=tmp / "cache", scaled=scaled, engine=OracleEngine(), temp=tmp).status == "Done"
    write_run(tmp, cases.alignment(3, 40, 5), [f"t{i}.fasta" for i in range(3)], db)
    return db


def test_a_run_without_columns_and_three_genomes(other_runs, tmp_path):
    with pytest.raises(SystemExit) as exit_:
        rundb.phylo_run(other_runs, tmp_path, run_id=1)
    assert str(exit_.value) == "Run-id 1 is a sourmash-hip run: it has no columns to resample (phylo-run needs an external-alignment-hip run)"
    with pytest.raises(SystemExit) as exit_:
        rundb.phylo_run(other_runs, tmp_path, run_id=2, replicates=5)
    assert str(exit_.value) == "Run-id 2 has 3 genomes: a tree of fewer than 4 has no internal edge to support"
    assert not list(tmp_path.iterdir())
    written = rundb.phylo_run(other_runs, tmp_path, run_id=2)  # without replicates three genomes have their table and tree
    assert [p.name for p in written] == names_of("k80") and written[1].read_text().count(",") == 2  # noqa: PLR2004


def test_the_order_of_the_opening_checks(made, other_runs, tmp_path):
    db = made[0]
    none, out = tmp_path / "none.sqlite", tmp_path / "new"
    with pytest.raises(SystemExit, match=f"Database {none} does not exist"):
        rundb.phylo_run(none, out, model="tn93")
    for options, message in (
        ({"model": "tn93", "replicates": -1}, "Unknown substitution model 'tn93': expected one of p, jc69, k80"),
        ({"replicates": -1, "seed": -1}, "Expected 0 to 100000 replicates, not -1"),
        ({"replicates": 100_001}, "Expected 0 to 100000 replicates, not 100001"),
        ({"seed": 1 << 64, "missing": -1.0}, r"Expected a seed from 0 to 2\^64 - 1, not 18446744073709551616"),
        ({"missing": float("nan"), "run_id": 9}, "The distance of a pair without identity must be finite and not negative, not nan"),
    ):
        with pytest.raises(SystemExit, match=message):
            rundb.phylo_run(db, out, **options)
        assert not out.exists()
    with pytest.raises(SystemExit, match=f"Database {db} has no run-id 9."):
        rundb.phylo_run(db, out, run_id=9, label="nonsense")
    assert out.is_dir()  # the output directory before the run
    # an incomplete run before its method, the method before the genomes and the labels, the labels before the alignment
    partial = tmp_path / "partial.sqlite"
    shutil.copy(other_runs, partial)
    with sqlite3.connect(partial) as conn:
        conn.execute("DELETE FROM comparisons WHERE comparison_id = (SELECT MAX(comparison_id) FROM comparisons WHERE configuration_id = "
                     "(SELECT configuration_id FROM runs WHERE run_id = 1))")  # fmt: skip
    conn.close()
    with pytest.raises(SystemExit, match=r"run-id 1 has 15 of 4\^2=16 comparisons, 1 needed"):
        rundb.phylo_run(partial, out, run_id=1)
    with pytest.raises(SystemExit, match="it has no columns to resample"):
        rundb.phylo_run(other_runs, out, run_id=1, label="nonsense", replicates=3)
    with pytest.raises(SystemExit, match="a tree of fewer than 4 has no internal edge to support"):
        rundb.phylo_run(other_runs, out, run_id=2, label="nonsense", replicates=3)
    with pytest.raises(SystemExit, match="Unexpected label scheme 'nonsense'"):
        rundb.phylo_run(db, out, label="nonsense", alignment=tmp_path / "none.fasta")
    with pytest.raises(SystemExit, match=f"Missing alignment file {tmp_path / 'none.fasta'}"):
        rundb.phylo_run(db, out, alignment=tmp_path / "none.fasta")
    assert not list(out.iterdir())


def test_main_prints_one_path_a_line(made, tmp_path, capsys):
    db = made[0]
    out = tmp_path / "out"
    assert rundb.main(["phylo-run", "-d", str(db), "-o", str(out), "--replicates", "5", "--seed", "2", "--keep-trees", "--model", "jc69"]) == 0
    assert capsys.readouterr().out.split("\n") == [*(str(out / name) for name in names_of("jc69", True, True)), ""]
    assert rundb.main(["phylo-run", "-d", str(db), "-o", str(out), "--label", "md5", "--missing", "0.5", "--keep-trees"]) == 0
    assert capsys.readouterr().out.split("\n") == [*(str(out / name) for name in names_of("k80")), ""]  # no replicates: no trees to keep
    with pytest.raises(SystemExit):
        rundb.main(["phylo-run", "-d", str(db), "-o", str(out), "--model", "tn93"])


def test_help_is_the_recorded_text(monkeypatch, capsys):
    monkeypatch.setenv("COLUMNS", "100")
    with pytest.raises(SystemExit) as exit_:
        rundb.main(["phylo-run", "--help"])
    assert exit_.value.code == 0
    assert capsys.readouterr().out == HELP.read_text()


def test_substitution_imports_neither_rundb_nor_reports():
    import subprocess
    import sys
    from pathlib import Path

    code = "import sys, pyani_plus_amd.substitution; print([m for m in ('rundb', 'reports') if 'pyani_plus_amd.' + m in sys.modules])"
    done = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, cwd=Path(__file__).parent.parent, check=False)
    assert done.returncode == 0, done.stderr
    assert done.stdout.strip() == "[]"
