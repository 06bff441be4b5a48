"""``bootstrap-run`` on the host path: an external-alignment-hip run of nine tiny genomes (made with the numpy stand-in of
the engine's MSA calls), the two files re-derived from the restatement of ``tests/bootstrap_cases.py``, the tree against
``tree-run``'s, the label schemes, the messages, the order of the opening checks, what ``main`` prints and ``--help``."""

from __future__ import annotations

import hashlib
import logging
import re
import shutil
import sqlite3

import numpy as np
import pytest

from pyani_plus_amd import reports, rundb
from pyani_plus_amd import tree as tree_mod
from tests import bootstrap_cases as cases
from tests import tree_cases
from tests.fake_engine import OracleEngine
from tests.helpers import FIXTURE_SETS, GOLDEN
from tests.msa_checker import NumpyMsaEngine

HELP = GOLDEN / "bootstrap" / "help.txt"
LOGGER = logging.getLogger("test")
N, COLUMNS, SEED = 9, 64, 13  # the third alignment of cases.SUPPORT_ALIGNMENTS
NWK = "external-alignment-hip_identity_nj_bootstrap.nwk"
TSV = "external-alignment-hip_identity_nj_bootstrap.tsv"
REPLICATES = "external-alignment-hip_identity_nj_replicates.nwk"
# file names whose order by stem, by file name and by md5 differ from the order of the alignment's records
NAMES = ["g7.fasta", "g2.fna", "g9.fas", "g1.fasta", "g5.fna", "g3.fasta", "g8.fas", "g4.fna", "g6.fasta"]


def stem(name: str) -> str:
    return name.rsplit(".", 1)[0]


@pytest.fixture(scope="module")
def made(tmp_path_factory):
    """``(database, alignment file, the alignment's rows, file name of each row)``: run 1 is the alignment's."""
    tmp = tmp_path_factory.mktemp("bootstrap_command")
    rows = cases.alignment(N, COLUMNS, SEED)
    fasta = tmp / "genomes"
    fasta.mkdir()
    for name, row in zip(NAMES, rows):
        (fasta / name).write_bytes(b">" + stem(name).encode() + b" some words\n" + bytes(row[row != cases.GAP]) + b"\n")
    aln = tmp / "nine.aln.fasta"
    aln.write_bytes(b"".join(b">" + stem(name).encode() + b"\n" + bytes(row) + b"\n" for name, row in zip(NAMES, rows)))
    db = tmp / "runs.sqlite"
    assert rundb.run_external_alignment_hip(fasta, db, alignment=aln, temp=tmp / "t", logger=LOGGER, engine=NumpyMsaEngine()).status == "Done"
    return db, aln, rows, NAMES


def _md5_of(db) -> dict[str, str]:
    """file name -> genome hash, of run 1"""
    conn = sqlite3.connect(db)
    try:
        return {str(filename).rsplit("/", 1)[-1]: md5 for md5, filename in conn.execute("SELECT genome_hash, fasta_filename FROM runs_genomes WHERE run_id = 1")}
    finally:
        conn.close()


def order_under(label: str, db, names: list[str]) -> list[int]:
    """The rows of the alignment in the order of tree-run's matrix: sorted by label."""
    if label == "md5":
        md5_of = _md5_of(db)
        shown = [md5_of[name] for name in names]
    else:
        shown = [stem(name) if label == "stem" else name for name in names]
    return sorted(range(len(names)), key=lambda i: shown[i])


def shown_labels(label: str, db, names: list[str]) -> list[str]:
    order = order_under(label, db, names)
    if label == "md5":
        md5_of = _md5_of(db)
        return [md5_of[names[i]] for i in order]
    return [stem(names[i]) if label == "stem" else names[i] for i in order]


def restated_files(rows: np.ndarray, labels: list[str], reference: tree_cases.Joins, replicates: int, seed: int, missing: float = 1.0):
    """The three files' texts from the restatement: the reference tree is tree-run's (given), the rest follows."""
    n, n_cols = rows.shape
    w = cases.weights(seed, n_cols, 0, replicates)
    trees = [tree_cases.neighbour_joining(cases.distances(*cases.counts(rows, w[r]), missing)) for r in range(replicates)]
    support = cases.support(n, reference.child, [cases.clades(n, t) for t in trees])
    # the Newick text, written here recursively and on its own
    below = {i: 1 for i in range(n)}
    above = {}
    for t in range(n - 2):
        lo, hi = int(reference.child[t][0]), int(reference.child[t][1])
        below[n + t] = below[lo] + below[hi]
        above[lo], above[hi] = float(reference.length[t][0]), float(reference.length[t][1])
    a, b = reference.last
    above[a] = float(reference.last_len)

    def text(node: int, supports) -> str:
        if node < n:
            return f"{labels[node]}:{above[node]!r}"
        t = node - n
        inner = f"({text(int(reference.child[t][0]), supports)},{text(int(reference.child[t][1]), supports)})"
        return f"{inner}{'' if supports is None else supports[t]}:{above[node]!r}"

    t = b - n
    nwk = f"({text(int(reference.child[t][0]), support)},{text(int(reference.child[t][1]), support)},{text(a, support)});\n"
    tsv = "#node\tn_leaves\tlength\tsupport\treplicates\n" + "".join(
        f"{n + t}\t{below[n + t]}\t{above[n + t]!r}\t{support[t]}\t{replicates}\n" for t in range(n - 3))
    kept = "".join(tree_mod.newick(tree_mod.JoinTable(n, x.child, x.length, x.last, x.last_len, False), labels) + "\n" for x in trees)
    return nwk, tsv, kept, support


def tree_run_table(db, label: str, tmp_path) -> tuple[str, tree_cases.Joins]:
    """tree-run's file of the run, and the restatement's tree of the distances tree-run reads."""
    written = rundb.tree_run(db, tmp_path / f"tree_{label}", label=label)
    conn, run, _n, _done = reports._open_complete_run(LOGGER, db, None, "Reading")
    identity = reports._relabelled(LOGGER, run, reports._score_frames(LOGGER, conn, run), label)[0]
    conn.close()
    return written.read_text(), tree_cases.neighbour_joining(tree_mod.run_distances(identity))


@pytest.mark.parametrize("label", ["stem", "filename", "md5"])
def test_the_files_are_the_restatements(made, tmp_path, label):
    db, _aln, rows, names = made
    written = rundb.bootstrap_run(db, tmp_path / "out", label=label, replicates=50, seed=0, keep_trees=True)
    assert [p.name for p in written] == [NWK, TSV, REPLICATES]
    order = order_under(label, db, names)
    if label == "stem":
        assert order != list(range(N))  # the alignment's rows are not in label order
    tree_text, reference = tree_run_table(db, label, tmp_path)
    nwk, tsv, kept, support = restated_files(rows[order], shown_labels(label, db, names), reference, 50, 0)
    assert written[0].read_text() == nwk
    assert written[1].read_text() == tsv
    assert written[2].read_text() == kept and kept.count("\n") == 50
    # the labels stripped: tree-run's file, byte for byte
    assert re.sub(r"\)\d+:", "):", written[0].read_text()) == tree_text
    labelled = support[:-1]
    assert len(labelled) == N - 3 and min(labelled) < 50 and all(0 <= s <= 50 for s in labelled)


def test_seed_replicates_missing_and_no_kept_trees(made, tmp_path):
    db, _aln, rows, names = made
    written = rundb.bootstrap_run(db, tmp_path, replicates=7, seed=(1 << 64) - 1, missing=0.5)
    assert [p.name for p in written] == [NWK, TSV] and not (tmp_path / REPLICATES).exists()
    _text, reference = tree_run_table(db, "stem", tmp_path)
    _nwk, tsv, _kept, _support = restated_files(rows[order_under("stem", db, names)], shown_labels("stem", db, names), reference, 7, (1 << 64) - 1, 0.5)
    assert written[1].read_text() == tsv
    assert written[1].read_text() != rundb.bootstrap_run(db, tmp_path / "other", replicates=7, seed=1)[1].read_text()


def test_alignment_elsewhere_and_its_checks(made, tmp_path):
    db, aln, _rows, _names = made
    moved = tmp_path / "db"
    moved.mkdir()
    shutil.copy(db, moved / "runs.sqlite")
    with pytest.raises(SystemExit) as exit_:
        rundb.bootstrap_run(moved / "runs.sqlite", tmp_path / "out", replicates=3)
    assert str(exit_.value) == f"Missing alignment file {moved / aln.name}"
    elsewhere = tmp_path / "copy.fasta"
    shutil.copy(aln, elsewhere)
    written = rundb.bootstrap_run(moved / "runs.sqlite", tmp_path / "out", replicates=3, alignment=elsewhere)
    assert written[1].read_text() == rundb.bootstrap_run(db, tmp_path / "out2", replicates=3)[1].read_text()
    elsewhere.write_bytes(aln.read_bytes() + b"\n")
    assert hashlib.md5(elsewhere.read_bytes()).hexdigest() != hashlib.md5(aln.read_bytes()).hexdigest()
    with pytest.raises(SystemExit) as exit_:
        rundb.bootstrap_run(db, tmp_path / "out", replicates=3, alignment=elsewhere)
    assert str(exit_.value) == f"MD5 checksum of {elsewhere} didn't match."
    with pytest.raises(SystemExit) as exit_:
        rundb.bootstrap_run(db, tmp_path / "out", replicates=3, alignment=tmp_path / "none.fasta")
    assert str(exit_.value) == f"Missing alignment file {tmp_path / 'none.fasta'}"


@pytest.fixture(scope="module")
def other_runs(tmp_path_factory):
    """A database with a sourmash-hip run (run 1) and an external-alignment-hip run of three genomes (run 2)."""
    tmp = tmp_path_factory.mktemp("bootstrap_other")
    db = tmp / "runs.sqlite"
    scaled, _genomes = FIXTURE_SETS["bacterial_example"]
    assert rundb.run_sourmash_hip(GOLDEN / "bacterial_example", db, cache=tmp / "cache", scaled=scaled, engine=OracleEngine(), temp=tmp).status == "Done"
    rows = cases.alignment(3, 40, 5)
    fasta = tmp / "three"
    fasta.mkdir()
    for i, row in enumerate(rows):
        (fasta / f"t{i}.fasta").write_bytes(b">t%d\n" % i + bytes(row[row != cases.GAP]) + b"\n")
    aln = tmp / "three.aln"
    aln.write_bytes(b"".join(b">t%d\n" % i + bytes(row) + b"\n" for i, row in enumerate(rows)))
    assert rundb.run_external_alignment_hip(fasta, db, alignment=aln, temp=tmp / "t", logger=LOGGER, engine=NumpyMsaEngine()).status == "Done"
    return db


def test_a_run_without_columns_and_a_run_without_an_internal_edge(other_runs, tmp_path):
    with pytest.raises(SystemExit) as exit_:
        rundb.bootstrap_run(other_runs, tmp_path, run_id=1)
    assert str(exit_.value) == "Run-id 1 is a sourmash-hip run: it has no columns to resample (bootstrap-run needs an external-alignment-hip run)"
    with pytest.raises(SystemExit) as exit_:
        rundb.bootstrap_run(other_runs, tmp_path, run_id=2)
    assert str(exit_.value) == "Run-id 2 has 3 genomes: a tree of fewer than 4 has no internal edge to support"
    assert not list(tmp_path.iterdir())


def test_the_order_of_the_opening_checks(made, other_runs, tmp_path):
    db = made[0]
    none, out = tmp_path / "none.sqlite", tmp_path / "new"
    with pytest.raises(SystemExit, match=f"Database {none} does not exist"):
        rundb.bootstrap_run(none, out, replicates=0)
    for options, message in (
        ({"replicates": 0, "seed": -1}, "Expected 1 to 100000 replicates, not 0"),
        ({"replicates": 100_001}, "Expected 1 to 100000 replicates, not 100001"),
        ({"seed": 1 << 64, "missing": -1.0}, r"Expected a seed from 0 to 2\^64 - 1, not 18446744073709551616"),
        ({"missing": float("nan"), "run_id": 9}, "The distance of a pair without identity must be finite and not negative, not nan"),
    ):
        with pytest.raises(SystemExit, match=message):
            rundb.bootstrap_run(db, out, **options)
        assert not out.exists()
    with pytest.raises(SystemExit, match=f"Database {db} has no run-id 9."):
        rundb.bootstrap_run(db, out, run_id=9, label="nonsense")
    assert out.is_dir()  # the output directory before the run
    # an incomplete run before its method, the method before the labels, the labels before the alignment
    partial = tmp_path / "partial.sqlite"
    shutil.copy(other_runs, partial)
    with sqlite3.connect(partial) as conn:
        conn.execute("DELETE FROM comparisons WHERE comparison_id = (SELECT MAX(comparison_id) FROM comparisons WHERE configuration_id = "
                     "(SELECT configuration_id FROM runs WHERE run_id = 1))")  # fmt: skip
    conn.close()
    with pytest.raises(SystemExit, match=r"run-id 1 has 15 of 4\^2=16 comparisons, 1 needed"):
        rundb.bootstrap_run(partial, out, run_id=1)
    with pytest.raises(SystemExit, match="it has no columns to resample"):
        rundb.bootstrap_run(other_runs, out, run_id=1, label="nonsense")
    with pytest.raises(SystemExit, match="Unexpected label scheme 'nonsense'"):
        rundb.bootstrap_run(db, out, label="nonsense", alignment=tmp_path / "none.fasta")
    assert not list(out.iterdir())


def test_main_prints_the_paths(made, tmp_path, capsys):
    db = made[0]
    out = tmp_path / "out"
    assert rundb.main(["bootstrap-run", "-d", str(db), "-o", str(out), "--replicates", "5", "--seed", "2", "--keep-trees"]) == 0
    assert capsys.readouterr().out.split("\n") == [str(out / NWK), str(out / TSV), str(out / REPLICATES), ""]
    assert rundb.main(["bootstrap-run", "-d", str(db), "-o", str(out), "--replicates", "5", "--label", "md5", "--missing", "0.5"]) == 0
    assert capsys.readouterr().out.split("\n") == [str(out / NWK), str(out / TSV), ""]


def test_help_is_the_recorded_text(monkeypatch, capsys):
    monkeypatch.setenv("COLUMNS", "100")
    with pytest.raises(SystemExit) as exit_:
        rundb.main(["bootstrap-run", "--help"])
    assert exit_.value.code == 0
    assert capsys.readouterr().out == HELP.read_text()


def test_bootstrap_imports_neither_rundb_nor_reports():
    import subprocess
    import sys
    from pathlib import Path

    code = "import sys, pyani_plus_amd.bootstrap; print([m for m in ('rundb', 'reports') if 'pyani_plus_amd.' + m in sys.modules])"
    done = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, cwd=Path(__file__).parent.parent, check=False)
    assert done.returncode == 0, done.stderr
    assert done.stdout.strip() == "[]"
