"""``dereplicate-run`` on the host path: a sourmash-hip run of the viral fixture set (three genomes; by length OP073605,
MGV-GENOME-0266457, MGV-GENOME-0264574), the two tables byte for byte at thresholds that give one, two and three
representatives, both preferences, every label scheme, the order of the opening checks, ``--help`` and what ``main``
prints.  The expected tables are derived here from the run's matrices with the restatement of tests/derep_cases.py."""

from __future__ import annotations

import logging
import shutil
import sqlite3
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

from pyani_plus_amd import reports, rundb
from tests import derep_cases as dc
from tests.fake_engine import OracleEngine
from tests.helpers import FIXTURE_SETS, GOLDEN

HELP = GOLDEN / "dereplicate" / "help.txt"
MEMBERS, REPRESENTATIVES = "sourmash-hip_dereplicate.tsv", "sourmash-hip_representatives.tsv"
LONG, MIDDLE, SHORT = "OP073605", "MGV-GENOME-0266457", "MGV-GENOME-0264574"  # 57793, 39594 and 39253 bases


@pytest.fixture(scope="module")
def db(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("derep_command")
    scaled, _genomes = FIXTURE_SETS["viral_example"]
    path = tmp / "runs.sqlite"
    assert rundb.run_sourmash_hip(GOLDEN / "viral_example", path, cache=tmp / "cache", scaled=scaled, engine=OracleEngine(), temp=tmp).status == "Done"
    return path


def run_matrices(db, label: str = "stem"):
    """``(labels, lengths, identity, coverage)`` of the run as ``classify`` reads it, by the public pieces."""
    logger = logging.getLogger("test")
    conn, run, _n, _done = reports._open_complete_run(logger, db, None, "Reading")
    frames = reports._score_frames(logger, conn, run)
    lengths = dict(conn.execute("SELECT genome_hash, length FROM genomes").fetchall())
    conn.close()
    mapping = reports._label_mapping(logger, run, label)
    identity, cov, _hadamard = reports._relabelled(logger, run, frames, label)
    by_label = {mapping[h]: lengths[h] for h in mapping}
    labels = [str(x) for x in cov.columns]
    return labels, [by_label[x] for x in labels], identity.to_numpy(dtype=float), cov.to_numpy(dtype=float)


def expected_tables(db, *, label="stem", prefer="length", mode="greedy", min_identity=0.95, cov_min=0.5, score_edges="mean", coverage_edges="min"):  # noqa: PLR0913
    """The two tables from the contract: rank the genomes, permute, restate, write."""
    labels, lengths, S, C = run_matrices(db, label)
    order = sorted(range(len(labels)), key=(lambda p: (-lengths[p], labels[p])) if prefer == "length" else (lambda p: labels[p]))
    S, C = S[np.ix_(order, order)], C[np.ix_(order, order)]
    names, sizes = [labels[p] for p in order], [lengths[p] for p in order]
    adj = dc.adjacency(S, C, score_edges, coverage_edges, min_identity, cov_min)
    is_rep = dc.select(adj, mode)
    rep, score = dc.assign(S, score_edges, adj, is_rep)

    def text(value) -> str:
        return "NA" if value != value else str(float(value))

    members, chosen = ["genome\trepresentative\tidentity\tlength"], ["representative\tn_members\tlength\tmin_identity"]
    for r in range(len(names)):
        if not is_rep[r]:
            continue
        group = [p for p in range(len(names)) if rep[p] == r and p != r]
        members += [f"{names[p]}\t{names[r]}\t{text(score[p])}\t{sizes[p]}" for p in [r, *group]]
        chosen.append(f"{names[r]}\t{len(group) + 1}\t{sizes[r]}\t{text(min((score[p] for p in group), default=float('nan')))}")
    return "\n".join(members) + "\n", "\n".join(chosen) + "\n", int(is_rep.sum())


def representatives(path) -> list[str]:
    return [line.split("\t")[0] for line in path.read_text().split("\n")[1:-1]]


# the mean identities of the three pairs are about 0.9997 (LONG, SHORT), 0.9979 (MIDDLE, SHORT) and 0.9962 (LONG, MIDDLE)
@pytest.mark.parametrize("min_identity,count,chosen", ((0.95, 1, [LONG]), (0.997, 2, [LONG, MIDDLE]), (0.9999, 3, [LONG, MIDDLE, SHORT])))
@pytest.mark.parametrize("mode", dc.MODES)
def test_the_tables_byte_for_byte(db, tmp_path, min_identity, count, chosen, mode):
    written = rundb.dereplicate_run(db, tmp_path / "out", min_identity=min_identity, mode=mode)
    assert [p.name for p in written] == [MEMBERS, REPRESENTATIVES]
    members, reps, n_reps = expected_tables(db, min_identity=min_identity, mode=mode)
    assert n_reps == (count if mode == "greedy" else len(representatives(written[1])))  # cover may need fewer
    assert written[0].read_text() == members and written[1].read_text() == reps
    if mode == "greedy":
        assert representatives(written[1]) == chosen
    rows = [line.split("\t") for line in written[0].read_text().split("\n")[1:-1]]
    assert sorted(row[0] for row in rows) == sorted([LONG, MIDDLE, SHORT])
    assert [row[3] for row in rows if row[0] == LONG] == ["57793"]


def test_one_representative_in_full(db, tmp_path):
    written = rundb.dereplicate_run(db, tmp_path)
    _labels, _lengths, S, _C = run_matrices(db)  # label order: SHORT, MIDDLE, LONG
    to_middle, to_short = (S[1, 2] + S[2, 1]) / 2.0, (S[0, 2] + S[2, 0]) / 2.0
    assert written[0].read_text() == (
        "genome\trepresentative\tidentity\tlength\n"
        f"{LONG}\t{LONG}\t1.0\t57793\n{MIDDLE}\t{LONG}\t{float(to_middle)}\t39594\n{SHORT}\t{LONG}\t{float(to_short)}\t39253\n"
    )
    assert written[1].read_text() == f"representative\tn_members\tlength\tmin_identity\n{LONG}\t3\t57793\t{float(min(to_middle, to_short))}\n"


def test_three_representatives_are_alone(db, tmp_path):
    written = rundb.dereplicate_run(db, tmp_path, min_identity=0.9999)
    assert written[1].read_text() == (
        f"representative\tn_members\tlength\tmin_identity\n{LONG}\t1\t57793\tNA\n{MIDDLE}\t1\t39594\tNA\n{SHORT}\t1\t39253\tNA\n"
    )


def test_prefer_label(db, tmp_path):
    """In label order SHORT comes first and is adjacent to both others at 0.997: one representative, where the length
    order gives two."""
    written = rundb.dereplicate_run(db, tmp_path, min_identity=0.997, prefer="label")
    members, reps, n_reps = expected_tables(db, min_identity=0.997, prefer="label")
    assert n_reps == 1 and representatives(written[1]) == [SHORT]
    assert written[0].read_text() == members and written[1].read_text() == reps
    assert [line.split("\t")[0] for line in written[0].read_text().split("\n")[1:-1]] == [SHORT, MIDDLE, LONG]


@pytest.mark.parametrize("options", ({"score_edges": "min", "coverage_edges": "max"}, {"score_edges": "max", "cov_min": 0.99, "min_identity": 0.99}))
def test_the_aggregators_and_the_coverage_threshold(db, tmp_path, options):
    written = rundb.dereplicate_run(db, tmp_path, **options)
    members, reps, _n_reps = expected_tables(db, **options)
    assert written[0].read_text() == members and written[1].read_text() == reps


@pytest.mark.parametrize("label", ("stem", "md5", "filename"))
def test_every_label_scheme(db, tmp_path, label):
    written = rundb.dereplicate_run(db, tmp_path, label=label, min_identity=0.997)
    members, reps, n_reps = expected_tables(db, label=label, min_identity=0.997)
    assert n_reps == 2 and written[0].read_text() == members and written[1].read_text() == reps
    first = representatives(written[1])[0]
    assert first == {"stem": LONG, "filename": LONG + ".fasta"}.get(label, first) and (label != "md5" or len(first) == 32)  # noqa: PLR2004


def test_duplicate_stems_and_the_way_out(db, tmp_path):
    twice = tmp_path / "twice.sqlite"
    shutil.copy(db, twice)
    with sqlite3.connect(twice) as conn:
        conn.execute("UPDATE runs_genomes SET fasta_filename = 'OP073605.fna' WHERE fasta_filename = 'MGV-GENOME-0264574.fas'")
    conn.close()
    with pytest.raises(SystemExit) as exit_:
        rundb.dereplicate_run(twice, tmp_path / "out")
    assert str(exit_.value) == "Duplicate filename stems, consider using MD5 labelling."
    assert not list((tmp_path / "out").iterdir())
    written = rundb.dereplicate_run(twice, tmp_path / "out", label="md5")
    assert len(representatives(written[1])) == 1


def test_the_order_of_the_opening_checks(db, tmp_path):
    none, out = tmp_path / "none.sqlite", tmp_path / "new"
    with pytest.raises(SystemExit, match=f"Database {none} does not exist"):
        rundb.dereplicate_run(none, out, mode="best", run_id=7)
    for options, message in (
        ({"min_identity": float("nan"), "cov_min": float("nan")}, "The minimum identity must be a number, not nan"),
        ({"cov_min": float("nan"), "score_edges": "median"}, "The minimum coverage must be a number, not nan"),
        ({"coverage_edges": "median", "score_edges": "mode"}, "Unknown coverage aggregator 'median': expected one of min, max, mean"),
        ({"score_edges": "median", "mode": "best"}, "Unknown score aggregator 'median': expected one of min, max, mean"),
        ({"mode": "best", "prefer": "quality"}, "Unknown dereplication mode 'best': expected one of greedy, cover"),
        ({"prefer": "quality", "run_id": 7}, "Unknown preference 'quality': expected one of length, label"),
    ):
        with pytest.raises(SystemExit) as exit_:
            rundb.dereplicate_run(db, out, **options)
        assert str(exit_.value) == message
        assert not out.exists()
    with pytest.raises(SystemExit) as exit_:
        rundb.dereplicate_run(db, out, run_id=7, label="name")
    assert str(exit_.value) == f"Database {db} has no run-id 7."
    assert out.is_dir()  # the output directory before the run
    with pytest.raises(SystemExit) as exit_:
        rundb.dereplicate_run(db, out, label="name")
    assert str(exit_.value) == "Unexpected label scheme 'name'"
    assert not list(out.iterdir())


def test_an_incomplete_run(db, tmp_path):
    partial = tmp_path / "partial.sqlite"
    shutil.copy(db, partial)
    with sqlite3.connect(partial) as conn:
        conn.execute("DELETE FROM comparisons WHERE comparison_id = (SELECT MAX(comparison_id) FROM comparisons)")
    conn.close()
    with pytest.raises(SystemExit) as exit_:
        rundb.dereplicate_run(partial, tmp_path / "out")
    assert str(exit_.value) == "run-id 1 has 8 of 3^2=9 comparisons, 1 needed"


def test_main_prints_one_path_per_line(db, tmp_path, capsys):
    out = tmp_path / "out"
    assert rundb.main(["dereplicate-run", "-d", str(db), "-o", str(out), "--min-identity", "0.997", "--mode", "cover", "--prefer", "label"]) == 0
    assert capsys.readouterr().out.split("\n") == [str(out / MEMBERS), str(out / REPRESENTATIVES), ""]
    members, reps, _n_reps = expected_tables(db, min_identity=0.997, mode="cover", prefer="label")
    assert (out / MEMBERS).read_text() == members and (out / REPRESENTATIVES).read_text() == reps


def test_main_defaults_are_the_functions(db, tmp_path, capsys):
    assert rundb.main(["dereplicate-run", "-d", str(db), "-o", str(tmp_path / "cli")]) == 0
    capsys.readouterr()
    direct = rundb.dereplicate_run(db, tmp_path / "direct")
    assert [(tmp_path / "cli" / p.name).read_bytes() for p in direct] == [p.read_bytes() for p in direct]


def test_help_is_the_recorded_text(monkeypatch, capsys):
    monkeypatch.setenv("COLUMNS", "100")
    with pytest.raises(SystemExit) as exit_:
        rundb.main(["dereplicate-run", "--help"])
    assert exit_.value.code == 0
    assert capsys.readouterr().out == HELP.read_text()


def test_rundb_exports_the_report():
    assert rundb.dereplicate_run is reports.dereplicate_run


def test_dereplicate_imports_neither_rundb_nor_reports():
    code = "import sys, pyani_plus_amd.dereplicate; print([m for m in ('rundb', 'reports') if 'pyani_plus_amd.' + m in sys.modules])"
    done = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, cwd=Path(__file__).parent.parent, check=False)
    assert done.returncode == 0, done.stderr
    assert done.stdout.strip() == "[]"
