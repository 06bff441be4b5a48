"""``mantel-run-comp`` on the host path: two sourmash-hip runs of the bacterial fixture set at two ``scaled`` values in one
database (run 3: three of the four genomes; run 4: two of them), the tables re-derived from ``mantel.mantel_test`` on the
runs' distances, the order of the failures, what ``main`` prints and its ``--help``."""

from __future__ import annotations

import logging
import shutil
import sqlite3

import numpy as np
import pytest

from pyani_plus_amd import mantel as mantel_mod
from pyani_plus_amd import reports, rundb
from pyani_plus_amd import tree as tree_mod
from tests.fake_engine import OracleEngine
from tests.helpers import FIXTURE_SETS, GOLDEN

HELP = GOLDEN / "mantel" / "help.txt"
SUMMARY = "sourmash-hip_identity_{ref}_mantel.tsv"
NULL = "sourmash-hip_identity_{ref}_vs_{other}_mantel_null.tsv"


@pytest.fixture(scope="module")
def db(tmp_path_factory):
    """Runs 1 and 2: the four genomes at ``scaled`` and twice that; run 3: three of them; run 4: two of them."""
    tmp = tmp_path_factory.mktemp("mantel_command")
    scaled, genomes = FIXTURE_SETS["bacterial_example"]
    names = sorted(genomes.values())
    path = tmp / "runs.sqlite"
    for value in (scaled, 2 * scaled):
        assert rundb.run_sourmash_hip(GOLDEN / "bacterial_example", path, cache=tmp / "cache", scaled=value, engine=OracleEngine(), temp=tmp).status == "Done"
    for count in (3, 2):
        subset = tmp / f"first_{count}"
        subset.mkdir()
        for name in names[:count]:
            shutil.copy(GOLDEN / "bacterial_example" / name, subset / name)
        assert rundb.run_sourmash_hip(subset, path, cache=tmp / "cache", scaled=scaled, engine=OracleEngine(), temp=tmp).status == "Done"
    return path


def run_distances(db, run_id: int, hashes=None) -> tuple[list[str], np.ndarray]:
    """The distances of a run over ``hashes`` (None: its own, sorted), from the database by the public pieces."""
    logger = logging.getLogger("test")
    conn, run, _n, _done = reports._open_complete_run(logger, db, run_id, "Reading")
    identity = reports._score_frames(logger, conn, run)[0]
    conn.close()
    hashes = sorted(identity.index) if hashes is None else hashes
    return hashes, tree_mod.run_distances(identity.loc[hashes, hashes])


def fields(path) -> list[list[str]]:
    return [line.split("\t") for line in path.read_text().split("\n")[:-1]]


def test_the_tables_are_the_test_of_the_runs_distances(db, tmp_path):
    written = rundb.mantel_run_comp(db, tmp_path / "out", "1,2", permutations=200, seed=3)
    assert [p.name for p in written] == [SUMMARY.format(ref=1), NULL.format(ref=1, other=2)]
    hashes, X = run_distances(db, 1)
    _hashes, Y = run_distances(db, 2)
    assert len(hashes) == 4 and not np.array_equal(X, Y)
    test = mantel_mod.mantel_test(X, Y, 200, 3)
    header, line = fields(written[0])
    assert "\t".join(header) == "#run_id\tmethod\tname\tgenomes\tpairs\tmantel_r\tpermutations\tseed\tat_least_observed\tp_value"
    name = sqlite3.connect(db).execute("SELECT name FROM runs WHERE run_id = 2").fetchone()[0]
    assert line == ["2", "sourmash-hip", name, "4", "6", repr(test.r), "200", "3", str(test.at_least), repr(test.p)]
    assert 0.0 < test.p <= 1.0 and test.p == (test.at_least + 1) / 201
    null = fields(written[1])
    assert null[0] == ["#permutation", "mantel_r"] and len(null) == 201
    assert null[1:] == [[str(q), repr(r)] for q, r in enumerate(test.null_r.tolist())]


def test_a_run_against_itself(db, tmp_path):
    written = rundb.mantel_run_comp(db, tmp_path, [1, 1], permutations=50)
    line = fields(written[0])[1]
    assert abs(float(line[5]) - 1.0) <= 1e-12 and int(line[8]) >= 1  # the identity is among 50 of 24 arrangements
    assert written[1].name == NULL.format(ref=1, other=1)


def test_no_permutations(db, tmp_path):
    written = rundb.mantel_run_comp(db, tmp_path, "1,2", permutations=0)
    line = fields(written[0])[1]
    assert line[6:] == ["0", "0", "0", "1.0"]
    assert written[1].read_text() == "#permutation\tmantel_r\n"


def test_several_runs_and_the_genomes_in_common(db, tmp_path):
    written = rundb.mantel_run_comp(db, tmp_path, "2,1,3", permutations=20, seed=9)
    assert [p.name for p in written] == [SUMMARY.format(ref=2), NULL.format(ref=2, other=1), NULL.format(ref=2, other=3)]
    lines = fields(written[0])
    assert [line[0] for line in lines[1:]] == ["1", "3"] and [line[3:5] for line in lines[1:]] == [["4", "6"], ["3", "3"]]
    common, Y = run_distances(db, 3)
    assert len(common) == 3
    _hashes, X = run_distances(db, 2, common)
    test = mantel_mod.mantel_test(X, Y, 20, 9)
    assert lines[2][5:] == [repr(test.r), "20", "9", str(test.at_least), repr(test.p)]


def test_fewer_than_three_genomes_in_common(db, tmp_path):
    with pytest.raises(SystemExit) as exit_:
        rundb.mantel_run_comp(db, tmp_path, "1,4")
    assert str(exit_.value) == "Runs 1 and 4 have 2 genomes in common: a Mantel test needs at least 3"


def test_an_incomplete_run(db, tmp_path):
    partial = tmp_path / "partial.sqlite"
    shutil.copy(db, partial)
    with sqlite3.connect(partial) as conn:
        conn.execute("DELETE FROM comparisons WHERE comparison_id = (SELECT MAX(comparison_id) FROM comparisons WHERE configuration_id = "
                     "(SELECT configuration_id FROM runs WHERE run_id = 2))")  # fmt: skip
    conn.close()
    with pytest.raises(SystemExit) as exit_:
        rundb.mantel_run_comp(partial, tmp_path / "out", "1,2")
    assert str(exit_.value) == "run-id 2 has 15 of 4^2=16 comparisons, 1 needed"
    assert not list((tmp_path / "out").iterdir())  # every run is opened before anything is written


def test_an_identity_above_one(db, tmp_path):
    broken = tmp_path / "broken.sqlite"
    shutil.copy(db, broken)
    with sqlite3.connect(broken) as conn:
        conn.execute("UPDATE comparisons SET identity = 3.0 WHERE comparison_id = (SELECT MIN(comparison_id) FROM comparisons WHERE "
                     "query_hash != subject_hash AND configuration_id = (SELECT configuration_id FROM runs WHERE run_id = 2))")  # fmt: skip
        conn.execute("UPDATE runs SET df_identity = NULL, df_cov_query = NULL, df_hadamard = NULL")
    conn.close()
    with pytest.raises(SystemExit) as exit_:
        rundb.mantel_run_comp(broken, tmp_path / "out", "1,2", permutations=5)
    assert str(exit_.value) == "An identity above 1 gives a negative distance: no Mantel test is defined"


def test_the_order_of_the_failures(db, tmp_path):
    none, out = tmp_path / "none.sqlite", tmp_path / "new"
    with pytest.raises(SystemExit, match=f"Database {none} does not exist"):
        rundb.mantel_run_comp(none, out, "x", permutations=-1)
    for options, message in (
        ({"permutations": -1, "seed": -1}, "Expected 0 to 1000000 permutations, not -1"),
        ({"permutations": 1_000_001}, "Expected 0 to 1000000 permutations, not 1000001"),
        ({"seed": 1 << 64, "missing": -1.0}, r"Expected a seed from 0 to 2\^64 - 1, not 18446744073709551616"),
        ({"seed": -1}, r"Expected a seed from 0 to 2\^64 - 1, not -1"),
        ({"missing": float("nan")}, "The distance of a pair without identity must be finite and not negative, not nan"),
        ({"missing": -0.5}, "The distance of a pair without identity must be finite and not negative, not -0.5"),
    ):
        with pytest.raises(SystemExit, match=message):
            rundb.mantel_run_comp(db, out, "x", **options)
        assert not out.exists()
    with pytest.raises(SystemExit, match="Expected comma separated list of runs, not: 1,x"):
        rundb.mantel_run_comp(db, out, "1,x")
    assert out.is_dir()  # the output directory before the runs
    with pytest.raises(SystemExit, match="Need at least two runs for a comparison"):
        rundb.mantel_run_comp(db, out, "1")
    with pytest.raises(SystemExit, match=f"Database {db} has no run-id 7."):
        rundb.mantel_run_comp(db, out, "1,7")
    assert not list(out.iterdir())


def test_the_largest_seed(db, tmp_path):
    written = rundb.mantel_run_comp(db, tmp_path, "1,2", permutations=5, seed=(1 << 64) - 1)
    assert fields(written[0])[1][7] == str((1 << 64) - 1)


def test_main_prints_the_paths(db, tmp_path, capsys):
    out = tmp_path / "out"
    assert rundb.main(["mantel-run-comp", "-d", str(db), "-o", str(out), "--run-ids", "1,2,3", "--permutations", "10", "--seed", "2"]) == 0
    printed = capsys.readouterr().out.split("\n")
    assert printed == [str(out / SUMMARY.format(ref=1)), str(out / NULL.format(ref=1, other=2)), str(out / NULL.format(ref=1, other=3)), ""]
    assert all((out / name).is_file() for name in (SUMMARY.format(ref=1), NULL.format(ref=1, other=2)))


def test_help_is_the_recorded_text(monkeypatch, capsys):
    monkeypatch.setenv("COLUMNS", "100")
    with pytest.raises(SystemExit) as exit_:
        rundb.main(["mantel-run-comp", "--help"])
    assert exit_.value.code == 0
    assert capsys.readouterr().out == HELP.read_text()


def test_mantel_imports_neither_rundb_nor_reports():
    import subprocess
    import sys
    from pathlib import Path

    code = "import sys, pyani_plus_amd.mantel; print([m for m in ('rundb', 'reports') if 'pyani_plus_amd.' + m in sys.modules])"
    done = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, cwd=Path(__file__).parent.parent, check=False)
    assert done.returncode == 0, done.stderr
    assert done.stdout.strip() == "[]"
