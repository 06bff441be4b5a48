"""What the six report commands (export-run, classify, tree-run, ordinate-run, plot-run, plot-run-comp) share, without a
GPU: the same failure gives the same text whichever command meets it, two failures at once give the one the command
checks first (with the side effects that come before it), ``--help`` of every subcommand is the recorded text, and the
three modules of the run driver import one way only.

The files under ``tests/golden/cli_help/`` are the standard output of ``rundb.main([<subcommand>, "--help"])`` with
``COLUMNS=100``, one per subcommand, recorded before the reports moved out of ``rundb``."""

from __future__ import annotations

import logging
import shutil
import sqlite3
import subprocess
import sys
from pathlib import Path

import pytest

from pyani_plus_amd import rundb
from tests.fake_engine import OracleEngine
from tests.helpers import FIXTURE_SETS, GOLDEN

HELP = GOLDEN / "cli_help"
SUBCOMMANDS = ("sourmash", "fastani", "external-alignment", "tetra", "resume", "export-run", "classify", "plot-run", "plot-run-comp",
               "tree-run", "ordinate-run")  # fmt: skip


def _plot_run_comp(database, outdir, *, run_id=None, **options):
    """plot-run-comp with the other commands' signature: ``run_id`` is its reference run, compared with run 2."""
    return rundb.plot_run_comp(database, outdir, "1,2" if run_id is None else f"{run_id},2", **options)


COMMANDS = {
    "export-run": rundb.export_run,
    "classify": rundb.classify,
    "tree-run": rundb.tree_run,
    "ordinate-run": rundb.ordinate_run,
    "plot-run": rundb.plot_run,
    "plot-run-comp": _plot_run_comp,
}
WITH_RUN = [c for c in COMMANDS if c != "plot-run-comp"]  # one run, which must be complete, under a label
WITH_FORMATS = ("ordinate-run", "plot-run", "plot-run-comp")
NO_MATPLOTLIB = r"Image formats \(png\) need matplotlib, which cannot be imported; only tsv is available"


@pytest.fixture(scope="module")
def dbs(tmp_path_factory):
    """``two_runs``: the viral fixture set run twice (run 2 finds every comparison there); ``duplicate_stems``: the same
    with two files of one stem; ``incomplete``: the same less the last comparison; ``no_runs``: the tables alone."""
    tmp = tmp_path_factory.mktemp("reports_common")
    scaled, _genomes = FIXTURE_SETS["viral_example"]
    out = {name: tmp / f"{name}.sqlite" for name in ("two_runs", "duplicate_stems", "incomplete", "no_runs")}
    for _ in range(2):
        run = rundb.run_sourmash_hip(GOLDEN / "viral_example", out["two_runs"], cache=tmp / "cache", scaled=scaled, engine=OracleEngine(), temp=tmp)
        assert run.status == "Done"
    shutil.copy(out["two_runs"], out["duplicate_stems"])
    with sqlite3.connect(out["duplicate_stems"]) as conn:
        conn.execute("UPDATE runs_genomes SET fasta_filename = 'OP073605.fna' WHERE fasta_filename = 'MGV-GENOME-0264574.fas'")
    conn.close()
    shutil.copy(out["two_runs"], out["incomplete"])
    with sqlite3.connect(out["incomplete"]) as conn:
        conn.execute("DELETE FROM comparisons WHERE comparison_id = (SELECT MAX(comparison_id) FROM comparisons)")
    conn.close()
    rundb.connect_to_db(out["no_runs"]).close()
    return out


@pytest.fixture
def no_matplotlib(monkeypatch):
    monkeypatch.setitem(sys.modules, "matplotlib", None)  # ``import matplotlib`` raises ImportError


# ------------------------------------------------------------------ one failure, one text
@pytest.mark.parametrize("command", COMMANDS)
def test_missing_database(command, tmp_path):
    for database in (tmp_path / "none.sqlite", ":memory:"):
        with pytest.raises(SystemExit) as exit_:
            COMMANDS[command](database, tmp_path)
        assert str(exit_.value) == f"Database {database} does not exist"


@pytest.mark.parametrize("command", COMMANDS)
def test_database_without_runs(command, dbs, tmp_path):
    with pytest.raises(SystemExit) as exit_:
        COMMANDS[command](dbs["no_runs"], tmp_path)
    # plot-run-comp is given its runs by number: it misses the first of them
    wanted = "has no run-id 1." if command == "plot-run-comp" else "contains no runs."
    assert str(exit_.value) == f"Database {dbs['no_runs']} {wanted}"


@pytest.mark.parametrize("command", COMMANDS)
def test_unknown_run_id(command, dbs, tmp_path):
    with pytest.raises(SystemExit) as exit_:
        COMMANDS[command](dbs["two_runs"], tmp_path, run_id=7)
    assert str(exit_.value) == f"Database {dbs['two_runs']} has no run-id 7."
    if command == "plot-run-comp":  # a further run that is not there, too
        with pytest.raises(SystemExit) as exit_:
            rundb.plot_run_comp(dbs["two_runs"], tmp_path, "1,7")
        assert str(exit_.value) == f"Database {dbs['two_runs']} has no run-id 7."


@pytest.mark.parametrize("command", COMMANDS)
def test_implicit_run_id_is_logged_with_what_the_command_does(command, dbs, tmp_path, caplog):
    caplog.set_level(logging.INFO)
    COMMANDS[command](dbs["two_runs"], tmp_path)
    if command == "plot-run-comp":
        assert "run-id" not in caplog.text  # its runs are always named
    else:
        assert ("Plotting run-id 2" if command == "plot-run" else "Exporting run-id 2") in caplog.messages


@pytest.mark.parametrize("command", WITH_RUN)
def test_unknown_label(command, dbs, tmp_path):
    with pytest.raises(SystemExit) as exit_:
        COMMANDS[command](dbs["two_runs"], tmp_path, label="name")
    assert str(exit_.value) == "Unexpected label scheme 'name'"


@pytest.mark.parametrize("command", WITH_RUN)
def test_duplicate_stems(command, dbs, tmp_path):
    with pytest.raises(SystemExit) as exit_:
        COMMANDS[command](dbs["duplicate_stems"], tmp_path)
    assert str(exit_.value) == "Duplicate filename stems, consider using MD5 labelling."
    assert COMMANDS[command](dbs["duplicate_stems"], tmp_path / "md5", label="md5")  # the way out
    assert COMMANDS[command](dbs["duplicate_stems"], tmp_path / "filename", label="filename")


@pytest.mark.parametrize("command", WITH_RUN)
def test_incomplete_run(command, dbs, tmp_path):
    for run_id in (None, 1):
        with pytest.raises(SystemExit) as exit_:
            COMMANDS[command](dbs["incomplete"], tmp_path, run_id=run_id)
        assert str(exit_.value) == f"run-id {run_id or 2} has 8 of 3^2=9 comparisons, 1 needed"


@pytest.mark.parametrize("command", WITH_RUN)
def test_run_without_genomes(command, dbs, tmp_path):
    db = tmp_path / "empty_run.sqlite"
    shutil.copy(dbs["two_runs"], db)
    with sqlite3.connect(db) as conn:
        conn.execute("DELETE FROM runs_genomes WHERE run_id = 2")
    conn.close()
    with pytest.raises(SystemExit) as exit_:
        COMMANDS[command](db, tmp_path)
    assert str(exit_.value) == "Run-id 2 has no genomes"


@pytest.mark.parametrize("command", WITH_FORMATS)
def test_image_format_without_matplotlib(command, dbs, tmp_path, no_matplotlib):
    with pytest.raises(SystemExit, match=NO_MATPLOTLIB) as exit_:
        COMMANDS[command](dbs["two_runs"], tmp_path, formats=("tsv", "png"))
    assert str(exit_.value).startswith("Image formats (png) need")
    with pytest.raises(SystemExit) as exit_:
        COMMANDS[command](dbs["two_runs"], tmp_path, formats=("svg", "tsv", "png"))
    assert str(exit_.value) == "Image formats (svg, png) need matplotlib, which cannot be imported; only tsv is available"
    assert COMMANDS[command](dbs["two_runs"], tmp_path / "tables_only")  # tsv alone needs none


@pytest.mark.parametrize("command", COMMANDS)
def test_missing_output_directory_is_made_with_the_warning(command, dbs, tmp_path, caplog):
    out = tmp_path / "new"
    written = COMMANDS[command](dbs["two_runs"], out)
    assert out.is_dir() and all(Path(p).parent == out for p in ([written] if isinstance(written, Path) else written))
    assert caplog.messages.count(f"Output directory {out} does not exist, making it.") == 1
    caplog.clear()
    COMMANDS[command](dbs["two_runs"], out)
    assert "making it" not in caplog.text
    with pytest.raises(FileNotFoundError):  # ``mkdir`` without parents, as the reference's
        COMMANDS[command](dbs["two_runs"], tmp_path / "a" / "b")


# ------------------------------------------------------------------ two failures at once: the first check wins
def test_order_database_before_the_command_s_own_arguments(tmp_path, no_matplotlib):
    none = tmp_path / "none.sqlite"
    own = {"classify": {"mode": "hadamard"}, "tree-run": {"method": "ml"}, "ordinate-run": {"dimensions": 0, "formats": ("png",)},
           "plot-run": {"formats": ("png",)}, "plot-run-comp": {"formats": ("png",)}, "export-run": {"label": "name"}}  # fmt: skip
    for command, options in own.items():
        with pytest.raises(SystemExit, match=f"Database {none} does not exist"):
            COMMANDS[command](none, tmp_path / "new", **options)
    assert not (tmp_path / "new").exists()


def test_order_classify_arguments_before_the_output_directory(dbs, tmp_path):
    out = tmp_path / "new"
    with pytest.raises(SystemExit, match="Unknown coverage aggregator 'sum'"):
        rundb.classify(dbs["two_runs"], out, coverage_edges="sum", score_edges="median", mode="hadamard")
    with pytest.raises(SystemExit, match="Unknown score aggregator 'median'"):
        rundb.classify(dbs["two_runs"], out, score_edges="median", mode="hadamard")
    with pytest.raises(SystemExit, match="Unknown classify mode 'hadamard'"):
        rundb.classify(dbs["two_runs"], out, mode="hadamard", run_id=7)
    assert not out.exists()


def test_order_tree_arguments_before_the_output_directory(dbs, tmp_path):
    out = tmp_path / "new"
    with pytest.raises(SystemExit, match="Unknown tree method 'ml'"):
        rundb.tree_run(dbs["two_runs"], out, method="ml", missing=-1.0)
    with pytest.raises(SystemExit, match="must be finite and not negative, not -1.0"):
        rundb.tree_run(dbs["two_runs"], out, missing=-1.0, run_id=7)
    assert not out.exists()


def test_order_ordinate_arguments_before_the_output_directory(dbs, tmp_path, no_matplotlib):
    out = tmp_path / "new"
    with pytest.raises(SystemExit, match=NO_MATPLOTLIB):
        rundb.ordinate_run(dbs["two_runs"], out, formats=("png",), dimensions=0, missing=-1.0)
    with pytest.raises(SystemExit, match="Expected 1 to 24 dimensions, not 0"):
        rundb.ordinate_run(dbs["two_runs"], out, dimensions=0, missing=-1.0)
    with pytest.raises(SystemExit, match="must be finite and not negative, not -1.0"):
        rundb.ordinate_run(dbs["two_runs"], out, missing=-1.0, run_id=7)
    assert not out.exists()
    # more axes than genomes is only known once the run is open
    with pytest.raises(SystemExit, match="Unexpected label scheme 'name'"):
        rundb.ordinate_run(dbs["two_runs"], out, dimensions=4, label="name")
    assert out.is_dir()


def test_order_plot_arguments_before_the_output_directory(dbs, tmp_path, no_matplotlib):
    out = tmp_path / "new"
    with pytest.raises(SystemExit, match=NO_MATPLOTLIB):
        rundb.plot_run(dbs["two_runs"], out, formats=("png",), scatter=True, scatter_bins=0)
    with pytest.raises(SystemExit, match="--scatter-bins 0: expected 1 to 1024"):
        rundb.plot_run(dbs["two_runs"], out, scatter=True, scatter_bins=0, run_id=7)
    with pytest.raises(SystemExit, match=NO_MATPLOTLIB):
        rundb.plot_run_comp(dbs["two_runs"], out, "1", formats=("png",))
    assert not out.exists()
    with pytest.raises(SystemExit, match="Expected comma separated list of runs, not: 1,x"):
        rundb.plot_run_comp(dbs["two_runs"], out, "1,x")
    assert out.is_dir()
    with pytest.raises(SystemExit, match="Need at least two runs for a comparison"):
        rundb.plot_run_comp(dbs["no_runs"], out, "7")


@pytest.mark.parametrize("command", WITH_RUN)
def test_order_output_directory_before_the_run(command, dbs, tmp_path):
    for name, options, message in (("no_run", {"run_id": 7}, "has no run-id 7"), ("label", {"label": "name"}, "Unexpected label scheme 'name'")):
        with pytest.raises(SystemExit, match=message):
            COMMANDS[command](dbs["two_runs"], tmp_path / name, **options)
        assert (tmp_path / name).is_dir() and not list((tmp_path / name).iterdir())


@pytest.mark.parametrize("command", WITH_RUN)
def test_order_incomplete_run_and_unknown_label(command, dbs, tmp_path):
    """export-run maps the labels for its long form, which it writes before it counts; the others count first."""
    wanted = "Unexpected label scheme 'name'" if command == "export-run" else r"run-id 2 has 8 of 3\^2=9 comparisons, 1 needed"
    with pytest.raises(SystemExit, match=wanted):
        COMMANDS[command](dbs["incomplete"], tmp_path, label="name")
    assert not list(tmp_path.iterdir())


@pytest.mark.parametrize("command", WITH_RUN)
def test_order_incomplete_run_before_duplicate_stems(command, dbs, tmp_path):
    db = tmp_path / "both.sqlite"
    shutil.copy(dbs["duplicate_stems"], db)
    with sqlite3.connect(db) as conn:
        conn.execute("DELETE FROM comparisons WHERE comparison_id = (SELECT MAX(comparison_id) FROM comparisons)")
    conn.close()
    with pytest.raises(SystemExit, match=r"run-id 2 has 8 of 3\^2=9 comparisons, 1 needed"):
        COMMANDS[command](db, tmp_path / "out")


def test_order_export_run_writes_the_long_form_of_an_incomplete_run(dbs, tmp_path, caplog):
    caplog.set_level(logging.INFO)
    with pytest.raises(SystemExit, match=r"run-id 2 has 8 of 3\^2=9 comparisons, 1 needed"):
        rundb.export_run(dbs["incomplete"], tmp_path / "out")
    assert [p.name for p in (tmp_path / "out").iterdir()] == ["sourmash-hip_run_2.tsv"]
    lines = (tmp_path / "out" / "sourmash-hip_run_2.tsv").read_text().split("\n")
    assert lines[0] == "#Query\tSubject\tIdentity\tQuery-Cov\tSubject-Cov\tHadamard\ttANI\tAlign-Len\tSim-Errors" and lines[-1] == ""
    stems = {rundb.filename_stem(f) for f in FIXTURE_SETS["viral_example"][1].values()}
    assert len(lines) == 10 and all(set(line.split("\t")[:2]) <= stems and len(line.split("\t")) == 9 for line in lines[1:-1])
    assert f"Wrote long-form to {tmp_path / 'out' / 'sourmash-hip_run_2.tsv'}" in caplog.messages
    complete = rundb.export_run(dbs["two_runs"], tmp_path / "complete")
    assert (tmp_path / "complete" / "sourmash-hip_run_2.tsv").read_text().split("\n")[:9] == lines[:9]
    assert len(complete) == 7


# ------------------------------------------------------------------ the command line
@pytest.mark.parametrize("subcommand", SUBCOMMANDS)
def test_help_is_the_recorded_text(subcommand, monkeypatch, capsys):
    monkeypatch.setenv("COLUMNS", "100")
    with pytest.raises(SystemExit) as exit_:
        rundb.main([subcommand, "--help"])
    assert exit_.value.code == 0
    assert capsys.readouterr().out == (HELP / f"{subcommand}.txt").read_text()


def test_every_subcommand_has_its_recorded_help():
    assert sorted(p.stem for p in HELP.glob("*.txt")) == sorted(SUBCOMMANDS)


def test_report_commands_print_one_path_a_line(dbs, tmp_path, capsys):
    for subcommand, files in (("export-run", 7), ("classify", 1), ("tree-run", 1), ("ordinate-run", 2), ("plot-run", 6)):
        assert rundb.main([subcommand, "-d", str(dbs["two_runs"]), "-o", str(tmp_path / subcommand)]) == 0
        printed = capsys.readouterr().out.split("\n")
        assert printed[-1] == "" and sorted(printed[:-1]) == sorted(str(p) for p in (tmp_path / subcommand).iterdir()) and len(printed) == files + 1
    assert rundb.main(["plot-run-comp", "-d", str(dbs["two_runs"]), "-o", str(tmp_path / "comp"), "--run-ids", "1,2", "--formats", "tsv,"]) == 0
    assert capsys.readouterr().out == f"{tmp_path / 'comp' / 'sourmash-hip_identity_1_vs_2.tsv'}\n"


# ------------------------------------------------------------------ imports one way only: rundb -> reports -> run_store
@pytest.mark.parametrize(("module", "absent"), [("reports", ("rundb",)), ("run_store", ("rundb", "reports"))])
def test_imports_go_one_way(module, absent):
    code = f"import sys, pyani_plus_amd.{module}; print([m for m in {absent!r} if 'pyani_plus_amd.' + m in sys.modules])"
    done = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, cwd=Path(__file__).parent.parent, check=False)
    assert done.returncode == 0, done.stderr
    assert done.stdout.strip() == "[]"


def test_rundb_has_no_module_getattr():
    assert "__getattr__" not in vars(rundb)
