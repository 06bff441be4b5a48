"""``search-run`` on the host path (the oracle-backed engine, the host twin for the selection): sourmash-hip runs of the
viral and the bacterial fixture sets searched with their own FASTA directories, a foreign genome, a query that shares
no hash, ``--top`` above N, both ranks, the thresholds, an incomplete run, a run of another method, the order of the
opening checks, ``--help`` and what ``main`` prints.  The expected rows are derived here from the signature cache and
the database with the restatement of tests/search_cases.py; every value is compared by its ``repr``."""

from __future__ import annotations

import logging
import shutil
import sqlite3
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

import oracle
from pyani_plus_amd import rundb, search
from tests import search_cases as sc
from tests.fake_engine import OracleEngine
from tests.helpers import FIXTURE_SETS, GOLDEN, read_fasta_bytes, sig_mins
from tests.msa_checker import NumpyMsaEngine

HELP = GOLDEN / "search" / "help.txt"
HITS, QUERIES = "sourmash-hip_search_hits.tsv", "sourmash-hip_search_queries.tsv"
K = 31
SETS = ("viral_example", "bacterial_example")


def stem(name: str) -> str:
    return rundb.filename_stem(name)


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    """set name -> ``(database, cache)`` of a complete sourmash-hip run of the fixture set."""
    tmp = tmp_path_factory.mktemp("search_command")
    made = {}
    for name in SETS:
        scaled, _genomes = FIXTURE_SETS[name]
        made[name] = (tmp / f"{name}.sqlite", tmp / f"{name}_cache")
        run = rundb.run_sourmash_hip(GOLDEN / name, made[name][0], cache=made[name][1], scaled=scaled, engine=OracleEngine(), temp=tmp / f"{name}_t")
        assert run.status == "Done"
    return made


def subjects_of(name: str, cache: Path, label: str = "stem"):
    """``(labels, sketches)`` of the run's genomes in the order of their md5: the subject index of the contract."""
    scaled, genomes = FIXTURE_SETS[name]
    hashes = sorted(genomes)
    shown = {"stem": lambda h: stem(genomes[h]), "filename": lambda h: genomes[h], "md5": lambda h: h}[label]
    return [shown(h) for h in hashes], [sig_mins(cache / f"sourmash_k={K}_scaled={scaled}" / f"{h}.sig") for h in hashes]


def expected_rows(query_sketches, subject_sketches, rank: str, top: int) -> list[list[tuple[int, int, int]]]:
    """Per query its hits ``(subject, I, m)`` in the restatement's order, at most ``top``."""
    sizes = [len(s) for s in subject_sketches]
    return [sc.ranked([oracle.intersect(q, s) for s in subject_sketches], len(q), sizes, rank)[:top] for q in query_sketches]


def table(path: Path) -> list[list[str]]:
    lines = path.read_text().split("\n")
    assert lines[-1] == "" and lines[0].startswith("#")
    return [line.split("\t") for line in lines[1:-1]]


def database_values(db: Path) -> dict:
    """(query stem, subject stem) -> (repr(identity), repr(cov_query)) as the database holds them."""
    with sqlite3.connect(db) as conn:
        name = dict(conn.execute("SELECT genome_hash, fasta_filename FROM runs_genomes WHERE run_id = 1"))
        rows = conn.execute("SELECT query_hash, subject_hash, identity, cov_query FROM comparisons").fetchall()
    conn.close()
    return {(stem(name[q]), stem(name[s])): (repr(i), repr(c)) for q, s, i, c in rows}


@pytest.mark.parametrize("rank", sc.RANKS)
@pytest.mark.parametrize("name", SETS)
def test_a_run_searched_with_its_own_genomes(runs, tmp_path, name, rank):
    db, cache = runs[name]
    before = db.read_bytes()
    written = rundb.search_run(GOLDEN / name, db, tmp_path / "out", cache=cache, rank=rank, engine=OracleEngine())
    assert [p.name for p in written] == [HITS, QUERIES] and db.read_bytes() == before  # nothing is written to the database
    labels, sketches = subjects_of(name, cache)
    _scaled, genomes = FIXTURE_SETS[name]
    by_file = sorted(genomes, key=lambda h: genomes[h])  # the queries are taken in file-name order
    queries = [sketches[sorted(genomes).index(h)] for h in by_file]
    want = expected_rows(queries, sketches, rank, 5)
    stored = database_values(db)
    hits = table(written[0])
    assert len(hits) == sum(len(w) for w in want)
    at = 0
    for q, h in enumerate(by_file):
        for r, (s, shared, _m) in enumerate(want[q]):
            row = hits[at]
            at += 1
            assert row[:3] == [stem(genomes[h]), labels[s], str(r + 1)]  # the order of the rows is the restatement's
            assert (row[3], row[4]) == stored[(row[0], row[1])]  # the values are the database's, by repr
            assert row[5:] == [str(shared), str(len(queries[q])), str(len(sketches[s]))]
        mine = [row for row in hits if row[0] == stem(genomes[h])]
        assert mine[0][1] == stem(genomes[h]) and mine[0][3] == "1.0"  # rank 1 of every query is itself
    lengths = {h: sum(len(line) for line in read_fasta_bytes(GOLDEN / name / genomes[h]).split(b"\n") if not line.startswith(b">")) for h in by_file}
    assert table(written[1]) == [[stem(genomes[h]), h, str(lengths[h]), str(len(queries[q])), stem(genomes[h]), "1.0", "1.0", str(len(want[q]))]
                                 for q, h in enumerate(by_file)]  # fmt: skip


def test_the_ranks_differ_where_the_contract_says(runs, tmp_path):
    """MGV-GENOME-0266457 shares 104 hashes with both others: under identity the smaller subject comes first (the
    larger of the two containments), under containment they tie on I / |Q| and on I, and the lower index wins."""
    db, cache = runs["viral_example"]
    second = {}
    for rank in sc.RANKS:
        hits = table(rundb.search_run(GOLDEN / "viral_example", db, tmp_path / rank, cache=cache, rank=rank, engine=OracleEngine())[0])
        second[rank] = [row[1] for row in hits if row[0] == "MGV-GENOME-0266457"][1]
    labels, _sketches = subjects_of("viral_example", cache)
    assert second == {"identity": "MGV-GENOME-0264574", "containment": "OP073605"} and labels.index("OP073605") < labels.index("MGV-GENOME-0264574")


def write_genome(path: Path, *parts: bytes) -> None:
    path.write_bytes(b">" + path.stem.encode() + b"\n" + b"".join(parts) + b"\n")


def random_bases(seed: int, n: int) -> bytes:
    return bytes(np.frombuffer(b"ACGT", dtype=np.uint8)[np.random.default_rng(seed).integers(0, 4, n)])


def test_a_foreign_genome_and_a_query_without_a_hit(runs, tmp_path):
    db, cache = runs["viral_example"]
    queries = tmp_path / "queries"
    queries.mkdir()
    shutil.copy(GOLDEN / "MIBY01000005.fasta", queries / "MIBY01000005.fasta")
    write_genome(queries / "noise.fna", random_bases(1, 20000))
    shutil.copy(GOLDEN / "viral_example" / "OP073605.fasta", queries / "a_copy.fasta")
    written = rundb.search_run(queries, db, tmp_path / "out", cache=cache, engine=OracleEngine(), top=2)
    labels, sketches = subjects_of("viral_example", cache)
    names = ["MIBY01000005.fasta", "a_copy.fasta", "noise.fna"]  # file-name order
    mine = [oracle.sketch_fasta_text(read_fasta_bytes(queries / n), K, 300)[0] for n in names]
    want = expected_rows(mine, sketches, "identity", 2)
    assert want[2] == [] and len(want[1]) == 2  # noqa: PLR2004
    hits = table(written[0])
    assert [row[:3] for row in hits] == [[stem(n), labels[s], str(r + 1)] for n, w in zip(names, want) for r, (s, _i, _m) in enumerate(w)]
    rows = table(written[1])
    assert [row[0] for row in rows] == [stem(n) for n in names]
    assert rows[2][3:] == [str(len(mine[2])), "NA", "NA", "NA", "0"] and rows[2][2] == "20000"
    assert rows[1][4:] == ["OP073605", "1.0", "1.0", "2"]
    if not want[0]:
        assert rows[0][4:] == ["NA", "NA", "NA", "0"]


def test_top_above_the_number_of_genomes(runs, tmp_path):
    db, cache = runs["bacterial_example"]
    written = rundb.search_run(GOLDEN / "bacterial_example", db, tmp_path, cache=cache, top=64, engine=OracleEngine())
    _labels, sketches = subjects_of("bacterial_example", cache)
    want = expected_rows(sketches, sketches, "identity", 64)
    assert len(table(written[0])) == sum(len(w) for w in want) <= 16  # noqa: PLR2004
    assert sorted(int(row[7]) for row in table(written[1])) == sorted(len(w) for w in want)


@pytest.fixture(scope="module")
def nested(tmp_path_factory):
    """A run of two genomes and a query for which the ranks disagree with the thresholds: ``small`` is the first third
    of the query (identity 1.0, a third of the query covered), ``large`` holds two thirds of it among other sequence."""
    tmp = tmp_path_factory.mktemp("search_nested")
    q = random_bases(2, 60000)
    (tmp / "genomes").mkdir()
    (tmp / "queries").mkdir()
    write_genome(tmp / "genomes" / "small.fasta", q[:20000])
    write_genome(tmp / "genomes" / "large.fasta", q[20000:], random_bases(3, 200000))
    write_genome(tmp / "queries" / "query.fasta", q)
    db = tmp / "runs.sqlite"
    assert rundb.run_sourmash_hip(tmp / "genomes", db, cache=tmp / "cache", scaled=300, engine=OracleEngine(), temp=tmp / "t").status == "Done"
    return db, tmp / "cache", tmp / "queries"


def test_the_thresholds_filter_the_top_hits(nested, tmp_path):
    db, cache, queries = nested
    options = {"cache": cache, "rank": "containment", "engine": OracleEngine()}
    everything = table(rundb.search_run(queries, db, tmp_path / "all", **options)[0])
    assert [row[:3] for row in everything] == [["query", "large", "1"], ["query", "small", "2"]]
    assert float(everything[0][3]) < 0.99 < float(everything[1][3]) == 1.0 and float(everything[0][4]) > float(everything[1][4])  # noqa: PLR2004
    written = rundb.search_run(queries, db, tmp_path / "some", min_identity=0.99, **options)
    assert table(written[0]) == [everything[1]] and everything[1][2] == "2"  # rank 1 is filtered out, rank 2 keeps its rank
    assert table(written[1])[0][4:] == ["large", everything[0][3], everything[0][4], "1"]  # best_* is rank 1 whatever the thresholds say
    written = rundb.search_run(queries, db, tmp_path / "cov", cov_min=float(everything[0][4]), **options)
    assert table(written[0]) == [everything[0]]  # a value at the threshold passes
    written = rundb.search_run(queries, db, tmp_path / "none", min_identity=1.0, cov_min=0.99, **options)
    assert table(written[0]) == [] and table(written[1])[0][4:] == ["large", everything[0][3], everything[0][4], "0"]
    written = rundb.search_run(queries, db, tmp_path / "top1", top=1, min_identity=0.99, **options)
    assert table(written[0]) == []  # the thresholds do not look further down the ranking
    identity = table(rundb.search_run(queries, db, tmp_path / "identity", cache=cache, engine=OracleEngine())[0])
    assert [row[1] for row in identity] == ["small", "large"]


def test_the_tables_of_a_hand_made_result():
    hits = search.Hits(np.array([[1, 0, -1]]), np.array([[5, 4, 0]], dtype=np.uint32), np.array([[0.5, 0.75, np.nan]]), np.array([[0.5, 0.25, np.nan]]),
                       np.array([10], dtype=np.uint64), np.array([8, 9], dtype=np.uint64))  # fmt: skip
    assert search.hits_tsv(hits, ["q"], ["a", "b"], min_identity=0.6) == search.HITS_HEADER + "\nq\ta\t2\t0.75\t0.25\t4\t10\t8\n"
    assert search.queries_tsv(hits, ["q"], ["md5"], [123], ["a", "b"], min_identity=0.6) == search.QUERIES_HEADER + "\nq\tmd5\t123\t10\tb\t0.5\t0.5\t1\n"


def test_an_incomplete_run_is_accepted(runs, tmp_path):
    db, cache = runs["viral_example"]
    partial = tmp_path / "partial.sqlite"
    shutil.copy(db, partial)
    with sqlite3.connect(partial) as conn:
        conn.execute("DELETE FROM comparisons WHERE comparison_id > 2")
        conn.execute("UPDATE runs SET status = 'Worker interrupted'")
    conn.close()
    written = rundb.search_run(GOLDEN / "viral_example", partial, tmp_path / "out", cache=cache, engine=OracleEngine())
    whole = rundb.search_run(GOLDEN / "viral_example", db, tmp_path / "whole", cache=cache, engine=OracleEngine())
    assert [p.read_bytes() for p in written] == [p.read_bytes() for p in whole]


def test_without_a_cache_the_subjects_are_sketched_again(runs, tmp_path):
    db, cache = runs["viral_example"]
    written = rundb.search_run(GOLDEN / "viral_example", db, tmp_path / "out", temp=tmp_path / "t", engine=OracleEngine(), label="md5")
    cached = rundb.search_run(GOLDEN / "viral_example", db, tmp_path / "cached", cache=cache, engine=OracleEngine(), label="md5")
    assert [p.read_bytes() for p in written] == [p.read_bytes() for p in cached]
    assert len(list((tmp_path / "t").glob("pyani_hip_cache_*/sourmash_k=31_scaled=300/*.sig"))) == 3  # noqa: PLR2004
    labels, _sketches = subjects_of("viral_example", cache, "md5")
    assert {row[1] for row in table(written[0])} == set(labels) and {row[0] for row in table(written[0])} == {"MGV-GENOME-0264574", "MGV-GENOME-0266457", "OP073605"}


def msa_run(tmp: Path) -> Path:
    rows = [random_bases(seed, 40) for seed in (4, 5, 6)]
    (tmp / "genomes").mkdir()
    for i, row in enumerate(rows):
        (tmp / "genomes" / f"g{i}.fasta").write_bytes(b">g%d\n" % i + row + b"\n")
    aln = tmp / "rows.aln.fasta"
    aln.write_bytes(b"".join(b">g%d\n" % i + row + b"\n" for i, row in enumerate(rows)))
    db = tmp / "msa.sqlite"
    assert rundb.run_external_alignment_hip(tmp / "genomes", db, alignment=aln, temp=tmp / "t", engine=NumpyMsaEngine()).status == "Done"
    return db


def test_a_run_of_another_method_is_refused(tmp_path):
    db = msa_run(tmp_path)
    with pytest.raises(SystemExit) as exit_:
        rundb.search_run(GOLDEN / "viral_example", db, tmp_path / "out", engine=OracleEngine())
    assert str(exit_.value) == "Run-id 1 is a external-alignment-hip run: search-run needs the sketches of a sourmash-hip run"
    assert not list((tmp_path / "out").iterdir())


def test_the_order_of_the_opening_checks(runs, tmp_path):
    db, _cache = runs["viral_example"]
    none, out, queries = tmp_path / "none.sqlite", tmp_path / "new", GOLDEN / "viral_example"
    with pytest.raises(SystemExit, match=f"Database {none} does not exist"):
        rundb.search_run(tmp_path / "nowhere", none, out, top=0)
    empty = tmp_path / "empty"
    empty.mkdir()
    for arguments, options, message in (
        ((tmp_path / "nowhere",), {"top": 0, "rank": "best"}, "Expected 1 to 64 hits a query, not 0"),
        ((tmp_path / "nowhere",), {"top": 65}, "Expected 1 to 64 hits a query, not 65"),
        ((tmp_path / "nowhere",), {"top": 2.0}, "Expected 1 to 64 hits a query, not 2.0"),
        ((tmp_path / "nowhere",), {"rank": "best", "min_identity": 2.0}, "Unknown rank 'best': expected one of identity, containment"),
        ((tmp_path / "nowhere",), {"min_identity": 1.5, "cov_min": -1.0}, "The minimum identity must be a number from 0 to 1, not 1.5"),
        ((tmp_path / "nowhere",), {"min_identity": float("nan")}, "The minimum identity must be a number from 0 to 1, not nan"),
        ((tmp_path / "nowhere",), {"cov_min": float("inf")}, "The minimum query coverage must be a number from 0 to 1, not inf"),
        ((tmp_path / "nowhere",), {"run_id": 7}, f"FASTA input {tmp_path / 'nowhere'} is not a directory"),
        ((empty,), {"run_id": 7}, f"No FASTA input genomes under {empty} with extensions .fa, .fas, .fasta, .fna"),
    ):
        with pytest.raises(SystemExit) as exit_:
            rundb.search_run(*arguments, db, out, **options)
        assert str(exit_.value) == message
        assert not out.exists()
    with pytest.raises(SystemExit) as exit_:
        rundb.search_run(queries, db, out, run_id=7, label="name")
    assert str(exit_.value) == f"Database {db} has no run-id 7."
    assert out.is_dir()  # the output directory before the run
    with pytest.raises(SystemExit) as exit_:
        rundb.search_run(queries, db, out, label="name")
    assert str(exit_.value) == "Unexpected label scheme 'name'"
    twice = tmp_path / "twice.sqlite"
    shutil.copy(db, twice)
    with sqlite3.connect(twice) as conn:
        conn.execute("UPDATE runs_genomes SET fasta_filename = 'OP073605.fna' WHERE fasta_filename = 'MGV-GENOME-0264574.fas'")
    conn.close()
    with pytest.raises(SystemExit) as exit_:
        rundb.search_run(queries, twice, out)
    assert str(exit_.value) == "Duplicate filename stems, consider using MD5 labelling."
    assert not list(out.iterdir())
    with sqlite3.connect(twice) as conn:
        conn.execute("DELETE FROM runs_genomes")
    conn.close()
    with pytest.raises(SystemExit) as exit_:
        rundb.search_run(queries, twice, out, label="name")
    assert str(exit_.value) == "Run-id 1 has no genomes"  # the genomes before the labels


def test_main_prints_one_path_per_line(runs, tmp_path, capsys):
    db, cache = runs["viral_example"]
    out = tmp_path / "out"
    arguments = ["search-run", str(GOLDEN / "viral_example"), "-d", str(db), "-o", str(out), "--cache", str(cache), "--engine-factory", "tests.fake_engine:OracleEngine"]
    assert rundb.main([*arguments, "--top", "2", "--rank", "containment", "--min-identity", "0.999", "--label", "filename"]) == 0
    assert capsys.readouterr().out.split("\n") == [str(out / HITS), str(out / QUERIES), ""]
    direct = rundb.search_run(GOLDEN / "viral_example", db, tmp_path / "direct", cache=cache, top=2, rank="containment", min_identity=0.999, label="filename",
                              engine=OracleEngine())  # fmt: skip
    assert [(out / p.name).read_bytes() for p in direct] == [p.read_bytes() for p in direct]
    assert rundb.main([*arguments[:5], str(tmp_path / "cli"), *arguments[6:]]) == 0  # the defaults are the function's
    capsys.readouterr()
    direct = rundb.search_run(GOLDEN / "viral_example", db, tmp_path / "defaults", cache=cache, engine=OracleEngine())
    assert [(tmp_path / "cli" / p.name).read_bytes() for p in direct] == [p.read_bytes() for p in direct]


def test_help_is_the_recorded_text(monkeypatch, capsys):
    monkeypatch.setenv("COLUMNS", "100")
    with pytest.raises(SystemExit) as exit_:
        rundb.main(["search-run", "--help"])
    assert exit_.value.code == 0
    text = capsys.readouterr().out
    assert text == HELP.read_text() and "does not look further down the ranking" in " ".join(text.split())


def test_search_imports_neither_rundb_nor_reports():
    code = "import sys, pyani_plus_amd.search; print([m for m in ('rundb', 'reports') if 'pyani_plus_amd.' + m in sys.modules])"
    done = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, cwd=Path(__file__).parent.parent, check=False)
    assert done.returncode == 0, done.stderr
    assert done.stdout.strip() == "[]"


def test_the_engine_of_the_tests_has_no_device_selection():
    assert not hasattr(OracleEngine(), "best_hits_device")  # search.search takes the host twin for it
    logging.getLogger("test").debug("the oracle-backed engine selects with pa_best_hits_host")
