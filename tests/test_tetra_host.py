"""TETRA-hip without a GPU: the host twins against the independent restatement of tests/tetra_cases.py (counts exactly;
Z, U and r bit for bit), r against numpy.corrcoef, the hand cases, and ``rundb.run_tetra_hip(engine=None)`` through
resume, export-run, plot-run, classify and the command line."""

from __future__ import annotations

import logging
import math
import shutil
import sqlite3

import numpy as np
import pytest

from pyani_plus_amd import rundb
from pyani_plus_amd.engine import pack_genomes, tetra_correlations_host, tetra_counts_host, tetra_zscores
from pyani_plus_amd.methods import tetra_hip
from tests import tetra_cases as tc
from tests.helpers import FIXTURE_SETS, GOLDEN

VIRAL = GOLDEN / "viral_example"


def _genomes():
    """Genomes of different composition, two of them degenerate (ACGT alone: every Z is 0; one base: no window), as FASTA
    texts.  A homopolymer is not degenerate under the contract: its AAAA and TTTT have a non-zero Z."""
    rng = np.random.default_rng(1969)
    texts = [tc.fasta(tc.random_bases(rng, 4000)), tc.fasta(tc.random_bases(rng, 2500, (0.4, 0.1, 0.1, 0.4)), tc.random_bases(rng, 900)),
             tc.fasta(b"ACGT"), tc.fasta(tc.markov_bases(rng, 3000, 0.3)), tc.fasta(b"A"), tc.fasta(tc.markov_bases(rng, 3000, 0.6))]  # fmt: skip
    seq = bytearray(tc.random_bases(rng, 5000, (0.2, 0.3, 0.3, 0.2)))
    seq[1000:1010] = b"NNNNNRYKMN"
    return texts + [tc.fasta(bytes(seq))]


@pytest.fixture(scope="module")
def genomes():
    texts = _genomes()
    counts = tetra_counts_host(pack_genomes(texts, fasta=True))
    z, u = tetra_zscores(counts)
    return texts, counts, z, u


@pytest.mark.parametrize("name", sorted(tc.count_cases()))
def test_host_counts_equal_the_oracle(name):
    arena, want = tc.case_arena(name)
    got = tetra_counts_host(arena, threads=3)
    assert got.shape == want.shape
    assert np.array_equal(got, want), f"{name}: genomes {np.flatnonzero((got != want).any(axis=1))[:8]} differ"


def test_kernel_constants_are_read():
    k = tc.kernel_constants()
    assert k["kThreads"] == 256 and k["kTile"] == 64 and tc.chunk_bases() % 64 == 0


def test_zscores_unit_rows_and_r_bit_for_bit(genomes):
    texts, counts, z, u = genomes
    assert np.array_equal(counts, np.stack([tc.forward_counts(t) for t in texts]))
    want_z = [tc.zscores(f) for f in counts]
    want_u = [tc.unit_row(row) for row in want_z]
    tc.same_bits(z, np.array(want_z))
    tc.same_bits(u, np.array(want_u))
    n = len(texts)
    tc.same_bits(tetra_correlations_host(u), tc.correlation_matrix(want_u))
    tc.same_bits(tetra_correlations_host(u, (1, n), (0, 3)), tc.correlation_matrix(want_u, (1, n), (0, 3)))
    tc.same_bits(tetra_correlations_host(u, (2, 3), (2, 3), threads=1), tc.correlation_matrix(want_u, (2, 3), (2, 3)))


@pytest.mark.parametrize("n", (7, 8, 9, 17))
def test_r_around_the_eight_pairs_side_by_side(n):
    """A row's pairs run eight at a time: the whole matrix (row i from the diagonal on: n - i pairs), a rectangle of
    three subjects, and a square range off zero against the same cells of the whole matrix; row 1 is all NaN."""
    unit = tc.unit_rows(n)
    assert np.isnan(unit[1]).all() and not np.isnan(np.delete(unit, 1, axis=0)).any()
    rows = unit.tolist()
    whole = tetra_correlations_host(unit)
    tc.same_bits(whole, tc.correlation_matrix(rows))
    tc.same_bits(tetra_correlations_host(unit, threads=1), whole)
    tc.same_bits(tetra_correlations_host(unit, (1, n), (0, 3)), tc.correlation_matrix(rows, (1, n), (0, 3)))
    tc.same_bits(tetra_correlations_host(unit, (2, n), (2, n)), whole[2:, 2:])
    tc.same_bits(tetra_correlations_host(unit, (2, n), (2, n)), tc.correlation_matrix(rows, (2, n), (2, n)))


def test_r_is_numpy_corrcoef(genomes):
    """Each computation's error on unit vectors is bounded by about 256 * 2^-53 = 3e-14; the bound asked is 1e-12."""
    _texts, _counts, z, u = genomes
    ok = ~np.isnan(u).any(axis=1)
    assert ok.sum() == 5
    r = tetra_correlations_host(u)
    ref = np.corrcoef(z[ok])
    assert np.abs(r[np.ix_(ok, ok)] - ref).max() <= 1e-12
    assert (np.diag(r)[ok] == 1.0).all()
    tc.same_bits(r, r.T)
    assert np.isnan(r[~ok]).all() and np.isnan(r[:, ~ok]).all()


def test_acgt_by_hand():
    """ACGT alone: one forward window of each length from each start, C_4[ACGT] = 2 (it is its own reverse complement),
    and every Z-score 0 -- N = E = 2, V = 0 -- so the genome is degenerate."""
    counts = tetra_counts_host(pack_genomes([b">x\nACGT\n"], fasta=True))[0]
    want = np.zeros(tc.BINS, dtype=np.uint64)
    want[0b00011011] = 1
    want[tc.OFF3 + 0b000110] = want[tc.OFF3 + 0b011011] = 1
    want[tc.OFF2 + 0b0001] = want[tc.OFF2 + 0b0110] = want[tc.OFF2 + 0b1011] = 1
    assert np.array_equal(counts, want)
    c4, c3, c2 = tc.both_strands(counts)
    assert c4[0b00011011] == 2 and sum(c4) == 2 and sum(c3) == 4 and sum(c2) == 6
    z, u = tetra_zscores(counts[None, :])
    assert (z == 0.0).all() and np.isnan(u).all()


def test_degenerate_genomes_are_nan(genomes):
    _texts, _counts, z, u = genomes
    _zh, uh = tetra_zscores(tetra_counts_host(pack_genomes([tc.fasta(b"A" * 500)], fasta=True)))
    assert not np.isnan(uh).any()  # a homopolymer has two non-zero Z-scores
    assert np.isnan(u[2]).all() and np.isnan(u[4]).all()  # ACGT alone and the single base
    assert not np.isnan(u[[0, 1, 3, 5, 6]]).any() and not np.isnan(z).any()
    r = tetra_correlations_host(u)
    assert np.isnan(r[2]).all() and np.isnan(r[:, 4]).all() and math.isnan(r[2, 2])


def test_clamp_of_hand_made_rows():
    """acc beyond [-1, 1] is cut to the bound, inside it is kept, NaN stays, the same index is 1.0 whatever acc is."""
    u = np.zeros((5, tc.WORDS))
    u[0, :2] = 1.0
    u[1, :2] = (1.0, 0.5)  # 0 x 1: acc = 1.5
    u[2, :2] = (-1.0, -0.5)  # 0 x 2: acc = -1.5
    u[3, 0] = 0.25  # 0 x 3: acc = 0.25
    u[4, 7] = math.nan
    r = tetra_correlations_host(u)
    assert r[0, 1] == 1.0 and r[0, 2] == -1.0 and r[0, 3] == 0.25 and r[3, 3] == 1.0 and r[1, 2] == -1.0
    assert np.isnan(r[4]).all() and np.isnan(r[:, 4]).all()
    tc.same_bits(r, r.T)


def test_a_genome_and_its_reverse_complement():
    """Both strands are counted, so a genome and its reverse complement have the same C_k, the same Z and the same unit
    row bit for bit, and their r is min(1, sum of U_k^2)."""
    seq = tc.random_bases(np.random.default_rng(2004), 10_000)
    counts = tetra_counts_host(pack_genomes([tc.fasta(seq), tc.fasta(tc.reverse_complement(seq))], fasta=True))
    assert not np.array_equal(counts[0], counts[1])
    z, u = tetra_zscores(counts)
    tc.same_bits(z[0], z[1])
    tc.same_bits(u[0], u[1])
    r = tetra_correlations_host(u)
    print("r(genome, reverse complement) =", repr(float(r[0, 1])))
    assert r[0, 1] == 1.0 and r[1, 0] == 1.0


# ---------------------------------------------------------------- the run driver on the host
def _rows(database):
    conn = sqlite3.connect(database)
    rows = conn.execute("SELECT query_hash, subject_hash, identity, cov_query, aln_length, sim_errors, cov_subject FROM comparisons ORDER BY 1, 2").fetchall()
    conn.close()
    return rows


@pytest.fixture(scope="module")
def viral_run(tmp_path_factory):
    work = tmp_path_factory.mktemp("tetra_viral")
    database = work / "run.db"
    run = rundb.run_tetra_hip(VIRAL, database, cache=work / "cache", temp=work / "tmp", engine=None)
    return work, database, run


def test_run_on_the_host(viral_run):
    work, database, run = viral_run
    hashes = sorted(FIXTURE_SETS["viral_example"][1])
    assert run.status == "Done" and run.name == "3 genomes using TETRA-hip"
    config = run.configuration
    assert (config.method, config.program) == ("TETRA-hip", "libpyani_hip")
    assert (config.fragsize, config.mode, config.kmersize, config.minmatch, config.extra) == (None,) * 5
    rows = _rows(database)
    assert [(q, s) for q, s, *_ in rows] == [(q, s) for q in hashes for s in hashes]
    from tests.helpers import read_fasta_bytes

    unit = [tc.unit_row(tc.zscores(tc.forward_counts(read_fasta_bytes(VIRAL / FIXTURE_SETS["viral_example"][1][h])))) for h in hashes]
    want = tc.correlation_matrix(unit)
    tc.same_bits(np.array([r[2] for r in rows]).reshape(3, 3), want)
    assert all(r[3:] == (None, None, None, None) for r in rows)
    assert all(want[i, i] == 1.0 for i in range(3)) and (np.abs(want) <= 1.0).all()
    for h in hashes:  # the count files: 336 forward counts each
        assert np.array_equal(tetra_hip.read_counts(logging.getLogger("test"), work / "cache", h),
                              tc.forward_counts(read_fasta_bytes(VIRAL / FIXTURE_SETS["viral_example"][1][h])))  # fmt: skip


def test_resume_after_deleting_rows(viral_run, tmp_path):
    work, database, _run = viral_run
    copy = tmp_path / "copy.db"
    shutil.copy(database, copy)
    before = _rows(copy)
    victim = sorted(FIXTURE_SETS["viral_example"][1])[1]
    conn = sqlite3.connect(copy)
    conn.execute("DELETE FROM comparisons WHERE subject_hash = ? AND query_hash != ?", (victim, victim))
    conn.execute("UPDATE runs SET status = 'Worker interrupted'")
    conn.commit()
    conn.close()
    assert len(_rows(copy)) == 7
    stamp = {p: p.stat().st_mtime_ns for p in (work / "cache" / "tetra_hip").iterdir()}
    run = rundb.resume(copy, cache=work / "cache", temp=tmp_path / "tmp")
    assert run.status == "Done"
    assert _rows(copy) == before
    assert {p: p.stat().st_mtime_ns for p in (work / "cache" / "tetra_hip").iterdir()} == stamp  # count files are not rewritten
    with pytest.raises(SystemExit, match="not supported"):
        rundb.resume(copy, cache=work / "cache", temp=tmp_path / "tmp2", gpus=2)  # complete, but the method is asked first


def test_more_than_one_gpu_is_refused(tmp_path):
    with pytest.raises(SystemExit, match="TETRA-hip runs on the host or on one GPU; --gpus 2 is not supported"):
        rundb.run_tetra_hip(VIRAL, tmp_path / "x.db", gpus=2)
    assert not (tmp_path / "x.db").exists()


def test_export_run_prints_na_for_coverage(viral_run, tmp_path):
    _work, database, _run = viral_run
    written = rundb.export_run(database, tmp_path / "out")
    assert written[0].name == "TETRA-hip_run_1.tsv"
    lines = written[0].read_text().splitlines()
    assert lines[0] == "#Query\tSubject\tIdentity\tQuery-Cov\tSubject-Cov\tHadamard\ttANI\tAlign-Len\tSim-Errors"
    assert len(lines) == 10
    for line in lines[1:]:
        fields = line.split("\t")
        assert fields[3:] == ["NA"] * 6 and -1.0 <= float(fields[2]) <= 1.0
    by_name = {p.name: p.read_text().splitlines() for p in written}
    for kind in ("query_cov", "hadamard", "tANI"):  # the matrices: labels and empty cells
        assert all(line.split("\t")[1:] == [""] * 3 for line in by_name[f"TETRA-hip_{kind}.tsv"][1:])


def test_plot_run_writes_identity_and_warns_for_the_rest(viral_run, tmp_path, caplog):
    _work, database, _run = viral_run
    with caplog.at_level(logging.WARNING, logger="pyani_plus_amd"):
        written = rundb.plot_run(database, tmp_path / "plots", formats=("tsv",))
    assert [p.name for p in written] == ["TETRA-hip_identity_heatmap.tsv"]
    assert len(written[0].read_text().splitlines()) == 4
    for name in ("query_cov", "hadamard", "tANI"):
        assert f"Cannot plot {name} as all NA" in caplog.text


def test_classify_gives_singletons(viral_run, tmp_path):
    _work, database, _run = viral_run
    table = rundb.classify(database, tmp_path / "cls").read_text().splitlines()
    assert len(table) == 4  # header and one clique per genome
    assert all(line.split("\t")[0] == "1" for line in table[1:])


def test_degenerate_genome_is_null_in_the_database(tmp_path):
    rng = np.random.default_rng(5)
    fasta_dir = tmp_path / "fasta"
    fasta_dir.mkdir()
    (fasta_dir / "a.fasta").write_bytes(tc.fasta(tc.random_bases(rng, 3000)))
    (fasta_dir / "b.fna").write_bytes(tc.fasta(tc.random_bases(rng, 3000, (0.35, 0.15, 0.15, 0.35))))
    (fasta_dir / "poly.fa").write_bytes(tc.fasta(b"ACGT"))  # every Z-score 0: degenerate
    run = rundb.run_tetra_hip(fasta_dir, tmp_path / "d.db", temp=tmp_path / "tmp")
    poly = next(a.genome_hash for a in run.fasta_hashes if a.fasta_filename == "poly.fa")
    rows = _rows(tmp_path / "d.db")
    assert len(rows) == 9 and run.status == "Done"
    for q, s, identity, *rest in rows:
        assert rest == [None] * 4
        assert (identity is None) == (poly in (q, s))


def test_command_line_end_to_end(tmp_path, viral_run):
    _work, database, _run = viral_run
    cli_db = tmp_path / "cli.db"
    assert rundb.main(["tetra", str(VIRAL), "-d", str(cli_db), "--temp", str(tmp_path / "tmp"), "--cache", str(tmp_path / "cache"), "--name", "cli"]) == 0
    assert _rows(cli_db) == _rows(database)
    conn = sqlite3.connect(cli_db)
    assert conn.execute("SELECT name, status FROM runs").fetchall() == [("cli", "Done")]
    conn.close()
