"""TETRA-hip on the MI355X: ``pa_tetra_counts`` against the numpy restatement of tests/tetra_cases.py, exactly, with the
arena's dirty bitmap and without; ``pa_tetra_corr`` against ``pa_tetra_corr_host``, bit for bit; ``run_tetra_hip`` on the
device against the host run's rows.  No step is tried twice."""

from __future__ import annotations

import sqlite3

import numpy as np
import pytest

from pyani_plus_amd import cluster, rundb
from pyani_plus_amd.engine import HipEngine, tetra_correlations_host
from tests import tetra_cases as tc
from tests.helpers import GOLDEN

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def engine():
    eng = HipEngine(0)
    yield eng
    eng.close()


@pytest.mark.parametrize("use_dirty", (True, False), ids=("dirty", "no_dirty"))
@pytest.mark.parametrize("name", sorted(tc.count_cases()))
def test_counts_equal_the_oracle(engine, name, use_dirty):
    arena, want = tc.case_arena(name)
    got = engine.tetra_counts(engine.upload(arena), use_dirty=use_dirty)
    assert got.shape == want.shape
    wrong = np.flatnonzero((got != want).any(axis=1))
    assert wrong.size == 0, f"{name}: {wrong.size} genomes differ, first {wrong[:8]}; genome {wrong[0]}: bins {np.flatnonzero(got[wrong[0]] != want[wrong[0]])[:8]}"


def test_counts_are_the_same_run_to_run(engine):
    arena, want = tc.case_arena("three_chunks")
    dev = engine.upload(arena)
    assert np.array_equal(engine.tetra_counts(dev), engine.tetra_counts(dev))
    assert tc.kernel_constants()["kTile"] == 64 and arena.arena_bases > 3 * tc.chunk_bases()  # the case spans four workgroups


def test_direct_counting_form_gives_the_same_counts(monkeypatch):
    """The kernel's other instance (three updates per start, nothing derived), which the tools build selects."""
    monkeypatch.setenv("PA_TETRA_DIRECT", "1")
    tools_engine = HipEngine(0, tools=True)
    try:
        for name in ("lengths", "separator", "n_runs", "three_chunks", "many_small"):
            arena, want = tc.case_arena(name)
            assert np.array_equal(tools_engine.tetra_counts(tools_engine.upload(arena)), want), name
    finally:
        tools_engine.close()


@pytest.mark.parametrize("n", (1, 2, 3, 63, 64, 65, 130))
def test_correlations_equal_the_host_twin(engine, n):
    unit = tc.unit_rows(n)
    got = engine.tetra_correlations(unit)  # square and on the diagonal: the symmetric form
    tc.same_bits(got, tetra_correlations_host(unit))
    tc.same_bits(got, got.T)
    ok = ~np.isnan(unit).any(axis=1)
    assert (np.diag(got)[ok] == 1.0).all() and np.isnan(got[~ok]).all() and np.isnan(got[:, ~ok]).all()
    assert (np.abs(got[np.ix_(ok, ok)]) <= 1.0).all()


def test_correlation_ranges_off_the_tile_grid(engine):
    unit = tc.unit_rows(130)
    for q_range, s_range in (((0, 130), (5, 6)), ((3, 70), (60, 129)), ((64, 130), (0, 64)), ((1, 2), (0, 130)), ((17, 82), (17, 82)), ((7, 7), (0, 9))):
        got = engine.tetra_correlations(unit, q_range, s_range)
        assert got.shape == (q_range[1] - q_range[0], s_range[1] - s_range[0])
        tc.same_bits(got, tetra_correlations_host(unit, q_range, s_range))
    full = tetra_correlations_host(unit)
    tc.same_bits(engine.tetra_correlations(unit, (17, 82), (17, 82)), full[17:82, 17:82])  # a square range: mirrored, same cells
    small = [tc.unit_row(tc.zscores(tc.forward_counts(tc.fasta(tc.random_bases(np.random.default_rng(s), 2000))))) for s in range(3)]
    tc.same_bits(engine.tetra_correlations(np.array(small)), tc.correlation_matrix(small))  # and the plain-Python restatement


def test_both_tile_instantiations_back_to_back(engine):
    """The tile skeleton's two instantiations (run-time columns in the row distances, 256 fixed here) alternate in one
    context; each result has its host twin's bits and the second distance call repeats the first."""
    unit = tc.unit_rows(130)
    finite = unit.copy()
    finite[1] = 0.0  # the distances take finite rows
    assert np.isnan(unit[1]).all() and np.isfinite(finite).all()
    first = engine.row_distances(finite)
    whole = engine.tetra_correlations(unit)
    second = engine.row_distances(finite)
    part = engine.tetra_correlations(unit, (3, 70), (60, 129))
    tc.same_bits(first, cluster.row_distances(finite))
    tc.same_bits(whole, tetra_correlations_host(unit))
    tc.same_bits(second, cluster.row_distances(finite))
    tc.same_bits(part, tetra_correlations_host(unit, (3, 70), (60, 129)))
    assert np.array_equal(first.view(np.uint64), second.view(np.uint64))


def _rows(database):
    conn = sqlite3.connect(database)
    rows = conn.execute("SELECT query_hash, subject_hash, identity, cov_query, aln_length, sim_errors, cov_subject FROM comparisons ORDER BY 1, 2").fetchall()
    conn.close()
    return rows


@pytest.mark.parametrize("fixture", ("viral_example", "bacterial_example"))
def test_run_on_the_device_equals_the_host_run(engine, fixture, tmp_path):
    host = rundb.run_tetra_hip(GOLDEN / fixture, tmp_path / "host.db", temp=tmp_path / "th", cache=tmp_path / "ch", engine=None)
    dev = rundb.run_tetra_hip(GOLDEN / fixture, tmp_path / "dev.db", temp=tmp_path / "td", cache=tmp_path / "cd", engine=engine)
    assert host.status == dev.status == "Done"
    rows = _rows(tmp_path / "dev.db")
    n = len(dev.fasta_hashes)
    assert len(rows) == n * n and rows == _rows(tmp_path / "host.db")
    assert all(r[2] is not None and r[3:] == (None,) * 4 for r in rows)
    for genome in dev.fasta_hashes:
        name = f"{genome.genome_hash}.json"
        assert (tmp_path / "cd" / "tetra_hip" / name).read_text() == (tmp_path / "ch" / "tetra_hip" / name).read_text()
