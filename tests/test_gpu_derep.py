"""dereplicate-run on the MI355X: ``pa_derep_adjacency``, ``pa_derep_select`` and ``pa_derep_assign`` each against its host
twin and the restatement of tests/derep_cases.py, exactly, on the size grid and every graph family; a multi-tile size;
the seam of a batch of rounds in both modes, crossed as ``n_rounds`` shows; the graph with no edges; twice on the same
tensors; the refusals with the twins' messages; and ``rundb.dereplicate_run`` with the engine against the host run.  No
step is tried twice."""

from __future__ import annotations

import numpy as np
import pytest

from pyani_plus_amd import _capi, rundb
from pyani_plus_amd._capi import PA_E_INVALID, HipBackendError
from pyani_plus_amd.engine import HipEngine, derep_adjacency_host, derep_assign_host, derep_select_host, dereplicate_host
from tests import derep_cases as dc
from tests.fake_engine import OracleEngine
from tests.helpers import FIXTURE_SETS, GOLDEN

pytestmark = pytest.mark.gpu
BATCH = _capi.PA_DEREP_BATCH


@pytest.fixture(scope="module")
def engine():
    eng = HipEngine(0)
    yield eng
    eng.close()


def words_of(tensor) -> np.ndarray:
    return tensor.cpu().numpy().view(np.uint64)


def three_calls(engine, case: dc.Case, mode: str):
    """The three device calls on one case: ``(bits, is_rep, n_reps, n_rounds, rep, rep_score)`` as host arrays."""
    bits = engine.derep_adjacency_device(case.S, case.C, **case.options)
    is_rep, n_reps, n_rounds = engine.derep_select_device(bits, case.n, mode)
    rep, rep_score = engine.derep_assign_device(case.S, bits, is_rep, score_edges=case.score_edges)
    return words_of(bits), is_rep.cpu().numpy(), n_reps, n_rounds, rep.cpu().numpy().view(np.uint32), rep_score.cpu().numpy()


def equals_the_twin(case: dc.Case, mode: str, got) -> None:
    bits, is_rep, n_reps, _n_rounds, rep, rep_score = got
    h_bits = derep_adjacency_host(case.S, case.C, **case.options)
    assert bits.shape == h_bits.shape and np.array_equal(bits, h_bits)
    h_is_rep, h_n_reps = derep_select_host(h_bits, case.n, mode)
    assert np.array_equal(is_rep, h_is_rep) and n_reps == h_n_reps == int(is_rep.sum())
    h_rep, h_score = derep_assign_host(case.S, h_bits, h_is_rep, score_edges=case.score_edges)
    assert np.array_equal(rep, h_rep) and dc.same_scores(rep_score, h_score)


def equals_the_restatement(case: dc.Case, mode: str, got) -> None:
    bits, is_rep, _n_reps, _n_rounds, rep, rep_score = got
    assert np.array_equal(bits, case.bits)
    assert np.array_equal(is_rep, case.is_rep(mode))
    want_rep, want_score = case.assignment(mode)
    assert np.array_equal(rep, want_rep) and dc.same_scores(rep_score, want_score)


def small_good_call(engine) -> None:
    case = dc.case("blocks", 65)
    equals_the_restatement(case, "greedy", three_calls(engine, case, "greedy"))


@pytest.mark.parametrize("family", dc.FAMILIES)
@pytest.mark.parametrize("n", dc.SIZES)
def test_device_equals_the_twin_and_the_restatement(engine, n, family):
    pairs = dc.aggregator_pairs()  # every pair of aggregators comes up across the grid
    score_edges, coverage_edges = pairs[(dc.SIZES.index(n) + dc.FAMILIES.index(family)) % len(pairs)]
    case = dc.case(family, n, score_edges, coverage_edges)
    for mode in dc.MODES:
        got = three_calls(engine, case, mode)
        equals_the_twin(case, mode, got)
        equals_the_restatement(case, mode, got)


@pytest.mark.parametrize("score_edges,coverage_edges", dc.aggregator_pairs())
def test_every_pair_of_aggregators(engine, score_edges, coverage_edges):
    case = dc.case("blocks", 129, score_edges, coverage_edges)
    for mode in dc.MODES:
        equals_the_restatement(case, mode, three_calls(engine, case, mode))


def test_several_tiles(engine):
    """4 097 nodes: 65 words a row, 65 x 65 tiles.  The restatement gives the graph and the greedy choice; the cover mode's
    some thousand rounds are compared with the twin, which the host tests hold to the restatement."""
    case = dc.Case(dc.graph("blocks", 4097), "mean", "min")
    for mode in dc.MODES:
        got = three_calls(engine, case, mode)
        equals_the_twin(case, mode, got)
        assert np.array_equal(got[0], case.bits)
        if mode == "greedy":
            assert np.array_equal(got[1], case.is_rep(mode))
        assert got[3] >= 1


@pytest.mark.parametrize("extra", (-1, 0, 1))
def test_the_seam_of_a_batch_greedy(engine, extra):
    """A path in index order settles two nodes a round: ceil(n / 2) rounds."""
    rounds = BATCH + extra
    case = dc.Case(dc.graph("path", 2 * rounds - 1), "mean", "min")
    got = three_calls(engine, case, "greedy")
    assert got[3] == rounds
    equals_the_twin(case, "greedy", got)
    equals_the_restatement(case, "greedy", got)
    assert np.array_equal(np.flatnonzero(got[1]), np.arange(0, case.n, 2))


@pytest.mark.parametrize("extra", (-1, 0, 1))
def test_the_seam_of_a_batch_cover(engine, extra):
    """Disjoint triangles: every choice covers one of them, a round each."""
    rounds = BATCH + extra
    case = dc.Case(dc.disjoint_triangles(rounds), "mean", "min")
    got = three_calls(engine, case, "cover")
    assert got[3] == rounds
    equals_the_twin(case, "cover", got)
    equals_the_restatement(case, "cover", got)
    assert np.array_equal(np.flatnonzero(got[1]), np.arange(0, case.n, 3))


@pytest.mark.parametrize("mode", dc.MODES)
def test_no_edges(engine, mode):
    """Every node is a representative, in one round: of free nodes in greedy mode, by the gain-1 rule in cover mode."""
    case = dc.case("none", 1025)
    result = engine.dereplicate(case.S, case.C, mode=mode, **case.options)
    assert result.is_rep.all() and result.n_reps == 1025 and result.rounds == 1
    assert np.array_equal(result.rep, np.arange(1025)) and dc.same_scores(result.rep_score, case.assignment(mode)[1])


def test_the_tail_of_single_nodes_is_one_round(engine):
    """Three triangles and 700 nodes alone in cover mode: three choices, then every node left at once."""
    adj = np.eye(709, dtype=bool)
    adj[:9, :9] = dc.disjoint_triangles(3)
    case = dc.Case(adj, "max", "max")
    got = three_calls(engine, case, "cover")
    assert got[3] == 4 and got[2] == 703
    equals_the_restatement(case, "cover", got)


@pytest.mark.parametrize("mode", dc.MODES)
def test_two_calls_on_the_same_tensors(engine, mode):
    t = engine.torch
    case = dc.case("gnp", 257)
    d_s, d_c = t.from_numpy(np.array(case.S)).to(engine.device), t.from_numpy(np.array(case.C)).to(engine.device)
    first = engine.dereplicate(d_s, d_c, mode=mode, **case.options)
    second = engine.dereplicate(d_s, d_c, mode=mode, **case.options)
    host = dereplicate_host(case.S, case.C, mode=mode, **case.options)
    for other in (second, host):
        assert np.array_equal(first.is_rep, other.is_rep) and np.array_equal(first.rep, other.rep) and first.n_reps == other.n_reps
        assert dc.same_scores(first.rep_score, other.rep_score)
    assert first.rounds == second.rounds and host.rounds is None
    assert dc.same_scores(d_s.cpu().numpy(), case.S) and dc.same_scores(d_c.cpu().numpy(), case.C)


@pytest.mark.parametrize("first_negative", (True, False))
def test_equal_scores_of_either_sign(engine, first_negative):
    S, C, min_score, cov_min = dc.zero_tie(first_negative)
    result = engine.dereplicate(S, C, score_edges="min", min_score=min_score, cov_min=cov_min)
    assert result.rep.tolist() == [0, 1, 0]
    assert np.array_equal(dc.bits(result.rep_score), dc.bits([1.0, 1.0, -0.0 if first_negative else 0.0]))


def refused(engine, match: str, device_call, host_call) -> None:
    with pytest.raises(HipBackendError, match=match) as err:
        device_call()
    assert err.value.status == PA_E_INVALID
    with pytest.raises(HipBackendError, match=match):  # the twin says the same
        host_call()
    small_good_call(engine)


def test_refuses_no_genomes(engine):
    empty, no_words, no_marks = np.zeros((0, 0)), np.zeros(0, dtype=np.uint64), np.zeros(0, dtype=np.uint8)
    refused(engine, r"pa_derep_adjacency: 0 genomes; 1 to 65535", lambda: engine.derep_adjacency_device(empty, empty),
            lambda: derep_adjacency_host(empty, empty))  # fmt: skip
    refused(engine, r"pa_derep_select: 0 genomes; 1 to 65535", lambda: engine.derep_select_device(no_words, 0), lambda: derep_select_host(no_words, 0))
    refused(engine, r"pa_derep_assign: 0 genomes; 1 to 65535", lambda: engine.derep_assign_device(empty, no_words, no_marks),
            lambda: derep_assign_host(empty, no_words, no_marks))  # fmt: skip


def test_refuses_nan_thresholds(engine):
    ones = np.ones((2, 2))
    for name in ("min_score", "cov_min"):
        options = {name: float("nan")}
        refused(engine, rf"pa_derep_adjacency: {name} is NaN", lambda: engine.derep_adjacency_device(ones, ones, **options),  # noqa: B023
                lambda: derep_adjacency_host(ones, ones, **options))  # noqa: B023  # fmt: skip


def test_refuses_unknown_codes_and_too_many_genomes(engine):
    """What the Python layer never lets through, given to the library itself: the device entry points and the twins answer
    with the same words, before anything is read or launched."""
    t, lib = engine.torch, engine.lib
    cell = t.ones(1, dtype=t.float64, device=engine.device)
    word = t.ones(1, dtype=t.int64, device=engine.device)
    mark = t.ones(1, dtype=t.uint8, device=engine.device)
    out32 = t.zeros(1, dtype=t.int32, device=engine.device)
    count, rounds = _capi.C.c_uint32(0), _capi.C.c_uint32(0)
    h_cell, h_word, h_mark, h_out32 = np.ones(1), np.ones(1, dtype=np.uint64), np.ones(1, dtype=np.uint8), np.zeros(1, dtype=np.uint32)
    by_ref = _capi.C.byref
    calls = (
        (lambda n, code: lib.pa_derep_adjacency(engine.ctx, cell.data_ptr(), cell.data_ptr(), n, code, 0, 0.95, 0.5, word.data_ptr()),
         lambda n, code: lib.pa_derep_adjacency_host(h_cell.ctypes.data, h_cell.ctypes.data, n, code, 0, 0.95, 0.5, h_word.ctypes.data, 0),
         "pa_derep_adjacency: aggregators 5, 0 (PA_AGG_MIN, PA_AGG_MAX or PA_AGG_MEAN)", "pa_derep_adjacency"),
        (lambda n, code: lib.pa_derep_select(engine.ctx, word.data_ptr(), n, code, mark.data_ptr(), by_ref(count), by_ref(rounds)),
         lambda n, code: lib.pa_derep_select_host(h_word.ctypes.data, n, code, h_mark.ctypes.data, by_ref(count)),
         "pa_derep_select: mode 5 (PA_DEREP_GREEDY or PA_DEREP_COVER)", "pa_derep_select"),
        (lambda n, code: lib.pa_derep_assign(engine.ctx, cell.data_ptr(), n, code, word.data_ptr(), mark.data_ptr(), out32.data_ptr(), cell.data_ptr()),
         lambda n, code: lib.pa_derep_assign_host(h_cell.ctypes.data, n, code, h_word.ctypes.data, h_mark.ctypes.data, h_out32.ctypes.data, h_cell.ctypes.data, 0),
         "pa_derep_assign: aggregator 5 (PA_AGG_MIN, PA_AGG_MAX or PA_AGG_MEAN)", "pa_derep_assign"),
    )  # fmt: skip
    for device_call, host_call, unknown, who in calls:
        for call in (device_call, host_call):
            assert call(1, 5) == PA_E_INVALID and lib.pa_last_error().decode() == unknown
            assert call(65536, 0) == PA_E_INVALID and lib.pa_last_error().decode() == f"{who}: 65536 genomes; 1 to 65535"
    small_good_call(engine)


def test_dereplicate_run_with_the_engine_writes_the_host_bytes(engine, tmp_path):
    scaled, _genomes = FIXTURE_SETS["viral_example"]
    db = tmp_path / "runs.sqlite"
    assert rundb.run_sourmash_hip(GOLDEN / "viral_example", db, cache=tmp_path / "cache", scaled=scaled, engine=OracleEngine(), temp=tmp_path).status == "Done"
    for number, options in enumerate(({}, {"min_identity": 0.997}, {"min_identity": 0.997, "mode": "cover", "prefer": "label"}, {"min_identity": 0.9999})):
        host = rundb.dereplicate_run(db, tmp_path / f"host{number}", **options)
        device = rundb.dereplicate_run(db, tmp_path / f"device{number}", engine=engine, **options)
        assert [p.name for p in device] == [p.name for p in host] == ["sourmash-hip_dereplicate.tsv", "sourmash-hip_representatives.tsv"]
        assert [p.read_bytes() for p in device] == [p.read_bytes() for p in host]
