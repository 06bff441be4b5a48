"""dereplicate-run's host twins (no GPU): ``pa_derep_adjacency_host``, ``pa_derep_select_host`` and
``pa_derep_assign_host`` against the restatement of tests/derep_cases.py on the whole grid of sizes, graph families,
aggregators and modes, exactly; the invariants of the bit matrix and of a selection; the refusals and their messages."""

from __future__ import annotations

import ctypes as C
import re
from pathlib import Path

import numpy as np
import pytest

from pyani_plus_amd import _capi
from pyani_plus_amd._capi import PA_E_INVALID, HipBackendError
from pyani_plus_amd.engine import derep_adjacency_host, derep_assign_host, derep_select_host, dereplicate_host
from tests import derep_cases as dc

ROOT = Path(__file__).resolve().parent.parent


@pytest.mark.parametrize("family", dc.FAMILIES)
@pytest.mark.parametrize("n", dc.SIZES)
def test_twins_equal_the_restatement(n, family):
    for score_edges, coverage_edges in dc.aggregator_pairs():
        case = dc.case(family, n, score_edges, coverage_edges)
        # the matrices realise the wanted graph under the restated edge rule
        assert np.array_equal(dc.adjacency(case.S, case.C, score_edges, coverage_edges, dc.MIN_SCORE, dc.COV_MIN), case.adj)
        words = derep_adjacency_host(case.S, case.C, **case.options)
        assert words.dtype == np.uint64 and words.shape == (n, (n + 63) // 64)
        assert np.array_equal(words, case.bits)
        for mode in dc.MODES:
            is_rep, n_reps = derep_select_host(words, n, mode)
            assert np.array_equal(is_rep, case.is_rep(mode)) and n_reps == int(is_rep.sum())
            rep, rep_score = derep_assign_host(case.S, words, is_rep, score_edges=score_edges)
            want_rep, want_score = case.assignment(mode)
            assert np.array_equal(rep, want_rep) and dc.same_scores(rep_score, want_score)


@pytest.mark.parametrize("family", dc.FAMILIES)
@pytest.mark.parametrize("n", (1, 2, 65, 129, 257))
def test_invariants(n, family):
    case = dc.case(family, n, "max", "mean")
    words = derep_adjacency_host(case.S, case.C, **case.options)
    adj = dc.unpack(words, n)
    assert np.array_equal(adj, adj.T) and adj.diagonal().all()
    if n % 64:  # the padding bits of the last word
        assert not (words[:, -1] >> np.uint64(n % 64)).any()
    greedy = derep_select_host(words, n, "greedy")[0].astype(bool)
    assert not (adj[np.ix_(greedy, greedy)] & ~np.eye(int(greedy.sum()), dtype=bool)).any()  # independent
    assert adj[:, greedy].any(axis=1).all()  # dominating
    cover = derep_select_host(words, n, "cover")[0].astype(bool)
    assert adj[:, cover].any(axis=1).all()
    for chosen in (greedy, cover):
        rep, _score = derep_assign_host(case.S, words, chosen.astype(np.uint8), score_edges="max")
        assert chosen[rep].all() and adj[np.arange(n), rep].all() and np.array_equal(rep[chosen], np.flatnonzero(chosen))


@pytest.mark.parametrize("mode", dc.MODES)
@pytest.mark.parametrize("n", (1, 64, 1025))
def test_no_edges_every_node_is_a_representative(n, mode):
    case = dc.case("none", n)
    result = dereplicate_host(case.S, case.C, mode=mode, **case.options)
    assert result.is_rep.all() and result.n_reps == n and np.array_equal(result.rep, np.arange(n)) and result.rounds is None


@pytest.mark.parametrize("mode", dc.MODES)
def test_cover_and_greedy_on_the_stars(mode):
    first, last = dc.case("star_first", 65), dc.case("star_last", 65)
    assert dereplicate_host(first.S, first.C, mode=mode, **first.options).n_reps == 1
    # the hub comes last: greedy keeps node 0, loses the hub to it and keeps every other leaf; cover takes the hub
    assert dereplicate_host(last.S, last.C, mode=mode, **last.options).n_reps == (64 if mode == "greedy" else 1)


@pytest.mark.parametrize("first_negative", (True, False))
def test_equal_scores_of_either_sign_go_to_the_smaller_representative(first_negative):
    S, C, min_score, cov_min = dc.zero_tie(first_negative)
    for score_edges in dc.AGGS:
        result = dereplicate_host(S, C, score_edges=score_edges, min_score=min_score, cov_min=cov_min)
        assert result.is_rep.tolist() == [True, True, False] and result.rep.tolist() == [0, 1, 0]
        assert np.array_equal(dc.bits(result.rep_score), dc.bits([1.0, 1.0, -0.0 if first_negative else 0.0]))
        adj = dc.adjacency(S, C, score_edges, "min", min_score, cov_min)
        assert np.array_equal(result.rep, dc.assign(S, score_edges, adj, dc.select(adj, "greedy"))[0])


def test_the_threshold_values():
    """score == min_score is an edge, cov == cov_min is not; a NaN in the first argument of min stays, in the second it is
    passed over."""
    nan = float("nan")
    S = np.array([[1.0, 0.5, 0.5, nan], [0.5, 1.0, 0.25, 0.5], [0.5, 0.25, 1.0, nan], [0.5, 0.5, 0.5, 1.0]])
    C = np.array([[1.0, 0.75, 0.5, 1.0], [0.75, 1.0, 1.0, 1.0], [0.5, 1.0, 1.0, 1.0], [1.0, 1.0, 1.0, 1.0]])
    words = derep_adjacency_host(S, C, score_edges="min", coverage_edges="min", min_score=0.5, cov_min=0.5)
    # (0, 1): at the score threshold, an edge; (0, 2): at the coverage threshold, none; (1, 2): below the score; (0, 3): NaN
    # is the second argument (S[lo, hi]), passed over; (2, 3) likewise; (1, 3): plain
    assert dc.unpack(words, 4).astype(int).tolist() == [[1, 1, 0, 1], [1, 1, 0, 1], [0, 0, 1, 1], [1, 1, 1, 1]]
    words = derep_adjacency_host(S.T, C, score_edges="min", coverage_edges="min", min_score=0.5, cov_min=0.5)
    assert dc.unpack(words, 4).astype(int).tolist() == [[1, 1, 0, 0], [1, 1, 0, 1], [0, 0, 1, 0], [0, 1, 0, 1]]  # the NaN comes first: it stays


def test_the_number_of_threads_does_not_show():
    case = dc.case("blocks", 257, "mean", "max")
    one = dereplicate_host(case.S, case.C, threads=1, **case.options)
    many = dereplicate_host(case.S, case.C, threads=7, **case.options)
    assert np.array_equal(one.rep, many.rep) and dc.same_scores(one.rep_score, many.rep_score)
    assert np.array_equal(derep_adjacency_host(case.S, case.C, threads=1, **case.options), derep_adjacency_host(case.S, case.C, threads=5, **case.options))


def test_the_inputs_are_left_alone():
    case = dc.case("gnp", 129)
    S, C = np.array(case.S), np.array(case.C)
    dereplicate_host(S, C, mode="cover", **case.options)
    assert dc.same_scores(S, case.S) and dc.same_scores(C, case.C)


# ------------------------------------------------------------------ refusals
def refused(match: str, call, *arguments, **options) -> None:
    with pytest.raises(HipBackendError, match=match) as err:
        call(*arguments, **options)
    assert err.value.status == PA_E_INVALID


def test_refuses_no_genomes():
    empty = np.zeros((0, 0))
    refused(r"pa_derep_adjacency: 0 genomes; 1 to 65535", derep_adjacency_host, empty, empty)
    refused(r"pa_derep_select: 0 genomes; 1 to 65535", derep_select_host, np.zeros(0, dtype=np.uint64), 0)
    refused(r"pa_derep_assign: 0 genomes; 1 to 65535", derep_assign_host, empty, np.zeros(0, dtype=np.uint64), np.zeros(0, dtype=np.uint8))


def test_refuses_too_many_genomes_before_anything_is_read():
    lib = _capi.load_library()
    word, mark, out32, out64, count = (C.c_uint64 * 1)(), (C.c_uint8 * 1)(), (C.c_uint32 * 1)(), (C.c_double * 1)(), C.c_uint32(0)
    address = C.addressof
    assert lib.pa_derep_adjacency_host(address(out64), address(out64), 65536, 2, 0, 0.95, 0.5, address(word), 0) == PA_E_INVALID
    assert lib.pa_last_error().decode() == "pa_derep_adjacency: 65536 genomes; 1 to 65535"
    assert lib.pa_derep_select_host(address(word), 65536, 0, address(mark), C.byref(count)) == PA_E_INVALID
    assert lib.pa_last_error().decode() == "pa_derep_select: 65536 genomes; 1 to 65535"
    assert lib.pa_derep_assign_host(address(out64), 65536, 2, address(word), address(mark), address(out32), address(out64), 0) == PA_E_INVALID
    assert lib.pa_last_error().decode() == "pa_derep_assign: 65536 genomes; 1 to 65535"
    assert lib.pa_derep_adjacency_host(None, address(out64), 1, 2, 0, 0.95, 0.5, address(word), 0) == PA_E_INVALID
    assert lib.pa_last_error().decode() == "pa_derep_adjacency: null argument"


def test_refuses_unknown_aggregators_and_modes():
    lib = _capi.load_library()
    one, word, mark, out32, count = (C.c_double * 1)(1.0), (C.c_uint64 * 1)(1), (C.c_uint8 * 1)(1), (C.c_uint32 * 1)(), C.c_uint32(0)
    address = C.addressof
    assert lib.pa_derep_adjacency_host(address(one), address(one), 1, 3, 0, 0.95, 0.5, address(word), 0) == PA_E_INVALID
    assert lib.pa_last_error().decode() == "pa_derep_adjacency: aggregators 3, 0 (PA_AGG_MIN, PA_AGG_MAX or PA_AGG_MEAN)"
    assert lib.pa_derep_adjacency_host(address(one), address(one), 1, 0, -1, 0.95, 0.5, address(word), 0) == PA_E_INVALID
    assert lib.pa_last_error().decode() == "pa_derep_adjacency: aggregators 0, -1 (PA_AGG_MIN, PA_AGG_MAX or PA_AGG_MEAN)"
    assert lib.pa_derep_select_host(address(word), 1, 2, address(mark), C.byref(count)) == PA_E_INVALID
    assert lib.pa_last_error().decode() == "pa_derep_select: mode 2 (PA_DEREP_GREEDY or PA_DEREP_COVER)"
    assert lib.pa_derep_assign_host(address(one), 1, 7, address(word), address(mark), address(out32), address(one), 0) == PA_E_INVALID
    assert lib.pa_last_error().decode() == "pa_derep_assign: aggregator 7 (PA_AGG_MIN, PA_AGG_MAX or PA_AGG_MEAN)"
    # the Python layer names what it does not know before the library is asked
    ones = np.ones((2, 2))
    with pytest.raises(ValueError, match="Unknown score aggregator 'median'"):
        derep_adjacency_host(ones, ones, score_edges="median")
    with pytest.raises(ValueError, match="Unknown dereplication mode 'best'"):
        dereplicate_host(ones, ones, mode="best")


def test_refuses_nan_thresholds():
    ones = np.ones((2, 2))
    refused(r"pa_derep_adjacency: min_score is NaN", derep_adjacency_host, ones, ones, min_score=float("nan"))
    refused(r"pa_derep_adjacency: cov_min is NaN", derep_adjacency_host, ones, ones, cov_min=float("nan"))
    # infinities are thresholds like any other
    assert derep_adjacency_host(ones, ones, min_score=float("inf")).tolist() == [[1], [2]]
    assert derep_adjacency_host(ones, ones, min_score=float("-inf"), cov_min=float("-inf")).tolist() == [[3], [3]]


def test_refuses_matrices_of_two_shapes():
    with pytest.raises(ValueError, match=r"shapes \(2, 2\) and \(3, 3\)"):
        derep_adjacency_host(np.ones((2, 2)), np.ones((3, 3)))
    with pytest.raises(ValueError, match="expected a square one"):
        derep_adjacency_host(np.ones((2, 3)), np.ones((2, 3)))


def test_the_abi_names_the_six_entry_points_and_the_batch():
    text = (ROOT / "include" / "pyani_hip.h").read_text()
    for symbol in ("pa_derep_adjacency", "pa_derep_select", "pa_derep_assign"):
        for name in (symbol, symbol + "_host"):
            assert name in _capi.SIGNATURES and re.search(rf"PA_API int {name}\(", text)
    # the binding reads the header, so each value is pinned here, against both
    for name, value in (("PA_DEREP_BATCH", 64), ("PA_DEREP_GREEDY", 0), ("PA_DEREP_COVER", 1)):
        assert getattr(_capi, name) == value and re.search(rf"#define {name} {value}\b", text), name
