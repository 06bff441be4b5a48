"""``pa_best_hits_host``, search-run's selection on the host, against the restatement of tests/search_cases.py: every
family at the lane, wave, block and tile seams, tiling invariance with ``accumulate``, a row stride above the width,
the thread count, every refusal with its text, and the header's constants.  Every comparison is of integers."""

from __future__ import annotations

import ctypes as C

import numpy as np
import pytest

from pyani_plus_amd import _capi
from pyani_plus_amd import engine as engine_mod
from tests import search_cases as sc

NS = (1, 2, 63, 64, 65, 257, 2049)
NQ = (1, 3, 65)
TOPS = (1, 2, 5, 64)


@pytest.mark.parametrize("ns", NS)
@pytest.mark.parametrize("nq", NQ)
@pytest.mark.parametrize("family", sc.FAMILIES)
def test_the_twin_is_the_restatement(family, nq, ns):
    counts, q_size, s_size = sc.case(family, nq, ns)
    for rank in sc.RANKS:
        for top in TOPS:
            got = engine_mod.best_hits_host(counts, q_size, s_size, 0, rank, top)
            assert sc.same(got, sc.expected_top(family, nq, ns, rank, top)), (rank, top)


def test_the_families_are_what_they_say():
    counts, q_size, s_size = sc.case("extreme", 3, 65)
    assert int(counts.min()) > sc.U32 - 10 and int(s_size.max()) < int(q_size.min()) == sc.U32  # noqa: PLR2004
    a = sc.U32 - 1  # the neighbouring ratios of the family: exact cross products one unit apart, equal as doubles
    assert (a - 1) * (a - 1) - (a - 2) * a == 1 and float(a - 1) / float(a) == float(a - 2) / float(a - 1)
    subject, shared, denom = sc.expected("equal_ratio", 1, 65, "identity")
    assert len({(int(i) * 2, int(m)) for i, m in zip(shared[0], denom[0])} - {(int(m), int(m)) for m in denom[0]}) == 0  # every ratio is 1/2
    assert list(shared[0]) == sorted(shared[0], reverse=True) and int(shared[0, 0]) > int(shared[0, -1])  # the larger I first
    subject, _shared, _denom = sc.expected("identical", 1, 65, "containment")
    assert list(subject[0]) == list(range(64))
    subject, _shared, _denom = sc.expected("last_column_wins", 3, 257, "identity")
    assert list(subject[:, 0]) == [256] * 3
    subject, _shared, _denom = sc.expected("winners_in_one_lane", 1, 2049, "identity")
    assert len({int(s) % 256 for s in subject[0, :8]}) == 1
    subject, _shared, _denom = sc.expected("all_zero", 3, 64, "identity")
    assert (subject == sc.NONE).all()
    _counts, q_size, s_size = sc.case("q_smaller", 3, 65)
    assert (s_size < q_size[0]).any() and (s_size > q_size[0]).any()
    _subject, shared, _denom = sc.expected("fewer_than_top", 3, 65, "identity")
    assert [int((row > 0).sum()) for row in shared] == [0, 1, 2]


@pytest.mark.parametrize("rank", sc.RANKS)
@pytest.mark.parametrize("family", ("random", "identical", "equal_ratio", "extreme", "q_smaller", "winners_in_one_lane"))
def test_any_cut_into_tiles_gives_the_one_call_result(family, rank):
    nq, ns = 3, 257
    counts, q_size, s_size = sc.case(family, nq, ns)
    rng = np.random.default_rng(7)
    for top in (1, 5, 64):
        want = sc.expected_top(family, nq, ns, rank, top)
        for pieces, ones in ((1, False), (2, False), (7, False), (7, True)):
            tiles = sc.cuts(ns, pieces, rng, ones=ones)
            for order in (tiles, tiles[::-1]):  # the tiles must not overlap; their order is free
                state = None
                for a, b in order:
                    state = engine_mod.best_hits_host(np.ascontiguousarray(counts[:, a:b]), q_size, s_size[a:b], a, rank, top, state)
                assert sc.same(state, want), (top, order)


def test_a_cut_inside_a_run_of_ties():
    counts, q_size, s_size = sc.case("identical", 1, 65)  # every column ties: the order is the index order across the cut
    state = engine_mod.best_hits_host(np.ascontiguousarray(counts[:, 3:]), q_size, s_size[3:], 3, "identity", 5)
    assert list(state[0][0]) == [3, 4, 5, 6, 7]
    state = engine_mod.best_hits_host(np.ascontiguousarray(counts[:, :3]), q_size, s_size[:3], 0, "identity", 5, state)
    assert list(state[0][0]) == [0, 1, 2, 3, 4] and sc.same(state, sc.expected_top("identical", 1, 65, "identity", 5))


def test_no_columns_and_no_queries():
    none = np.empty((2, 0), dtype=np.uint32)
    got = engine_mod.best_hits_host(none, [5, 6], [], 0, "identity", 3)
    assert (got[0] == sc.NONE).all() and not got[1].any() and not got[2].any()
    counts, q_size, s_size = sc.case("random", 3, 65)
    state = engine_mod.best_hits_host(counts, q_size, s_size, 0, "identity", 3)
    kept = tuple(x.copy() for x in state)
    again = engine_mod.best_hits_host(np.empty((3, 0), dtype=np.uint32), q_size, [], 65, "identity", 3, state)
    assert sc.same(again, kept)  # accumulating nothing leaves the lists
    assert [x.shape for x in engine_mod.best_hits_host(np.empty((0, 4), dtype=np.uint32), [], [1, 2, 3, 4], 0, "containment", 2)] == [(0, 2)] * 3


@pytest.mark.parametrize("rank", sc.RANKS)
def test_a_row_stride_above_the_width(rank):
    nq, ns, ld = 3, 65, 80
    counts, q_size, s_size = sc.case("random", nq, ns)
    wide = np.full((nq, ld), 0xDEADBEEF, dtype=np.uint32)  # what lies between the rows is not read
    wide[:, :ns] = counts
    got = engine_mod.best_hits_host(wide.reshape(-1)[: (nq - 1) * ld + ns], q_size, s_size, 0, rank, 5, ld=ld)
    assert sc.same(got, sc.expected_top("random", nq, ns, rank, 5))


@pytest.mark.parametrize("family", ("random", "identical"))
def test_one_and_sixteen_threads_give_the_same_bits(family):
    counts, q_size, s_size = sc.case(family, 65, 2049)
    one = engine_mod.best_hits_host(counts, q_size, s_size, 0, "identity", 64, threads=1)
    many = engine_mod.best_hits_host(counts, q_size, s_size, 0, "identity", 64, threads=16)
    assert sc.same(one, many) and sc.same(one, sc.expected_top(family, 65, 2049, "identity", 64))


def call(counts, nq, ns, ld, q_size, s_size, s_base, rank, top, accumulate=0, outs=None):  # noqa: PLR0913
    """The twin through ctypes alone: ``(status, message)``; None is a NULL pointer."""
    lib = _capi.load_library()
    keep = [None if a is None else np.ascontiguousarray(a, dtype=np.uint32) for a in (counts, q_size, s_size)]
    outs = [np.zeros(max(nq * max(min(top, 64), 1), 1), dtype=np.uint32) for _ in range(3)] if outs is None else outs
    ptr = lambda a: None if a is None else a.ctypes.data  # noqa: E731
    status = lib.pa_best_hits_host(ptr(keep[0]), nq, ns, ld, ptr(keep[1]), ptr(keep[2]), s_base, rank, top, accumulate, *(ptr(o) for o in outs), 1)
    return status, _capi.last_error(lib)


REFUSALS = (
    ({"top": 0}, "pa_best_hits: top 0 (1 to 64)"),
    ({"top": 65}, "pa_best_hits: top 65 (1 to 64)"),
    ({"rank": 2}, "pa_best_hits: rank 2 (PA_HITS_RANK_IDENTITY or PA_HITS_RANK_CONTAINMENT)"),
    ({"rank": -1}, "pa_best_hits: rank -1 (PA_HITS_RANK_IDENTITY or PA_HITS_RANK_CONTAINMENT)"),
    ({"ld": 3}, "pa_best_hits: ld 3 is less than ns 4"),
    ({"s_base": 0xFFFFFFFF - 4}, "pa_best_hits: index overflow: s_base 4294967291 + ns 4 reaches PA_HITS_NONE"),
    ({"ld": 1 << 62}, "pa_best_hits: index overflow: nq 2 rows of ld 4611686018427387904 counts"),
    ({"counts": None}, "pa_best_hits: null counts"),
    ({"q_size": None}, "pa_best_hits: null q_size"),
    ({"s_size": None}, "pa_best_hits: null s_size"),
    ({"outs": 0}, "pa_best_hits: null hit_subject"),
    ({"outs": 1}, "pa_best_hits: null hit_shared"),
    ({"outs": 2}, "pa_best_hits: null hit_denom"),
    ({"q_size": [5, 0]}, "pa_best_hits_host: q_size[1] is 0 (sizes are 1 to 2^32 - 1)"),
    ({"s_size": [5, 6, 0, 7]}, "pa_best_hits_host: s_size[2] is 0 (sizes are 1 to 2^32 - 1)"),
)


def refusal_arguments(change: dict) -> dict:
    """A valid call of 2 queries against 4 columns with one argument made wrong."""
    args = {"counts": np.ones(8, dtype=np.uint32), "nq": 2, "ns": 4, "ld": 4, "q_size": [5, 6], "s_size": [5, 6, 7, 8], "s_base": 0, "rank": 0, "top": 3}
    args.update(change)
    if isinstance(args.get("outs"), int):
        outs = [np.zeros(6, dtype=np.uint32) for _ in range(3)]
        outs[args["outs"]] = None
        args["outs"] = outs
    return args


@pytest.mark.parametrize("change,message", REFUSALS)
def test_every_refusal_with_its_text(change, message):
    status, text = call(**refusal_arguments(change))
    assert status == _capi.PA_E_INVALID and text == message
    assert call(**refusal_arguments({}))[0] == _capi.PA_OK


def test_the_refusals_come_in_the_stated_order():
    assert call(**refusal_arguments({"top": 0, "rank": 9, "ld": 1, "counts": None}))[1] == "pa_best_hits: top 0 (1 to 64)"
    assert call(**refusal_arguments({"rank": 9, "ld": 1, "counts": None}))[1].startswith("pa_best_hits: rank 9")
    assert call(**refusal_arguments({"ld": 1, "counts": None}))[1] == "pa_best_hits: ld 1 is less than ns 4"


def test_an_array_without_elements_may_be_null():
    assert call(None, 2, 0, 0, [5, 6], None, 0, 0, 3)[0] == _capi.PA_OK
    assert call(None, 0, 4, 4, None, [5, 6, 7, 8], 0, 0, 3, outs=[None] * 3)[0] == _capi.PA_OK


def test_the_python_layer_checks_the_sizes():
    counts = np.ones((1, 2), dtype=np.uint32)
    with pytest.raises(ValueError, match="subject sizes: sketch sizes must be 1 to 2\\^32 - 1, found 0 to 5"):
        engine_mod.best_hits_host(counts, [5], [5, 0], 0, "identity", 1)
    with pytest.raises(ValueError, match="query sizes: sketch sizes must be 1 to 2\\^32 - 1"):
        engine_mod.best_hits_host(counts, [1 << 32], [5, 5], 0, "identity", 1)
    with pytest.raises(ValueError, match="Unknown rank 'best': expected one of identity, containment"):
        engine_mod.best_hits_host(counts, [5], [5, 5], 0, "best", 1)


def test_the_header_constants_reach_python():
    assert (_capi.PA_HITS_MAX_TOP, _capi.PA_HITS_NONE, _capi.PA_HITS_RANK_IDENTITY, _capi.PA_HITS_RANK_CONTAINMENT) == (64, 0xFFFFFFFF, 0, 1)
    assert _capi.PA_HITS_RANK == {"identity": 0, "containment": 1} and sc.NONE == _capi.PA_HITS_NONE and sc.MAX_TOP == _capi.PA_HITS_MAX_TOP
    for name in ("pa_best_hits", "pa_best_hits_host"):
        restype, argtypes = _capi.SIGNATURES[name]
        assert restype is C.c_int and len(argtypes) == 14  # noqa: PLR2004
    assert _capi.SIGNATURES["pa_best_hits"][1][4] is C.c_uint64 and _capi.SIGNATURES["pa_best_hits_host"][1][3] is C.c_uint64  # ld is 64 bits wide
