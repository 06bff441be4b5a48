"""search-run on the MI355X: ``pa_best_hits`` against its host twin and the restatement of tests/search_cases.py,
exactly, on every family at the lane, wave, block and tile seams (the kernel's columns-per-lane stride is its block of
256 lanes; it stages nothing in LDS); tiling invariance with ``accumulate``; twice on the same tensors; the refusals
with the twin's messages (argument checks made before any launch); ``rundb.search_run`` with the engine against the
files of the oracle-backed run; and synthetic genomes whose counts come from ``pa_pair_counts`` on the device.  No step
is tried twice."""

from __future__ import annotations

import numpy as np
import pytest

import oracle
from pyani_plus_amd import _capi, rundb, search
from pyani_plus_amd._capi import PA_E_INVALID, HipBackendError
from pyani_plus_amd.engine import HipEngine, best_hits_host
from pyani_plus_amd.synth import synth_arena_numpy
from tests import search_cases as sc
from tests.fake_engine import OracleEngine
from tests.helpers import FIXTURE_SETS, GOLDEN

pytestmark = pytest.mark.gpu
NS = (1, 63, 64, 65, 255, 256, 257, 2047, 2048, 2049)
NQ = (1, 3, 130)
TOPS = (1, 5, 64)


@pytest.fixture(scope="module")
def engine():
    eng = HipEngine(0)
    yield eng
    eng.close()


def on_device(engine, array):
    return engine.torch.from_numpy(np.ascontiguousarray(array, dtype=np.uint32).view(np.int32).copy()).to(engine.device)


def to_host(state):
    return tuple(x.cpu().numpy().view(np.uint32) for x in state)


@pytest.mark.parametrize("ns", NS)
@pytest.mark.parametrize("nq", NQ)
def test_device_equals_the_twin_and_the_restatement(engine, nq, ns):
    for family in sc.FAMILIES:
        counts, q_size, s_size = sc.case(family, nq, ns)
        d_counts, d_q, d_s = (on_device(engine, x) for x in (counts, q_size, s_size))  # uploaded once per case
        for rank in sc.RANKS:
            for top in TOPS:
                got = to_host(engine.best_hits_device(d_counts, d_q, d_s, 0, rank, top))
                assert sc.same(got, sc.expected_top(family, nq, ns, rank, top)), (family, rank, top)
                if top == TOPS[-1]:
                    assert sc.same(got, best_hits_host(counts, q_size, s_size, 0, rank, top)), (family, rank)


@pytest.mark.parametrize("rank", sc.RANKS)
@pytest.mark.parametrize("family", ("random", "identical", "equal_ratio", "extreme", "q_smaller", "winners_in_one_lane"))
def test_any_cut_into_tiles_gives_the_one_call_result(engine, family, rank):
    nq, ns = 3, 257
    counts, q_size, s_size = sc.case(family, nq, ns)
    d_counts, d_q, d_s = (on_device(engine, x) for x in (counts, q_size, s_size))
    rng = np.random.default_rng(7)  # the cuts of the host test
    for top in (1, 5, 64):
        want = sc.expected_top(family, nq, ns, rank, top)
        for pieces, ones in ((1, False), (2, False), (7, False), (7, True)):
            tiles = sc.cuts(ns, pieces, rng, ones=ones)
            for order in (tiles, tiles[::-1]):
                state = None
                for a, b in order:  # a slice of the columns: the rows stay ns apart, ld > the tile's width
                    state = engine.best_hits_device(d_counts[:, a:b], d_q, d_s[a:b], a, rank, top, state)
                assert sc.same(to_host(state), want), (top, order)


@pytest.mark.parametrize("rank", sc.RANKS)
def test_a_long_row_walked_in_tiles_of_2048(engine, rank):
    nq, ns, top = 3, 5000, 64
    rng = np.random.default_rng(11)
    counts = rng.choice(np.array([0, 0, 0, 7, 8, 9, 1000, 2000], dtype=np.uint32), (nq, ns))
    counts[:, ns - 1] = 2500
    q_size, s_size = np.full(nq, 5000, dtype=np.uint32), rng.integers(2500, 7000, ns).astype(np.uint32)
    want = best_hits_host(counts, q_size, s_size, 0, rank, top)
    restated = sc.best_hits(counts[:1], q_size[:1], s_size, rank, top)
    assert sc.same(tuple(x[:1] for x in want), restated)
    d_q, d_s = on_device(engine, q_size), on_device(engine, s_size)
    state = None
    for s0 in range(0, ns, 2048):
        tile = on_device(engine, counts[:, s0 : s0 + 2048])
        state = engine.best_hits_device(tile, d_q, d_s[s0 : s0 + 2048], s0, rank, top, state)
    assert sc.same(to_host(state), want)
    assert sc.same(to_host(engine.best_hits_device(on_device(engine, counts), d_q, d_s, 0, rank, top)), want)


def test_twice_on_the_same_tensors(engine):
    counts, q_size, s_size = sc.case("random", 130, 2049)
    d_counts, d_q, d_s = (on_device(engine, x) for x in (counts, q_size, s_size))
    first = to_host(engine.best_hits_device(d_counts, d_q, d_s, 0, "identity", 64))
    second = to_host(engine.best_hits_device(d_counts, d_q, d_s, 0, "identity", 64))
    assert sc.same(first, second) and sc.same(first, sc.expected_top("random", 130, 2049, "identity", 64))
    assert np.array_equal(d_counts.cpu().numpy().view(np.uint32), counts)  # the input is left alone


def test_no_columns_and_no_queries(engine):
    t = engine.torch
    none = t.empty((2, 0), dtype=t.int32, device=engine.device)
    got = to_host(engine.best_hits_device(none, np.array([5, 6]), np.array([], dtype=np.uint32), 0, "identity", 3))
    assert (got[0] == sc.NONE).all() and not got[1].any() and not got[2].any()
    counts, q_size, s_size = sc.case("random", 3, 65)
    state = engine.best_hits_device(on_device(engine, counts), q_size, s_size, 0, "identity", 3)
    kept = to_host(state)
    again = engine.best_hits_device(t.empty((3, 0), dtype=t.int32, device=engine.device), q_size, np.array([], dtype=np.uint32), 65, "identity", 3, state)
    assert sc.same(to_host(again), kept)
    empty = engine.best_hits_device(t.empty((0, 4), dtype=t.int32, device=engine.device), np.array([], dtype=np.uint32), np.array([1, 2, 3, 4]), 0, "containment", 2)
    assert [tuple(x.shape) for x in empty] == [(0, 2)] * 3


def small_good_call(engine) -> None:
    counts, q_size, s_size = sc.case("random", 3, 65)
    assert sc.same(to_host(engine.best_hits_device(on_device(engine, counts), q_size, s_size, 0, "identity", 5)), sc.expected_top("random", 3, 65, "identity", 5))


def test_the_refusals_with_the_twins_messages(engine):
    """Every refusal is an argument check made before any launch; the twin says the same words."""
    counts = np.ones((2, 4), dtype=np.uint32)
    q_size, s_size = np.array([5, 6], dtype=np.uint32), np.array([5, 6, 7, 8], dtype=np.uint32)
    d_counts, d_q, d_s = (on_device(engine, x) for x in (counts, q_size, s_size))
    outs = [engine.torch.zeros((2, 3), dtype=engine.torch.int32, device=engine.device) for _ in range(3)]
    h_outs = [np.zeros((2, 3), dtype=np.uint32) for _ in range(3)]
    lib = engine.lib

    def both(message, *, ld=4, s_base=0, rank=0, top=3, null=None):
        d_args = [d_counts.data_ptr(), 2, 4, ld, d_q.data_ptr(), d_s.data_ptr(), s_base, rank, top, 0, *(o.data_ptr() for o in outs)]
        h_args = [counts.ctypes.data, 2, 4, ld, q_size.ctypes.data, s_size.ctypes.data, s_base, rank, top, 0, *(o.ctypes.data for o in h_outs)]
        if null is not None:
            d_args[null] = h_args[null] = None
        assert lib.pa_best_hits(engine.ctx, *d_args) == PA_E_INVALID and _capi.last_error(lib) == message
        assert lib.pa_best_hits_host(*h_args, 1) == PA_E_INVALID and _capi.last_error(lib) == message

    both("pa_best_hits: top 0 (1 to 64)", top=0)
    both("pa_best_hits: top 65 (1 to 64)", top=65)
    both("pa_best_hits: rank 2 (PA_HITS_RANK_IDENTITY or PA_HITS_RANK_CONTAINMENT)", rank=2)
    both("pa_best_hits: ld 3 is less than ns 4", ld=3)
    both("pa_best_hits: index overflow: s_base 4294967291 + ns 4 reaches PA_HITS_NONE", s_base=0xFFFFFFFF - 4)
    both("pa_best_hits: index overflow: nq 2 rows of ld 4611686018427387904 counts", ld=1 << 62)
    for position, name in ((0, "counts"), (4, "q_size"), (5, "s_size"), (10, "hit_subject"), (11, "hit_shared"), (12, "hit_denom")):
        both(f"pa_best_hits: null {name}", null=position)
    with pytest.raises(HipBackendError, match=r"pa_best_hits: top 65 \(1 to 64\)") as err:
        engine.best_hits_device(d_counts, d_q, d_s, 0, "identity", 65)
    assert err.value.status == PA_E_INVALID
    with pytest.raises(ValueError, match="subject sizes: sketch sizes must be 1 to 2\\^32 - 1"):
        engine.best_hits_device(d_counts, q_size, np.array([5, 6, 0, 8]), 0, "identity", 3)
    small_good_call(engine)


@pytest.mark.parametrize("name", ("viral_example", "bacterial_example"))
def test_search_run_with_the_engine_writes_the_oracle_runs_files(engine, tmp_path, name):
    scaled, _genomes = FIXTURE_SETS[name]
    db = tmp_path / "runs.sqlite"
    assert rundb.run_sourmash_hip(GOLDEN / name, db, cache=tmp_path / "cache", scaled=scaled, engine=OracleEngine(), temp=tmp_path / "t").status == "Done"
    for options in ({}, {"rank": "containment", "top": 64}):
        host = rundb.search_run(GOLDEN / name, db, tmp_path / f"host{len(options)}", cache=tmp_path / "cache", engine=OracleEngine(), **options)
        device = rundb.search_run(GOLDEN / name, db, tmp_path / f"device{len(options)}", temp=tmp_path / "t2", engine=engine, **options)
        assert [p.name for p in device] == [p.name for p in host]
        assert [p.read_bytes() for p in device] == [p.read_bytes() for p in host]  # the subjects sketched on the device too: no cache was given


@pytest.mark.parametrize("rank", sc.RANKS)
def test_synthetic_genomes_counted_on_the_device(engine, rank):
    n_queries, n_subjects, k, scaled, top = 10, 40, 31, 100, 5
    arena = synth_arena_numpy(n_queries + n_subjects, 30000, n_species=4)
    sketches = engine.sketch(engine.upload(arena), k, scaled).to_host()
    queries, subjects = sketches[:n_queries], sketches[n_queries:]
    hits = search.search(subjects, queries, k, top=top, rank=rank, engine=engine)
    counts = oracle.pair_counts(sketches, (0, n_queries), (n_queries, n_queries + n_subjects))
    want = sc.best_hits(counts, [len(q) for q in queries], [len(s) for s in subjects], rank, top)
    assert int((want[0] != sc.NONE).sum()) > n_queries  # the species share hashes: there is something to rank
    assert np.array_equal(hits.subject, np.where(want[0] == sc.NONE, -1, want[0].astype(np.int64))) and np.array_equal(hits.shared, want[1])
    host = search.search(subjects, queries, k, top=top, rank=rank, engine=OracleEngine())
    for got, other in zip(hits, host):
        assert np.array_equal(got, other, equal_nan=got.dtype.kind == "f")
