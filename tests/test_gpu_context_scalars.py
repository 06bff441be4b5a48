"""No call depends on a device scalar another call left behind in the context (``pa_ctx::counters``, the dictionary's
scalars, the fragment-ANI workspace's, the pinned read-back block): every call gives, on one engine shared by all of
them and in two different orders, the very bits it gives on an engine of its own."""

from __future__ import annotations

import numpy as np
import pytest

from pyani_plus_amd import _capi, run_comp
from pyani_plus_amd.synth import synth_arena_numpy, synth_classify_matrices

pytestmark = pytest.mark.gpu

K, SCALED, BOTTOM_M, FRAG_K, FRAG_LEN, BINS = 31, 200, 64, 16, 3000, 30
NONE = 0xFFFFFFFF


def _inputs() -> dict:
    rng = np.random.default_rng(20)
    lengths = [20_000, 19_000, 21_000]
    arena = synth_arena_numpy(3, lengths, n_species=1)
    _labels, score, cov = synth_classify_matrices(70, seed=7, nan_frac=0.05)  # two 64 x 64 tiles a side
    assert np.isnan(score).any()
    ref = rng.random((10, 10))
    ref[rng.random((10, 10)) < 0.2] = np.nan
    q = rng.integers(0, 10, 200).astype(np.uint32)
    s = rng.integers(0, 10, 200).astype(np.uint32)
    q[::17], s[5::23], s[7::31] = NONE, 10, 4_000_000  # not a genome of the reference run
    y = rng.random(200)
    y[::11] = np.nan
    values = rng.normal(0.0, 1.0, 1000)
    return {"arena": arena, "lengths": np.array(lengths, dtype=np.uint32), "score": score, "cov": cov, "ref": ref, "q": q, "s": s, "y": y,
            "values": values, "edges": run_comp.hist_edges(values.min(), values.max(), BINS)}


def _calls(inp: dict, sketches: list[np.ndarray], counts: np.ndarray) -> dict:
    """name -> function of an engine; every input is host data, so a call needs no other call on its engine."""
    arena = inp["arena"]

    def on_device(engine, array):
        return engine.torch.from_numpy(array).to(engine.device)

    def sketch(engine):
        return engine.sketch(engine.upload(arena), K, SCALED).to_host()

    def sketch_bottom(engine):
        return engine.sketch_bottom(engine.upload(arena), K, BOTTOM_M).to_host()

    def pair_counts(algo):
        return lambda engine: [engine.pair_counts(engine.sketches_from_host(sketches), algo=algo).cpu().numpy()]

    def ani(engine):
        return [v.cpu().numpy() for v in engine.ani(on_device(engine, counts), engine.sketches_from_host(sketches), K)]

    def fragani(engine):
        starts = np.ascontiguousarray(arena.genome_start[:-1])
        return list(engine.fragani(engine.upload(arena), starts, inp["lengths"], np.arange(3, dtype=np.uint32), FRAG_K, FRAG_LEN))

    return {
        "sketch": sketch,
        "sketch_bottom": sketch_bottom,
        "pair_counts_bitrow": pair_counts(_capi.PA_PAIRS_BITROW),
        "pair_counts_auto": pair_counts(_capi.PA_PAIRS_AUTO),
        "ani": ani,
        "classify_edges": lambda engine: list(engine.classify_edges(inp["score"], inp["cov"])),
        "run_join": lambda engine: list(engine.run_join(inp["ref"], inp["q"], inp["s"], inp["y"])),
        "minmax": lambda engine: [np.array(engine.minmax(inp["values"]))],
        "hist_uniform": lambda engine: [engine.hist_uniform(inp["values"], inp["edges"])],
        "fragani": fragani,
    }


def _bits(result) -> list[tuple]:
    return [(a.dtype.str, a.shape, np.ascontiguousarray(a).tobytes()) for a in map(np.asarray, result)]


def test_calls_on_a_shared_engine_equal_calls_on_fresh_engines():
    from pyani_plus_amd.engine import HipEngine

    def fresh(call):
        engine = HipEngine(0)
        try:
            return call(engine)
        finally:
            engine.close()

    inp = _inputs()
    # the inputs of the pair phase and of ani, each from an engine of its own
    sketches = fresh(lambda engine: engine.sketch(engine.upload(inp["arena"]), K, SCALED).to_host())
    counts = fresh(lambda engine: engine.pair_counts(engine.sketches_from_host(sketches)).cpu().numpy())
    calls = _calls(inp, sketches, counts)
    alone = {name: fresh(call) for name, call in calls.items()}
    # the inputs are what the test means them to be: results that a scalar gone wrong would change
    assert all(len(sk) > 50 for sk in sketches) and counts.min() > 0  # noqa: PLR2004
    assert 0 < len(alone["classify_edges"][0]) < 70 * 69 // 2
    assert 0 < len(alone["run_join"][0]) < 200  # noqa: PLR2004
    assert alone["fragani"][1].min() > 0
    alone = {name: _bits(result) for name, result in alone.items()}

    names = list(calls)
    orders = (names, names[1::2] + names[0::2][::-1])
    shared = HipEngine(0)
    try:
        for order in orders:
            for name in order:
                assert _bits(calls[name](shared)) == alone[name], f"{name} on the shared engine, in the order {order}"
    finally:
        shared.close()
