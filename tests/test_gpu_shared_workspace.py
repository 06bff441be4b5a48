"""One ``HipEngine``, one context, the entry-point families mixed: a dictionary built ahead (``pair_dict_prepare``)
followed by Mash pair calls, by classify, plot-run-comp and plot-run calls, and by the radix pair algorithm, then the pair
counts of the prepared tile.  ``pa_pair_mash``'s tile path and ``PA_PAIRS_BITROW`` sort their postings in the buffer that
holds the prepared hash table, so they drop the preparation and the next default ``pair_counts`` builds its dictionary
again; the other families leave the context's pair buffers alone and the preparation survives them.

Every intermediate result is checked against an expectation computed once on the host.  The sequences run twice: in
order on the larger inputs, then in reverse order on smaller ones, when the workspaces hold what the larger run left."""

from __future__ import annotations

from functools import lru_cache

import numpy as np
import pytest

import oracle
from pyani_plus_amd import classify as cl
from pyani_plus_amd import cluster, run_comp
from pyani_plus_amd.synth import synth_classify_matrices
from tests import mash_cases
from tests.plot_run_cases import numpy_distances
from tests.run_comp_cases import join_inputs, join_reference, numpy_hist, numpy_join

PASSES = ("larger", "smaller")
TILE_SUBJECTS = 30
# per pass: hashes per sketch of the prepared tile (at most), the Mash tile-path set (sketches, hashes each, m), the two
# lists of the wave-path set, genomes of classify, (genomes, rows) of the join, (rows, columns) of the distances
SIZES = {
    "larger": {"tile": 300, "mash": (40, 1000, 1000), "wave": (25_000, 20_000), "classify": 130, "join": (130, 5000), "rows": (65, 33)},
    "smaller": {"tile": 100, "mash": (20, 400, 300), "wave": (19_968, 7), "classify": 65, "join": (33, 1000), "rows": (33, 17)},
}
HIST_BINS = 30


@pytest.fixture(scope="module")
def engine():
    from pyani_plus_amd.engine import HipEngine

    eng = HipEngine(0)
    yield eng
    eng.close()


def _drawn(rng, pool: np.ndarray, size: int) -> np.ndarray:
    return np.sort(pool[rng.choice(pool.size, size=size, replace=False)])


@lru_cache(maxsize=None)
def host_side(which: str) -> dict:
    """The inputs of one pass and what the host says about them, computed once and left unchanged."""
    sizes = SIZES[which]
    rng = np.random.default_rng([31, PASSES.index(which)])
    out: dict = {}
    # the prepared tile: 30 sketches of at most `tile` hashes of one pool (an empty one among them), below 2^63 so that
    # "the same sketches, every hash one larger" exists
    pool = np.unique(rng.integers(0, 2**63, size=3 * sizes["tile"], dtype=np.uint64))
    tile = [_drawn(rng, pool, int(rng.integers(1, sizes["tile"] + 1))) for _ in range(TILE_SUBJECTS)]
    tile[0], tile[7] = _drawn(rng, pool, sizes["tile"]), pool[:0]
    out["tile"], out["tile_counts"] = tile, oracle.pair_counts(tile)
    out["tile_shifted"] = [s + np.uint64(1) for s in tile]
    # Mash on the tile path, more postings than the prepared tile holds
    n, size, m = sizes["mash"]
    pool = np.unique(rng.integers(0, 2**64, size=3 * size, dtype=np.uint64))
    out["mash"], out["mash_m"] = [_drawn(rng, pool, size) for _ in range(n)], m
    assert sum(len(s) for s in out["mash"]) > sum(len(s) for s in tile)
    assert mash_cases.launch_plan(out["mash"], m)["path"] == "tile"
    out["mash_want"] = oracle.mash_pairs(out["mash"], m)
    # Mash on the wave path
    first, second = sizes["wave"]
    pool = np.unique(rng.integers(0, 2**64, size=first + second, dtype=np.uint64))
    a = _drawn(rng, pool, first)
    wave = [a, _drawn(rng, pool, second), a[:50].copy()]
    out["wave"], out["wave_m"] = wave, first
    assert mash_cases.launch_plan(wave, first)["path"] == "wave"
    out["wave_want"] = oracle.mash_pairs(wave, first)
    # classify
    _labels, ident, cov = synth_classify_matrices(sizes["classify"], seed=4, nan_frac=0.05)
    out["classify"], out["edges"] = (ident, cov), cl.edges_host(ident, cov)
    assert len(out["edges"][0]) > sizes["classify"]
    # plot-run-comp
    n_ref, n_rows = sizes["join"]
    ref = join_reference(n_ref)
    q, s, y, survivors = join_inputs(n_rows, ref, "mixed")
    joined = run_comp.join_host(ref, q, s, y)
    assert len(joined[0]) == survivors > 0
    for mine, restated in zip(joined, numpy_join(ref, q, s, y)):
        assert np.array_equal(mine.view(np.uint64), np.ascontiguousarray(restated).view(np.uint64))
    d = joined[2]
    out["join"], out["joined"] = (ref, q, s, y), joined
    out["minmax"] = (float(d.min()), float(d.max()), len(d))
    out["edges_of_hist"] = run_comp.hist_edges(d.min(), d.max(), HIST_BINS)
    out["hist"] = numpy_hist(d, out["edges_of_hist"])
    assert out["hist"].sum() == len(d)
    # plot-run
    rows, columns = sizes["rows"]
    x = rng.uniform(0.0, 1.0, (rows, columns))
    out["matrix"], out["distances"] = x, cluster.row_distances(x)
    assert np.array_equal(out["distances"].view(np.uint64), numpy_distances(x).view(np.uint64))
    return out


class Pass:
    """One pass's inputs on the device, and the steps of the sequences."""

    def __init__(self, engine, which: str):
        self.engine, self.which, self.host = engine, which, host_side(which)
        self.tile = engine.sketches_from_host(self.host["tile"])
        self.tile_shifted = engine.sketches_from_host(self.host["tile_shifted"])
        self.mash = engine.sketches_from_host(self.host["mash"])
        self.wave = engine.sketches_from_host(self.host["wave"])
        assert self.tile.total == self.tile_shifted.total

    def prepare(self) -> None:
        self.engine.pair_dict_prepare(self.tile.hashes, self.tile.total)

    def counts(self, what: str, algo: int = 0) -> None:
        got = self.engine.pair_counts(self.tile, algo=algo).cpu().numpy().view(np.uint32)
        want = self.host["tile_counts"]
        assert np.array_equal(got, want), f"{self.which}, pair counts after {what}: {int((got != want).sum())} of {want.size} differ, first at {np.argwhere(got != want)[:4].tolist()}"

    def pair_mash(self, name: str) -> None:
        common, denom = self.engine.pair_mash(getattr(self, name), self.host[f"{name}_m"])
        for part, got, want in zip(("common", "denom"), (common, denom), self.host[f"{name}_want"]):
            assert np.array_equal(got.cpu().numpy().view(np.uint32), want), f"{self.which}, pair_mash ({name} set): {part}"

    def other_families(self) -> None:
        e, h = self.engine, self.host
        got = e.classify_edges(*h["classify"])
        for g, w, kind in zip(got, h["edges"], (np.uint32, np.uint32, np.uint64, np.uint64)):
            assert g.shape == w.shape and np.array_equal(np.ascontiguousarray(g).view(kind), np.ascontiguousarray(w).view(kind)), f"{self.which}, classify_edges"
        x, y, d = e.run_join_device(*h["join"])
        for g, w in zip((x, y, d), h["joined"]):
            g = g.cpu().numpy()
            assert g.shape == w.shape and np.array_equal(g.view(np.uint64), w.view(np.uint64)), f"{self.which}, run_join"
        assert np.array_equal(e.hist_uniform(d, h["edges_of_hist"]), h["hist"]), f"{self.which}, hist_uniform"
        assert e.minmax(d) == h["minmax"], f"{self.which}, minmax"
        got = e.row_distances(h["matrix"])
        assert got.shape == h["distances"].shape and np.array_equal(got.view(np.uint64), h["distances"].view(np.uint64)), f"{self.which}, row_distances"

    # ---- the sequences, each from a freshly prepared dictionary
    def mash_tile_then_counts(self) -> None:
        self.prepare()
        self.pair_mash("mash")  # sorts its postings over the prepared table: the preparation is dropped
        self.counts("pair_dict_prepare and pair_mash on the tile path")

    def mash_wave_then_counts(self) -> None:
        self.prepare()
        self.pair_mash("wave")  # reads the sketches only: the table is intact whether the preparation is kept or not
        self.counts("pair_dict_prepare and pair_mash on the wave path")

    def other_families_then_counts(self) -> None:
        from pyani_plus_amd._capi import HipBackendError

        self.prepare()
        self.other_families()
        self.counts("pair_dict_prepare, classify_edges, run_join, hist_uniform, minmax and row_distances")
        # that the preparation is still held after them: other postings of the same number are refused by content
        self.prepare()
        self.other_families()
        with pytest.raises(HipBackendError, match="other postings"):
            self.engine.pair_counts(self.tile_shifted)
        self.counts("a refused preparation")

    def bitrow_then_default(self) -> None:
        self.prepare()
        self.counts("pair_dict_prepare, with the radix dictionary", algo=1)  # PA_PAIRS_BITROW: the same sort, the same buffer
        self.counts("pair_dict_prepare and PA_PAIRS_BITROW")

    SEQUENCES = ("mash_tile_then_counts", "mash_wave_then_counts", "other_families_then_counts", "bitrow_then_default")


def test_host_expectations_are_sized_as_named():
    """Needs no GPU: the inputs of the two passes.  The second pass's inputs are smaller, family by family."""
    big, small = host_side("larger"), host_side("smaller")
    for h, sizes in ((big, SIZES["larger"]), (small, SIZES["smaller"])):
        assert len(h["tile"]) == TILE_SUBJECTS and max(len(s) for s in h["tile"]) == sizes["tile"] <= 300 and min(len(s) for s in h["tile"]) == 0
        assert h["tile_counts"].shape == (TILE_SUBJECTS, TILE_SUBJECTS) and np.count_nonzero(h["tile_counts"]) > 500
        assert max(len(s) for s in h["wave"]) <= 25_000 and len(h["classify"][0]) <= 130
    for key in ("tile", "mash", "wave"):
        assert sum(len(s) for s in small[key]) < sum(len(s) for s in big[key])
    for key in ("matrix", "distances", "hist"):
        assert small[key].size <= big[key].size
    assert len(small["joined"][0]) < len(big["joined"][0]) and len(small["edges"][0]) < len(big["edges"][0])


@pytest.mark.gpu
def test_families_share_one_context(engine):
    larger, smaller = Pass(engine, "larger"), Pass(engine, "smaller")
    for name in Pass.SEQUENCES:
        getattr(larger, name)()
    for name in reversed(Pass.SEQUENCES):
        getattr(smaller, name)()
