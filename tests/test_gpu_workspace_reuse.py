"""The device workspaces that are cut into several arrays (``pa_carve``, csrc/pa_internal.h), each through its entry
point on ONE engine at three shapes in the order large, small, larger: the workspace grows, is used again while it
holds what the larger call left, and grows again.  Every result is compared bit for bit with the entry point's host
twin, or with ``oracle.pair_counts`` / ``oracle.sketch_seq`` for the pair and sketch sites.

The shapes sit at the seams: 130, 5, 131 rows cross a 64-row tile and a 64-bit word; 300, 3, 513 permutations and 33, 1,
65 replicates lie on both sides of a batch; the bin counts on both sides of what a workgroup's LDS holds.

``moments`` and ``kde_gauss`` promise their twins a bound, not bits, because the device adds in another order.  Their
inputs here make every sum exact, so that the order cannot show: the values are multiples of 2^-10 placed symmetrically
about 1/2 (the mean is 1/2, every deviation and square is exact), and the density's bandwidth is so small against the
grid's spacing that every term is exp(-0.0) = 1 (a value on the grid point) or underflows to 0."""

from __future__ import annotations

from functools import lru_cache

import numpy as np
import pytest

import oracle
from pyani_plus_amd import _capi, distribution, run_comp, scatter
from pyani_plus_amd import engine as engine_mod
from pyani_plus_amd.synth import arena_to_ascii, synth_arena_numpy
from tests import bootstrap_cases, derep_cases, mantel_cases, scatter_cases
from tests.run_comp_cases import join_inputs, join_reference

ORDER = (0, 1, 2)  # large, small, larger
ROWS = (130, 5, 131)
PERMUTATIONS = (300, 3, 513)
BOOT = ((65, 33), (1, 1), (257, 65))  # (columns, replicates) of 6 rows
BIN2D = (70, 8, 100)
WIDE_BINS = (9000, 30, 20000)
VALUES = (5000, 10, 9000)
KDE_GRIDS = (1024, 7, 1024)
GENOMES = (40, 3, 41)
K = 21


@pytest.fixture(scope="module")
def engine():
    eng = engine_mod.HipEngine(0)
    yield eng
    eng.close()


def bits(x) -> np.ndarray:
    return np.ascontiguousarray(x, dtype=np.float64).view(np.uint64)


def same(got, want, what: str) -> None:
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, f"{what}: shape {got.shape}, expected {want.shape}"
    if want.dtype == np.float64:
        got, want = bits(got), bits(want)
    assert np.array_equal(got, want), f"{what}: {int((got != want).sum())} of {want.size} differ, first at {np.argwhere(got != want)[:4].tolist()}"


@lru_cache(maxsize=None)
def distances(n: int) -> np.ndarray:
    d = mantel_cases.random_distances(n, 900 + n)
    d.setflags(write=False)
    return d


@lru_cache(maxsize=None)
def exact_values(n: int) -> np.ndarray:
    """n multiples of 2^-10 in (0, 1), v and 1 - v in pairs: their mean is exactly 1/2 in any order of addition."""
    half = np.random.default_rng(n).integers(1, 512, size=n // 2) / 1024.0
    v = np.concatenate([half, 1.0 - half])
    np.random.default_rng(n + 1).shuffle(v)
    return v  # left writable: torch wraps writable arrays only


def test_the_shapes_lie_where_they_are_said_to():
    """Needs no GPU."""
    assert PERMUTATIONS[0] + 1 > _capi.PA_MANTEL_BATCH > PERMUTATIONS[1] + 1 and PERMUTATIONS[2] + 1 > 2 * _capi.PA_MANTEL_BATCH
    assert BOOT[0][1] > _capi.PA_MSA_BOOT_BATCH > BOOT[1][1] and BOOT[2][1] > 2 * _capi.PA_MSA_BOOT_BATCH
    assert BIN2D[0] ** 2 > _capi.PA_BIN2D_LDS_CELLS > BIN2D[1] ** 2 and BIN2D[2] ** 2 > BIN2D[0] ** 2
    assert WIDE_BINS[0] > _capi.PA_HIST_WIDE_LDS_BINS > WIDE_BINS[1] and WIDE_BINS[2] > WIDE_BINS[0]
    for sizes in (ROWS, PERMUTATIONS, VALUES, GENOMES, [c * r for c, r in BOOT]):
        assert sizes[1] < sizes[0] < sizes[2]
    for n in VALUES:
        v = exact_values(n)
        assert len(v) == n and v.mean() == 0.5 and np.array_equal(v * 1024, np.round(v * 1024))  # noqa: PLR2004


@pytest.mark.gpu
def test_nj(engine):
    for i in ORDER:
        D = distances(ROWS[i])
        got, want = engine.nj_tree(D), engine_mod.nj_tree_host(D)
        for g, w, part in zip(got[:3], want[:3], ("child", "length", "last")):
            same(g, w, f"nj_tree of {ROWS[i]} nodes, {part}")
        assert bits(got[3]) == bits(want[3])


@pytest.mark.gpu
def test_gower_center(engine):
    for i in ORDER:
        D = distances(ROWS[i])
        got, want = engine.gower_center(D), engine_mod.gower_center_host(D)
        same(got[0], want[0], f"gower_center of {ROWS[i]} rows")
        assert bits(got[1]) == bits(want[1]) and bits(got[2]) == bits(want[2])


@pytest.mark.gpu
@pytest.mark.parametrize("p", (1, 32))
def test_mul_tall(engine, p):
    for i in ORDER:
        n = ROWS[i]
        rng = np.random.default_rng([n, p])
        A, Q = rng.standard_normal((n, n)), rng.standard_normal((n, p))
        same(engine.mul_tall(A, Q), engine_mod.mul_tall_host(A, Q), f"mul_tall, n = {n}, p = {p}")


@pytest.mark.gpu
def test_symm_top_eigs(engine):
    for i in ORDER:
        B, _trace, fro2 = engine_mod.gower_center_host(distances(ROWS[i]))
        got, want = engine.symm_top_eigs(B, 3, fro2), engine_mod.symm_top_eigs_host(B, 3, fro2)
        for g, w, part in zip(got[:3], want[:3], ("values", "vectors", "residuals")):
            same(g, w, f"symm_top_eigs of {ROWS[i]} rows, {part}")
        assert got[3][:2] == want[3][:2] and bits(got[3][2]) == bits(want[3][2])


@pytest.mark.gpu
@pytest.mark.parametrize("mode", derep_cases.MODES)
def test_derep(engine, mode):
    for i in ORDER:
        case = derep_cases.case("gnp", ROWS[i])
        got = engine.dereplicate(case.S, case.C, **case.options, mode=mode)
        want = engine_mod.dereplicate_host(case.S, case.C, **case.options, mode=mode)
        for part in ("is_rep", "rep", "rep_score"):
            same(getattr(got, part), getattr(want, part), f"dereplicate ({mode}) of {ROWS[i]} nodes, {part}")
        assert got.n_reps == want.n_reps


@pytest.mark.gpu
def test_mantel(engine):
    for i in ORDER:
        n = ROWS[i]
        X, Y = distances(n), mantel_cases.random_distances(n, 1900 + n)
        perms = engine_mod.mantel_permutations(7, n, 0, PERMUTATIONS[i])
        got, want = engine.mantel(X, Y, perms), engine_mod.mantel_host(X, Y, perms)
        same(got[0], want[0], f"mantel, n = {n}, {PERMUTATIONS[i]} permutations, stats")
        same(got[1], want[1], f"mantel, n = {n}, {PERMUTATIONS[i]} permutations, cross")


def loaded(rows: np.ndarray) -> engine_mod.LoadedMSA:
    n, length = rows.shape
    padded = np.full((n, max(32, (length + 31) // 32 * 32)), bootstrap_cases.GAP, dtype=np.uint8)
    padded[:, :length] = rows
    hist = np.bincount(rows.ravel(), minlength=256).astype(np.uint64)
    return engine_mod.LoadedMSA("", [f"r{i}".encode() for i in range(n)], np.full(n, length, np.uint64), hist, padded, length)


def u32(tensor) -> np.ndarray:
    return tensor.cpu().numpy().view(np.uint32)


@pytest.mark.gpu
def test_msa_boot_counts(engine):
    for i in ORDER:
        n_cols, reps = BOOT[i]
        rows = bootstrap_cases.alignment(6, n_cols, 40 + i)
        weights = engine_mod.msa_boot_weights(3, n_cols, 0, reps)
        match, both = engine.msa_boot_counts(engine.msa_upload(loaded(rows)), weights)
        want_m, want_b = engine_mod.msa_boot_counts_host(rows, n_cols, weights)
        same(u32(match), want_m, f"msa_boot_counts, {n_cols} columns, {reps} replicates, match")
        same(u32(both), want_b, f"msa_boot_counts, {n_cols} columns, {reps} replicates, both")


@pytest.mark.gpu
def test_bin2d(engine):
    for i in ORDER:
        xedges, yedges = scatter_cases.grid_edges(BIN2D[i], BIN2D[i])
        x, y = scatter_cases.random_points(3000, xedges, yedges, seed=i)
        got, want = engine.bin2d(x, y, xedges, yedges), scatter.bin2d_host(x, y, xedges, yedges)
        same(got[0], want[0], f"bin2d, {BIN2D[i]} x {BIN2D[i]} bins, counts")
        same(got[1], want[1], f"bin2d, {BIN2D[i]} x {BIN2D[i]} bins, last")
        assert int(got[0].sum()) > 1000  # noqa: PLR2004


@pytest.mark.gpu
def test_hist_uniform_wide(engine):
    v = np.random.default_rng(5).random(20_000)
    for i in ORDER:
        edges = run_comp.hist_edges(0.0, 1.0, WIDE_BINS[i])
        got = engine.hist_uniform_wide(v, edges)
        same(got, distribution.hist_uniform_wide_host(v, edges), f"hist_uniform_wide, {WIDE_BINS[i]} bins")
        assert int(got.sum()) == len(v)


@pytest.mark.gpu
def test_minmax_moments_and_kde(engine):
    """One after the other at each shape: all three cut c->hist, ``kde_gauss`` after its own call of ``minmax``."""
    for i in ORDER:
        v, n_grid = exact_values(VALUES[i]), KDE_GRIDS[i]
        assert engine.minmax(v) == run_comp.minmax_host(v) == (float(v.min()), float(v.max()), len(v))
        got, want = engine.moments(v), distribution.moments_host(v)
        assert (bits(got[0]), bits(got[1])) == (bits(want[0]), bits(want[1])) and got[0] == 0.5, f"moments of {len(v)} values: {got}, the twin {want}"  # noqa: PLR2004
        # the grid: every multiple of 2^-10 in [0, 1), or the smallest values themselves; a bandwidth of 2^-20 puts a value
        # that is not on a grid point at least 1024 bandwidths from it
        grid, bw = (np.arange(1024) / 1024.0 if n_grid == 1024 else np.unique(v)[:n_grid]), 2.0**-20  # noqa: PLR2004
        assert len(grid) == n_grid
        density = engine.kde_gauss(v, grid, bw)
        same(density, distribution.kde_gauss_host(v, grid, bw), f"kde_gauss, {len(v)} values, {n_grid} grid points")
        on_grid = np.array([int((v == g).sum()) for g in grid])
        same(density, on_grid * (1.0 / (float(len(v)) * bw * np.sqrt(2.0 * np.pi))), f"kde_gauss, {len(v)} values: the counts on the grid points")
        assert on_grid.sum() == len(v) if n_grid == 1024 else on_grid.min() >= 1  # noqa: PLR2004


@pytest.mark.gpu
def test_run_join(engine):
    ref = join_reference(33)
    for i in ORDER:
        q, s, y, survivors = join_inputs(VALUES[i], ref, "mixed", seed=11 + i)
        got, want = engine.run_join(ref, q, s, y), run_comp.join_host(ref, q, s, y)
        assert len(want[0]) == survivors
        for g, w, part in zip(got, want, ("x", "y", "d")):
            same(g, w, f"run_join of {VALUES[i]} rows, {part}")


@lru_cache(maxsize=None)
def genomes(n: int):
    """n small genomes, the first long enough that its candidate region is past what the LDS sort takes at scaled = 1:
    the call takes the general path (one candidate list, two radix sorts, flags | pos)."""
    arena = synth_arena_numpy(n, [14_000] + [1000 + 37 * g for g in range(1, n)], n_species=2, seed=50 + n)
    want = [oracle.sketch_seq(arena_to_ascii(arena, g), K, 1) for g in range(n)]
    return arena, want


@pytest.mark.gpu
def test_sketch_on_the_general_path_and_bitrow_pair_counts(engine):
    for i in ORDER:
        arena, want = genomes(GENOMES[i])
        assert int(14_000 * 1.25) + 128 > 16384  # noqa: PLR2004  kLdsSortMax, csrc/pa_internal.h
        sk = engine.sketch(engine.upload(arena), K, 1)
        for g, (a, b) in enumerate(zip(sk.to_host(), want)):
            same(a, b, f"sketch of genome {g} of {GENOMES[i]}")
        _arena, streamed = engine.sketch_streamed(engine.pin_arena(arena), K, 1)  # the mask from its runs: start | len
        for g, (a, b) in enumerate(zip(streamed.to_host(), want)):
            same(a, b, f"streamed sketch of genome {g} of {GENOMES[i]}")
        counts = engine.pair_counts(sk, algo=_capi.PA_PAIRS_BITROW).cpu().numpy().view(np.uint32)
        same(counts, oracle.pair_counts(want), f"pair_counts (bit rows) of {GENOMES[i]} sketches")
