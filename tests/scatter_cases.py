"""Inputs and oracles for plot-run's scatter figures: random points with NaNs and values outside the range, points on
every edge of a grid and on the doubles either side, points aimed at the slots of the device's direct-mapped cache, and
numpy's answers.

Used by tests/test_scatter_host.py (no GPU: the host twin, ``scatter.describe``, ``rundb.plot_run(scatter=True)``) and
tests/test_gpu_scatter.py (the kernel).  The boundary cases are built from the kernel's constants as ``_capi`` states
them: ``LDS_CELLS``, up to which a workgroup keeps every cell in LDS, and ``SLOTS``, the slots of the cache above it
(the slot of a cell is ``cell % SLOTS``)."""

from __future__ import annotations

import numpy as np

from pyani_plus_amd import _capi, run_comp, scatter
from tests.run_comp_cases import adversarial_values

LDS_CELLS = _capi.PA_BIN2D_LDS_CELLS
SLOTS = _capi.PA_BIN2D_SLOTS
NONE = np.uint64(scatter.NONE)

GRIDS = ((1, 1), (1, 7), (7, 1), (64, 64), (256, 256), (1024, 1024))
# either side of the full-privatisation boundary: exactly LDS_CELLS cells, and one column more
BOUNDARY_GRIDS = ((64, LDS_CELLS // 64), (64, LDS_CELLS // 64 + 1))
DEVICE_GRIDS = ((1, 1), (1, 7), (7, 1), *BOUNDARY_GRIDS, (256, 256), (1024, 1024))
DEVICE_SIZES = (0, 1, 63, 64, 65, 255, 256, 257, 1023, 1025, 300_001)  # the last is past one stride of the grid (1024 x 256)
assert BOUNDARY_GRIDS[0][0] * BOUNDARY_GRIDS[0][1] == LDS_CELLS < BOUNDARY_GRIDS[1][0] * BOUNDARY_GRIDS[1][1]


def grid_edges(bins_x: int, bins_y: int, seed: int = 0) -> tuple[np.ndarray, np.ndarray]:
    """Edges over two random ranges inside (-2, 2)."""
    rng = np.random.default_rng(1000 * bins_x + bins_y + 17 * seed)
    (x0, x1), (y0, y1) = sorted(rng.random(2) * 4 - 2), sorted(rng.random(2) * 4 - 2)
    return run_comp.hist_edges(x0, x1, bins_x), run_comp.hist_edges(y0, y1, bins_y)


def random_points(n: int, xedges, yedges, seed: int = 0) -> tuple[np.ndarray, np.ndarray]:
    """``n`` points over the ranges widened by a tenth each way (so about a sixth lie outside on either axis); of every
    13 points one has NaN in x only, one in y only and one in both."""
    rng = np.random.default_rng(31 * n + seed)
    out = []
    for edges in (xedges, yedges):
        span = edges[-1] - edges[0]
        out.append(edges[0] - 0.1 * span + 1.2 * span * rng.random(n))
    x, y = out
    x[3::13] = np.nan
    y[5::13] = np.nan
    x[8::13] = np.nan
    y[8::13] = np.nan
    return x, y


def edge_points(xedges, yedges, seed: int = 0) -> tuple[np.ndarray, np.ndarray]:
    """Every edge of each axis, its two neighbouring doubles and the bins' midpoints (``adversarial_values``), each paired
    with a random value of the other axis and, position by position, with the other axis' own; then NaN in x only, in y
    only and in both, and a value outside the range below and above on each axis."""
    rng = np.random.default_rng(len(xedges) * 4099 + len(yedges) + seed)
    ax, ay = adversarial_values(xedges), adversarial_values(yedges)
    k = min(len(ax), len(ay))
    mid_x, mid_y = (xedges[0] + xedges[-1]) / 2, (yedges[0] + yedges[-1]) / 2
    x = np.concatenate([ax, xedges[0] + (xedges[-1] - xedges[0]) * rng.random(len(ay)), ax[:k], [np.nan, mid_x, np.nan, xedges[0] - 1.0, xedges[-1] + 1.0, mid_x, mid_x]])
    y = np.concatenate([yedges[0] + (yedges[-1] - yedges[0]) * rng.random(len(ax)), ay, ay[:k], [mid_y, np.nan, np.nan, mid_y, mid_y, yedges[0] - 1.0, yedges[-1] + 1.0]])
    order = rng.permutation(len(x))
    return x[order], y[order]


def cell_centres(cells, xedges, yedges) -> tuple[np.ndarray, np.ndarray]:
    """A point in the middle of each of these cells (cell ``ix * bins_y + iy``)."""
    ix, iy = np.divmod(np.asarray(cells, dtype=np.int64), len(yedges) - 1)
    return (xedges[ix] + xedges[ix + 1]) / 2, (yedges[iy] + yedges[iy + 1]) / 2


def slot_conflict_points(n: int, xedges, yedges, hot_shares_the_slot: bool, seed: int = 0) -> tuple[np.ndarray, np.ndarray, np.ndarray]:
    """``(x, y, cells)``: 40 % of the points alternate between four cells that share slot 5 of the device's cache (one of
    them owns it in a workgroup, the other three go to global memory), 60 % at random places fall into one hot cell,
    which shares that slot too or has slot 77.  ``cells``: the cell of every point."""
    cells_total = (len(xedges) - 1) * (len(yedges) - 1)
    assert cells_total >= 6 * SLOTS  # noqa: PLR2004
    rng = np.random.default_rng(n + seed)
    sharing = 5 + SLOTS * np.array([0, 1, 3, 4])
    hot = 5 + 5 * SLOTS if hot_shares_the_slot else 77 + 2 * SLOTS
    cells = sharing[np.arange(n) % 4]
    cells[rng.random(n) < 0.6] = hot  # noqa: PLR2004
    return (*cell_centres(cells, xedges, yedges), cells)


def oracle(x, y, xedges, yedges) -> tuple[np.ndarray, np.ndarray]:
    """``(counts, last)`` with numpy: ``histogram2d`` over the edges for the counts; for ``last``, ``maximum.at`` over
    ``searchsorted(edges, v, "right") - 1`` clipped to the last bin."""
    x, y = np.asarray(x, dtype=np.float64).reshape(-1), np.asarray(y, dtype=np.float64).reshape(-1)
    bins_x, bins_y = len(xedges) - 1, len(yedges) - 1
    both = ~(np.isnan(x) | np.isnan(y))
    counts = np.histogram2d(x[both], y[both], bins=(xedges, yedges))[0]
    assert np.array_equal(counts, counts.astype(np.uint64))
    inside = both & (x >= xedges[0]) & (x <= xedges[-1]) & (y >= yedges[0]) & (y <= yedges[-1])
    t = np.nonzero(inside)[0]
    ix = np.minimum(np.searchsorted(xedges, x[t], "right") - 1, bins_x - 1)
    iy = np.minimum(np.searchsorted(yedges, y[t], "right") - 1, bins_y - 1)
    last = np.full(bins_x * bins_y, -1, dtype=np.int64)
    np.maximum.at(last, ix * bins_y + iy, t)
    return counts.astype(np.uint64), np.where(last < 0, NONE, last.astype(np.uint64)).reshape(bins_x, bins_y)


def assert_cells(got, want, what="") -> None:
    """``(counts, last)`` against ``(counts, last)``: shape, dtype and every integer."""
    for name, a, b in zip(("counts", "last"), got, want):
        assert a.dtype == np.uint64 == b.dtype and a.shape == b.shape, (what, name, a.dtype, a.shape, b.shape)
        assert np.array_equal(a, b), (what, name, int((a != b).sum()), "cells differ")


def ani_like(n_genomes: int, seed: int = 0) -> tuple[np.ndarray, np.ndarray, np.ndarray]:
    """``(identity, coverage, lengths)`` of ``n_genomes`` genomes in clusters of about eight: identity 1.0 and coverage 1.0
    on the diagonal, high values within a cluster, low ones between, rounded to 10 decimals, a NaN here and there."""
    rng = np.random.default_rng(n_genomes + seed)
    cluster = np.arange(n_genomes) // 8
    same = cluster[:, None] == cluster[None, :]
    identity = np.where(same, 0.97 + 0.03 * rng.random((n_genomes, n_genomes)), 0.75 + 0.1 * rng.random((n_genomes, n_genomes)))
    coverage = np.where(same, 0.8 + 0.2 * rng.random((n_genomes, n_genomes)), 0.4 * rng.random((n_genomes, n_genomes)))
    np.fill_diagonal(identity, 1.0)
    np.fill_diagonal(coverage, 1.0)
    identity[rng.random(identity.shape) < 0.01] = np.nan  # noqa: PLR2004
    coverage[rng.random(coverage.shape) < 0.01] = np.nan  # noqa: PLR2004
    return np.round(identity, 10), np.round(coverage, 10), rng.integers(30_000, 9_000_000, n_genomes)
