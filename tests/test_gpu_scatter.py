"""plot-run's scatter figures on the GPU: ``pa_bin2d_f64`` against its host twin and numpy over both of its regimes, the
boundary between them, one hot cell, cells that fight for one slot of the cache, edges and NaN; ``scatter.describe``
and ``rundb.plot_run(scatter=True)`` through the device against the host.  Every comparison is of integers or bits."""

from __future__ import annotations

import numpy as np
import pytest

from pyani_plus_amd import rundb, scatter
from pyani_plus_amd._capi import HipBackendError
from tests.distribution_cases import same_bits
from tests.helpers import FIXTURE_SETS, GOLDEN
from tests.scatter_cases import (
    BOUNDARY_GRIDS,
    DEVICE_GRIDS,
    DEVICE_SIZES,
    LDS_CELLS,
    NONE,
    SLOTS,
    ani_like,
    assert_cells,
    edge_points,
    grid_edges,
    oracle,
    random_points,
    slot_conflict_points,
)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def engine():
    from pyani_plus_amd.engine import HipEngine

    eng = HipEngine(0)
    yield eng
    eng.close()


def on_device(engine, values):
    return engine.torch.from_numpy(np.ascontiguousarray(values, dtype=np.float64)).to(engine.device)


# ------------------------------------------------------------------ the kernel
@pytest.mark.parametrize("grid", DEVICE_GRIDS, ids=lambda g: f"{g[0]}x{g[1]}")
def test_bin2d_equals_host_twin_and_numpy(engine, grid):
    xedges, yedges = grid_edges(*grid)
    for n in DEVICE_SIZES:
        x, y = random_points(n, xedges, yedges)
        d_x, d_y = on_device(engine, x), on_device(engine, y)
        got = engine.bin2d(d_x, d_y, xedges, yedges)
        assert got[0].shape == grid
        assert_cells(got, scatter.bin2d_host(x, y, xedges, yedges), f"host twin, n={n}")
        assert_cells(got, oracle(x, y, xedges, yedges), f"numpy, n={n}")
        # the inputs are read, never written
        same_bits(d_x.cpu().numpy(), x)
        same_bits(d_y.cpu().numpy(), y)
        if n == DEVICE_SIZES[-1]:
            assert_cells(engine.bin2d(d_x, d_y, xedges, yedges), got, "a second run")
            assert int(got[0].sum()) > n // 2


@pytest.mark.parametrize("grid", DEVICE_GRIDS, ids=lambda g: f"{g[0]}x{g[1]}")
def test_bin2d_on_the_edges_and_with_nan(engine, grid):
    xedges, yedges = grid_edges(*grid, seed=1)
    x, y = edge_points(xedges, yedges)
    got = engine.bin2d(x, y, xedges, yedges)
    assert_cells(got, scatter.bin2d_host(x, y, xedges, yedges), "host twin")
    assert_cells(got, oracle(x, y, xedges, yedges), "numpy")
    nan = np.full(100, np.nan)
    for a, b in ((nan, np.full(100, yedges[0])), (np.full(100, xedges[0]), nan), (nan, nan)):
        counts, last = engine.bin2d(a, b, xedges, yedges)
        assert not counts.any() and (last == NONE).all()


@pytest.mark.parametrize("grid", (BOUNDARY_GRIDS[0], (256, 256)), ids=("all cells in LDS", "cache"))
def test_bin2d_of_one_cell_many_times(engine, grid):
    n = 1 << 20
    xedges, yedges = grid_edges(*grid, seed=2)
    x, y = np.full(n, (xedges[3] + xedges[4]) / 2), np.full(n, (yedges[-2] + yedges[-1]) / 2)
    counts, last = engine.bin2d(x, y, xedges, yedges)
    assert counts[3, grid[1] - 1] == n == counts.sum() and last[3, grid[1] - 1] == n - 1
    assert int((last != NONE).sum()) == 1


@pytest.mark.parametrize("hot_shares_the_slot", (False, True))
def test_bin2d_with_cells_that_share_a_slot(engine, hot_shares_the_slot):
    n = 300_001
    xedges, yedges = grid_edges(256, 256, seed=3)
    x, y, cells = slot_conflict_points(n, xedges, yedges, hot_shares_the_slot)
    assert len({int(c) % SLOTS for c in np.unique(cells)}) == (1 if hot_shares_the_slot else 2) and len(np.unique(cells)) == 5  # noqa: PLR2004
    got = engine.bin2d(x, y, xedges, yedges)
    assert_cells(got, scatter.bin2d_host(x, y, xedges, yedges), "host twin")
    assert_cells(got, oracle(x, y, xedges, yedges), "numpy")
    assert np.array_equal(np.nonzero(got[0].reshape(-1))[0], np.unique(cells)) and got[0].sum() == n
    assert_cells(engine.bin2d(x, y, xedges, yedges), got, "a second run")


def test_bin2d_arguments(engine):
    ok = np.linspace(0.0, 1.0, 5)
    for xedges, yedges, message in (
        (np.linspace(0, 1, 1026), ok, "1025 x bins; 1 to 1024"),
        (ok, np.linspace(0, 1, 1026), "1025 y bins; 1 to 1024"),
        ([0.0, np.inf], ok, "x edge 1 is not finite"),
        (ok, [0.0, np.nan, 1.0], "y edge 1 is not finite"),
        ([0.0, 0.5, 0.25, 1.0], ok, "x edge 2 is below edge 1"),
        (ok, [1.0, 0.0], "y edge 1 is below edge 0"),
        ([0.5, 0.5], ok, "the last x edge must be above the first"),
        (ok, [-1e308, 1e308], "the last y edge must be above the first and their difference finite"),
    ):  # fmt: skip
        with pytest.raises(HipBackendError, match=message):
            engine.bin2d([0.5], [0.5], xedges, yedges)
    with pytest.raises(ValueError, match="2 x values and 1 y values"):
        engine.bin2d([0.5, 0.5], [0.5], ok, ok)
    with pytest.raises(ValueError, match="expected at least two"):
        engine.bin2d([0.5], [0.5], [0.5], ok)
    counts, last = engine.bin2d([], [], ok, ok)
    assert counts.shape == (4, 4) and not counts.any() and (last == NONE).all()
    assert LDS_CELLS == 4096 and SLOTS == 2048  # noqa: PLR2004  (what DESIGN.md section 7f measures)


# ------------------------------------------------------------------ describe and plot_run
def assert_same_scatter(device: scatter.Scatter, host: scatter.Scatter) -> None:
    assert (device.n_valid, device.n_total, device.c_min, device.c_max) == (host.n_valid, host.n_total, host.c_min, host.c_max)
    for name in ("xedges", "yedges", "colour"):
        same_bits(getattr(device, name), getattr(host, name))
    assert_cells((device.counts, device.last), (host.counts, host.last))
    for a, b in ((device.x_hist, host.x_hist), (device.y_hist, host.y_hist)):
        assert (a.n, a.lo, a.hi) == (b.n, b.lo, b.hi) and np.array_equal(a.counts, b.counts)
        same_bits(a.edges, b.edges)


@pytest.mark.parametrize("bins", (scatter.GRID, 7))
def test_describe_through_the_device(engine, bins):
    identity, coverage, lengths = ani_like(300)
    host = scatter.describe(identity, coverage, lengths, 300, bins=bins)
    assert_same_scatter(scatter.describe(on_device(engine, identity), on_device(engine, coverage), lengths, 300, engine, bins), host)
    assert_same_scatter(scatter.describe(identity, coverage, lengths, 300, engine, bins), host)  # host arrays are uploaded
    assert host.counts.shape == (bins, bins) and 0 < host.n_valid < host.n_total == host.counts.sum() + (host.n_total - host.n_valid)
    nan = np.full((3, 3), np.nan)
    assert scatter.describe(on_device(engine, nan), on_device(engine, nan), lengths[:3], 3, engine) is None


def test_plot_run_scatter_on_the_device(engine, tmp_path):
    scaled, _genomes = FIXTURE_SETS["viral_example"]
    db = tmp_path / "run.sqlite"
    assert rundb.run_sourmash_hip(GOLDEN / "viral_example", db, cache=tmp_path / "cache", scaled=scaled, engine=engine, temp=tmp_path).status == "Done"
    host = rundb.plot_run(db, tmp_path / "host", scatter=True)
    device = rundb.plot_run(db, tmp_path / "device", scatter=True, engine=engine)
    assert [p.name for p in device] == [p.name for p in host] and len(host) == 6 + 6
    for a, b in zip(host, device):
        assert a.read_bytes() == b.read_bytes() and len(a.read_bytes()) > 20, a.name  # noqa: PLR2004
    default = rundb.plot_run(db, tmp_path / "default", engine=engine)
    assert [p.name for p in default] == [p.name for p in host[:6]] and sorted(p.name for p in default) == sorted(p.name for p in (tmp_path / "default").iterdir())
    for a, b in zip(host, default):
        assert a.read_bytes() == b.read_bytes(), a.name
