"""plot-run's scatter figures without a GPU: the host twin of the 2-D binning against numpy, its argument checks,
``distribution.auto_histogram``, ``scatter.describe``, ``rundb.plot_run(scatter=True)`` on the viral fixture and the
figure."""

from __future__ import annotations

import logging
import sqlite3

import numpy as np
import pytest

from pyani_plus_amd import _capi, classify, distribution, run_comp, rundb, scatter
from pyani_plus_amd._capi import HipBackendError
from tests.distribution_cases import EDGE_FAMILIES, edge_values, kde_values, same_bits
from tests.fake_engine import OracleEngine
from tests.helpers import FIXTURE_SETS, GOLDEN
from tests.run_comp_cases import adversarial_values, numpy_hist
from tests.scatter_cases import GRIDS, LDS_CELLS, NONE, SLOTS, ani_like, assert_cells, edge_points, grid_edges, oracle, random_points

DEFAULT_NAMES = ["sourmash-hip_query_cov_scatter.tsv", "sourmash-hip_tANI_scatter.tsv"] + [
    f"sourmash-hip_{s}_heatmap.tsv" for s in ("identity", "query_cov", "hadamard", "tANI")
]
SCATTER_TABLES = [f"sourmash-hip_{y}_scatter_{what}.tsv" for y in ("query_cov", "tANI") for what in ("grid", "x_hist", "y_hist")]


# ------------------------------------------------------------------ the host twin
@pytest.mark.parametrize("grid", GRIDS, ids=lambda g: f"{g[0]}x{g[1]}")
def test_host_bin2d_equals_numpy(grid):
    xedges, yedges = grid_edges(*grid)
    for n in (1, 257, 20_011):
        x, y = random_points(n, xedges, yedges)
        before = (x.copy(), y.copy())
        got = scatter.bin2d_host(x, y, xedges, yedges)
        assert got[0].shape == grid
        assert_cells(got, oracle(x, y, xedges, yedges), f"n={n}")
        same_bits(x, before[0])
        same_bits(y, before[1])
    assert 0 < got[0].sum() < n and (got[1][got[0] == 0] == NONE).all() and (got[1][got[0] > 0] < n).all()


@pytest.mark.parametrize("grid", GRIDS, ids=lambda g: f"{g[0]}x{g[1]}")
def test_host_bin2d_on_the_edges_with_nan_and_outside(grid):
    xedges, yedges = grid_edges(*grid, seed=1)
    x, y = edge_points(xedges, yedges)
    assert np.isnan(x).sum() == 2 == np.isnan(y).sum() and (np.isnan(x) & np.isnan(y)).sum() == 1  # noqa: PLR2004
    assert (x < xedges[0]).any() and (x > xedges[-1]).any() and (y < yedges[0]).any() and (y > yedges[-1]).any()
    assert_cells(scatter.bin2d_host(x, y, xedges, yedges), oracle(x, y, xedges, yedges))
    nan = np.full(10, np.nan)
    for a, b in ((nan, np.full(10, yedges[0])), (np.full(10, xedges[0]), nan), (nan, nan)):
        counts, last = scatter.bin2d_host(a, b, xedges, yedges)
        assert not counts.any() and (last == NONE).all()
    # the corners belong to the first and the last cell
    counts, last = scatter.bin2d_host([xedges[0], xedges[-1]], [yedges[0], yedges[-1]], xedges, yedges)
    assert counts[0, 0] >= 1 and counts[-1, -1] >= 1 and counts.sum() == 2 and last[-1, -1] == 1  # noqa: PLR2004


def test_host_bin2d_of_no_points_and_arguments():
    ok = np.linspace(0.0, 1.0, 5)
    counts, last = scatter.bin2d_host([], [], ok, np.linspace(0, 1, 3))
    assert counts.shape == (4, 2) == last.shape and not counts.any() and (last == NONE).all()
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
            scatter.bin2d_host([0.5], [0.5], xedges, yedges)
    with pytest.raises(ValueError, match="2 x values and 1 y values"):
        scatter.bin2d_host([0.5, 0.5], [0.5], ok, ok)
    with pytest.raises(ValueError, match="expected at least two"):
        scatter.bin2d_host([0.5], [0.5], ok, [0.5])
    # too many points: refused before any of them is read (the arrays hold one)
    lib = _capi.load_library()
    one, cells = np.array([0.5]), np.zeros((2, 16), dtype=np.uint64)
    for n, status in (((1 << 32) - 1, -1), (1 << 40, -1)):
        assert lib.pa_bin2d_f64_host(one.ctypes.data, one.ctypes.data, n, ok.ctypes.data, 4, ok.ctypes.data, 4, cells[0].ctypes.data, cells[1].ctypes.data) != _capi.PA_OK
        assert f"{n} points; at most 2^32 - 2" in _capi.last_error() and status
    assert lib.pa_bin2d_f64_host(None, None, 1, ok.ctypes.data, 4, ok.ctypes.data, 4, cells[0].ctypes.data, cells[1].ctypes.data) != _capi.PA_OK
    assert "null argument" in _capi.last_error()


def test_host_bin2d_summed_over_y_is_the_histogram_of_x():
    """The 1-D and the 2-D use of the one bin rule: with a y range that holds every point, the cells of a column add up
    to the histogram of x."""
    xedges, yedges = run_comp.hist_edges(0.1, 0.7, 3), run_comp.hist_edges(-1.0, 2.0, 2)
    x = np.resize(np.concatenate([adversarial_values(xedges), [np.nan, -3.0, 3.0]]), 257)
    y = np.random.default_rng(257).random(257)
    cells, _last = scatter.bin2d_host(x, y, xedges, yedges)
    assert cells.shape == (3, 2) and cells.min() > 0
    assert np.array_equal(cells.sum(axis=1), run_comp.hist_uniform_host(x, xedges)) and np.array_equal(cells.sum(axis=1), numpy_hist(x, xedges))


def test_the_binding_states_the_library_constants():
    header = (GOLDEN.parent.parent / "include" / "pyani_hip.h").read_text()
    # the binding reads the header, so each value is pinned here, against both
    for name, value in (("PA_BIN2D_MAX_BINS", 1024), ("PA_BIN2D_LDS_CELLS", 4096), ("PA_BIN2D_SLOTS", 2048)):
        assert getattr(_capi, name) == value and f"#define {name} {value}\n" in header, name
    assert "#define PA_BIN2D_NONE 0xFFFFFFFFFFFFFFFFULL\n" in header and _capi.PA_BIN2D_NONE == 2**64 - 1
    assert "#define PA_ABI_VERSION 5\n" in header
    assert SLOTS & (SLOTS - 1) == 0 and LDS_CELLS < scatter.GRID**2 <= scatter.MAX_BINS**2


# ------------------------------------------------------------------ the margins
@pytest.mark.parametrize("family", EDGE_FAMILIES)
def test_auto_histogram_equals_numpy(family):
    for n in (1, 2, 5, 257, 3000):
        x = edge_values(family, n)
        hist = distribution.auto_histogram(x)
        counts, edges = np.histogram(x, "auto")
        assert (hist.n, hist.lo, hist.hi) == (n, x.min(), x.max()) and np.array_equal(hist.counts, counts)
        same_bits(hist.edges, edges)
    with pytest.raises(ValueError, match="no value that is not NaN"):
        distribution.auto_histogram([np.nan, np.nan])


def test_describe_of_a_distribution_is_unchanged():
    x = kde_values("nan", 3000)
    dist, hist = distribution.describe(x), distribution.auto_histogram(x)
    assert (dist.n, dist.lo, dist.hi) == (hist.n, hist.lo, hist.hi) and np.array_equal(dist.counts, hist.counts) and len(dist.density) == 200  # noqa: PLR2004
    same_bits(dist.edges, hist.edges)
    same_bits(dist.edges, np.histogram_bin_edges(x[~np.isnan(x)], "auto"))


# ------------------------------------------------------------------ describe
def check_scatter(data: scatter.Scatter, x, y, lengths, bins: int) -> None:
    """Every field re-derived with numpy from the matrices."""
    n = len(lengths)
    x, y = np.asarray(x, dtype=float).reshape(-1), np.asarray(y, dtype=float).reshape(-1)
    valid = ~(np.isnan(x) | np.isnan(y))
    assert (data.n_valid, data.n_total) == (int(valid.sum()), n * n) and data.counts.sum() == data.n_valid
    same_bits(data.xedges, np.linspace(x[valid].min(), x[valid].max(), bins + 1) if x[valid].min() < x[valid].max() else np.linspace(x[valid][0] - 0.5, x[valid][0] + 0.5, bins + 1))
    same_bits(data.yedges, np.linspace(y[valid].min(), y[valid].max(), bins + 1) if y[valid].min() < y[valid].max() else np.linspace(y[valid][0] - 0.5, y[valid][0] + 0.5, bins + 1))
    assert_cells((data.counts, data.last), oracle(np.where(valid, x, np.nan), np.where(valid, y, np.nan), data.xedges, data.yedges))
    seen = data.counts > 0
    # every last point lies inside its cell
    t = data.last[seen].astype(np.int64)
    ix, iy = np.nonzero(seen)
    assert valid[t].all()
    assert ((x[t] >= data.xedges[ix]) & (x[t] <= data.xedges[ix + 1]) & (y[t] >= data.yedges[iy]) & (y[t] <= data.yedges[iy + 1])).all()
    assert (data.last[~seen] == NONE).all() and np.isnan(data.colour[~seen]).all()
    assert np.array_equal(data.colour[seen], np.asarray(lengths)[t // n])
    rows = valid.reshape(n, n).any(1)
    assert (data.c_min, data.c_max) == (np.asarray(lengths)[rows].min(), np.asarray(lengths)[rows].max())
    for hist, v in ((data.x_hist, x[valid]), (data.y_hist, y[valid])):
        counts, edges = np.histogram(v, "auto")
        assert np.array_equal(hist.counts, counts)
        same_bits(hist.edges, edges)


@pytest.mark.parametrize("bins", (scatter.GRID, 1, 7, 1024))
def test_describe_on_the_host(bins):
    identity, coverage, lengths = ani_like(60)
    check_scatter(scatter.describe(identity, coverage, lengths, 60, bins=bins), identity, coverage, lengths, bins)


def test_describe_edge_cases_and_arguments():
    identity, coverage, lengths = ani_like(16)
    # a query without a valid point does not stretch the colour scale
    lengths[5] = 10**9
    coverage[5, :] = np.nan
    data = scatter.describe(identity, coverage, lengths, 16)
    assert data.c_max < 10**9
    check_scatter(data, identity, coverage, lengths, scatter.GRID)
    # one point: both ranges are widened by 0.5
    one = scatter.describe([[0.75]], [[0.25]], [1234], 1)
    assert (one.n_valid, one.c_min, one.c_max) == (1, 1234.0, 1234.0) and one.xedges[[0, -1]].tolist() == [0.25, 1.25] and one.yedges[[0, -1]].tolist() == [-0.25, 0.75]
    assert one.counts.sum() == 1 and one.last[one.counts > 0].tolist() == [0] and one.x_hist.edges.tolist() == [0.25, 1.25]
    nan = np.full((2, 2), np.nan)
    assert scatter.describe(nan, np.ones((2, 2)), [1, 2], 2) is None and scatter.describe([[np.nan, 1.0], [1.0, 1.0]], [[1.0, np.nan], [np.nan, np.nan]], [1, 2], 2) is None
    for bins in (0, 1025):
        with pytest.raises(ValueError, match="cells per axis; 1 to 1024"):
            scatter.describe(identity, coverage, lengths, 16, bins=bins)
    with pytest.raises(ValueError, match="lengths for 16 queries"):
        scatter.describe(identity, coverage, lengths[:3], 16)
    with pytest.raises(ValueError, match="for 15 x 15 points"):
        scatter.describe(identity, coverage, lengths[:15], 15)


def test_describe_on_the_viral_fixture(viral_db):
    matrices, lengths = fixture_matrices(viral_db)
    for name in ("query_cov", "tANI"):
        data = scatter.describe(matrices["identity"], matrices[name], lengths, 3)
        assert (data.n_valid, data.n_total) == (9, 9) and (data.c_min, data.c_max) == (min(lengths), max(lengths)) and data.counts.sum() == 9  # noqa: PLR2004
        check_scatter(data, matrices["identity"], matrices[name], lengths, scatter.GRID)


# ------------------------------------------------------------------ rundb.plot_run
@pytest.fixture(scope="module")
def viral_db(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("plot_run_scatter_db")
    scaled, _genomes = FIXTURE_SETS["viral_example"]
    db = tmp / "run.sqlite"
    assert rundb.run_sourmash_hip(GOLDEN / "viral_example", db, cache=tmp / "cache", scaled=scaled, engine=OracleEngine(), temp=tmp).status == "Done"
    return db


def fixture_matrices(db) -> tuple[dict, list[int]]:
    """The label-sorted (by stem) cached matrices of run 1, tANI among them, and the query length of every row."""
    from io import StringIO

    import pandas as pd

    conn = sqlite3.connect(db)
    cached = conn.execute("SELECT df_identity, df_cov_query, df_hadamard FROM runs WHERE run_id = 1").fetchone()
    stems = {h: rundb.filename_stem(f) for h, f in conn.execute("SELECT genome_hash, fasta_filename FROM runs_genomes WHERE run_id = 1")}
    length = {stems[h]: n for h, n in conn.execute("SELECT genome_hash, length FROM genomes") if h in stems}
    conn.close()
    frames = [pd.read_json(StringIO(c), orient="split", dtype=float).rename(index=stems, columns=stems).sort_index(axis=0).sort_index(axis=1) for c in cached]
    matrices = {name: f.to_numpy(dtype=float) for name, f in zip(("identity", "query_cov", "hadamard"), frames)}
    matrices["tANI"] = -classify.tani_scores(matrices["hadamard"])
    return matrices, [length[s] for s in frames[0].index]


def read_rows(path) -> tuple[str, np.ndarray]:
    header, *lines = path.read_text().split("\n")[:-1]
    return header, np.array([[float(f) for f in line.split("\t")] for line in lines]).reshape(len(lines), -1)


def check_grid_table(path, x, y, lengths, bins: int) -> None:
    """The rows of a grid table re-derived from the matrices with numpy."""
    x, y = np.asarray(x).reshape(-1), np.asarray(y).reshape(-1)
    valid = ~(np.isnan(x) | np.isnan(y))
    xm, ym = np.where(valid, x, np.nan), np.where(valid, y, np.nan)
    xedges, yedges = np.histogram_bin_edges(x[valid], bins), np.histogram_bin_edges(y[valid], bins)
    counts, last = oracle(xm, ym, xedges, yedges)
    ix, iy = np.nonzero(counts)  # x-major
    header, rows = read_rows(path)
    assert header == "#x_left\tx_right\ty_left\ty_right\tcount\tquery_length" and len(rows) == len(ix) > 0
    for column, want in enumerate((xedges[ix], xedges[ix + 1], yedges[iy], yedges[iy + 1])):
        same_bits(rows[:, column], want)
    assert np.array_equal(rows[:, 4], counts[ix, iy]) and rows[:, 4].sum() == valid.sum()
    assert np.array_equal(rows[:, 5], np.asarray(lengths)[last[ix, iy].astype(np.int64) // len(lengths)])


def test_plot_run_scatter_tables(viral_db, tmp_path, caplog):
    caplog.set_level(logging.INFO)
    plain = rundb.plot_run(viral_db, tmp_path / "plain")
    off = rundb.plot_run(viral_db, tmp_path / "off", scatter=False, scatter_bins=7)
    written = rundb.plot_run(viral_db, tmp_path / "out", scatter=True)
    # the default call is what it was: the same files in the same order with the same bytes, and the flag adds to its end
    assert [p.name for p in plain] == [p.name for p in off] == [p.name for p in written[:6]] and sorted(p.name for p in plain) == sorted(DEFAULT_NAMES)
    assert sorted(p.name for p in (tmp_path / "plain").iterdir()) == sorted(DEFAULT_NAMES)
    for p in plain:
        assert p.read_bytes() == (tmp_path / "off" / p.name).read_bytes() == (tmp_path / "out" / p.name).read_bytes()
    assert [p.name for p in written[6:]] == SCATTER_TABLES and sorted(p.name for p in (tmp_path / "out").iterdir()) == sorted(DEFAULT_NAMES + SCATTER_TABLES)
    assert f"Wrote 12 images to {tmp_path / 'out'}/sourmash-hip_*.*" in caplog.text
    matrices, lengths = fixture_matrices(viral_db)
    for name in ("query_cov", "tANI"):
        check_grid_table(tmp_path / "out" / f"sourmash-hip_{name}_scatter_grid.tsv", matrices["identity"], matrices[name], lengths, scatter.GRID)
        for axis, values in (("x", matrices["identity"]), ("y", matrices[name])):
            header, rows = read_rows(tmp_path / "out" / f"sourmash-hip_{name}_scatter_{axis}_hist.tsv")
            counts, edges = np.histogram(values.reshape(-1), "auto")
            assert header == "#left\tright\tcount" and np.array_equal(rows[:, 2], counts)
            same_bits(rows[:, 0], edges[:-1])
            same_bits(rows[:, 1], edges[1:])
    # another raster
    rundb.plot_run(viral_db, tmp_path / "seven", scatter=True, scatter_bins=7)
    check_grid_table(tmp_path / "seven" / "sourmash-hip_tANI_scatter_grid.tsv", matrices["identity"], matrices["tANI"], lengths, 7)
    for bins in (0, 1025):
        with pytest.raises(SystemExit):
            rundb.plot_run(viral_db, tmp_path / "bad", scatter=True, scatter_bins=bins)
    assert "--scatter-bins 1025: expected 1 to 1024" in caplog.text
    # the command line form
    assert rundb.main(["plot-run", "-d", str(viral_db), "-o", str(tmp_path / "cli"), "--scatter"]) == 0
    assert rundb.main(["plot-run", "-d", str(viral_db), "-o", str(tmp_path / "cli7"), "--scatter", "--scatter-bins", "7"]) == 0
    for name in SCATTER_TABLES:
        assert (tmp_path / "cli" / name).read_bytes() == (tmp_path / "out" / name).read_bytes()
        assert (tmp_path / "cli7" / name).read_bytes() == (tmp_path / "seven" / name).read_bytes()
    assert rundb.main(["plot-run", "-d", str(viral_db), "-o", str(tmp_path / "cli_off")]) == 0
    assert sorted(p.name for p in (tmp_path / "cli_off").iterdir()) == sorted(DEFAULT_NAMES)


def test_plot_run_scatter_with_other_labels(viral_db, tmp_path):
    stem = rundb.plot_run(viral_db, tmp_path / "stem", scatter=True)
    for label in ("md5", "filename"):
        written = rundb.plot_run(viral_db, tmp_path / label, scatter=True, label=label)
        assert [p.name for p in written] == [p.name for p in stem]
        for p in written[7:9]:  # the margins do not depend on the order of the rows
            assert p.read_bytes() == (tmp_path / "stem" / p.name).read_bytes()
        _header, rows = read_rows(written[6])
        assert rows[:, 4].sum() == 9  # noqa: PLR2004


def test_plot_run_scatter_figures(viral_db, tmp_path):
    pytest.importorskip("matplotlib")
    written = rundb.plot_run(viral_db, tmp_path / "out", formats=("tsv", "png"), scatter=True)
    pngs = [p for p in written if p.suffix == ".png"]
    assert [p.name for p in pngs[4:]] == ["sourmash-hip_query_cov_scatter.png", "sourmash-hip_tANI_scatter.png"] and len(pngs) == 6  # noqa: PLR2004
    assert all(p.read_bytes()[:8] == b"\x89PNG\r\n\x1a\n" and p.stat().st_size > 1000 for p in pngs)  # noqa: PLR2004
    assert [p.name for p in written[10:]] == [*SCATTER_TABLES[:3], pngs[4].name, *SCATTER_TABLES[3:], pngs[5].name]
    only = rundb.plot_run(viral_db, tmp_path / "png_only", formats=("png",), scatter=True)
    assert [p.name for p in only] == [p.name for p in pngs] == sorted((p.name for p in (tmp_path / "png_only").iterdir()), key=[p.name for p in pngs].index)
    # without the flag: exactly the four heatmaps
    assert len(rundb.plot_run(viral_db, tmp_path / "plain", formats=("png",))) == 4  # noqa: PLR2004


def test_scatter_figure_holds_what_was_computed():
    pytest.importorskip("matplotlib")
    import matplotlib.pyplot as plt

    from pyani_plus_amd import scatter_figure

    identity, coverage, lengths = ani_like(60)
    data = scatter.describe(identity, coverage, lengths, 60, bins=64)
    figure = scatter_figure.scatter_figure(data, "Query coverage")
    try:
        axes = {ax.get_label(): ax for ax in figure.axes}
        assert sorted(axes) == ["colour bar", "joint", "x margin", "y margin"] and tuple(figure.get_size_inches()) == (6.0, 6.0)
        joint = axes["joint"]
        assert (joint.get_xlabel(), joint.get_ylabel()) == ("Percent identity (ANI)", "Query coverage") and axes["colour bar"].get_ylabel() == "Query length (bp)"
        (mesh,) = joint.collections
        image = np.ma.masked_invalid(data.colour.T)
        drawn = np.ma.asarray(mesh.get_array()).reshape(image.shape)
        assert np.array_equal(np.ma.getmaskarray(drawn), np.ma.getmaskarray(image)) and np.array_equal(drawn.compressed(), image.compressed())
        assert int((~np.ma.getmaskarray(drawn)).sum()) == int((data.counts > 0).sum()) > 10  # noqa: PLR2004
        assert (mesh.norm.vmin, mesh.norm.vmax) == (data.c_min, data.c_max) and mesh.get_cmap().name == "viridis"
        assert joint.get_xlim() == (data.xedges[0], data.xedges[-1]) and joint.get_ylim() == (data.yedges[0], data.yedges[-1])
        assert np.allclose(axes["colour bar"].get_position().bounds, (0.85, 0.25, 0.05, 0.4))
        bounds = [axes[k].get_position() for k in ("joint", "x margin", "y margin")]
        assert np.isclose(bounds[0].x0, 0.2) and np.isclose(bounds[0].y0, 0.2) and np.isclose(bounds[2].x1, 0.8) and np.isclose(bounds[1].y1, 0.8)
        for key, hist in (("x margin", data.x_hist), ("y margin", data.y_hist)):
            (stairs,) = axes[key].patches
            values, edges, _baseline = stairs.get_data()
            assert np.array_equal(values, hist.counts) and np.array_equal(edges, hist.edges)
    finally:
        plt.close(figure)


def edited_copy(db, path, *statements):
    path.write_bytes(db.read_bytes())
    conn = sqlite3.connect(path)
    for statement in statements:
        conn.execute(statement)
    conn.execute("UPDATE runs SET df_identity = NULL, df_cov_query = NULL, df_hadamard = NULL")
    conn.commit()
    conn.close()
    return path


def test_plot_run_scatter_of_an_all_null_run(viral_db, tmp_path, caplog):
    copy = edited_copy(viral_db, tmp_path / "nulls.sqlite", "UPDATE comparisons SET identity = NULL, cov_query = NULL")
    for formats in (("tsv",), ("png",), ("tsv", "png")):
        caplog.clear()
        assert rundb.plot_run(copy, tmp_path / "-".join(formats), formats=formats, scatter=True) == []
        assert caplog.text.count("No valid identity, Query coverage values from sourmash-hip run") == 1 and "No valid identity, tANI" not in caplog.text
        assert list((tmp_path / "-".join(formats)).iterdir()) == []
    # some cells NULL: they are left out
    copy = edited_copy(viral_db, tmp_path / "some.sqlite", "UPDATE comparisons SET identity = NULL WHERE comparison_id = (SELECT MIN(comparison_id) FROM comparisons WHERE query_hash != subject_hash)")
    written = rundb.plot_run(copy, tmp_path / "some", scatter=True)
    _header, rows = read_rows(written[6])
    assert rows[:, 4].sum() == 8  # noqa: PLR2004


def test_plot_run_scatter_with_a_zero_hadamard_cell(viral_db, tmp_path, caplog):
    copy = edited_copy(viral_db, tmp_path / "zero.sqlite", "UPDATE comparisons SET cov_query = 0.0 WHERE comparison_id = (SELECT MIN(comparison_id) FROM comparisons WHERE query_hash != subject_hash)")
    written = rundb.plot_run(copy, tmp_path / "out", scatter=True)
    assert "1 sourmash-hip comparisons have a zero Hadamard product" in caplog.text
    assert [p.name for p in written[6:]] == SCATTER_TABLES
    counts = {p.name: read_rows(p)[1][:, 4 if "grid" in p.name else 2].sum() for p in written[6:]}
    assert [counts[name] for name in SCATTER_TABLES] == [9, 9, 9, 8, 8, 8]  # tANI of the zero cell is NaN: the point drops out


def test_plot_run_scatter_of_a_single_genome(tmp_path):
    fasta = tmp_path / "one"
    fasta.mkdir()
    (fasta / "OP073605.fasta").write_bytes((GOLDEN / "viral_example" / "OP073605.fasta").read_bytes())
    db = tmp_path / "one.sqlite"
    assert rundb.run_sourmash_hip(fasta, db, cache=tmp_path / "cache", scaled=300, engine=OracleEngine(), temp=tmp_path).status == "Done"
    written = rundb.plot_run(db, tmp_path / "out", scatter=True, scatter_bins=2)
    assert len(written) == 6 + 6
    conn = sqlite3.connect(db)
    (length,) = conn.execute("SELECT length FROM genomes").fetchone()
    conn.close()
    # one point at (1, 1) and at (1, -0.0): the ranges are widened by 0.5 each way, the point is on the middle edge
    assert (tmp_path / "out" / "sourmash-hip_query_cov_scatter_grid.tsv").read_text() == f"#x_left\tx_right\ty_left\ty_right\tcount\tquery_length\n1.0\t1.5\t1.0\t1.5\t1\t{length}\n"
    assert (tmp_path / "out" / "sourmash-hip_tANI_scatter_grid.tsv").read_text() == f"#x_left\tx_right\ty_left\ty_right\tcount\tquery_length\n1.0\t1.5\t0.0\t0.5\t1\t{length}\n"
    assert (tmp_path / "out" / "sourmash-hip_tANI_scatter_x_hist.tsv").read_text() == "#left\tright\tcount\n0.5\t1.5\t1\n"
    assert (tmp_path / "out" / "sourmash-hip_tANI_scatter_y_hist.tsv").read_text() == "#left\tright\tcount\n-0.5\t0.5\t1\n"


# ------------------------------------------------------------------ the host code under sanitizers
def test_host_twin_under_sanitizers():
    """AddressSanitizer + UBSan over ``scatter_host.cpp`` in a stand-alone CPU program: random points with NaNs, values
    outside and on the edges in exact-size buffers, grids of up to 1024 bins an axis, checked against a search of the edges."""
    import shutil
    import subprocess
    from pathlib import Path

    if shutil.which("g++") is None:
        pytest.skip("no host compiler")
    script = Path(__file__).resolve().parent / "tools" / "sanitize" / "run_scatter.sh"
    done = subprocess.run(["bash", str(script), "300"], capture_output=True, text=True, timeout=600)
    assert done.returncode == 0 and "sanitizer runs clean" in done.stdout, done.stdout[-2000:] + done.stderr[-2000:]
    assert "MISMATCH" not in done.stdout
