"""plot-run's distributions without a GPU: ``auto_bin_edges`` against ``numpy.histogram_bin_edges(x, "auto")`` in bits,
the host twins of csrc/dist.hip against numpy, scipy (where it imports) and the golden densities, and
``rundb.plot_run(distributions=True)`` on the viral fixture."""

from __future__ import annotations

import logging
import sqlite3

import numpy as np
import pytest

from pyani_plus_amd import _capi, distribution, rundb
from pyani_plus_amd._capi import HipBackendError
from tests.distribution_cases import (
    ATOL_SCIPY,
    CHAIN,
    EDGE_FAMILIES,
    EDGE_RANDOM_SIZES,
    EDGE_SMALL_SIZES,
    RTOL_SCIPY,
    SELECT_KINDS,
    SELECT_SIZES,
    WIDE_BINS,
    close,
    edge_values,
    edges_from_sorted,
    golden_inputs,
    golden_specs,
    kde_grid,
    kde_values,
    load_golden,
    numpy_hist,
    numpy_kde,
    same_bits,
    scott_bw,
    select_rank_sets,
    select_values,
    sorted_valid,
    values_md5,
    wide_inputs,
    worst,
)
from tests.fake_engine import OracleEngine
from tests.helpers import FIXTURE_SETS, GOLDEN

SCORES = ("identity", "query_cov", "hadamard", "tANI")
DEFAULT_NAMES = sorted([f"sourmash-hip_{s}_heatmap.tsv" for s in SCORES] + [f"sourmash-hip_{s}_scatter.tsv" for s in ("query_cov", "tANI")])
DIST_TABLES = sorted(f"sourmash-hip_{s}_dist_{kind}.tsv" for s in SCORES for kind in ("hist", "kde"))


# ------------------------------------------------------------------ the automatic bin rule
@pytest.mark.parametrize("family", EDGE_FAMILIES)
def test_auto_bin_edges_have_numpys_bits(family):
    for n in (*EDGE_SMALL_SIZES, *EDGE_RANDOM_SIZES):
        x = edge_values(family, n)
        same_bits(edges_from_sorted(x), np.histogram_bin_edges(x, "auto"))


def test_auto_bin_edges_rules_and_arguments():
    assert distribution.quartile_ranks(1) == (0, 0, 0, 0) and distribution.quartile_ranks(2) == (0, 1, 0, 1)
    assert distribution.quartile_ranks(5) == (1, 2, 3, 4) and distribution.quartile_ranks(8) == (1, 2, 5, 6)
    same_bits(distribution.auto_bin_edges(1, 0.75, 0.75, (0.75,) * 4), [0.25, 1.25])  # one value: one bin, widened
    # an interquartile range of 0 leaves Sturges' width alone: 10 values, ptp 1 -> ceil(log2(10) + 1) = 5 bins
    x = np.array([0.0] + [0.5] * 8 + [1.0])
    assert len(edges_from_sorted(x)) - 1 == 5 == len(np.histogram_bin_edges(x, "auto")) - 1  # noqa: PLR2004
    for bad in ((0, 0.0, 1.0), (3, 1.0, 0.0), (3, 0.0, np.inf), (3, np.nan, 1.0)):
        with pytest.raises(ValueError, match="finite ascending range"):
            distribution.auto_bin_edges(*bad, (0.0,) * 4)


# ------------------------------------------------------------------ host twins
@pytest.mark.parametrize("n", SELECT_SIZES)
def test_host_select_equals_numpy_sort(n):
    for kind in SELECT_KINDS:
        x = select_values(kind, n)
        want = sorted_valid(x)
        for ranks in select_rank_sets(len(want)):
            got = distribution.select_host(x, ranks)
            assert np.array_equal(got, want[ranks]), (kind, ranks)  # as values: -0.0 and 0.0 are one


def test_host_select_arguments():
    for x, ranks, message in (([np.nan, np.nan], [0], "rank 0 of 0 values"), ([1.0, np.nan, 2.0], [1, 2], "rank 2 of 2 values"), ([], [0], "rank 0 of 0")):
        with pytest.raises(HipBackendError, match=message) as caught:
            distribution.select_host(x, ranks)
        assert caught.value.status == -1  # PA_E_INVALID
    with pytest.raises(HipBackendError, match="9 ranks; at most 8"):
        distribution.select_host([1.0] * 20, list(range(9)))
    assert len(distribution.select_host([1.0], [])) == 0


@pytest.mark.parametrize("bins", WIDE_BINS)
def test_host_wide_histogram_equals_numpy(bins):
    v, edges = wide_inputs(bins)
    counts = distribution.hist_uniform_wide_host(v, edges)
    assert counts.dtype == np.uint64 and np.array_equal(counts, numpy_hist(v, edges))
    assert int(counts.sum()) == len(v) - 4 - 2  # two NaN, two outside; and the neighbours below the first and above the last edge


def test_host_wide_histogram_arguments():
    for bad, message in (([0.0, 0.5, 0.25, 1.0], "edge 2 is below edge 1"), ([0.0, np.inf], "edge 1 is not finite"), ([1.0, 1.0], "above the first")):
        with pytest.raises(HipBackendError, match=message):
            distribution.hist_uniform_wide_host([0.5], bad)
    assert distribution.hist_uniform_wide_host([], [0.0, 1.0]).tolist() == [0]


@pytest.mark.parametrize("n", (1, 2, 65, 3000, 100_003))
def test_host_moments(n):
    x = kde_values("nan" if n > 2 else "identity", n)  # noqa: PLR2004
    v = x[~np.isnan(x)]
    mean, squares = distribution.moments_host(x)
    assert mean == pytest.approx(v.mean(), rel=1e-13) and squares == pytest.approx(((v - v.mean()) ** 2).sum(), rel=1e-11, abs=1e-300)
    if len(v) > 1:
        scipy_stats = pytest.importorskip("scipy.stats")
        bw = np.sqrt(squares / (len(v) - 1)) * len(v) ** -0.2
        assert bw == pytest.approx(float(np.sqrt(scipy_stats.gaussian_kde(v).covariance[0, 0])), rel=1e-13)
    assert all(np.isnan(m) for m in distribution.moments_host(np.full(n, np.nan)))


def test_the_golden_file_covers_what_it_should():
    cases = load_golden()
    assert [c["name"] for c in cases] == [s["name"] for s in golden_specs()]
    assert (GOLDEN / "plot_run_dist" / "cases.json").stat().st_size < 200_000  # noqa: PLR2004
    assert {c["n"] for c in cases} >= {63, 64, 65, CHAIN - 1, CHAIN, CHAIN + 1, 100_003} and {c["n_grid"] for c in cases} == {1, 200, 1024}
    for case in cases:
        x, grid = golden_inputs(case)
        assert values_md5(x) == case["md5"] and len(grid) == case["n_grid"] == len(case["density"]), case["name"]
        if "bw_target" not in case:
            assert scott_bw(x) == pytest.approx(case["bw"], rel=1e-14), case["name"]
    clusters = next(c for c in cases if c["kind"] == "clusters")
    assert clusters["density"][100] == 0.0 and clusters["density"].max() > 50 and (clusters["density"] > 0).sum() > 20  # noqa: PLR2004
    through = next(c for c in cases if c.get("through_datum"))
    x, grid = golden_inputs(through)
    assert x[0] in grid and np.all(np.diff(grid) > 0)


@pytest.mark.parametrize("case", load_golden(), ids=lambda c: c["name"])
def test_host_density_equals_the_golden_case(case):
    x, grid = golden_inputs(case)
    got = distribution.kde_gauss_host(x, grid, case["bw"])
    assert close(got, case["density"], RTOL_SCIPY, ATOL_SCIPY), worst(got, case["density"])
    if case["n"] <= 3000:  # noqa: PLR2004
        assert close(got, numpy_kde(x, grid, case["bw"]), 16 * 2.0**-53, ATOL_SCIPY)  # the same terms, an all but exact sum


def test_host_density_against_scipy_and_arguments():
    scipy_stats = pytest.importorskip("scipy.stats")
    for n in (2, 64, CHAIN + 1):
        x = kde_values("identity", n, seed=1)
        bw = scott_bw(x)
        grid = kde_grid(x, bw, 200)
        got = distribution.kde_gauss_host(x, grid, bw)
        want = scipy_stats.gaussian_kde(x)(grid)
        assert close(got, want, RTOL_SCIPY, ATOL_SCIPY), (n, worst(got, want))
    for bw, message in ((0.0, "must be positive and finite"), (-1.0, "must be positive"), (np.inf, "positive and finite"), (np.nan, "positive and finite")):
        with pytest.raises(HipBackendError, match=message):
            distribution.kde_gauss_host([0.5, 0.6], [0.5], bw)
    for x, grid, message in (([0.5, np.inf], [0.5], "an infinite value"), ([np.nan], [0.5], "no value that is not NaN"), ([0.5], [np.nan], "grid point 0 is not finite"),
                             ([0.5], np.zeros(1025), "1025 grid points")):  # fmt: skip
        with pytest.raises(HipBackendError, match=message):
            distribution.kde_gauss_host(x, grid, 0.1)


def test_describe_on_the_host():
    x = kde_values("nan", 3000)
    v = x[~np.isnan(x)]
    dist = distribution.describe(x.reshape(60, 50))
    assert (dist.n, dist.lo, dist.hi) == (len(v), v.min(), v.max())
    same_bits(dist.edges, np.histogram_bin_edges(v, "auto"))
    assert np.array_equal(dist.counts, np.histogram(v, "auto")[0])
    assert dist.bw == pytest.approx(scott_bw(x), rel=1e-13) and len(dist.grid) == 200 == len(dist.density)  # noqa: PLR2004
    assert close(dist.density, numpy_kde(x, dist.grid, dist.bw), 16 * 2.0**-53)
    for flat in ([0.5], [0.5, np.nan, 0.5, 0.5]):
        dist = distribution.describe(flat)
        assert dist.bw is None and dist.grid is None and dist.density is None and dist.counts.tolist() == [dist.n] and dist.edges.tolist() == [0.0, 1.0]
    with pytest.raises(ValueError, match="no value that is not NaN"):
        distribution.describe([np.nan])
    edges, counts = distribution.rug_counts(x, "identity", distribution.describe(x))
    assert (edges[0], edges[-1], len(counts)) == (0.80, 1.01, 1024) and counts.sum() == ((v >= 0.80) & (v <= 1.01)).sum()  # noqa: PLR2004
    edges, counts = distribution.rug_counts(x, "query_cov", distribution.describe(x))
    assert (edges[0], edges[-1]) == (v.min(), v.max()) and counts.sum() == len(v)


def test_the_binding_states_the_library_constants():
    header = (GOLDEN.parent.parent / "include" / "pyani_hip.h").read_text()
    # the binding reads the header, so each value is pinned here, against both
    for name, value in (("PA_SELECT_MAX_RANKS", 8), ("PA_KDE_CHAIN", 2048), ("PA_HIST_WIDE_LDS_BINS", 8192)):
        assert getattr(_capi, name) == value and f"#define {name} {value}\n" in header, name
    assert distribution.kde_tree_depth(1, 1) == 10 and distribution.kde_tree_depth(100_003, 200) == 2 + 4 and distribution.kde_tree_depth(CHAIN + 1, 1024) == 1  # noqa: PLR2004


# ------------------------------------------------------------------ rundb.plot_run
@pytest.fixture(scope="module")
def viral_db(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("plot_run_dist_db")
    scaled, _genomes = FIXTURE_SETS["viral_example"]
    db = tmp / "run.sqlite"
    assert rundb.run_sourmash_hip(GOLDEN / "viral_example", db, cache=tmp / "cache", scaled=scaled, engine=OracleEngine(), temp=tmp).status == "Done"
    return db


def read_rows(path) -> tuple[str, np.ndarray]:
    header, *lines = path.read_text().split("\n")[:-1]
    return header, np.array([[float(f) for f in line.split("\t")] for line in lines])


def test_plot_run_default_is_unchanged(viral_db, tmp_path, caplog):
    caplog.set_level(logging.INFO)
    written = rundb.plot_run(viral_db, tmp_path / "out")
    assert sorted(p.name for p in written) == DEFAULT_NAMES == sorted(p.name for p in (tmp_path / "out").iterdir())
    assert f"Wrote 6 images to {tmp_path / 'out'}/sourmash-hip_*.*" in caplog.text
    assert rundb.plot_run(viral_db, tmp_path / "off", distributions=False) == [tmp_path / "off" / p.name for p in written]


def test_plot_run_distribution_tables(viral_db, tmp_path, caplog):
    import pandas as pd

    caplog.set_level(logging.INFO)
    written = rundb.plot_run(viral_db, tmp_path / "out", distributions=True)
    assert sorted(p.name for p in written) == sorted(DEFAULT_NAMES + DIST_TABLES) == sorted(p.name for p in (tmp_path / "out").iterdir())
    assert f"Wrote 14 images to {tmp_path / 'out'}/sourmash-hip_*.*" in caplog.text
    for score in SCORES:
        cells = pd.read_csv(tmp_path / "out" / f"sourmash-hip_{score}_heatmap.tsv", sep="\t", index_col=0, float_precision="round_trip").to_numpy(dtype=float).reshape(-1)
        header, rows = read_rows(tmp_path / "out" / f"sourmash-hip_{score}_dist_hist.tsv")
        edges = np.histogram_bin_edges(cells, "auto")
        assert header == "#left\tright\tcount"
        same_bits(rows[:, 0], edges[:-1])
        same_bits(rows[:, 1], edges[1:])
        assert np.array_equal(rows[:, 2], np.histogram(cells, "auto")[0]) and rows[:, 2].sum() == 9  # noqa: PLR2004
        header, rows = read_rows(tmp_path / "out" / f"sourmash-hip_{score}_dist_kde.tsv")
        bw = scott_bw(cells)
        assert header == "#x\tdensity" and rows.shape == (200, 2)
        assert close(rows[:, 0], np.linspace(cells.min() - 3 * bw, cells.max() + 3 * bw, 200), 1e-13, 1e-15)
        assert close(rows[:, 1], numpy_kde(cells, rows[:, 0], bw), RTOL_SCIPY, ATOL_SCIPY), score
    # the command line form
    assert rundb.main(["plot-run", "-d", str(viral_db), "-o", str(tmp_path / "cli"), "--distributions"]) == 0
    for name in DIST_TABLES:
        assert (tmp_path / "cli" / name).read_bytes() == (tmp_path / "out" / name).read_bytes()
    assert rundb.main(["plot-run", "-d", str(viral_db), "-o", str(tmp_path / "cli_off")]) == 0
    assert sorted(p.name for p in (tmp_path / "cli_off").iterdir()) == DEFAULT_NAMES


def test_plot_run_distribution_figures(viral_db, tmp_path):
    pytest.importorskip("matplotlib")
    written = rundb.plot_run(viral_db, tmp_path / "out", formats=("tsv", "png"), distributions=True)
    pngs = [p for p in written if p.suffix == ".png"]
    assert sorted(p.name for p in pngs) == sorted(f"sourmash-hip_{s}_{what}.png" for s in SCORES for what in ("heatmap", "dist"))
    assert all(p.read_bytes()[:8] == b"\x89PNG\r\n\x1a\n" and p.stat().st_size > 1000 for p in pngs)  # noqa: PLR2004
    assert len(written) == 6 + 4 + 8 + 4
    only = rundb.plot_run(viral_db, tmp_path / "png_only", formats=("png",), distributions=True)
    assert sorted(p.name for p in only) == sorted(p.name for p in pngs)


def test_distribution_figure_holds_what_was_computed():
    pytest.importorskip("matplotlib")
    import matplotlib.pyplot as plt

    from pyani_plus_amd import distribution_figure

    x = kde_values("identity", 3000)
    dist = distribution.describe(x)
    rug = distribution.rug_counts(x, "identity", dist)
    figure = distribution_figure.distribution_figure(dist, rug, "identity")
    try:
        left, right = figure.axes
        assert tuple(figure.get_size_inches()) == (15.0, 5.0) and figure.get_suptitle() == "identity distribution"
        assert left.get_xlim() == right.get_xlim() == (0.80, 1.01) and left.get_ylim()[0] == 0
        (curve,) = right.get_lines()
        assert np.array_equal(curve.get_xdata(), dist.grid) and np.array_equal(curve.get_ydata(), dist.density)
        (lines,) = [c for c in right.collections if c.get_label() == "rug"]
        assert len(lines.get_segments()) == int((rug[1] > 0).sum()) <= 1024  # noqa: PLR2004
        alpha = lines.get_colors()[:, 3]
        assert np.allclose(alpha, 1 - 0.9 ** rug[1][rug[1] > 0]) and alpha.min() >= 0.1 - 1e-12  # noqa: PLR2004
    finally:
        plt.close(figure)
    unlimited = distribution_figure.distribution_figure(dist, distribution.rug_counts(x, "query_cov", dist), "query_cov")
    try:
        assert unlimited.axes[0].get_xlim() != (0.80, 1.01)
    finally:
        plt.close(unlimited)


def test_plot_run_distributions_skip_an_all_na_matrix(viral_db, tmp_path, caplog):
    copy = tmp_path / "nulls.sqlite"
    copy.write_bytes(viral_db.read_bytes())
    conn = sqlite3.connect(copy)
    conn.execute("UPDATE comparisons SET identity = NULL, cov_query = NULL")
    conn.execute("UPDATE runs SET df_identity = NULL, df_cov_query = NULL, df_hadamard = NULL")
    conn.commit()
    conn.close()
    assert rundb.plot_run(copy, tmp_path / "none", distributions=True) == []
    assert "Cannot plot tANI as all NA" in caplog.text and list((tmp_path / "none").iterdir()) == []
    # some cells NULL: they are left out of the distribution, as out of the scatter tables
    copy.write_bytes(viral_db.read_bytes())
    conn = sqlite3.connect(copy)
    ids = [r[0] for r in conn.execute("SELECT comparison_id FROM comparisons WHERE query_hash != subject_hash ORDER BY comparison_id LIMIT 2")]
    conn.execute(f"UPDATE comparisons SET identity = NULL, cov_query = NULL WHERE comparison_id IN ({ids[0]}, {ids[1]})")
    conn.execute("UPDATE runs SET df_identity = NULL, df_cov_query = NULL, df_hadamard = NULL")
    conn.commit()
    conn.close()
    rundb.plot_run(copy, tmp_path / "some", distributions=True)
    _header, rows = read_rows(tmp_path / "some" / "sourmash-hip_identity_dist_hist.tsv")
    assert rows[:, 2].sum() == 7  # noqa: PLR2004


def test_plot_run_distributions_of_a_single_genome(tmp_path):
    fasta = tmp_path / "one"
    fasta.mkdir()
    (fasta / "OP073605.fasta").write_bytes((GOLDEN / "viral_example" / "OP073605.fasta").read_bytes())
    db = tmp_path / "one.sqlite"
    assert rundb.run_sourmash_hip(fasta, db, cache=tmp_path / "cache", scaled=300, engine=OracleEngine(), temp=tmp_path).status == "Done"
    written = rundb.plot_run(db, tmp_path / "out", distributions=True)
    assert len(written) == 6 + 8
    assert (tmp_path / "out" / "sourmash-hip_identity_dist_hist.tsv").read_text() == "#left\tright\tcount\n0.5\t1.5\t1\n"
    assert (tmp_path / "out" / "sourmash-hip_tANI_dist_hist.tsv").read_text() == "#left\tright\tcount\n-0.5\t0.5\t1\n"
    assert (tmp_path / "out" / "sourmash-hip_identity_dist_kde.tsv").read_text() == "#x\tdensity\n"


# ------------------------------------------------------------------ the host code under sanitizers
def test_host_twins_under_sanitizers():
    """AddressSanitizer + UBSan over ``dist_host.cpp`` in a stand-alone CPU program: random vectors with NaNs and ties in
    exact-size buffers, ranks at and past the end, histograms of up to 70 000 bins checked against a search of the edges."""
    import shutil
    import subprocess
    from pathlib import Path

    if shutil.which("g++") is None:
        pytest.skip("no host compiler")
    script = Path(__file__).resolve().parent / "tools" / "sanitize" / "run_dist.sh"
    done = subprocess.run(["bash", str(script), "300"], capture_output=True, text=True, timeout=600)
    assert done.returncode == 0 and "sanitizer runs clean" in done.stdout, done.stdout[-2000:] + done.stderr[-2000:]
    assert "MISMATCH" not in done.stdout
