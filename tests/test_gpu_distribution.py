"""plot-run's distributions on the device: ``pa_select_f64`` against ``numpy.sort`` at the wave, workgroup and grid
edges and on keys decided by the first and by the last pass; ``pa_moments_f64``; ``pa_kde_gauss_f64`` against its host
twin within the summation bound and against scipy's golden densities, the same bits run to run;
``pa_hist_uniform_f64_wide`` against ``numpy.histogram`` on both sides of its LDS capacity; ``distribution.describe``
and ``rundb.plot_run(distributions=True)`` through the device next to the host."""

from __future__ import annotations

import ctypes as C

import numpy as np
import pytest

from pyani_plus_amd import distribution, rundb
from pyani_plus_amd._capi import HipBackendError
from tests.distribution_cases import (
    ATOL_SCIPY,
    CHAIN,
    KDE_GRIDS,
    KDE_SIZES,
    LDS_BINS,
    RTOL_SCIPY,
    SELECT_KINDS,
    SELECT_SIZES,
    WIDE_BINS_DEVICE,
    close,
    device_bound,
    golden_inputs,
    kde_grid,
    kde_values,
    load_golden,
    numpy_hist,
    same_bits,
    scott_bw,
    select_rank_sets,
    select_values,
    sorted_valid,
    wide_inputs,
    worst,
)
from tests.helpers import FIXTURE_SETS, GOLDEN

pytestmark = pytest.mark.gpu

SCORES = ("identity", "query_cov", "hadamard", "tANI")


@pytest.fixture(scope="module")
def engine():
    from pyani_plus_amd.engine import HipEngine

    eng = HipEngine(0)
    yield eng
    eng.close()


# ------------------------------------------------------------------ select
@pytest.mark.parametrize("n", SELECT_SIZES)
def test_select_equals_numpy_sort(engine, n):
    for kind in SELECT_KINDS:
        x = select_values(kind, n)
        d_x = engine.torch.from_numpy(x).to(engine.device)
        want = sorted_valid(x)
        for ranks in select_rank_sets(len(want)):
            got = engine.select(d_x, ranks)
            assert np.array_equal(got, want[ranks]), (kind, ranks)  # as values: -0.0 and 0.0 are one
            assert np.array_equal(got, distribution.select_host(x, ranks)), (kind, ranks)
        assert np.array_equal(d_x.cpu().numpy().view(np.uint64), x.view(np.uint64))  # the data is neither sorted nor changed


def test_select_arguments(engine):
    for x, ranks, message in (([np.nan] * 70, [0], "rank 0 of 0 values"), ([1.0, np.nan, 2.0], [1, 2], "rank 2 of 2 values"), ([], [0], "rank 0 of 0")):
        with pytest.raises(HipBackendError, match=message) as caught:
            engine.select(x, ranks)
        assert caught.value.status == -1  # PA_E_INVALID
    with pytest.raises(HipBackendError, match="9 ranks; at most 8"):
        engine.select([1.0] * 20, list(range(9)))
    out = (C.c_double * 1)(7.0)
    ranks = (C.c_uint64 * 1)(5)
    assert engine.lib.pa_select_f64(engine.ctx, None, 0, ranks, 1, out) == -1 and out[0] == 7.0  # noqa: PLR2004
    assert len(engine.select([1.0], [])) == 0
    assert engine.select([3.0, 1.0, 2.0], [2, 0, 1]).tolist() == [3.0, 1.0, 2.0]  # host arrays too, the ranks in any order


# ------------------------------------------------------------------ moments
@pytest.mark.parametrize("n", (1, 2, 65, 257, 3000, 300_001))
def test_moments(engine, n):
    x = kde_values("nan" if n > 2 else "identity", n)  # noqa: PLR2004
    v = x[~np.isnan(x)]
    d_x = engine.torch.from_numpy(x).to(engine.device)
    mean, squares = engine.moments(d_x)
    # positive values and squares: a sum is off by at most (additions a term passes through) * 2^-53, here at most
    # n / 2^18 + 1 in a lane, 8 levels in the workgroup, 4 + 8 over the workgroups; 64 covers all of it with the mean's own
    # error in the deviations
    assert mean == pytest.approx(v.mean(), rel=64 * 2.0**-53) and squares == pytest.approx(((v - v.mean()) ** 2).sum(), rel=1e-12, abs=1e-300)
    assert (mean, squares) == engine.moments(d_x)  # the same bits run to run
    host = distribution.moments_host(x)
    assert mean == pytest.approx(host[0], rel=1e-13) and squares == pytest.approx(host[1], rel=1e-11, abs=1e-300)
    assert all(np.isnan(m) for m in engine.moments(np.full(n, np.nan))) and all(np.isnan(m) for m in engine.moments([]))


# ------------------------------------------------------------------ density
@pytest.mark.parametrize("n_grid", KDE_GRIDS)
@pytest.mark.parametrize("n", KDE_SIZES)
def test_density_equals_the_host_twin(engine, n, n_grid):
    for kind in ("identity", "nan") if 2 < n < 10_000 else ("nan" if n > 2 else "identity",):  # noqa: PLR2004
        x = kde_values(kind, n)
        bw = scott_bw(x) if n > 1 else 0.01
        grid = kde_grid(x, bw, n_grid)
        d_x = engine.torch.from_numpy(x).to(engine.device)
        got = engine.kde_gauss(d_x, grid, bw)
        same_bits(got, engine.kde_gauss(d_x, grid, bw))  # run to run
        twin = distribution.kde_gauss_host(x, grid, bw)
        print(f"n {n}, grid {n_grid}, {kind}: worst relative difference {worst(got, twin):.3e}, bound {device_bound(n, n_grid):.3e}")
        assert close(got, twin, device_bound(n, n_grid), ATOL_SCIPY), (kind, worst(got, twin))
        assert got.min() >= 0 and got.max() > 0


@pytest.mark.parametrize("case", load_golden(), ids=lambda c: c["name"])
def test_density_equals_the_golden_case(engine, case):
    x, grid = golden_inputs(case)
    got = engine.kde_gauss(x, grid, case["bw"])
    print(f"{case['name']}: worst relative difference to scipy {worst(got, case['density']):.3e}")
    assert close(got, case["density"], RTOL_SCIPY, ATOL_SCIPY), worst(got, case["density"])
    assert close(got, distribution.kde_gauss_host(x, grid, case["bw"]), device_bound(case["n"], case["n_grid"]), ATOL_SCIPY)
    if case["kind"] == "clusters":
        assert got[100] == 0.0 and got.max() > 50  # noqa: PLR2004
    if case.get("through_datum"):
        assert x[0] in grid


def test_density_arguments(engine):
    for bw, message in ((0.0, "must be positive and finite"), (-1.0, "must be positive"), (np.inf, "positive and finite"), (np.nan, "positive and finite")):
        with pytest.raises(HipBackendError, match=message) as caught:
            engine.kde_gauss([0.5, 0.6], [0.5], bw)
        assert caught.value.status == -1  # PA_E_INVALID
    for x, grid, message in (([0.5, np.inf], [0.5], "an infinite value"), ([-np.inf] + [0.5] * 300, [0.5], "an infinite value"), ([np.nan], [0.5], "no value that is not NaN"),
                             ([], [0.5], "no value that is not NaN"), ([0.5], [np.nan], "grid point 0 is not finite"), ([0.5], np.zeros(1025), "1025 grid points")):  # fmt: skip
        with pytest.raises(HipBackendError, match=message):
            engine.kde_gauss(x, grid, 0.1)
    one = engine.kde_gauss([0.5], [0.5], 0.1)  # one value under its own grid point: the kernel's peak
    assert one[0] == pytest.approx(1 / (0.1 * np.sqrt(2 * np.pi)), rel=4 * 2.0**-53)


# ------------------------------------------------------------------ wide histogram
@pytest.mark.parametrize("bins", WIDE_BINS_DEVICE)
def test_wide_histogram_equals_numpy(engine, bins):
    v, edges = wide_inputs(bins)
    counts = engine.hist_uniform_wide(v, edges)
    assert counts.dtype == np.uint64 and np.array_equal(counts, numpy_hist(v, edges))
    assert np.array_equal(counts, distribution.hist_uniform_wide_host(v, edges))


@pytest.mark.parametrize("bins", (LDS_BINS, LDS_BINS + 1))
def test_wide_histogram_of_one_value_many_times(engine, bins):
    """2^20 copies of one value: every lane adds to the same counter, in LDS and in global memory."""
    edges = np.linspace(0.0, 1.0, bins + 1)
    v = np.full(2**20, 0.7)
    counts = engine.hist_uniform_wide(v, edges)
    assert np.array_equal(counts, numpy_hist(v, edges)) and counts.max() == 2**20 == counts.sum()


def test_wide_histogram_arguments(engine):
    for bad, message in (([0.0, 0.5, 0.25, 1.0], "edge 2 is below edge 1"), ([0.0, np.inf], "edge 1 is not finite"), ([1.0, 1.0], "above the first")):
        with pytest.raises(HipBackendError, match=message):
            engine.hist_uniform_wide([0.5], bad)
    with pytest.raises(HipBackendError, match="1048577 bins; 1 to 1048576"):
        engine.hist_uniform_wide([0.5], np.linspace(0, 1, 2**20 + 2))
    assert engine.hist_uniform_wide([], [0.0, 1.0]).tolist() == [0]
    with pytest.raises(HipBackendError, match="1025 bins; 1 to 1024"):  # the narrow one keeps its limit
        engine.hist_uniform([0.5], np.linspace(0, 1, 1026))


# ------------------------------------------------------------------ describe and plot_run
def test_describe_through_the_device(engine):
    x = kde_values("nan", 300_001)
    host = distribution.describe(x)
    device = distribution.describe(engine.torch.from_numpy(x).to(engine.device), engine)
    assert (device.n, device.lo, device.hi) == (host.n, host.lo, host.hi)
    same_bits(device.edges, host.edges)
    same_bits(device.edges, np.histogram_bin_edges(x[~np.isnan(x)], "auto"))
    assert np.array_equal(device.counts, host.counts) and len(host.counts) > 50  # noqa: PLR2004
    assert device.bw == pytest.approx(host.bw, rel=1e-13)
    assert close(device.grid, host.grid, 1e-13) and close(device.density, host.density, RTOL_SCIPY, ATOL_SCIPY), worst(device.density, host.density)
    for flat in ([0.5], [0.5, np.nan, 0.5, 0.5]):
        dist = distribution.describe(engine.torch.tensor(flat, dtype=engine.torch.float64, device=engine.device), engine)
        assert dist.bw is None and dist.counts.tolist() == [dist.n] and dist.edges.tolist() == [0.0, 1.0]
    for name in ("identity", "query_cov"):
        for a, b in zip(distribution.rug_counts(x, name, host), distribution.rug_counts(x, name, device, engine)):
            assert np.array_equal(a, b)


def read_rows(path) -> np.ndarray:
    return np.array([[float(f) for f in line.split("\t")] for line in path.read_text().split("\n")[1:-1]])


def test_plot_run_distributions_on_the_device(engine, tmp_path):
    scaled, _genomes = FIXTURE_SETS["viral_example"]
    db = tmp_path / "run.sqlite"
    assert rundb.run_sourmash_hip(GOLDEN / "viral_example", db, cache=tmp_path / "cache", scaled=scaled, engine=engine, temp=tmp_path).status == "Done"
    host = rundb.plot_run(db, tmp_path / "host", distributions=True)
    device = rundb.plot_run(db, tmp_path / "device", distributions=True, engine=engine)
    assert [p.name for p in device] == [p.name for p in host] and len(host) == 6 + 8
    for a, b in zip(host, device):
        if a.name.endswith("_dist_kde.tsv"):
            rows_a, rows_b = read_rows(a), read_rows(b)
            assert rows_a.shape == (200, 2) and close(rows_b[:, 0], rows_a[:, 0], 1e-13, 1e-15) and close(rows_b[:, 1], rows_a[:, 1], RTOL_SCIPY, ATOL_SCIPY), a.name
        else:
            assert a.read_bytes() == b.read_bytes() and len(a.read_bytes()) > 20, a.name  # noqa: PLR2004
    default = rundb.plot_run(db, tmp_path / "default", engine=engine)
    assert sorted(p.name for p in default) == sorted(p.name for p in host if "_dist_" not in p.name) == sorted(p.name for p in (tmp_path / "default").iterdir())
    assert len(default) == 6  # noqa: PLR2004
    assert CHAIN == distribution.KDE_CHAIN
