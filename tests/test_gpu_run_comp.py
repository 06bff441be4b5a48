"""plot-run-comp on the device: ``pa_runcomp_join`` against its host twin and a numpy restatement at the group and
workgroup edges, with cell indices past 2^31; ``pa_hist_uniform_f64`` against ``numpy.histogram`` at the bin edges and
under counter contention; ``pa_minmax_f64``; ``run_comp.compare`` and ``rundb.plot_run_comp`` through the device."""

from __future__ import annotations

import ctypes as C

import numpy as np
import pytest

from pyani_plus_amd import distribution, run_comp, rundb
from tests.run_comp_cases import (
    HIST_BINS,
    HIST_FAMILIES,
    HIST_SIZES,
    JOIN_PATTERNS,
    JOIN_REFS,
    JOIN_ROWS,
    NONE,
    adversarial_values,
    hist_inputs,
    join_inputs,
    join_reference,
    make_viral_db,
    numpy_hist,
    numpy_join,
    same_bits,
)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def engine():
    from pyani_plus_amd.engine import HipEngine

    eng = HipEngine(0)
    yield eng
    eng.close()


# ------------------------------------------------------------------ join
@pytest.mark.parametrize("n_ref", JOIN_REFS)
@pytest.mark.parametrize("n_rows", JOIN_ROWS)
def test_join_equals_the_host_twin(engine, n_rows, n_ref):
    ref = join_reference(n_ref)
    d_ref = engine.torch.from_numpy(ref).to(engine.device)
    for pattern in JOIN_PATTERNS:
        q, s, y, survivors = join_inputs(n_rows, ref, pattern)
        got = engine.run_join(d_ref, q, s, y)
        assert len(got[0]) == survivors, pattern
        for mine, twin, restated in zip(got, run_comp.join_host(ref, q, s, y), numpy_join(ref, q, s, y)):
            same_bits(mine, twin)
            same_bits(mine, restated)


def test_join_with_cell_indices_past_31_bits(engine):
    t = engine.torch
    n_ref = 46400
    free, _total = t.cuda.mem_get_info(engine.device)
    if free < 20e9:
        pytest.skip(f"{free / 1e9:.1f} GB free on the device, the 46400 x 46400 matrix takes 17.2 GB")
    rng = np.random.default_rng(46400)
    n_rows = 1000
    q = rng.integers(46282, n_ref, n_rows)  # 46282 * 46400 >= 2^31
    s = rng.permutation(n_ref)[:n_rows]
    q[:4], s[:4] = (46399, 46340, 0, 46281), (46399, 46341, 0, 46399)  # the last: 1151 past 2^31
    cells = q * n_ref + s
    assert len(set(cells.tolist())) == n_rows and cells[0] == n_ref * n_ref - 1 and cells[1] >= 2**31 and cells[2] < 2**31 <= cells[3] < 2**31 + 2000 and cells[4:].min() >= 2**31
    values, y = rng.random(n_rows), rng.random(n_rows)
    filled = np.arange(n_rows) % 5 != 4  # every fifth cell stays NaN  # noqa: PLR2004
    ref = t.full((n_ref, n_ref), float("nan"), dtype=t.float64, device=engine.device)
    ref[t.from_numpy(q[filled]).to(engine.device), t.from_numpy(s[filled]).to(engine.device)] = t.from_numpy(values[filled]).to(engine.device)
    x, yy, d = engine.run_join(ref, q.astype(np.uint32), s.astype(np.uint32), y)
    del ref
    assert filled[:4].all() and filled.sum() == 800  # noqa: PLR2004
    same_bits(x, values[filled])
    same_bits(yy, y[filled])
    same_bits(d, y[filled] - values[filled])


def test_join_arguments(engine):
    count = C.c_uint64(7)
    assert engine.lib.pa_runcomp_join(engine.ctx, None, 65537, None, None, None, 0, None, None, None, C.byref(count)) == -1  # PA_E_INVALID
    assert "at most 65536" in (engine.lib.pa_last_error() or b"").decode()
    x, y, d = engine.run_join(np.empty((0, 0)), [0, NONE], [NONE, 0], [0.5, 0.25])
    assert len(x) == len(y) == len(d) == 0
    with pytest.raises(ValueError, match="expected a square one"):
        engine.run_join(np.zeros((2, 3)), [0], [0], [0.5])
    with pytest.raises(ValueError, match="vectors of one length"):
        engine.run_join(np.zeros((2, 2)), [0, 1], [0], [0.5])


# ------------------------------------------------------------------ histogram
@pytest.mark.parametrize("bins", HIST_BINS)
@pytest.mark.parametrize("n", HIST_SIZES)
def test_histogram_equals_numpy(engine, n, bins):
    for family in HIST_FAMILIES:
        v, edges = hist_inputs(family, n, bins)
        counts = engine.hist_uniform(v, edges)
        assert counts.dtype == np.uint64 and np.array_equal(counts, numpy_hist(v, edges)), family
        assert np.array_equal(counts, run_comp.hist_uniform_host(v, edges)), family


@pytest.mark.parametrize("bins", HIST_BINS)
def test_histogram_of_one_value_many_times(engine, bins):
    """2^20 copies of one value inside one bin: every lane of every wave adds to the same counter."""
    edges = run_comp.hist_edges(0.0, 1.0, bins)
    v = np.full(2**20, 0.7)
    counts = engine.hist_uniform(v, edges)
    assert np.array_equal(counts, numpy_hist(v, edges)) and counts.max() == 2**20 and counts.sum() == 2**20


def test_histogram_arguments(engine):
    from pyani_plus_amd._capi import HipBackendError

    for bad, message in (([0.0, 0.5, 0.25, 1.0], "edge 2 is below edge 1"), ([0.0, np.inf], "edge 1 is not finite"), ([1.0, 1.0], "above the first")):
        with pytest.raises(HipBackendError, match=message) as caught:
            engine.hist_uniform([0.5], bad)
        assert caught.value.status == -1  # PA_E_INVALID
    with pytest.raises(HipBackendError, match="1025 bins; 1 to 1024"):
        engine.hist_uniform([0.5], np.linspace(0, 1, 1026))
    v = np.random.default_rng(8).random(5000)
    edges = run_comp.hist_edges(v.min(), v.max(), 1024)
    assert np.array_equal(engine.hist_uniform(v, edges), numpy_hist(v, edges))
    assert engine.hist_uniform([], [0.0, 1.0]).tolist() == [0]


@pytest.mark.parametrize("bins", [1, 2, 1024])
@pytest.mark.parametrize("n", [1, 255, 256, 257, 262_145])  # the last: one past 1024 workgroups of 256, where the grid starts to stride
def test_both_entry_points_and_both_host_twins_count_alike(engine, n, bins):
    """One device vector and one set of edges through ``pa_hist_uniform_f64`` and ``pa_hist_uniform_f64_wide``: every
    edge, its neighbouring doubles (one of them outside at each end), the midpoints and NaN."""
    edges = run_comp.hist_edges(0.1, 0.7, bins)
    rest = np.random.default_rng(n + bins).permutation(np.concatenate([adversarial_values(edges), [np.nan, edges[0] - 0.25, edges[-1] + 0.25]]))
    v = np.resize(np.concatenate([edges[-1:], rest]), n)  # the last edge, which belongs to the last bin, is in every size
    d_v = engine.torch.from_numpy(v).to(engine.device)
    narrow, wide = engine.hist_uniform(d_v, edges), engine.hist_uniform_wide(d_v, edges)
    want = numpy_hist(v, edges)
    assert narrow.dtype == wide.dtype == np.uint64 and want[-1] >= 1
    assert np.array_equal(narrow, wide) and np.array_equal(narrow, want)
    assert np.array_equal(narrow, run_comp.hist_uniform_host(v, edges)) and np.array_equal(narrow, distribution.hist_uniform_wide_host(v, edges))


def test_the_2d_binning_summed_over_y_is_the_histogram_of_x(engine):
    """The 1-D and the 2-D use of the one bin rule: with a y range that holds every point, the cells of a column add up
    to the histogram of x."""
    xedges, yedges = run_comp.hist_edges(0.1, 0.7, 3), run_comp.hist_edges(-1.0, 2.0, 2)
    x = np.resize(np.concatenate([adversarial_values(xedges), [np.nan, -3.0, 3.0]]), 257)
    y = np.random.default_rng(257).random(257)
    cells, _last = engine.bin2d(x, y, xedges, yedges)
    assert cells.shape == (3, 2) and cells.min() > 0
    assert np.array_equal(cells.sum(axis=1), engine.hist_uniform(x, xedges)) and np.array_equal(cells.sum(axis=1), numpy_hist(x, xedges))


# ------------------------------------------------------------------ minimum and maximum
@pytest.mark.parametrize("n", HIST_SIZES)
def test_minmax_equals_numpy(engine, n):
    rng = np.random.default_rng(n)
    v = rng.random(n) * 4 - 3  # negative values too
    assert engine.minmax(v) == (v.min(), v.max(), n)
    v[rng.random(n) < 0.3] = np.nan
    if not np.isnan(v).all():
        assert engine.minmax(v) == (np.nanmin(v), np.nanmax(v), int((~np.isnan(v)).sum())) == run_comp.minmax_host(v)
    lo, hi, valid = engine.minmax(np.full(n, np.nan))
    assert np.isnan(lo) and np.isnan(hi) and valid == 0
    one = np.full(n, np.nan)
    one[n - 1] = -0.125
    assert engine.minmax(one) == (-0.125, -0.125, 1)
    assert engine.minmax(engine.torch.from_numpy(one).to(engine.device)) == (-0.125, -0.125, 1)
    lo, hi, valid = engine.minmax([])
    assert np.isnan(lo) and valid == 0


# ------------------------------------------------------------------ compare and plot_run_comp
def test_compare_through_the_device_forms(engine):
    ref = join_reference(1000)
    q, s, y, survivors = join_inputs(10**6, ref, "mixed")
    host = run_comp.compare(ref, q, s, y)
    device = run_comp.compare(engine.torch.from_numpy(ref).to(engine.device), q, s, y, engine)
    assert len(host.x) == survivors > 5 * 10**5
    for name in ("x", "y", "d"):
        same_bits(getattr(device, name), getattr(host, name))
    for name in ("x_range", "y_range", "d_range"):
        assert getattr(device, name) == getattr(host, name), name
    for name in ("x_counts", "y_counts", "d_counts"):
        assert np.array_equal(getattr(device, name), getattr(host, name)), name
    assert np.array_equal(host.d_counts, np.histogram(host.d, 30)[0]) and np.array_equal(host.x_counts, np.histogram(ref[~np.isnan(ref)], 30)[0])
    # the device forms keep the joined values on the device
    d_x, d_y, d_d = engine.run_join_device(ref, q, s, y)
    assert d_x.is_cuda and d_x.shape == d_y.shape == d_d.shape == (survivors,)
    assert np.array_equal(engine.hist_uniform(d_d, run_comp.hist_edges(*host.d_range)), host.d_counts)


def test_plot_run_comp_on_the_device_writes_the_same_bytes(engine, tmp_path):
    db = make_viral_db(tmp_path)
    host = rundb.plot_run_comp(db, tmp_path / "host", "1,2,3,4")
    device = rundb.plot_run_comp(db, tmp_path / "device", "1,2,3,4", engine=engine)
    assert [p.name for p in device] == [p.name for p in host] and len(host) == 3  # noqa: PLR2004
    for a, b in zip(host, device):
        assert a.read_bytes() == b.read_bytes() and len(a.read_bytes()) > 50  # noqa: PLR2004
