"""plot-run's score distributions: what the reference's ``plot_distribution`` (pyani_plus/plot_run.py:153-215) has
seaborn's ``histplot``, ``kdeplot`` and ``rugplot`` compute from all N x N cells of a score matrix, restated with
numpy's and scipy's definitions (which are what seaborn calls) and without sorting or copying the cells.

* the histogram: ``numpy.histogram(v, bins=numpy.histogram_bin_edges(v, "auto"))``.  The automatic rule needs the
  count, the range and four order statistics (``quartile_ranks``); ``auto_bin_edges`` makes the edges from those with
  numpy's arithmetic, and the counts are the library's uniform-bin histogram;
* the density: scipy's ``gaussian_kde(v)`` with Scott's factor on seaborn's grid, 200 points from ``min - 3 bw`` to
  ``max + 3 bw``, ``bw = std(v, ddof=1) * n ** -0.2``; no curve for fewer than two values or when all are equal;
* the rug: counts per pixel column over the axis range instead of a line per value.

``v`` is the matrix without its NaN cells.  With an ``engine`` (a ``HipEngine``) the passes over the cells run on the
GPU (``pa_minmax_f64``, ``pa_select_f64``, ``pa_moments_f64``, ``pa_kde_gauss_f64``, ``pa_hist_uniform_f64_wide``);
with None the host twins of the library do the same.  DESIGN.md section 7e has the definitions and the error bound.
"""

from __future__ import annotations

import ctypes as C
import logging
import math
from dataclasses import dataclass

import numpy as np

from . import _capi, run_comp
from ._capi import check

KDE_GRID = 200  # seaborn's gridsize
KDE_CUT = 3  # seaborn's cut: the grid reaches this many bandwidths past the data
KDE_CHAIN = _capi.PA_KDE_CHAIN  # the longest run of sequential additions of the device's density sum
WIDE_MAX_BINS = 1 << 20  # pa_hist_uniform_f64_wide
RUG_BINS = 1024  # pixel columns of the rug, at most
# the x-limits of the reference's figure, which are also its mask for the rug; query_cov has neither: the reference
# tests the name against "coverage", which it never passes
X_LIMITS = {"identity": (0.80, 1.01), "hadamard": (0.0, 1.01), "tANI": (0.0, 5.01)}


# ------------------------------------------------------------------ the automatic bin rule
def _virtual_index(n: int, percent: int) -> np.float64:
    """numpy's ``_compute_virtual_index(n, q, alpha=1, beta=1)`` for ``q = float64(percent) / 100``."""
    q = np.float64(percent) / 100
    return n * q + (1 + q * (1 - 1 - 1)) - 1


def quartile_ranks(n: int) -> tuple[int, int, int, int]:
    """The zero-based ranks of the order statistics numpy's linear percentile reads for 25 % and for 75 % of ``n``
    values: ``floor(vi)`` and ``floor(vi) + 1``, the latter clipped to ``n - 1``."""
    ranks = []
    for percent in (25, 75):
        low = int(math.floor(_virtual_index(n, percent)))
        ranks += [low, min(low + 1, n - 1)]
    return tuple(ranks)


def _linear_percentile(n: int, percent: int, below, above) -> np.float64:
    """``numpy.percentile(v, percent)`` from the two order statistics at ``quartile_ranks`` (``_get_indexes``,
    ``_get_gamma`` and ``_lerp`` of numpy/lib/_function_base_impl.py)."""
    vi = _virtual_index(n, percent)
    previous = np.floor(vi)
    a, b = np.float64(below), np.float64(above)
    if vi >= n - 1:  # numpy reads the last element for both, through the index -1, which also enters gamma
        previous, a = np.float64(-1), b
    t = vi - previous
    diff = b - a
    return b - diff * (1 - t) if t >= 0.5 else a + diff * t  # noqa: PLR2004


def auto_bin_edges(n: int, lo: float, hi: float, order_stats) -> np.ndarray:
    """``numpy.histogram_bin_edges(v, "auto")`` with numpy's bits, from the number of values, their minimum and
    maximum, and the four values at ``quartile_ranks(n)`` (numpy/lib/_histograms_impl.py: ``_get_outer_edges``,
    ``_hist_bin_auto``, ``_get_bin_edges``).  The width is the smaller of Freedman-Diaconis' and Sturges', Sturges' alone
    where the interquartile range is 0; a width of 0 gives one bin; ``lo == hi`` widens the range by 0.5 each way."""
    n = int(n)
    lo, hi = np.float64(lo), np.float64(hi)
    if n < 1 or not (np.isfinite(lo) and np.isfinite(hi)) or lo > hi:
        msg = f"{n} values from {lo} to {hi}: expected at least one and a finite ascending range"
        raise ValueError(msg)
    first, last = (lo - 0.5, hi + 0.5) if lo == hi else (lo, hi)
    p25_low, p25_high, p75_low, p75_high = order_stats
    iqr = _linear_percentile(n, 75, p75_low, p75_high) - _linear_percentile(n, 25, p25_low, p25_high)
    fd = 2.0 * iqr * n ** (-1.0 / 3.0)
    sturges = (hi - lo) / (np.log2(n) + 1.0)
    width = min(fd, sturges) if fd else sturges
    bins = int(np.ceil((last - first) / width)) if width else 1
    return np.linspace(first, last, bins + 1, endpoint=True, dtype=np.float64)


# ------------------------------------------------------------------ the host twins
def _vector(values) -> np.ndarray:
    return np.ascontiguousarray(values, dtype=np.float64).reshape(-1)


def select_host(values, ranks) -> np.ndarray:
    """``pa_select_f64_host``: the values at the zero-based ``ranks`` (at most 8) among the non-NaN elements in
    ascending order, ``numpy.sort(v)[ranks]``."""
    v = _vector(values)
    h_ranks = np.ascontiguousarray(ranks, dtype=np.uint64).reshape(-1)
    out = np.empty(len(h_ranks), dtype=np.float64)
    check(_capi.load_library().pa_select_f64_host(v.ctypes.data, len(v), h_ranks.ctypes.data, len(h_ranks), out.ctypes.data), "pa_select_f64_host")
    return out


def moments_host(values) -> tuple[float, float]:
    """``pa_moments_f64_host``: the mean of the non-NaN elements and the sum of their squared deviations from it;
    ``(nan, nan)`` when there is none."""
    v = _vector(values)
    out = (C.c_double * 2)(float("nan"), float("nan"))
    check(_capi.load_library().pa_moments_f64_host(v.ctypes.data, len(v), out), "pa_moments_f64_host")
    return float(out[0]), float(out[1])


def kde_gauss_host(values, grid, bw: float) -> np.ndarray:
    """``pa_kde_gauss_f64_host``: the Gaussian kernel density of the non-NaN elements with bandwidth ``bw`` at the
    ``grid`` points (at most 1024)."""
    v = _vector(values)
    h_grid = np.ascontiguousarray(grid, dtype=np.float64).reshape(-1)
    density = np.empty(len(h_grid), dtype=np.float64)
    check(_capi.load_library().pa_kde_gauss_f64_host(v.ctypes.data, len(v), h_grid.ctypes.data, len(h_grid), float(bw), density.ctypes.data), "pa_kde_gauss_f64_host")
    return density


def hist_uniform_wide_host(values, edges) -> np.ndarray:
    """``pa_hist_uniform_f64_wide_host``: ``numpy.histogram``'s uint64 counts over the uniform bins with these edges."""
    return run_comp._hist_uniform_host("pa_hist_uniform_f64_wide_host", values, edges)  # noqa: SLF001


def kde_tree_depth(n: int, n_grid: int) -> int:
    """The additions a term of the device's density sum passes through after its run of ``KDE_CHAIN``: the levels of
    the tree over the partial sums ``pa_kde_gauss_f64`` makes of ``n`` data for ``n_grid`` grid points (csrc/dist.hip:
    S slices in a workgroup, S the largest power of two with ``S * n_grid <= 1024``, a workgroup per ``KDE_CHAIN * S``
    data), ``ceil(log2(partials))``."""
    slices = 1
    while 2 * slices * n_grid <= 1024:  # noqa: PLR2004
        slices *= 2
    workgroups = max(1, -(-n // (KDE_CHAIN * slices)))
    return int(math.log2(slices)) + (workgroups - 1).bit_length()


# ------------------------------------------------------------------ one score's distribution
@dataclass
class Distribution:
    """``n`` values from ``lo`` to ``hi``; the histogram's ``edges`` and uint64 ``counts``; the density's bandwidth
    ``bw``, ``grid`` and ``density``, all three None when there is no curve (fewer than two values, or all equal)."""

    n: int
    lo: float
    hi: float
    edges: np.ndarray
    counts: np.ndarray
    bw: float | None
    grid: np.ndarray | None
    density: np.ndarray | None


@dataclass
class Histogram:
    """``n`` values from ``lo`` to ``hi`` and their automatic histogram: ``edges`` and uint64 ``counts``."""

    n: int
    lo: float
    hi: float
    edges: np.ndarray
    counts: np.ndarray


def auto_histogram(values, engine=None, logger: logging.Logger | None = None) -> Histogram:
    """``numpy.histogram(v, "auto")`` of the non-NaN elements ``v`` of ``values`` (a host array, or with an ``engine`` a
    float64 tensor on its device, which is read in place): the range, the four order statistics of the automatic rule,
    ``auto_bin_edges`` and the uniform-bin counts; above ``WIDE_MAX_BINS`` bins the device's values are counted on the
    host.  ``ValueError`` when every element is NaN."""
    on_device = engine is not None
    lo, hi, n = engine.minmax(values) if on_device else run_comp.minmax_host(values)
    if not n:
        msg = "no value that is not NaN"
        raise ValueError(msg)
    ranks = quartile_ranks(n)
    stats = engine.select(values, ranks) if on_device else select_host(values, ranks)
    edges = auto_bin_edges(n, lo, hi, stats)
    bins = len(edges) - 1
    if on_device and bins > WIDE_MAX_BINS:
        (logger or logging.getLogger("pyani_plus_amd")).info("%d bins are more than the device histogram takes (%d): counting on the host", bins, WIDE_MAX_BINS)
        counts = hist_uniform_wide_host(values.cpu().numpy() if hasattr(values, "cpu") else values, edges)
    else:
        counts = engine.hist_uniform_wide(values, edges) if on_device else hist_uniform_wide_host(values, edges)
    return Histogram(n, lo, hi, edges, counts)


def describe(values, engine=None, logger: logging.Logger | None = None) -> Distribution:
    """The histogram and the density of the non-NaN elements of ``values``: a host array, or with an ``engine`` a
    float64 tensor on its device, which is read in place.  Both backends take the same steps."""
    on_device = engine is not None
    hist = auto_histogram(values, engine, logger)
    n, lo, hi, edges, counts = hist.n, hist.lo, hist.hi, hist.edges, hist.counts
    if n < 2 or lo == hi:  # noqa: PLR2004
        return Distribution(n, lo, hi, edges, counts, None, None, None)
    _mean, squares = engine.moments(values) if on_device else moments_host(values)
    bw = math.sqrt(squares / (n - 1)) * n ** (-1.0 / 5.0)
    grid = np.linspace(lo - KDE_CUT * bw, hi + KDE_CUT * bw, KDE_GRID)
    density = engine.kde_gauss(values, grid, bw) if on_device else kde_gauss_host(values, grid, bw)
    return Distribution(n, lo, hi, edges, counts, bw, grid, density)


def rug_counts(values, name: str, dist: Distribution, engine=None) -> tuple[np.ndarray, np.ndarray]:
    """``(edges, counts)`` of the rug of score ``name``: the values inside the reference's mask for that score (for
    query_cov, which has none, all of them) counted per pixel column, ``RUG_BINS`` uniform bins over that range."""
    lo, hi = X_LIMITS.get(name, (dist.lo, dist.hi))
    edges = run_comp.hist_edges(lo, hi, RUG_BINS)
    return edges, (engine.hist_uniform(values, edges) if engine is not None else run_comp.hist_uniform_host(values, edges))


def write_hist_tsv(path, dist: Distribution | Histogram) -> None:
    """``#left TAB right TAB count`` and a line per bin, the floats as ``repr``."""
    with open(path, "w") as handle:
        handle.write("#left\tright\tcount\n")
        edges = dist.edges.tolist()
        for left, right, count in zip(edges[:-1], edges[1:], dist.counts.tolist()):
            handle.write(f"{left!r}\t{right!r}\t{count}\n")


def write_kde_tsv(path, dist: Distribution) -> None:
    """``#x TAB density`` and a line per grid point, the floats as ``repr``; the header alone when there is no curve."""
    with open(path, "w") as handle:
        handle.write("#x\tdensity\n")
        if dist.grid is not None:
            for x, y in zip(dist.grid.tolist(), dist.density.tolist()):
                handle.write(f"{x!r}\t{y!r}\n")
