"""plot-run's scatter figures: what the reference's ``plot_scatter`` (pyani_plus/plot_run.py:218-299) hands
``seaborn.jointplot(kind="scatter", joint_kws={"s": 2, "c": query_lengths})`` -- one marker per comparison, coloured by
the query's length, with automatic-bin histograms on both margins -- restated as a raster that N = 10^4 genomes (10^8
markers) can be drawn from.

* the points: the cells of two N x N score matrices (rows = query) in row-major order.  Point ``t = i * N + j`` has
  ``x = identity[i, j]`` and ``y = query_cov[i, j]`` or ``tANI[i, j]``; its colour is the length of query ``i``; it is
  valid iff neither is NaN.  ``x'`` is ``x`` with NaN wherever ``y`` is NaN, ``y'`` likewise;
* the margins: ``numpy.histogram(x', "auto")`` and ``numpy.histogram(y', "auto")`` (``distribution.auto_histogram``),
  which is what jointplot's marginal ``histplot`` computes;
* the joint panel: ``bins`` x ``bins`` uniform cells (``GRID`` = 256 by default, about 1.5 px of a 6 in panel at
  100 dpi, close to the reference's ``s=2`` marker) over the ranges of ``x'`` and ``y'``, with numpy's bin rule on each
  axis.  A cell holds ``count``, the number of valid points in it, and ``last``, the largest ``t`` among them; it is
  drawn in the colour of ``lengths[last // N]``, which is what overdrawn markers show: the last one.  The colour scale
  runs from the smallest to the largest length over the rows that have a valid point, the reference's
  ``Normalize(min(c_values), max(c_values))``.

Two departures from the reference, both this project's definitions.  The order: the reference draws its markers in
``comparison_id`` order, which matters only for which of several points in a cell is the last; here it is the row-major
order of the label-sorted matrix.  The rounding: for runs that fit the cache the matrices are the cached 10-decimal
ones, as for the distributions.

With an ``engine`` (a ``HipEngine``) the passes over the points run on the GPU (``pa_bin2d_f64`` and the distribution's
kernels); with None the host twins do the same, with the same bits.  DESIGN.md section 7f.
"""

from __future__ import annotations

import logging
from dataclasses import dataclass

import numpy as np

from . import _capi, distribution, run_comp
from ._capi import check

GRID = 256  # cells per axis of the joint panel
MAX_BINS = _capi.PA_BIN2D_MAX_BINS
NONE = _capi.PA_BIN2D_NONE  # the ``last`` of an empty cell


def _edges(edges) -> np.ndarray:
    h_edges = np.ascontiguousarray(edges, dtype=np.float64)
    if h_edges.ndim != 1 or len(h_edges) < 2:  # noqa: PLR2004
        msg = f"edges of shape {h_edges.shape}, expected at least two in one dimension"
        raise ValueError(msg)
    return h_edges


def bin2d_host(x, y, xedges, yedges) -> tuple[np.ndarray, np.ndarray]:
    """``pa_bin2d_f64_host``: ``(counts, last)``, uint64 arrays of shape ``(len(xedges) - 1, len(yedges) - 1)``:
    ``numpy.histogram2d(x, y, (xedges, yedges))``'s counts over uniform edges, and the largest index among each cell's
    points (``NONE`` for an empty cell)."""
    hx = np.ascontiguousarray(x, dtype=np.float64).reshape(-1)
    hy = np.ascontiguousarray(y, dtype=np.float64).reshape(-1)
    if hx.shape != hy.shape:
        msg = f"{hx.size} x values and {hy.size} y values"
        raise ValueError(msg)
    h_xe, h_ye = _edges(xedges), _edges(yedges)
    shape = (len(h_xe) - 1, len(h_ye) - 1)
    counts, last = np.empty(shape, dtype=np.uint64), np.empty(shape, dtype=np.uint64)
    check(
        _capi.load_library().pa_bin2d_f64_host(hx.ctypes.data, hy.ctypes.data, hx.size, h_xe.ctypes.data, shape[0], h_ye.ctypes.data, shape[1],
                                               counts.ctypes.data, last.ctypes.data),
        "pa_bin2d_f64_host",
    )  # fmt: skip
    return counts, last


@dataclass
class Scatter:
    """``n_valid`` of ``n_total`` points; the joint panel's ``xedges`` and ``yedges``, its uint64 ``counts`` and ``last``
    (shape ``(bins, bins)``, x first; ``NONE`` in an empty cell) and ``colour``, the query length each cell is drawn
    with (float64, NaN in an empty cell); ``c_min`` and ``c_max``, the ends of the colour scale; ``x_hist`` and
    ``y_hist``, the marginal ``distribution.Histogram``s."""

    n_valid: int
    n_total: int
    xedges: np.ndarray
    yedges: np.ndarray
    counts: np.ndarray
    last: np.ndarray
    colour: np.ndarray
    c_min: float
    c_max: float
    x_hist: distribution.Histogram
    y_hist: distribution.Histogram


def describe(x, y, lengths, n: int, engine=None, bins: int = GRID, logger: logging.Logger | None = None) -> Scatter | None:
    """The raster and the margins of the ``n * n`` points ``(x, y)``: ``n`` x ``n`` matrices as host arrays, or with an
    ``engine`` also as float64 tensors on its device; ``lengths[i]`` is the length of query ``i``.  None when no point
    is valid.  Both backends take the same steps."""
    n, bins = int(n), int(bins)
    if not 1 <= bins <= MAX_BINS:
        msg = f"{bins} cells per axis; 1 to {MAX_BINS}"
        raise ValueError(msg)
    lengths = np.asarray(lengths)
    if lengths.shape != (n,):
        msg = f"{lengths.shape} lengths for {n} queries"
        raise ValueError(msg)
    if engine is not None:
        t = engine.torch
        xv, yv = engine._f64_on_device(x).reshape(-1), engine._f64_on_device(y).reshape(-1)  # noqa: SLF001
        lib, nan = t, t.tensor(float("nan"), dtype=t.float64, device=engine.device)
    else:
        xv, yv = (np.ascontiguousarray(v, dtype=np.float64).reshape(-1) for v in (x, y))
        lib, nan = np, np.float64("nan")
    if xv.shape != (n * n,) or yv.shape != (n * n,):
        msg = f"{tuple(xv.shape)} x and {tuple(yv.shape)} y values for {n} x {n} points"
        raise ValueError(msg)
    xm, ym = lib.where(lib.isnan(yv), nan, xv), lib.where(lib.isnan(xv), nan, yv)  # plumbing: x', y'
    try:
        x_hist = distribution.auto_histogram(xm, engine, logger)
    except ValueError:  # no value that is not NaN
        return None
    y_hist = distribution.auto_histogram(ym, engine, logger)
    xedges, yedges = run_comp.hist_edges(x_hist.lo, x_hist.hi, bins), run_comp.hist_edges(y_hist.lo, y_hist.hi, bins)
    counts, last = engine.bin2d(xm, ym, xedges, yedges) if engine is not None else bin2d_host(xm, ym, xedges, yedges)
    rows = (~lib.isnan(xm)).reshape(n, n).any(1)  # the queries with a valid point
    rows = rows.cpu().numpy() if engine is not None else rows
    seen = counts > 0
    colour = np.full(counts.shape, np.nan)
    colour[seen] = lengths[(last[seen] // np.uint64(n)).astype(np.int64)]
    return Scatter(x_hist.n, n * n, xedges, yedges, counts, last, colour, float(lengths[rows].min()), float(lengths[rows].max()), x_hist, y_hist)


def write_grid_tsv(path, scatter: Scatter) -> None:
    """``#x_left TAB x_right TAB y_left TAB y_right TAB count TAB query_length`` and a line per non-empty cell, x-major,
    the floats as ``repr``."""
    xe, ye = scatter.xedges.tolist(), scatter.yedges.tolist()
    with open(path, "w") as handle:
        handle.write("#x_left\tx_right\ty_left\ty_right\tcount\tquery_length\n")
        for ix, iy in zip(*(a.tolist() for a in np.nonzero(scatter.counts))):
            handle.write(f"{xe[ix]!r}\t{xe[ix + 1]!r}\t{ye[iy]!r}\t{ye[iy + 1]!r}\t{int(scatter.counts[ix, iy])}\t{int(scatter.colour[ix, iy])}\n")
