"""plot-run-comp's arithmetic: two runs joined pair by pair and the 30-bin histograms of the joined values, what the
reference's ``plot_run_comparison`` computes with dictionaries keyed by ``(query_hash, subject_hash)`` and ``Axes.hist``
(pyani_plus/plot_run.py:389-588), without a Python object per comparison.

The reference run is its N x N identity matrix (NaN: no value); the other run is one row per comparison in
``comparison_id`` order: the row and column of its genomes in that matrix (``NONE``: not a genome of the reference
run) and its own identity (NaN: NULL).  A row survives iff both identities exist.  The histograms are
``numpy.histogram(values, bins=30)``'s, bit rule included; DESIGN.md section 7d has the definition.

With an ``engine`` (a ``HipEngine``) the join, the ranges and the counts are computed on the GPU (``pa_runcomp_join``,
``pa_minmax_f64``, ``pa_hist_uniform_f64``) and the joined values leave the device once; with None the host twins of
the library do the same with the same bits.
"""

from __future__ import annotations

import ctypes as C
from dataclasses import dataclass
from pathlib import Path

import numpy as np

from . import _capi
from ._capi import check

NONE = 0xFFFFFFFF  # the index of a genome the reference run does not have
BINS = 30  # hist_bins of plot_run_comparison


@dataclass
class Comparison:
    """The joined values (``d = y - x``), the ``(first, last)`` range of each histogram (None: no values) and the
    uint64 counts; ``x_range`` and ``x_counts`` are over all of the reference run's identities, joined or not."""

    x: np.ndarray
    y: np.ndarray
    d: np.ndarray
    x_range: tuple[float, float] | None
    y_range: tuple[float, float] | None
    d_range: tuple[float, float] | None
    x_counts: np.ndarray
    y_counts: np.ndarray
    d_counts: np.ndarray


def hist_edges(lo: float, hi: float, bins: int = BINS) -> np.ndarray:
    """The ``bins + 1`` edges ``numpy.histogram(values, bins)`` uses for values from ``lo`` to ``hi``: a range of one
    value is widened by 0.5 on each side, then ``numpy.linspace``."""
    lo, hi = float(lo), float(hi)
    if not (np.isfinite(lo) and np.isfinite(hi)) or lo > hi:
        msg = f"histogram range ({lo}, {hi}) must be finite and ascending"
        raise ValueError(msg)
    if lo == hi:
        lo, hi = lo - 0.5, hi + 0.5
    return np.linspace(lo, hi, int(bins) + 1)


def join_host(ref, q, s, y) -> tuple[np.ndarray, np.ndarray, np.ndarray]:
    """``pa_runcomp_join_host``: ``(x, y, d)`` of the rows both runs have a value for, in input order."""
    ref = np.ascontiguousarray(ref, dtype=np.float64)
    q, s = np.ascontiguousarray(q, dtype=np.uint32), np.ascontiguousarray(s, dtype=np.uint32)
    y = np.ascontiguousarray(y, dtype=np.float64)
    if ref.ndim != 2 or ref.shape[0] != ref.shape[1]:
        msg = f"reference matrix of shape {ref.shape}, expected a square one"
        raise ValueError(msg)
    n_rows = len(y)
    if q.shape != (n_rows,) or s.shape != (n_rows,) or y.shape != (n_rows,):
        msg = f"q {q.shape}, s {s.shape} and y {y.shape} must be vectors of one length"
        raise ValueError(msg)
    out = np.empty((3, n_rows), dtype=np.float64)
    count = C.c_uint64(0)
    check(
        _capi.load_library().pa_runcomp_join_host(
            ref.ctypes.data, len(ref), q.ctypes.data, s.ctypes.data, y.ctypes.data, n_rows, out[0].ctypes.data, out[1].ctypes.data,
            out[2].ctypes.data, C.byref(count),
        ),  # fmt: skip
        "pa_runcomp_join_host",
    )
    m = count.value
    return out[0, :m], out[1, :m], out[2, :m]


def minmax_host(values) -> tuple[float, float, int]:
    """``pa_minmax_f64_host``: ``(minimum, maximum, n_valid)`` of the non-NaN values; ``(nan, nan, 0)`` without any."""
    v = np.ascontiguousarray(values, dtype=np.float64).reshape(-1)
    out = (C.c_double * 2)(float("nan"), float("nan"))
    valid = C.c_uint64(0)
    check(_capi.load_library().pa_minmax_f64_host(v.ctypes.data, len(v), out, C.byref(valid)), "pa_minmax_f64_host")
    return float(out[0]), float(out[1]), int(valid.value)


def _hist_uniform_host(symbol: str, values, edges) -> np.ndarray:
    v = np.ascontiguousarray(values, dtype=np.float64).reshape(-1)
    h_edges = np.ascontiguousarray(edges, dtype=np.float64)
    if h_edges.ndim != 1 or len(h_edges) < 2:  # noqa: PLR2004
        msg = f"edges of shape {h_edges.shape}, expected at least two in one dimension"
        raise ValueError(msg)
    counts = np.zeros(len(h_edges) - 1, dtype=np.uint64)
    check(getattr(_capi.load_library(), symbol)(v.ctypes.data, len(v), h_edges.ctypes.data, len(counts), counts.ctypes.data), symbol)
    return counts


def hist_uniform_host(values, edges) -> np.ndarray:
    """``pa_hist_uniform_f64_host``: ``numpy.histogram``'s uint64 counts over the uniform bins with these edges."""
    return _hist_uniform_host("pa_hist_uniform_f64_host", values, edges)


def range_and_counts(values, engine=None, bins: int = BINS) -> tuple[tuple[float, float] | None, np.ndarray]:
    """``((min, max), counts)`` of ``numpy.histogram(values without NaN, bins)``; ``(None, zeros)`` without values.
    ``values``: a host array, or with an ``engine`` a tensor on its device."""
    lo, hi, valid = engine.minmax(values) if engine is not None else minmax_host(values)
    if not valid:
        return None, np.zeros(bins, dtype=np.uint64)
    edges = hist_edges(lo, hi, bins)
    return (lo, hi), (engine.hist_uniform(values, edges) if engine is not None else hist_uniform_host(values, edges))


def compare(ref_matrix, q, s, y, engine=None, *, x_hist=None) -> Comparison:
    """Join one other run (``q, s, y``) with the reference run's matrix and take the three histograms.  ``x_hist``:
    ``range_and_counts`` of the reference matrix when the caller has it already (it is the same for every other run);
    with an ``engine``, ``ref_matrix`` may be a tensor on its device, uploaded once for all the other runs."""
    x_range, x_counts = x_hist if x_hist is not None else range_and_counts(ref_matrix, engine)
    if engine is None:
        x, yy, d = join_host(ref_matrix, q, s, y)
        (y_range, y_counts), (d_range, d_counts) = range_and_counts(yy), range_and_counts(d)
    else:
        d_x, d_y, d_d = engine.run_join_device(ref_matrix, q, s, y)
        (y_range, y_counts), (d_range, d_counts) = range_and_counts(d_y, engine), range_and_counts(d_d, engine)
        x, yy, d = d_x.cpu().numpy(), d_y.cpu().numpy(), d_d.cpu().numpy()
    return Comparison(x, yy, d, x_range, y_range, d_range, x_counts, y_counts, d_counts)


def write_pairs_tsv(path: Path | str, header: str, x, y) -> None:
    """``pa_write_pairs_tsv``: ``header`` and a newline, then a line ``f"{x}\\t{y}\\n"`` per pair."""
    x, y = np.ascontiguousarray(x, dtype=np.float64), np.ascontiguousarray(y, dtype=np.float64)
    if x.ndim != 1 or x.shape != y.shape:
        msg = f"x {x.shape} and y {y.shape} must be vectors of one length"
        raise ValueError(msg)
    check(_capi.load_library().pa_write_pairs_tsv(str(path).encode(), header.encode(), x.ctypes.data, y.ctypes.data, len(x)), "pa_write_pairs_tsv")
