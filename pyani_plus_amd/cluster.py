"""Clustered heatmap order: what seaborn's ``clustermap`` computes for the reference's ``plot-run``
(pyani_plus/plot_run.py:114-147), without seaborn or scipy.

seaborn's defaults are ``scipy.cluster.hierarchy.linkage(rows, method="average", metric="euclidean")`` and the
``leaves`` of ``dendrogram(..., no_plot=True)``; the row order is applied to both axes of the table.  The row distances
(``pa_rowdist_euclid`` on the device, ``pa_rowdist_euclid_host`` without one) and the linkage (``pa_linkage_average``, on
the host) give the same bits as scipy, ties included; DESIGN.md section 7c has the contract.
"""

from __future__ import annotations

import numpy as np

from . import _capi
from ._capi import check


def row_distances(matrix, engine=None, *, threads: int = 0) -> np.ndarray:
    """Condensed Euclidean distances between the rows of ``matrix`` (n x m, finite float64), as
    ``scipy.spatial.distance.pdist(matrix, "euclidean")`` gives them.  ``engine``: a ``HipEngine`` computes them on the
    GPU; None on ``threads`` host threads (0: as many as the process may use)."""
    if engine is not None:
        return engine.row_distances(matrix)
    x = np.ascontiguousarray(matrix, dtype=np.float64)
    if x.ndim != 2:
        msg = f"matrix has shape {x.shape}, expected two dimensions"
        raise ValueError(msg)
    n, m = x.shape
    if n > 1 << 16:
        msg = f"{n} rows; at most 65536"
        raise ValueError(msg)
    out = np.empty(n * (n - 1) // 2, dtype=np.float64)
    check(_capi.load_library().pa_rowdist_euclid_host(x.ctypes.data, n, m, out.ctypes.data, int(threads)), "pa_rowdist_euclid_host")
    return out


def linkage_average(condensed, n: int) -> tuple[np.ndarray, np.ndarray]:
    """``(Z, leaves)`` of ``n`` observations with the condensed distances ``condensed``: scipy's
    ``linkage(condensed, method="average")`` table, (n - 1) x 4 float64, and ``dendrogram(Z, no_plot=True)["leaves"]`` as
    uint32.  One observation gives no rows and the leaves ``[0]``."""
    d = np.ascontiguousarray(condensed, dtype=np.float64)
    n = int(n)
    if n < 0 or d.shape != (n * (n - 1) // 2,):
        msg = f"{d.shape} condensed distances for {n} observations, expected ({n * (n - 1) // 2},)"
        raise ValueError(msg)
    z = np.empty((max(n - 1, 0), 4), dtype=np.float64)
    leaves = np.empty(n, dtype=np.uint32)
    check(_capi.load_library().pa_linkage_average(n, d.ctypes.data, z.ctypes.data, leaves.ctypes.data), "pa_linkage_average")
    return z, leaves


def cluster_tree(matrix, na_fill: float, engine=None) -> tuple[np.ndarray, np.ndarray]:
    """``(Z, leaves)`` of the rows of ``matrix`` with its NaN cells replaced by ``na_fill``."""
    x = np.array(matrix, dtype=np.float64)  # a copy: the caller's matrix keeps its NaNs
    x[np.isnan(x)] = na_fill
    if not np.isfinite(x).all():
        msg = "the matrix holds infinite values: row distances are defined for finite values only"
        raise ValueError(msg)
    return linkage_average(row_distances(x, engine), len(x))


def cluster_order(matrix, na_fill: float, engine=None) -> np.ndarray:
    """The leaf order of the average-linkage clustering of the rows of ``matrix`` (NaN cells counted as ``na_fill``)."""
    return cluster_tree(matrix, na_fill, engine)[1]


def heatmap_table(frame, na_fill: float, engine=None):
    """``frame.iloc[leaves, leaves]``: the table of ``<method>_<score>_heatmap.tsv``, rows and columns in the leaf order
    of the clustering of the rows; the NaN cells stay NaN in the output."""
    leaves = cluster_order(frame.to_numpy(dtype=float), na_fill, engine)
    return frame.iloc[leaves, leaves]
