"""classify: the genome cliques of a run from its score and coverage matrices (pyani_plus/classify.py:64-207,433-464).

The reference removes the lowest edge of a networkx graph again and again, recomputes the connected components after
every removal and recurses into them: about quadratic in the number of edges.  Here the edges are put into removal
order once (``pa_classify_edges`` on the device, ``pa_classify_edges_host`` without one) and ``pa_classify_cliques``
walks them backwards with a union-find; DESIGN.md section 7b has the equivalence argument.

Defined by this project, not by the reference (whose output depends on ``PYTHONHASHSEED`` there):

* among equal scores the edge with the smaller ``(i, j)`` (label positions, ``i < j``) is removed first;
* row order: if the graph has several components, those that are cliques by smallest member; then the component tree in
  pre-order (roots and children by smallest member), rows already listed skipped; members in label order.
"""

from __future__ import annotations

import ctypes as C
from io import StringIO
from typing import NamedTuple

import numpy as np

from . import _capi
from ._capi import check

AGG_NAMES = ("min", "max", "mean")
MIN_COVERAGE = 0.50
MODES = ("identity", "tANI")


class CliqueInfo(NamedTuple):
    """One row of ``<method>_classify.tsv`` (the reference's ``classify.CliqueInfo``)."""

    n_nodes: int
    max_cov: float | None
    min_score: float | None
    max_score: float | None
    members: list


def agg_code(name: str, role: str) -> int:
    """The library's code of an aggregator name; the reference meets an unknown name as a ``KeyError`` in a logged traceback."""
    if name not in _capi.PA_AGG:
        msg = f"Unknown {role} aggregator {name!r}: expected one of {', '.join(AGG_NAMES)}"
        raise ValueError(msg)
    return _capi.PA_AGG[name]


def _square(matrix, n: int, what: str) -> np.ndarray:
    out = np.ascontiguousarray(matrix, dtype=np.float64)
    if out.shape != (n, n):
        msg = f"{what} matrix has shape {out.shape}, expected ({n}, {n})"
        raise ValueError(msg)
    return out


def tani_scores(hadamard) -> np.ndarray:
    """The score matrix of tANI mode: ``-log(h) if h else nan`` per cell, NaN kept, then ``* -1`` (db_orm.py:588,
    public_cli.py:1269), with the host libm ``log`` that Python's ``math.log`` calls."""
    h = np.ascontiguousarray(hadamard, dtype=np.float64)
    out = np.empty_like(h)
    check(_capi.load_library().pa_classify_tani_host(h.ctypes.data, h.size, out.ctypes.data), "pa_classify_tani_host")
    return out


def edges_host(score, cov, *, score_edges: str = "mean", coverage_edges: str = "min", cov_min: float = MIN_COVERAGE):
    """``(i, j, score, cov)`` of the edges in removal order, computed on the CPU (``pa_classify_edges_host``)."""
    s = np.ascontiguousarray(score, dtype=np.float64)
    n = s.shape[0]
    s, c = _square(s, n, "score"), _square(cov, n, "coverage")
    cap = n * (n - 1) // 2
    e_i, e_j = np.empty(cap, dtype=np.uint32), np.empty(cap, dtype=np.uint32)
    e_s, e_c = np.empty(cap, dtype=np.float64), np.empty(cap, dtype=np.float64)
    count = C.c_uint64(0)
    check(
        _capi.load_library().pa_classify_edges_host(
            s.ctypes.data, c.ctypes.data, n, agg_code(score_edges, "score"), agg_code(coverage_edges, "coverage"), float(cov_min), cap,
            e_i.ctypes.data, e_j.ctypes.data, e_s.ctypes.data, e_c.ctypes.data, C.byref(count),
        ),  # fmt: skip
        "pa_classify_edges_host",
    )
    m = count.value
    return e_i[:m], e_j[:m], e_s[:m], e_c[:m]


def cliques_from_edges(labels: list, e_i, e_j, e_score, e_cov) -> list[CliqueInfo]:
    """The rows from the edges in removal order (``pa_classify_cliques``), in this project's row order."""
    lib = _capi.load_library()
    e_i = np.ascontiguousarray(e_i, dtype=np.uint32)
    e_j = np.ascontiguousarray(e_j, dtype=np.uint32)
    e_score = np.ascontiguousarray(e_score, dtype=np.float64)
    e_cov = np.ascontiguousarray(e_cov, dtype=np.float64)
    assert len(e_i) == len(e_j) == len(e_score) == len(e_cov)
    handle = C.c_void_p()
    check(
        lib.pa_classify_cliques(len(labels), len(e_i), e_i.ctypes.data, e_j.ctypes.data, e_score.ctypes.data, e_cov.ctypes.data, C.byref(handle)),
        "pa_classify_cliques",
    )
    try:
        n_rows, n_members = C.c_uint64(0), C.c_uint64(0)
        check(lib.pa_cliques_info(handle, C.byref(n_rows), C.byref(n_members)), "pa_cliques_info")
        r = n_rows.value
        n_nodes = np.empty(r, dtype=np.uint32)
        max_cov, min_score, max_score = (np.empty(r, dtype=np.float64) for _ in range(3))
        present = np.empty(r, dtype=np.uint8)
        off = np.empty(r + 1, dtype=np.uint64)
        members = np.empty(n_members.value, dtype=np.uint32)
        check(
            lib.pa_cliques_copy(handle, n_nodes.ctypes.data, max_cov.ctypes.data, min_score.ctypes.data, max_score.ctypes.data,
                                present.ctypes.data, off.ctypes.data, members.ctypes.data),
            "pa_cliques_copy",
        )  # fmt: skip
    finally:
        lib.pa_cliques_free(handle)
    rows = []
    for k in range(r):
        flags = int(present[k])
        rows.append(
            CliqueInfo(
                int(n_nodes[k]),
                float(max_cov[k]) if flags & 1 else None,
                float(min_score[k]) if flags & 2 else None,
                float(max_score[k]) if flags & 4 else None,
                [labels[p] for p in members[int(off[k]) : int(off[k + 1])]],
            )
        )
    return rows


def classify_matrices(labels, score, cov, *, coverage_edges: str = "min", score_edges: str = "mean", cov_min: float = MIN_COVERAGE,
                      engine=None) -> list[CliqueInfo]:
    """The clique rows of the graph over ``labels`` (node p = row and column p of ``score`` and ``cov``; rows are
    queries, columns subjects; pass them sorted by label, as the reference's ``relabelled_matrix`` leaves them).

    ``engine``: a ``HipEngine`` builds and sorts the edges on the GPU (``score`` and ``cov`` may then be device
    tensors); None takes the host path.  Both give the same edge list bit for bit."""
    labels = list(labels)
    agg_code(coverage_edges, "coverage")
    agg_code(score_edges, "score")
    if len(labels) != len(score):
        msg = f"{len(labels)} labels for a matrix of {len(score)} rows"
        raise ValueError(msg)
    if engine is None:
        edges = edges_host(score, cov, score_edges=score_edges, coverage_edges=coverage_edges, cov_min=cov_min)
    else:
        edges = engine.classify_edges(score, cov, score_edges=score_edges, coverage_edges=coverage_edges, cov_min=cov_min)
    return cliques_from_edges(labels, *edges)


def classify_tsv(rows: list[CliqueInfo], mode: str = "identity") -> str:
    """The text of ``<method>_classify.tsv`` as the reference writes it (classify.py:454-462): pandas ``round(7)`` and
    ``to_csv(sep="\\t", index=False)``, members joined by commas, ``min_score`` / ``max_score`` named after the mode."""
    import pandas as pd  # loaded when a table is written, not with the module

    suffix = "identity" if mode == "identity" else "-tANI"
    frame = pd.DataFrame(rows)
    frame["members"] = frame["members"].apply(lambda x: ",".join(x))  # noqa: PLW0108
    frame = frame.rename(columns={"min_score": f"min_{suffix}", "max_score": f"max_{suffix}"})
    out = StringIO()
    frame.round(7).to_csv(out, sep="\t", index=False)
    return out.getvalue()
