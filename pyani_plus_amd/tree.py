"""Trees of a run: distances from its identity matrix, neighbour joining and UPGMA, and the Newick text.

The reference writes no tree, so everything here is this project's own definition; DESIGN.md section 7h has the
contract of the neighbour joining (``pa_nj`` on the device, ``pa_nj_host`` without one: the same bits) and
``tests/tree_cases.py`` restates it independently.  UPGMA is the existing average linkage (``pa_linkage_average``, on the
host) applied to the distances themselves, not to matrix rows as ``plot-run`` applies it.
"""

from __future__ import annotations

import logging
import re
from typing import NamedTuple

import numpy as np

from . import cluster as cluster_mod
from . import engine as engine_mod

METHODS = ("nj", "upgma")
_PLAIN_LABEL = re.compile(r"[A-Za-z0-9_.\-]+")


class JoinTable(NamedTuple):
    """A tree over the leaves ``0 .. n - 1``: join ``t`` makes node ``n + t`` from ``child[t]`` with the branch lengths
    ``length[t]``.  Neighbour joining (``rooted`` False) makes n - 2 joins and ends with the edge ``last`` of length
    ``last_len`` between the two nodes that remain; UPGMA (``rooted`` True) makes n - 1 and its last node is the root."""

    n: int
    child: np.ndarray  # (joins, 2) uint32
    length: np.ndarray  # (joins, 2) float64
    last: tuple[int, int] | None
    last_len: float
    rooted: bool


def run_distances(identity, missing: float = 1.0, logger: logging.Logger | None = None) -> np.ndarray:
    """The symmetric distance matrix of a run's identity matrix (a frame or an array, NaN where there is no value):
    ``d = 1.0 - s`` with ``s = 0.5 * (id[i, j] + id[j, i])``; where one direction is NaN the other is used alone; where
    both are, ``d = missing`` (the number of such pairs is logged: fastANI runs have many); the diagonal is 0."""
    x = np.array(identity.to_numpy(dtype=float) if hasattr(identity, "to_numpy") else identity, dtype=np.float64)
    if x.ndim != 2 or x.shape[0] != x.shape[1]:
        msg = f"identity matrix of shape {x.shape}, expected a square one"
        raise ValueError(msg)
    y = x.T
    one = np.isnan(x) & ~np.isnan(y)
    s = 0.5 * (np.where(one, y, x) + np.where(np.isnan(y) & ~np.isnan(x), x, y))
    none = np.isnan(s)
    d = np.where(none, float(missing), 1.0 - s)
    np.fill_diagonal(d, 0.0)
    n_missing = (int(none.sum()) - int(np.isnan(np.diagonal(x)).sum())) // 2
    if n_missing:
        (logger or logging.getLogger("pyani_plus_amd")).warning(
            "%d of %d genome pairs have no identity in either direction: distance %r", n_missing, x.shape[0] * (x.shape[0] - 1) // 2, float(missing)
        )
    return np.ascontiguousarray(d)


def neighbour_joining(D, engine=None, threads: int = 0) -> JoinTable:
    """The neighbour-joining tree of the distance matrix ``D`` (finite, >= 0, symmetric, zero diagonal): every join on
    the GPU of ``engine``, or on the host without one -- the same table bit for bit."""
    d = np.ascontiguousarray(D, dtype=np.float64)
    child, length, last, last_len = engine.nj_tree(d) if engine is not None else engine_mod.nj_tree_host(d, threads)
    n = d.shape[0]
    return JoinTable(n, child, length, (int(last[0]), int(last[1])) if n >= 2 else None, float(last_len), False)


def upgma(D) -> JoinTable:
    """The UPGMA tree of ``D``: average linkage of the condensed distances (``pa_linkage_average``), a node's height half
    the distance at which it was made, a branch's length its parent's height minus its child's."""
    d = np.ascontiguousarray(D, dtype=np.float64)
    if d.ndim != 2 or d.shape[0] != d.shape[1]:
        msg = f"distance matrix of shape {d.shape}, expected a square one"
        raise ValueError(msg)
    n = d.shape[0]
    if n < 2:
        return JoinTable(n, np.empty((0, 2), np.uint32), np.empty((0, 2), np.float64), None, 0.0, True)
    z, _ = cluster_mod.linkage_average(d[np.triu_indices(n, 1)], n)
    child = z[:, :2].astype(np.uint32)
    height = np.concatenate([np.zeros(n), z[:, 2] / 2.0])
    length = height[n:, None] - height[child]
    return JoinTable(n, child, length, None, 0.0, True)


def quote_label(label: str) -> str:
    """A Newick label: as it is when made of ``[A-Za-z0-9_.-]`` only, else single-quoted with inner quotes doubled."""
    label = str(label)
    return label if _PLAIN_LABEL.fullmatch(label) else "'" + label.replace("'", "''") + "'"


def newick(table: JoinTable, labels, support=None) -> str:
    """The tree as one line of Newick text.  Lengths are ``repr(float)``, which round-trips the bits.  A neighbour-joining
    tree is unrooted, so its root is a trifurcation: the two children of the last node made, then the other remaining
    node, which carries ``last_len``; two leaves give ``(A:h,B:h);`` with ``h = 0.5 * d`` and one gives ``(A);``.  A
    UPGMA tree starts from its last node.  The writer keeps its own stack: a caterpillar tree is as deep as it is long.

    ``support``: one integer per join; every internal node but the root of the text then carries, as its label, the
    entry of its join, which is the support of the edge above it (``bootstrap-run``).  Without it the text has no
    internal labels."""
    names = [quote_label(x) for x in labels]
    n = table.n
    if support is not None and len(support) != len(table.child):
        msg = f"{len(support)} support values for {len(table.child)} joins"
        raise ValueError(msg)
    if len(names) != n:
        msg = f"{len(names)} labels for {n} leaves"
        raise ValueError(msg)
    if n == 0:
        return ";"
    if n == 1:
        return f"({names[0]});"
    child, length = table.child, table.length

    def lens(t: int) -> tuple[float, float]:
        return float(length[t, 0]), float(length[t, 1])

    if table.rooted:
        t = len(child) - 1
        top = [(int(child[t, 0]), lens(t)[0]), (int(child[t, 1]), lens(t)[1])]
    elif n == 2:
        half = 0.5 * table.last_len
        top = [(table.last[0], half), (table.last[1], half)]
    else:
        a, b = table.last  # b is the last node made: the largest id of all
        t = b - n
        top = [(int(child[t, 0]), lens(t)[0]), (int(child[t, 1]), lens(t)[1]), (a, table.last_len)]
    out: list[str] = ["("]
    # (node, its branch length, 0: to open / 1: to close), last to first
    stack: list[tuple[int, float, int]] = []
    for k, (node, ln) in enumerate(reversed(top)):
        stack.append((node, ln, 0))
        if k + 1 < len(top):
            stack.append((-1, 0.0, 2))  # a comma
    while stack:
        node, ln, state = stack.pop()
        if state == 2:
            out.append(",")
        elif state == 1:
            out.append(f"):{ln!r}" if support is None else f"){int(support[node - n])}:{ln!r}")
        elif node < n:
            out.append(f"{names[node]}:{ln!r}")
        else:
            t = node - n
            out.append("(")
            stack.append((node, ln, 1))
            stack.append((int(child[t, 1]), float(length[t, 1]), 0))
            stack.append((-1, 0.0, 2))
            stack.append((int(child[t, 0]), float(length[t, 0]), 0))
    out.append(");")
    return "".join(out)
