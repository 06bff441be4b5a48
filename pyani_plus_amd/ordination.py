"""Ordination of a run: the principal coordinates (classical scaling, Gower 1966) of its distance matrix.

The reference writes no ordination, so everything here is this project's own definition; DESIGN.md section 7i has the
contract of the three steps below (``pa_gower_center``, ``pa_symm_top_eigs`` and, inside it, ``pa_mul_tall_f64`` on the
device; their ``*_host`` twins without one: the same bits) and ``tests/pcoa_cases.py`` restates it independently.
"""

from __future__ import annotations

from typing import NamedTuple

import numpy as np

from . import engine as engine_mod

TOL = 1e-10


class Ordination(NamedTuple):
    """``dimensions`` principal axes of n genomes.  ``eigenvalues`` are the algebraically largest eigenvalues of the
    centred matrix, descending; column c of ``coordinates`` (n x dimensions) is the unit eigenvector times
    ``sqrt(eigenvalue)`` where the eigenvalue is positive and zeros where it is not; ``proportions`` are
    ``eigenvalue / trace``.  The trace is the sum of *all* eigenvalues, the negative ones included (distances from ANI
    are not Euclidean, so there are some): the positive axes together carry more than the trace, and the proportion of
    a positive axis is an upper bound of its share of the positive variation.  Only the whole spectrum could do better,
    and that is what this computation avoids.  ``residuals`` are the pairs' ``||B v - lambda v||``; ``info`` is
    ``(iterations of phase 1, iterations in all, shift used)`` of the solver."""

    eigenvalues: np.ndarray
    coordinates: np.ndarray
    proportions: np.ndarray
    residuals: np.ndarray
    info: tuple[int, int, float]
    trace: float


def pcoa(D, dimensions: int = 3, engine=None, tol: float = TOL, threads: int = 0) -> Ordination:
    """The principal coordinates of the distance matrix ``D`` (finite, >= 0, symmetric, zero diagonal): the centring and
    the solver's products on the GPU of ``engine``, or on ``threads`` host threads without one -- the same numbers bit
    for bit.  One genome is one point at the origin: its only eigenvalue is 0, no axis carries anything."""
    d = np.ascontiguousarray(D, dtype=np.float64)
    if d.ndim != 2 or d.shape[0] != d.shape[1]:
        msg = f"distance matrix of shape {d.shape}, expected a square one"
        raise ValueError(msg)
    n = d.shape[0]
    dimensions = int(dimensions)
    if dimensions < 1:
        msg = f"{dimensions} dimensions; at least 1"
        raise ValueError(msg)
    if dimensions > n:
        msg = f"{dimensions} dimensions for {n} genomes: at most as many axes as genomes"
        raise ValueError(msg)
    if engine is not None:
        b, trace, fro2 = engine.gower_center_device(d)
        values, vectors, residuals, info = engine.symm_top_eigs(b, dimensions, fro2, tol)
    else:
        b, trace, fro2 = engine_mod.gower_center_host(d, threads)
        values, vectors, residuals, info = engine_mod.symm_top_eigs_host(b, dimensions, fro2, tol, threads=threads)
    positive = values > 0
    coordinates = np.where(positive[None, :], vectors * np.sqrt(np.where(positive, values, 0.0))[None, :], 0.0)
    with np.errstate(divide="ignore", invalid="ignore"):
        proportions = np.where(trace > 0, values / trace, 0.0)
    return Ordination(values, coordinates, proportions, residuals, info, trace)


def coordinates_tsv(result: Ordination, labels) -> str:
    """``genome, PC1 .. PCk``: one row per genome in the order of ``labels``, values as ``repr(float)``."""
    k = result.coordinates.shape[1]
    lines = ["\t".join(["genome"] + [f"PC{c + 1}" for c in range(k)])]
    for name, row in zip(labels, result.coordinates.tolist()):
        lines.append("\t".join([str(name)] + [repr(float(x)) for x in row]))
    return "\n".join(lines) + "\n"


def eigenvalues_tsv(result: Ordination) -> str:
    """``component, eigenvalue, proportion_of_trace, cumulative, residual``; ``cumulative`` is the running sum of the
    proportions."""
    lines = ["component\teigenvalue\tproportion_of_trace\tcumulative\tresidual"]
    running = 0.0
    for c, (value, share, residual) in enumerate(zip(result.eigenvalues.tolist(), result.proportions.tolist(), result.residuals.tolist())):
        running = running + share
        lines.append(f"PC{c + 1}\t{value!r}\t{share!r}\t{running!r}\t{residual!r}")
    return "\n".join(lines) + "\n"
