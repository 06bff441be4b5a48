"""Substitution distances of an alignment's rows (``phylo-run``): the p distance and the Jukes-Cantor (JC69) and Kimura
two-parameter (K80) corrections of it, their neighbour-joining tree and its column bootstrap.

The reference has no such distance, so everything here is this project's own definition; DESIGN.md section 7m has the
contract and ``tests/subst_cases.py`` restates it independently.  Per pair of rows three counts are taken over the
columns where both rows hold a nucleotide -- the columns themselves, the transitions and the transversions among them
(``pa_msa_subst_counts`` on the device, ``pa_msa_subst_counts_host`` without one: the same integers) -- and the model
turns them into a distance (``pa_subst_distances`` and its twin: the same bits, the logarithm included).  The tree is
``tree.neighbour_joining`` of those distances; the bootstrap is ``bootstrap.bootstrap`` with the counts and distances of
a batch of replicates made here: the same column draws, the same loop, the same ``pa_tree_support``.
"""

from __future__ import annotations

from typing import NamedTuple

import numpy as np

from . import bootstrap as bootstrap_mod
from . import engine as engine_mod
from .tree import JoinTable, neighbour_joining

MODELS = tuple(engine_mod.SUBST_MODELS)  # p, jc69, k80
DEFAULT_MODEL = "k80"
DEFAULT_MISSING = 3.0
# counts (three uint32) and distances (one float64) of a replicate are 20 bytes a cell
CELL_BYTES = 20


class Phylo(NamedTuple):
    """The distances of the alignment's rows (n x n float64), the pairs without a shared nucleotide column and the
    saturated pairs among them, their neighbour-joining tree, and its bootstrap (None without replicates)."""

    distances: np.ndarray
    no_columns: int
    saturated: int
    table: JoinTable
    bootstrap: bootstrap_mod.Bootstrap | None


def batch_distances(rows, n_cols: int, weights, model: str, missing: float, *, engine=None, device_msa=None, threads: int = 0):
    """``(D, undefined)`` of the alignment under each row of ``weights`` (None: every column once, one matrix):
    float64 ``[R, n, n]`` -- on the device with ``engine`` and ``device_msa`` (the rows as ``HipEngine.msa_subst_upload``
    packs them), on the host without -- and uint64 ``[R, 2]``, the undefined pairs of each matrix by kind."""
    if engine is not None:
        return engine.subst_distances(*engine.msa_subst_counts(device_msa, weights), model, missing)
    return engine_mod.subst_distances_host(*engine_mod.msa_subst_counts_host(rows, n_cols, weights, threads), model, missing, threads)


def replicate_step(model: str) -> bootstrap_mod.DistanceStep:
    """The step ``bootstrap.replicate_trees`` makes a batch's distances with, for ``model``."""

    def distances(rows, n_cols, weights, missing, *, engine=None, device_msa=None, threads=0):
        return batch_distances(rows, n_cols, weights, model, missing, engine=engine, device_msa=device_msa, threads=threads)[0]

    return bootstrap_mod.DistanceStep(distances, CELL_BYTES)


def phylo(rows: np.ndarray, n_cols: int, model: str = DEFAULT_MODEL, missing: float = DEFAULT_MISSING, replicates: int = 0, seed: int = 0, *,
          engine=None, device_msa=None, threads: int = 0) -> Phylo:  # fmt: skip
    """Distances, tree and -- with ``replicates`` > 0 -- bootstrap of the alignment ``rows`` (uint8, n x stride, the first
    ``n_cols`` bytes of a row its columns), in the rows' order."""
    d, undefined = batch_distances(rows, n_cols, None, model, missing, engine=engine, device_msa=device_msa, threads=threads)
    distances = d[0].cpu().numpy() if engine is not None else d[0]
    table = neighbour_joining(distances, engine=engine, threads=threads)
    result = None
    if replicates:
        result = bootstrap_mod.bootstrap(table, rows, n_cols, replicates, seed, missing, engine=engine, device_msa=device_msa, threads=threads,
                                         step=replicate_step(model))  # fmt: skip
    return Phylo(distances, int(undefined[0, 0]), int(undefined[0, 1]), table, result)


def distances_tsv(distances: np.ndarray, labels) -> str:
    """A labelled square matrix in the layout of export-run's matrices (an empty corner cell, the labels across, then a
    line per row that starts with its label), the values as ``repr``."""
    lines = ["\t".join(["", *labels]) + "\n"]
    for label, row in zip(labels, distances):
        lines.append("\t".join([label, *(repr(float(v)) for v in row)]) + "\n")
    return "".join(lines)
