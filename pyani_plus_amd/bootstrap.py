"""Column-bootstrap support of a neighbour-joining tree (``bootstrap-run``): Felsenstein's bootstrap over the columns of
the alignment of an ``external-alignment-hip`` run.

The reference writes no tree and no support, so everything here is this project's own definition; DESIGN.md section 7l
has the contract and ``tests/bootstrap_cases.py`` restates it independently.  A replicate draws as many columns as the
alignment has, with replacement (``pa_msa_boot_weights``); its pair counts are the alignment's under those column
weights (``pa_msa_boot_counts`` on the device, ``pa_msa_boot_counts_host`` without one: the same integers), its
distances ``1 - M / aln_length`` (``pa_msa_boot_distances`` and its twin: the same bits) and its tree the
neighbour-joining tree of those (``pa_nj`` / ``pa_nj_host``, unchanged).  The support of an edge of the reference tree
is the number of replicate trees that have an edge with the same leaves on either side (``pa_tree_support``).

This module owns the loop over the batches of replicates.  On the device a batch's counts, distances and joins stay
there: per replicate only the weights go up and the join table comes back.
"""

from __future__ import annotations

from typing import Callable, NamedTuple

import numpy as np

from . import _capi
from . import engine as engine_mod
from .tree import JoinTable, newick

MAX_REPLICATES = 100_000
# what a batch may hold of its replicates' counts and distances
DEVICE_BATCH_BYTES = 4 << 30
HOST_BATCH_BYTES = 1 << 30


class Bootstrap(NamedTuple):
    """The reference tree, ``support[t]`` of the edge above its node ``n + t`` among ``replicates`` replicate trees, and
    the replicate trees themselves in replicate order."""

    table: JoinTable
    support: np.ndarray  # (joins,) uint32
    replicates: int
    trees: list  # JoinTable per replicate


class DistanceStep(NamedTuple):
    """What a batch of replicates' distances are made with: ``distances(rows, n_cols, weights, missing, engine=,
    device_msa=, threads=)`` gives the batch's matrices (``[R, n, n]`` float64, on the device with an engine, on the host
    without), and ``cell_bytes`` is what a replicate's counts and distances take a cell."""

    distances: Callable
    cell_bytes: int


def _identity_distances(rows, n_cols: int, weights, missing: float, *, engine=None, device_msa=None, threads: int = 0):
    """``1 - identity`` of the weighted pair counts (sections 3 and 4 of the contract)."""
    if engine is not None:
        return engine.msa_boot_distances(*engine.msa_boot_counts(device_msa, weights), missing)
    return engine_mod.msa_boot_distances_host(*engine_mod.msa_boot_counts_host(rows, n_cols, weights, threads), missing, threads)


# counts (two uint32) and distances (one float64) of a replicate are 16 bytes a cell
IDENTITY_STEP = DistanceStep(_identity_distances, 16)


def batch_size(n: int, replicates: int, on_device: bool, cell_bytes: int = IDENTITY_STEP.cell_bytes) -> int:
    """Replicates per batch: at most a launch's ``PA_MSA_BOOT_BATCH``, and what the batch's matrices may take."""
    fit = (DEVICE_BATCH_BYTES if on_device else HOST_BATCH_BYTES) // max(cell_bytes * n * n, 1)
    return int(max(1, min(_capi.PA_MSA_BOOT_BATCH, replicates, fit)))


def replicate_trees(rows: np.ndarray, n_cols: int, replicates: int, seed: int, missing: float = 1.0, *, engine=None, device_msa=None,
                    threads: int = 0, step: DistanceStep = IDENTITY_STEP) -> list[JoinTable]:  # fmt: skip
    """The neighbour-joining trees of replicates ``0 .. replicates - 1`` of ``seed`` over the alignment ``rows`` (uint8,
    n x stride, the first ``n_cols`` bytes of a row its columns).  ``engine`` with ``device_msa`` (the rows as the step's
    upload packs them; ``HipEngine.msa_upload`` for the default): counts, distances and joins on the GPU; None: on the
    host, the same tables.  ``step``: how a batch's distances are made (default: ``1 - identity``, bootstrap-run's;
    ``substitution.replicate_step`` for phylo-run's models)."""
    n = int(rows.shape[0])
    trees: list[JoinTable] = []
    batch = batch_size(n, replicates, engine is not None, step.cell_bytes)
    for first in range(0, replicates, batch):
        count = min(batch, replicates - first)
        weights = engine_mod.msa_boot_weights(seed, n_cols, first, count)
        distances = step.distances(rows, n_cols, weights, missing, engine=engine, device_msa=device_msa, threads=threads)
        if engine is not None:
            joined = [engine.nj_tree_inplace(distances[r]) for r in range(count)]
        else:
            joined = [engine_mod.nj_tree_host(distances[r], threads) for r in range(count)]
        for child, length, last, last_len in joined:
            trees.append(JoinTable(n, child, length, (int(last[0]), int(last[1])), float(last_len), False))
    return trees


def bootstrap(table: JoinTable, rows: np.ndarray, n_cols: int, replicates: int, seed: int, missing: float = 1.0, *, engine=None, device_msa=None,
              threads: int = 0, step: DistanceStep = IDENTITY_STEP) -> Bootstrap:  # fmt: skip
    """The support of every edge of the reference tree ``table`` (over the rows of ``rows``, in their order) among the
    replicate trees of ``replicate_trees``."""
    trees = replicate_trees(rows, n_cols, replicates, seed, missing, engine=engine, device_msa=device_msa, threads=threads, step=step)
    joins = max(table.n - 2, 0)
    rep_child = np.stack([t.child for t in trees]) if trees else np.empty((0, joins, 2), dtype=np.uint32)
    return Bootstrap(table, engine_mod.tree_support(table.n, table.child, rep_child), replicates, trees)


def labelled_nodes(table: JoinTable) -> list[tuple[int, int, float]]:
    """``(node, leaves below it in the join table, length of the edge above it)`` of every node that carries a label in
    the Newick text: the nodes made, but for the last, which is the root of the text; ascending."""
    n, child, length = table.n, table.child, table.length
    leaves = np.ones(n + len(child), dtype=np.int64)
    above = np.full(n + len(child), float(table.last_len))  # the one node no join takes has the last edge above it
    for t in range(len(child)):
        leaves[n + t] = leaves[int(child[t, 0])] + leaves[int(child[t, 1])]
        above[int(child[t, 0])], above[int(child[t, 1])] = float(length[t, 0]), float(length[t, 1])
    return [(n + t, int(leaves[n + t]), float(above[n + t])) for t in range(len(child) - 1)]


def support_tsv(result: Bootstrap) -> str:
    """``#node TAB n_leaves TAB length TAB support TAB replicates``, a line per labelled node; the length as ``repr``."""
    lines = ["#node\tn_leaves\tlength\tsupport\treplicates\n"]
    for node, leaves, length in labelled_nodes(result.table):
        lines.append(f"{node}\t{leaves}\t{length!r}\t{int(result.support[node - result.table.n])}\t{result.replicates}\n")
    return "".join(lines)


def support_newick(result: Bootstrap, labels) -> str:
    """The reference tree with each internal node's support as its label."""
    return newick(result.table, labels, support=result.support)
