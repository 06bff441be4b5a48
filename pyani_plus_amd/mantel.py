"""Mantel's permutation test between two distance matrices over the same genomes: do two runs tell the same story, and
is the agreement more than chance?

The reference compares runs with figures only, so everything here is this project's own definition; DESIGN.md section 7j
has the contract of the primitive (``pa_mantel`` on the device, ``pa_mantel_host`` without one: the same bits) and of
the permutations of a seed (``pa_mantel_permutations``), and ``tests/mantel_cases.py`` restates both independently.
"""

from __future__ import annotations

import logging
import math
from pathlib import Path
from typing import NamedTuple

import numpy as np

from . import engine as engine_mod

SLICE_BYTES = 64 << 20  # permutations generated and handed to the primitive at a time, at most
MAX_PERMUTATIONS = 1_000_000
SUMMARY_HEADER = "#run_id\tmethod\tname\tgenomes\tpairs\tmantel_r\tpermutations\tseed\tat_least_observed\tp_value"
NULL_HEADER = "#permutation\tmantel_r"


class MantelTest(NamedTuple):
    """The test of n genomes (``pairs`` = n (n - 1) / 2 distances a matrix).  ``r`` is Mantel's statistic of the matrices
    as they are, ``null_r[q]`` that of permutation q of ``seed``, ``at_least`` the number of permutations whose cross sum
    is at least the observed one (ties count: compared on the cross sums, before any division) and
    ``p = (at_least + 1) / (permutations + 1)``.  Where one matrix is constant off the diagonal no correlation is
    defined: ``r``, ``p`` and ``null_r`` are None.  ``stats`` = (mean_x, mean_y, ss_x, ss_y), ``cross`` the observed
    cross sum."""

    genomes: int
    pairs: int
    r: float | None
    permutations: int
    seed: int
    at_least: int | None
    p: float | None
    null_r: np.ndarray | None
    stats: tuple[float, float, float, float]
    cross: float


def mantel_test(X, Y, permutations: int = 9999, seed: int = 0, engine=None, logger: logging.Logger | None = None, threads: int = 0) -> MantelTest:
    """Mantel's test of the n x n distance matrices ``X`` and ``Y`` (finite, >= 0, symmetric, zero diagonal, n >= 3) with
    ``permutations`` permutations of the genomes of ``Y`` from ``seed``: the cross sums on the GPU of ``engine``, or on
    ``threads`` host threads without one -- the same numbers bit for bit.  The permutations are generated, and handed to
    the primitive, in slices of at most ``SLICE_BYTES``; the matrices go to the device once."""
    x = np.ascontiguousarray(X, dtype=np.float64)
    y = np.ascontiguousarray(Y, dtype=np.float64)
    if x.ndim != 2 or x.shape[0] != x.shape[1] or y.shape != x.shape:
        msg = f"distance matrices of shapes {x.shape} and {y.shape}, expected two square ones of one size"
        raise ValueError(msg)
    permutations, seed = int(permutations), int(seed)
    if permutations < 0:
        msg = f"{permutations} permutations; at least 0"
        raise ValueError(msg)
    n = x.shape[0]
    if engine is not None:
        x, y = (engine.torch.from_numpy(np.array(m)).to(engine.device) for m in (x, y))  # uploaded once
    per_slice = max(1, SLICE_BYTES // (4 * max(n, 1)))
    stats, observed, null = None, None, []
    for first in range(0, max(permutations, 1), per_slice):
        count = min(per_slice, permutations - first)
        perms = engine_mod.mantel_permutations(seed, n, first, count) if count else np.empty((0, n), dtype=np.uint32)
        stats, cross = engine.mantel(x, y, perms) if engine is not None else engine_mod.mantel_host(x, y, perms, threads)
        observed = float(cross[0])  # the same in every slice
        null.append(cross[1:])
    null_cross = np.concatenate(null)
    mean_x, mean_y, ss_x, ss_y = (float(v) for v in stats)
    pairs = n * (n - 1) // 2
    if ss_x == 0 or ss_y == 0:
        (logger or logging.getLogger("pyani_plus_amd")).warning(
            "The distances of %s are all equal: no correlation is defined", "both matrices" if ss_x == 0 and ss_y == 0 else "one matrix")
        return MantelTest(n, pairs, None, permutations, seed, None, None, None, (mean_x, mean_y, ss_x, ss_y), observed)
    scale = math.sqrt(ss_x * ss_y)
    at_least = int(np.count_nonzero(null_cross >= observed))
    return MantelTest(n, pairs, observed / scale, permutations, seed, at_least, (at_least + 1) / (permutations + 1), null_cross / scale,
                      (mean_x, mean_y, ss_x, ss_y), observed)


def _number(value) -> str:
    return "NA" if value is None else repr(value)


def summary_line(run_id: int, method: str, name: str, test: MantelTest) -> str:
    """One line of the summary table under ``SUMMARY_HEADER``: floats as ``repr``, ``NA`` where undefined."""
    return (f"{run_id}\t{method}\t{name}\t{test.genomes}\t{test.pairs}\t{_number(test.r)}\t{test.permutations}\t{test.seed}"
            f"\t{_number(test.at_least)}\t{_number(test.p)}")  # fmt: skip


def write_summary_tsv(path: Path, lines: list[str]) -> None:
    """``SUMMARY_HEADER`` and the lines of ``summary_line``, one per run compared with the reference run."""
    Path(path).write_text("\n".join([SUMMARY_HEADER, *lines]) + "\n")


def write_null_tsv(path: Path, test: MantelTest) -> None:
    """``#permutation TAB mantel_r``: a line per permutation, its number and its statistic as ``repr``; the header alone
    where no correlation is defined."""
    rows = [] if test.null_r is None else [f"{q}\t{r!r}" for q, r in enumerate(test.null_r.tolist())]
    Path(path).write_text("\n".join([NULL_HEADER, *rows]) + "\n")
