"""dereplicate-run: one representative genome per group of a run's threshold graph -- the genome set to carry forward
once an all-vs-all run exists (what dRep, galah and skDER are used for).

The reference has no such command, so everything here is this project's own definition; DESIGN.md section 7k has the
contract of the three primitives (``pa_derep_adjacency``, ``pa_derep_select``, ``pa_derep_assign`` on the device, their
``_host`` twins without one: the same bits) and ``tests/derep_cases.py`` restates it independently.  The primitives know
one priority only, the index of a node; this module turns a preference (the longer genome first, or label order) into
that order and maps the answer back.
"""

from __future__ import annotations

import math
from pathlib import Path
from typing import NamedTuple

import numpy as np

from . import engine as engine_mod

MODES = ("greedy", "cover")
PREFERENCES = ("length", "label")
MIN_IDENTITY = 0.95
MEMBERS_HEADER = "genome\trepresentative\tidentity\tlength"
REPRESENTATIVES_HEADER = "representative\tn_members\tlength\tmin_identity"


class Dereplicated(NamedTuple):
    """The genomes in rank order (``labels``, ``lengths``), ``representative[p]`` the rank of the representative of the
    genome of rank p (its own for a representative), ``identity[p]`` the score of that pair, and the rounds the device
    took (None on the host)."""

    labels: list[str]
    lengths: list[int]
    representative: np.ndarray
    identity: np.ndarray
    rounds: int | None


def rank_order(labels: list[str], lengths: list[int], prefer: str = "length") -> list[int]:
    """The positions of the genomes, the preferred first: ``length`` puts the longer genome first and breaks ties by
    ascending label, ``label`` is label order."""
    if prefer not in PREFERENCES:
        msg = f"Unknown preference {prefer!r}: expected one of {', '.join(PREFERENCES)}"
        raise ValueError(msg)
    if prefer == "label":
        return sorted(range(len(labels)), key=lambda p: labels[p])
    return sorted(range(len(labels)), key=lambda p: (-lengths[p], labels[p]))


def dereplicate_matrices(labels, lengths, score, cov, *, prefer: str = "length", min_identity: float = MIN_IDENTITY, cov_min: float = 0.5,  # noqa: PLR0913
                         score_edges: str = "mean", coverage_edges: str = "min", mode: str = "greedy", engine=None) -> Dereplicated:
    """Dereplicate the genomes ``labels`` (node p = row and column p of ``score`` and ``cov``; rows are queries): the
    matrices are permuted so that index equals rank before they reach the primitives -- on the GPU of ``engine``, or on
    the host without one, with the same bits."""
    labels, lengths = [str(x) for x in labels], [int(x) for x in lengths]
    order = np.array(rank_order(labels, lengths, prefer), dtype=np.int64)
    s = np.ascontiguousarray(np.asarray(score, dtype=np.float64)[np.ix_(order, order)])
    c = np.ascontiguousarray(np.asarray(cov, dtype=np.float64)[np.ix_(order, order)])
    options = {"score_edges": score_edges, "coverage_edges": coverage_edges, "min_score": float(min_identity), "cov_min": float(cov_min), "mode": mode}
    result = engine.dereplicate(s, c, **options) if engine is not None else engine_mod.dereplicate_host(s, c, **options)
    return Dereplicated([labels[p] for p in order], [lengths[p] for p in order], result.rep.astype(np.int64), result.rep_score, result.rounds)


def _number(value: float) -> str:
    return "NA" if math.isnan(value) else str(float(value))


def members_tsv(d: Dereplicated) -> str:
    """``genome, representative, identity, length``: a row per genome, grouped by representative in rank order; within a
    group the representative's own row, then its members in rank order.  ``identity`` as ``str(float)``, ``NA`` for NaN."""
    rows = [MEMBERS_HEADER]
    for r in np.flatnonzero(d.representative == np.arange(len(d.labels))):
        for p in [int(r), *(int(p) for p in np.flatnonzero(d.representative == r) if p != r)]:
            rows.append(f"{d.labels[p]}\t{d.labels[r]}\t{_number(d.identity[p])}\t{d.lengths[p]}")
    return "\n".join(rows) + "\n"


def representatives_tsv(d: Dereplicated) -> str:
    """``representative, n_members, length, min_identity``: a row per representative in rank order; ``n_members`` counts
    the representative itself; ``min_identity`` is the smallest member score, ``NA`` for a representative alone."""
    rows = [REPRESENTATIVES_HEADER]
    for r in np.flatnonzero(d.representative == np.arange(len(d.labels))):
        members = [int(p) for p in np.flatnonzero(d.representative == r) if p != r]
        lowest = min((float(d.identity[p]) for p in members), default=math.nan)
        rows.append(f"{d.labels[r]}\t{len(members) + 1}\t{d.lengths[r]}\t{_number(lowest)}")
    return "\n".join(rows) + "\n"


def write_tables(outdir: Path, method: str, d: Dereplicated) -> list[Path]:
    written = [Path(outdir) / f"{method}_dereplicate.tsv", Path(outdir) / f"{method}_representatives.tsv"]
    written[0].write_text(members_tsv(d))
    written[1].write_text(representatives_tsv(d))
    return written
