"""search-run: for new genomes, the nearest genomes of a ``sourmash-hip`` run -- the question asked of a curated run
most often, answered without adding the genomes to it.

The reference has no such command, so everything here is this project's own definition; DESIGN.md section 7n has the
contract of the primitive (``pa_best_hits`` on the device, ``pa_best_hits_host`` without one: the same bits) and
``tests/search_cases.py`` restates it independently.  The M x N intersection counts never leave the device: per tile of
subjects one ``pair_counts`` of all queries against it and one accumulating ``best_hits``, and M x top numbers cross the
bus at the end.  Only the hits get their ``identity`` and ``query_cov``, from ``engine.ani_host`` (the reference's bits).
"""

from __future__ import annotations

import math
from pathlib import Path
from typing import NamedTuple

import numpy as np

from . import _capi
from . import engine as engine_mod
from .methods import sourmash_hip

RANKS = ("identity", "containment")
TOP = 5
MAX_TOP = _capi.PA_HITS_MAX_TOP
NONE = _capi.PA_HITS_NONE
# the counts of one device call, nq x DEVICE_TILE_COLUMNS x 4 bytes, stay under this: 131 072 queries a batch
COUNTS_BUDGET_BYTES = 1 << 30
HITS_HEADER = "#query\tsubject\trank\tidentity\tquery_cov\tshared_hashes\tquery_hashes\tsubject_hashes"
QUERIES_HEADER = "#query\tmd5\tlength\thashes\tbest_subject\tbest_identity\tbest_query_cov\thits"


class Hits(NamedTuple):
    """Per query (row) its hits, best first, ``top`` columns: ``subject`` the subject's position (-1: no such rank),
    ``shared`` = |Q n S|, ``identity`` and ``query_cov`` as the run stores them for such a pair (NaN: no such rank), and
    the sketch sizes of the queries and the subjects."""

    subject: np.ndarray
    shared: np.ndarray
    identity: np.ndarray
    query_cov: np.ndarray
    q_size: np.ndarray
    s_size: np.ndarray


def _sizes(sketches, what: str) -> np.ndarray:
    sizes = np.array([len(s) for s in sketches], dtype=np.uint64)
    if sizes.size and (int(sizes.min()) < 1 or int(sizes.max()) >= 1 << 32):
        empty = int(np.flatnonzero(sizes < 1)[0]) if int(sizes.min()) < 1 else int(np.argmax(sizes))
        msg = f"{what} {empty} has a sketch of {int(sizes[empty])} hashes: search needs 1 to 2^32 - 1"
        raise ValueError(msg)
    return sizes


def query_batch(n_queries: int, budget_bytes: int = COUNTS_BUDGET_BYTES) -> int:
    """Queries per device call: all of them, unless their counts against one tile of subjects would pass the budget."""
    return max(1, min(max(int(n_queries), 1), int(budget_bytes) // (sourmash_hip.DEVICE_TILE_COLUMNS * 4)))


def search(subject_sketches, query_sketches, k: int, *, top: int = TOP, rank: str = "identity", engine=None,  # noqa: PLR0913
           budget_bytes: int = COUNTS_BUDGET_BYTES) -> Hits:
    """The ``top`` nearest subjects of every query under ``rank``: the sketches (ascending
    duplicate-free uint64 arrays, none empty) are uploaded once, the subjects are walked in tiles of
    ``sourmash_hip.DEVICE_TILE_COLUMNS``, and the queries are cut into batches only so that the counts of one call stay
    under ``budget_bytes``.  An engine without ``best_hits_device`` (the oracle-backed test engine) makes the selection
    with the host twin, on the counts it returns."""
    if isinstance(top, bool) or not isinstance(top, (int, np.integer)) or not 1 <= top <= MAX_TOP:
        msg = f"Expected 1 to {MAX_TOP} hits a query, not {top!r}"
        raise ValueError(msg)
    if rank not in RANKS:
        msg = f"Unknown rank {rank!r}: expected one of {', '.join(RANKS)}"
        raise ValueError(msg)
    top = int(top)
    q_size, s_size = _sizes(query_sketches, "query"), _sizes(subject_sketches, "subject")
    m, n = len(q_size), len(s_size)
    subject = np.full((m, top), NONE, dtype=np.uint32)
    shared = np.zeros((m, top), dtype=np.uint32)
    if m and n:
        eng = engine or sourmash_hip.get_engine()
        sketches = eng.sketches_from_host([*query_sketches, *subject_sketches])  # the queries first, then the subjects
        on_device = hasattr(eng, "best_hits_device")
        q32, s32 = q_size.astype(np.uint32), s_size.astype(np.uint32)
        if on_device:
            t = eng.torch
            q_dev, s_dev = (t.from_numpy(x.view(np.int32).copy()).to(eng.device) for x in (q32, s32))
        step = query_batch(m, budget_bytes)
        for q0 in range(0, m, step):
            q1 = min(q0 + step, m)
            state = None
            for s0 in range(0, n, sourmash_hip.DEVICE_TILE_COLUMNS):
                s1 = min(s0 + sourmash_hip.DEVICE_TILE_COLUMNS, n)
                counts = eng.pair_counts(sketches, (q0, q1), (m + s0, m + s1))
                if on_device:
                    state = eng.best_hits_device(counts, q_dev[q0:q1], s_dev[s0:s1], s0, rank, top, state)
                else:
                    state = engine_mod.best_hits_host(counts.cpu().numpy().view(np.uint32), q32[q0:q1], s32[s0:s1], s0, rank, top, state)
            found = [x.cpu().numpy().view(np.uint32) for x in state[:2]] if on_device else state[:2]
            subject[q0:q1], shared[q0:q1] = found
    identity = np.full((m, top), math.nan)
    query_cov = np.full((m, top), math.nan)
    for q in range(m):  # the hits only: one row of at most `top` pows per query
        held = int((subject[q] != NONE).sum())
        if held:
            ident, cov, _null = engine_mod.ani_host(shared[q : q + 1, :held], q_size[q : q + 1], s_size[subject[q, :held]], k, threads=1)
            identity[q, :held], query_cov[q, :held] = ident[0], cov[0]
    position = subject.astype(np.int64)
    position[subject == NONE] = -1
    return Hits(position, shared, identity, query_cov, q_size, s_size)


def _kept(hits: Hits, q: int, min_identity: float, cov_min: float) -> list[int]:
    """The ranks (from 0) of query q's hits that pass the thresholds: they filter the top hits and look no further."""
    return [r for r in range(hits.subject.shape[1])
            if hits.subject[q, r] >= 0 and hits.identity[q, r] >= min_identity and hits.query_cov[q, r] >= cov_min]  # fmt: skip


def hits_tsv(hits: Hits, query_labels, subject_labels, *, min_identity: float = 0.0, cov_min: float = 0.0) -> str:
    """``#query subject rank identity query_cov shared_hashes query_hashes subject_hashes``: a row per hit among a query's
    top with identity >= ``min_identity`` and query_cov >= ``cov_min``, queries in order, a query's hits best first;
    ``rank`` (from 1) is the hit's rank before filtering; floats as ``repr``."""
    rows = [HITS_HEADER]
    for q, name in enumerate(query_labels):
        for r in _kept(hits, q, min_identity, cov_min):
            s = int(hits.subject[q, r])
            rows.append(f"{name}\t{subject_labels[s]}\t{r + 1}\t{float(hits.identity[q, r])!r}\t{float(hits.query_cov[q, r])!r}"
                        f"\t{int(hits.shared[q, r])}\t{int(hits.q_size[q])}\t{int(hits.s_size[s])}")  # fmt: skip
    return "\n".join(rows) + "\n"


def queries_tsv(hits: Hits, query_labels, query_md5, query_lengths, subject_labels, *, min_identity: float = 0.0, cov_min: float = 0.0) -> str:  # noqa: PLR0913
    """``#query md5 length hashes best_subject best_identity best_query_cov hits``: a row per query; ``best_*`` is rank 1
    whatever the thresholds say, ``NA`` for a query that shares no hash with any subject; ``hits`` counts the query's
    rows of ``hits_tsv``."""
    rows = [QUERIES_HEADER]
    for q, name in enumerate(query_labels):
        best = ("NA", "NA", "NA")
        if hits.subject.shape[1] and hits.subject[q, 0] >= 0:
            best = (str(subject_labels[int(hits.subject[q, 0])]), repr(float(hits.identity[q, 0])), repr(float(hits.query_cov[q, 0])))
        rows.append(f"{name}\t{query_md5[q]}\t{int(query_lengths[q])}\t{int(hits.q_size[q])}\t" + "\t".join(best)
                    + f"\t{len(_kept(hits, q, min_identity, cov_min))}")  # fmt: skip
    return "\n".join(rows) + "\n"


def write_tables(outdir: Path, method: str, hits: Hits, query_labels, query_md5, query_lengths, subject_labels, *,  # noqa: PLR0913
                 min_identity: float = 0.0, cov_min: float = 0.0) -> list[Path]:
    written = [Path(outdir) / f"{method}_search_hits.tsv", Path(outdir) / f"{method}_search_queries.tsv"]
    written[0].write_text(hits_tsv(hits, query_labels, subject_labels, min_identity=min_identity, cov_min=cov_min))
    written[1].write_text(queries_tsv(hits, query_labels, query_md5, query_lengths, subject_labels, min_identity=min_identity, cov_min=cov_min))
    return written
