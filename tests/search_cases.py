"""search-run's ranking rule restated in plain Python, and the cases the tests share.

The restatement is written from the contract, not from the C++ or from ``pyani_plus_amd/search.py``, and shares no code
with either: per query, every subject with I = |Q n S| > 0 is a hit with the exact ratio ``Fraction(I, m)`` -- m is
min(|Q|, |S|) under ``identity`` and |Q| under ``containment`` -- and the hits are ``sorted`` by descending ratio, then
descending I, then ascending subject index.  The best ``top`` of them are the answer; every comparison made with it is
an exact comparison of integers.

The cases are synthetic ``counts`` / ``q_size`` / ``s_size`` (they need not come from real sketches) and do not depend
on ``top`` or on the rank, so one restatement at the largest ``top`` serves all of them: the best ``top`` of a sorted
list are its first ``top``.  Past ``THIN_FROM`` columns only every ``DENSE_EVERY``-th query keeps a dense row; the others
keep the columns their family is about and a random hundred more, which keeps the exact arithmetic of the
restatement affordable without taking a column seam away from any family.
"""

from __future__ import annotations

import functools
from fractions import Fraction

import numpy as np

NONE = 0xFFFFFFFF
MAX_TOP = 64
RANKS = ("identity", "containment")
FAMILIES = ("random", "all_zero", "one_hit", "fewer_than_top", "equal_ratio", "identical", "last_column_wins", "winners_in_one_lane",
            "extreme", "q_smaller")  # fmt: skip
U32 = (1 << 32) - 1
THIN_FROM, DENSE_EVERY, THIN_KEEP = 128, 32, 100


# ------------------------------------------------------------------ the contract
def denominator(rank: str, q: int, s: int) -> int:
    if rank == "identity":
        return min(q, s)
    if rank == "containment":
        return q
    raise ValueError(rank)


@functools.lru_cache(maxsize=1 << 16)
def ratio(shared: int, denom: int) -> Fraction:
    return Fraction(shared, denom)


def ranked(row, q: int, s_size, rank: str, s_base: int = 0, before=()) -> list[tuple[int, int, int]]:
    """All hits of one query as ``(subject, I, m)``, best first.  ``before``: hits of other tiles, as such triples."""
    row, sizes, q = np.asarray(row, dtype=np.uint64).tolist(), np.asarray(s_size, dtype=np.uint64).tolist(), int(q)  # Python integers: exact
    hits = [(s_base + c, i, denominator(rank, q, sizes[c])) for c, i in enumerate(row) if i > 0]
    hits += [tuple(int(x) for x in h) for h in before]
    return sorted(hits, key=lambda h: (-ratio(h[1], h[2]), -h[1], h[0]))


def best_hits(counts, q_size, s_size, rank: str, top: int, s_base: int = 0):
    """``(subject, shared, denom)``: three nq x top uint32 arrays, a missing rank ``NONE``, 0, 0."""
    nq = len(q_size)
    out = (np.full((nq, top), NONE, dtype=np.uint32), np.zeros((nq, top), dtype=np.uint32), np.zeros((nq, top), dtype=np.uint32))
    for q in range(nq):
        for r, hit in enumerate(ranked(counts[q] if len(s_size) else (), q_size[q], s_size, rank, s_base)[:top]):
            for array, value in zip(out, hit):
                array[q, r] = value
    return out


# ------------------------------------------------------------------ the cases
def _thin(rng, counts: np.ndarray, special) -> None:
    """Past THIN_FROM columns, the rows that are not every DENSE_EVERY-th keep ``special`` and THIN_KEEP random columns."""
    nq, ns = counts.shape
    if ns <= THIN_FROM:
        return
    for q in range(nq):
        if q % DENSE_EVERY:
            keep = np.zeros(ns, dtype=bool)
            keep[rng.choice(ns, THIN_KEEP, replace=False)] = True
            keep[np.asarray(special(q), dtype=np.int64)] = True
            counts[q, ~keep] = 0


@functools.lru_cache(maxsize=None)
def case(family: str, nq: int, ns: int):  # noqa: C901, PLR0912, PLR0915
    """``(counts [nq x ns], q_size [nq], s_size [ns])`` as uint32 arrays; read-only, shared between tests."""
    rng = np.random.default_rng([FAMILIES.index(family), nq, ns])
    q_size = rng.integers(3000, 7000, nq).astype(np.uint32)
    s_size = rng.integers(3000, 7000, ns).astype(np.uint32)
    counts = np.zeros((nq, ns), dtype=np.uint32)
    none = lambda _q: []  # noqa: E731
    if family == "random":  # a small palette of counts, so equal ratios and equal counts are common
        counts[:] = rng.choice(np.array([0, 0, 1, 2, 3, 1000, 1500, 2000, 2999, 3000], dtype=np.uint32), (nq, ns))
        _thin(rng, counts, none)
    elif family == "all_zero":
        pass
    elif family == "one_hit":
        counts[np.arange(nq), rng.integers(0, ns, nq)] = rng.integers(1, 3000, nq)
    elif family == "fewer_than_top":  # 0, 1, 2, 3 hits, query by query: fewer than any top for some query
        for q in range(nq):
            cols = rng.choice(ns, min(q % 4, ns), replace=False)
            counts[q, cols] = rng.integers(1, 3000, len(cols))
    elif family == "equal_ratio":  # 1/2, 2/4, 3/6, ... under identity (every |S| below every |Q|): the larger I first
        q_size[:] = 60000
        s_size[:] = 2 * (1 + rng.integers(0, 12, ns))
        counts[:] = s_size // 2
        _thin(rng, counts, none)
    elif family == "identical":  # the same I and m everywhere: index order
        q_size[:], s_size[:], counts[:] = 5000, 4000, 1234
        _thin(rng, counts, none)
    elif family == "last_column_wins":
        s_size[:] = 4000
        counts[:] = rng.integers(1, 2000, (nq, ns))
        counts[:, ns - 1] = 2500
        _thin(rng, counts, lambda _q: [ns - 1])
    elif family == "winners_in_one_lane":  # the best MAX_TOP all at columns = lane (mod 64), and (mod 256) where ns allows
        s_size[:] = 4000
        counts[:] = rng.integers(1, 1000, (nq, ns))
        stride = 256 if ns > 256 * 8 else 64  # noqa: PLR2004
        lanes = [int(rng.integers(0, min(stride, ns))) for _ in range(nq)]
        for q in range(nq):
            counts[q, lanes[q] :: stride] = 2000 + rng.integers(0, 3, len(range(lanes[q], ns, stride)))
        _thin(rng, counts, lambda q: list(range(lanes[q], ns, stride)))
    elif family == "extreme":  # (a - 1) / a against (a - 2) / (a - 1): one unit of the u64 cross product apart
        q_size[:] = U32  # above every subject size, so that m = |S| under identity
        s_size[:] = U32 - 1 - rng.integers(0, 6, ns)
        counts[:] = s_size - 1 - rng.integers(0, 2, (nq, ns)).astype(np.uint32)
        _thin(rng, counts, none)
    elif family == "q_smaller":  # under identity the denominator switches between |Q| and |S| along the row
        q_size[:] = rng.integers(4990, 5010, nq)
        s_size[:] = rng.integers(4980, 5020, ns)
        counts[:] = rng.integers(4900, 4980, (nq, ns))
        _thin(rng, counts, none)
    else:
        raise ValueError(family)
    for array in (counts, q_size, s_size):
        array.flags.writeable = False
    return counts, q_size, s_size


@functools.lru_cache(maxsize=None)
def expected(family: str, nq: int, ns: int, rank: str):
    """The restatement of ``case(family, nq, ns)`` at ``MAX_TOP``; its first ``top`` columns are the answer for ``top``."""
    out = best_hits(*case(family, nq, ns), rank, MAX_TOP)
    for array in out:
        array.flags.writeable = False
    return out


def expected_top(family: str, nq: int, ns: int, rank: str, top: int):
    return tuple(np.ascontiguousarray(a[:, :top]) for a in expected(family, nq, ns, rank))


def same(got, want) -> bool:
    return all(np.asarray(g).dtype == np.uint32 and np.array_equal(g, w) for g, w in zip(got, want)) and len(got) == len(want) == 3  # noqa: PLR2004


def cuts(ns: int, pieces: int, rng, *, ones: bool = False) -> list[tuple[int, int]]:
    """``pieces`` column ranges that tile [0, ns) (fewer when ns is smaller); ``ones``: ranges of width 1 among them."""
    pieces = max(1, min(pieces, ns))
    inner = sorted(rng.choice(np.arange(1, ns), pieces - 1, replace=False).tolist()) if pieces > 1 else []
    if ones and pieces > 2 and ns > 3:  # noqa: PLR2004
        inner = sorted({*inner[:-2], 1, ns - 1})
    edges = [0, *inner, ns]
    return [(a, b) for a, b in zip(edges[:-1], edges[1:]) if b > a]
