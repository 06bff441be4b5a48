"""dereplicate-run's contract restated in plain Python and numpy, and the cases the tests share.

The restatement is written from the contract, not from the C++: the aggregate of a pair's two cells, the edge rule, the
bit matrix, the two selection rules as loops over sets of nodes, and the assignment.  Every comparison made with it is
exact: selections are integers and scores are compared by their bits (a NaN with a NaN: which NaN an addition of two
NaNs gives is the hardware's business, and only a representative whose own diagonal cell is NaN has such a score).

The cases: a wanted graph from one of the ``FAMILIES`` at one of the ``SIZES`` (around a word of 64 bits, a wave and a
tile), realised by asymmetric score and coverage matrices for a pair of aggregators, with NaN cells, values exactly at
both thresholds (score == min_score is an edge, cov == cov_min is not), scores from a small palette so that equal scores
to two representatives are common, and anything at all on the diagonals.
"""

from __future__ import annotations

import functools

import numpy as np

SIZES = (1, 2, 3, 63, 64, 65, 127, 128, 129, 257, 1025)
FAMILIES = ("none", "complete", "path", "path_reverse", "star_first", "star_last", "blocks", "gnp")
AGGS = ("min", "max", "mean")
MODES = ("greedy", "cover")
MIN_SCORE = 0.90625  # every number below is a multiple of 2^-10, so a mean of two of them is exact
COV_MIN = 0.5
STEP = 1.0 / 1024.0
NONE = 0xFFFFFFFF


def bits(values) -> np.ndarray:
    return np.ascontiguousarray(values, dtype=np.float64).view(np.uint64)


def same_scores(got, want) -> bool:
    """Equal bit for bit; a NaN equals a NaN."""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    nan = np.isnan(want)
    return got.shape == want.shape and np.array_equal(np.isnan(got), nan) and np.array_equal(bits(got[~nan]), bits(want[~nan]))


# ------------------------------------------------------------------ the contract
def agg(how: str, a: float, b: float) -> float:
    """classify's aggregators on a = M[hi, lo], b = M[lo, hi]: Python's ``min([a, b])``, ``max([a, b])``, ``numpy.mean``."""
    if how == "min":
        return b if b < a else a
    if how == "max":
        return b if b > a else a
    return (np.float64(a) + np.float64(b)) / np.float64(2.0)


def pair_value(M: np.ndarray, how: str, p: int, q: int) -> float:
    lo, hi = min(p, q), max(p, q)
    return agg(how, M[hi, lo], M[lo, hi])


def pair_values(M: np.ndarray, how: str) -> np.ndarray:
    """``pair_value`` of every (p, q) at once: the same three formulas on whole arrays."""
    n = len(M)
    upper = np.arange(n)[:, None] < np.arange(n)[None, :]  # p < q: hi = q
    a = np.where(upper, M.T, M)  # M[hi, lo]
    b = np.where(upper, M, M.T)  # M[lo, hi]
    with np.errstate(invalid="ignore"):
        if how == "min":
            return np.where(b < a, b, a)
        if how == "max":
            return np.where(b > a, b, a)
        return (a + b) / 2.0


def adjacency(S, C, score_edges: str, coverage_edges: str, min_score: float, cov_min: float) -> np.ndarray:
    """The n x n boolean adjacency: neither aggregate NaN, cov > cov_min, score >= min_score; the diagonal set."""
    score, cov = pair_values(np.asarray(S), score_edges), pair_values(np.asarray(C), coverage_edges)
    with np.errstate(invalid="ignore"):
        adj = ~np.isnan(score) & ~np.isnan(cov) & (cov > cov_min) & (score >= min_score)
    np.fill_diagonal(adj, True)
    return adj


def pack(adj: np.ndarray) -> np.ndarray:
    """The bit matrix: bit b of word w of row a is adj[a, 64 w + b]; padding bits zero."""
    n = len(adj)
    words = (n + 63) // 64
    out = np.zeros((n, words), dtype=np.uint64)
    for col in range(n):
        out[:, col // 64] |= adj[:, col].astype(np.uint64) << np.uint64(col % 64)
    return out


def unpack(words: np.ndarray, n: int) -> np.ndarray:
    words = np.asarray(words, dtype=np.uint64).reshape(n, (n + 63) // 64)
    cols = np.arange(n)
    return ((words[:, cols // 64] >> (cols % 64).astype(np.uint64)) & np.uint64(1)).astype(bool)


def select_greedy(adj: np.ndarray) -> list[int]:
    reps: list[int] = []
    for p in range(len(adj)):
        if not adj[p, reps].any():  # no earlier representative beside it
            reps.append(p)
    return reps


def select_cover(adj: np.ndarray) -> list[int]:
    n = len(adj)
    uncovered = np.ones(n, dtype=bool)
    chosen: list[int] = []
    while uncovered.any():
        gain = (adj & uncovered[None, :]).sum(axis=1)
        gain[chosen] = -1
        top = gain.max()
        best = min((p for p in range(n) if gain[p] == top), key=lambda p: (not uncovered[p], p))
        chosen.append(best)
        uncovered &= ~adj[best]
    return sorted(chosen)


def select(adj: np.ndarray, mode: str) -> np.ndarray:
    is_rep = np.zeros(len(adj), dtype=np.uint8)
    is_rep[select_greedy(adj) if mode == "greedy" else select_cover(adj)] = 1
    return is_rep


def assign(S, score_edges: str, adj: np.ndarray, is_rep) -> tuple[np.ndarray, np.ndarray]:
    S = np.asarray(S)
    n = len(adj)
    rep, rep_score = np.full(n, NONE, dtype=np.uint32), np.full(n, np.nan)
    for p in range(n):
        if is_rep[p]:
            rep[p], rep_score[p] = p, pair_value(S, score_edges, p, p)
            continue
        best = None
        for r in np.flatnonzero(adj[p] & (np.asarray(is_rep) != 0)):
            score = pair_value(S, score_edges, p, int(r))
            if best is None or score > best[0]:  # ascending r: an equal score stays with the smaller r
                best = (score, int(r))
        if best is not None:
            rep_score[p], rep[p] = best
    return rep, rep_score


# ------------------------------------------------------------------ the wanted graphs
def graph(family: str, n: int, seed: int = 0) -> np.ndarray:
    rng = np.random.default_rng([seed, n, FAMILIES.index(family)])
    adj = np.zeros((n, n), dtype=bool)
    idx = np.arange(n)
    if family == "complete":
        adj[:] = True
    elif family in ("path", "path_reverse"):
        # the reverse of the path 0 - 1 - ... is the same labelled graph; this one runs 0, n-1, 1, n-2, ...: every node's
        # neighbours lie at the other end of the index range, in other words and other tiles
        order = idx if family == "path" else np.array([k // 2 if k % 2 == 0 else n - 1 - k // 2 for k in range(n)])
        adj[order[:-1], order[1:]] = True
    elif family == "star_first":
        adj[0, :] = True
    elif family == "star_last":
        adj[:, n - 1] = True
    elif family == "blocks":
        order, at = rng.permutation(n), 0
        while at < n:
            size = int(rng.integers(1, 9))
            members = order[at : at + size]
            adj[np.ix_(members, members)] = True
            at += size
        for _ in range(n // 8):  # noise: pairs that change sides
            p, q = rng.integers(0, n, 2)
            adj[p, q] = not adj[p, q]
            adj[q, p] = adj[p, q]
    elif family == "gnp":
        adj = np.triu(rng.random((n, n)) < min(1.0, 3.0 / max(n, 1)), 1)
    adj = adj | adj.T
    np.fill_diagonal(adj, True)
    return adj


def disjoint_triangles(count: int) -> np.ndarray:
    adj = np.zeros((3 * count, 3 * count), dtype=bool)
    for t in range(count):
        adj[3 * t : 3 * t + 3, 3 * t : 3 * t + 3] = True
    return adj


# ------------------------------------------------------------------ matrices that realise a graph
def _cells(how: str, target: np.ndarray, delta: np.ndarray, side: np.ndarray, nan_b: np.ndarray) -> tuple[np.ndarray, np.ndarray]:
    """(a, b) with agg(how, a, b) == target exactly and a != b where delta != 0; where ``nan_b`` (min and max only) b is
    NaN, which the aggregators pass over."""
    if how == "mean":
        return target - delta, target + delta
    away = target + delta if how == "min" else target - delta
    a = np.where(side, target, away)
    b = np.where(side, away, target)
    return np.where(nan_b, target, a), np.where(nan_b, np.nan, b)


def matrices(adj: np.ndarray, score_edges: str, coverage_edges: str, seed: int = 0) -> tuple[np.ndarray, np.ndarray]:
    """Asymmetric S and C whose graph under (score_edges, coverage_edges, MIN_SCORE, COV_MIN) is ``adj``."""
    n = len(adj)
    rng = np.random.default_rng([seed, n, AGGS.index(score_edges), AGGS.index(coverage_edges)])
    shape = (n, n)
    # an edge: a score from a small palette that starts exactly at the threshold, a coverage just above its own
    score = rng.choice([MIN_SCORE, MIN_SCORE + STEP, 0.96875, 1.0], shape)
    cov = rng.choice([COV_MIN + STEP, 0.75, 1.0], shape)
    # no edge, for one of six reasons
    why = rng.integers(0, 6, shape)
    no = ~adj
    score = np.where(no & (why == 0), MIN_SCORE - STEP, score)
    cov = np.where(no & (why == 1), COV_MIN, cov)  # exactly at the threshold: not above it
    cov = np.where(no & (why == 2), COV_MIN - STEP, cov)
    nan_score, nan_cov = no & ((why == 3) | (why == 5)), no & ((why == 4) | (why == 5))
    delta_s, delta_c = rng.integers(0, 4, shape) * STEP, rng.integers(0, 4, shape) * STEP
    side_s, side_c = rng.random(shape) < 0.5, rng.random(shape) < 0.5
    pass_s = adj & (rng.random(shape) < 0.1) & (score_edges != "mean")
    pass_c = adj & (rng.random(shape) < 0.1) & (coverage_edges != "mean")
    s_a, s_b = _cells(score_edges, score, delta_s, side_s, pass_s)
    c_a, c_b = _cells(coverage_edges, cov, delta_c, side_c, pass_c)
    # a NaN aggregate: the first argument for min and max (a NaN there stays), either for the mean
    s_a, c_a = np.where(nan_score, np.nan, s_a), np.where(nan_cov, np.nan, c_a)
    upper = np.triu(np.ones(shape, dtype=bool), 1)  # decisions are read at (lo, hi)
    S, C = np.zeros(shape), np.zeros(shape)
    for M, a, b in ((S, s_a, s_b), (C, c_a, c_b)):
        M[upper] = b[upper]  # M[lo, hi]
        M.T[upper] = a[upper]  # M[hi, lo]
    diagonal = rng.choice([np.nan, 0.0, 1.0, 0.25, -3.0], (2, n))
    np.fill_diagonal(S, diagonal[0])
    np.fill_diagonal(C, diagonal[1])
    return S, C


class Case:
    """A wanted graph, its matrices for a pair of aggregators, and the restatement's answers (made once, on demand)."""

    def __init__(self, adj: np.ndarray, score_edges: str, coverage_edges: str, seed: int = 0) -> None:
        self.adj, self.score_edges, self.coverage_edges = adj, score_edges, coverage_edges
        self.n = len(adj)
        self.S, self.C = matrices(adj, score_edges, coverage_edges, seed)
        for M in (self.S, self.C):
            M.setflags(write=False)
        self.options = {"score_edges": score_edges, "coverage_edges": coverage_edges, "min_score": MIN_SCORE, "cov_min": COV_MIN}

    @functools.cached_property
    def bits(self) -> np.ndarray:
        return pack(self.adj)

    @functools.lru_cache(maxsize=None)  # noqa: B019  the cases live as long as the session
    def is_rep(self, mode: str) -> np.ndarray:
        return _selection(self.adj.tobytes(), self.n, mode)

    @functools.lru_cache(maxsize=None)  # noqa: B019
    def assignment(self, mode: str) -> tuple[np.ndarray, np.ndarray]:
        return assign(self.S, self.score_edges, self.adj, self.is_rep(mode))


@functools.lru_cache(maxsize=None)
def _selection(adj_bytes: bytes, n: int, mode: str) -> np.ndarray:
    """The selection depends on the graph alone: shared by the cases that realise one graph with different aggregators."""
    out = select(np.frombuffer(adj_bytes, dtype=bool).reshape(n, n), mode)
    out.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def case(family: str, n: int, score_edges: str = "mean", coverage_edges: str = "min") -> Case:
    return Case(graph(family, n), score_edges, coverage_edges)


def aggregator_pairs() -> list[tuple[str, str]]:
    """Every score aggregator and every coverage aggregator, each with each of the others at least once."""
    return [(s, c) for s in AGGS for c in AGGS]


def zero_tie(first_negative: bool) -> tuple[np.ndarray, np.ndarray, float, float]:
    """Three nodes: 0 and 1 are not adjacent, 2 is adjacent to both with the scores 0.0 and -0.0 (which one is negative
    is the argument), at min_score 0.0: equal under ==, so 2 goes to 0 and its score keeps its own sign."""
    z0, z1 = (-0.0, 0.0) if first_negative else (0.0, -0.0)
    S = np.array([[1.0, -1.0, z0], [-1.0, 1.0, z1], [z0, z1, 1.0]])
    C = np.ones((3, 3))
    return S, C, 0.0, COV_MIN
