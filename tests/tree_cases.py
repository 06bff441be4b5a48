"""Neighbour joining as tree-run defines it, restated in plain numpy, and the matrices the tree tests share.

The contract (include/pyani_hip.h), restated here without looking at how the library stores anything:

* ``D`` is n x n float64, finite, >= 0, bitwise symmetric, zero diagonal, 1 <= n <= 65535.
* Leaves are nodes 0 .. n - 1; the node made by join t (t = 0, 1, ...) is n + t.
* ``r[i]`` is ``D[i, 0] + ... + D[i, n - 1]`` added in this order into one accumulator; m = n nodes are live.
* While m > 2: the score of a live pair with ids lo < hi is ``q = ((m - 2) * d(lo, hi) - r[lo]) - r[hi]``, every operation
  rounded (no FMA).  The pair with the smallest q is joined; among pairs of equal q (``==``: -0.0 ties with 0.0) the one
  with the smallest lo, then the smallest hi -- node ids, whatever the storage.  With ``d = d(lo, hi)``:
  ``len_lo = 0.5 * d + (r[lo] - r[hi]) / (2.0 * (m - 2))`` and ``len_hi = d - len_lo`` (negative lengths are kept); the
  record is (lo, hi, len_lo, len_hi).  For every other live k, ``d(u, k) = 0.5 * ((d(lo, k) + d(hi, k)) - d)`` and
  ``r[k] = ((r[k] - d(lo, k)) - d(hi, k)) + d(u, k)``; ``r[u] = 0.5 * ((r[lo] + r[hi]) - m * d)``; m decreases by 1.
* When m = 2 the two remaining nodes a < b and d(a, b) are the last edge.  n = 2: no join, the last edge (0, 1, D[0, 1]);
  n = 1: no join and no edge.

Here the nodes are never moved: the matrix is indexed by node id and has room for every node a run makes, and the live
ids are kept as an ascending array, so "first in row-major order of the live sub-matrix" is "smallest lo, then smallest
hi".  numpy's elementwise operations are single IEEE operations, each a call of its own.
"""

from __future__ import annotations

import functools
import re
from pathlib import Path
from typing import NamedTuple

import numpy as np

from tests.helpers import invalid_distance_matrices

ROOT = Path(__file__).resolve().parent.parent


def kernel_constants() -> dict[str, int]:
    """kThreads and kTile as csrc/nj.hip states them: the lanes of a workgroup and the side of a scan tile."""
    text = (ROOT / "pyani_plus_amd" / "csrc" / "nj.hip").read_text()
    out = {}
    for name in ("kThreads", "kTile"):
        found = re.search(rf"constexpr int {name} = (\d+);", text)
        assert found, f"{name} not found in nj.hip"
        out[name] = int(found.group(1))
    return out


class Joins(NamedTuple):
    child: np.ndarray  # (n - 2, 2) uint32
    length: np.ndarray  # (n - 2, 2) float64
    last: tuple[int, int] | None
    last_len: float


def neighbour_joining(D: np.ndarray, tied: list[int] | None = None) -> Joins:
    """The contract above, one join at a time.  ``tied``, if given, receives per join the number of live pairs whose
    score equals the smallest: more than 1 where the tie rule decided."""
    D = np.asarray(D, dtype=np.float64)
    n = D.shape[0]
    joins = max(n - 2, 0)
    child = np.zeros((joins, 2), dtype=np.uint32)
    length = np.zeros((joins, 2), dtype=np.float64)
    if n == 1:
        return Joins(child, length, None, 0.0)
    size = 2 * n
    M = np.zeros((size, size), dtype=np.float64)
    M[:n, :n] = D
    r = np.zeros(size, dtype=np.float64)
    for k in range(n):
        r[:n] = r[:n] + D[:, k]
    live = np.arange(n)
    for t in range(joins):
        m = len(live)
        sub = M[np.ix_(live, live)]
        q = (np.float64(m - 2) * sub - r[live][:, None]) - r[live][None, :]  # row = lo, column = hi above the diagonal
        q[np.tril_indices(m)] = np.inf
        at = int(np.argmin(q))  # the first of the smallest in row-major order
        assert q.flat[at] < np.inf
        if tied is not None:
            tied.append(int((q == q.flat[at]).sum()))
        lo, hi = int(live[at // m]), int(live[at % m])
        d = M[lo, hi]
        len_lo = np.float64(0.5) * d + (r[lo] - r[hi]) / (np.float64(2.0) * np.float64(m - 2))
        child[t] = (lo, hi)
        length[t] = (len_lo, d - len_lo)
        u = n + t
        others = live[(live != lo) & (live != hi)]
        d_lo, d_hi = M[lo, others], M[hi, others]
        d_u = np.float64(0.5) * ((d_lo + d_hi) - d)
        r[others] = ((r[others] - d_lo) - d_hi) + d_u
        r[u] = np.float64(0.5) * ((r[lo] + r[hi]) - np.float64(m) * d)
        M[u, others] = d_u
        M[others, u] = d_u
        live = np.append(others, u)  # u is the largest id so far: still ascending
    a, b = int(live[0]), int(live[1])
    return Joins(child, length, (a, b), float(M[a, b]))


def tied_pairs_per_join(D: np.ndarray) -> list[int]:
    """Per join of the restatement, the live pairs at the smallest score (join t is made with ``len(D) - t`` nodes live)."""
    tied: list[int] = []
    neighbour_joining(D, tied)
    return tied


# ---------------------------------------------------------------- trees as sets of leaf bipartitions
def _side(leaves: frozenset, n: int) -> frozenset:
    """One name for the two sides of an edge: the side without leaf 0."""
    return frozenset(range(n)) - leaves if 0 in leaves else leaves


def joins_bipartitions(n: int, child, length, last, last_len) -> dict[frozenset, float]:
    """Every edge of a join table as (the leaves on the side away from leaf 0) -> its length."""
    below: dict[int, frozenset] = {i: frozenset([i]) for i in range(n)}
    out: dict[frozenset, float] = {}
    for t in range(len(child)):
        lo, hi = int(child[t][0]), int(child[t][1])
        below[n + t] = below[lo] | below[hi]
        for node, ln in ((lo, length[t][0]), (hi, length[t][1])):
            side = _side(below[node], n)
            assert side not in out, "two edges with the same bipartition"
            out[side] = float(ln)
    if last is not None:
        side = _side(below[int(last[0])], n)
        assert side not in out and below[int(last[0])] | below[int(last[1])] == frozenset(range(n))
        out[side] = float(last_len)
    return out


class AdditiveTree(NamedTuple):
    D: np.ndarray
    edges: dict[frozenset, float]  # bipartition -> length


def random_additive_tree(n: int, seed: int) -> AdditiveTree:
    """A random unrooted binary tree over n >= 2 leaves, every branch a multiple of 2^-10 in (0, 1], and its leaf
    distances: sums of at most 2n dyadic lengths, exact in double."""
    rng = np.random.default_rng(seed)
    edges: list[tuple[int, int]] = [(0, 1)] if n == 2 else [(0, n), (1, n), (2, n)]
    nxt = n + 1
    for leaf in range(3, n):  # split a random edge with a new inner node and hang the leaf on it
        x, y = edges.pop(int(rng.integers(len(edges))))
        edges += [(x, nxt), (y, nxt), (leaf, nxt)]
        nxt += 1
    weights = rng.integers(1, 1025, size=len(edges)) / 1024.0
    nodes = nxt if n > 2 else 2
    adj: list[list[tuple[int, float]]] = [[] for _ in range(nodes)]
    for (x, y), w in zip(edges, weights):
        adj[x].append((y, float(w)))
        adj[y].append((x, float(w)))
    D = np.zeros((n, n), dtype=np.float64)
    for src in range(n):
        dist = np.full(nodes, -1.0)
        dist[src] = 0.0
        stack = [src]
        while stack:
            v = stack.pop()
            for w_, ln in adj[v]:
                if dist[w_] < 0:
                    dist[w_] = dist[v] + ln
                    stack.append(w_)
        D[src] = dist[:n]
    # the leaves behind each edge, seen from leaf 0: one walk in pre-order, sets joined on the way back
    parent = {0: -1}
    order = [0]
    for v in order:
        for w_, _ in adj[v]:
            if w_ not in parent:
                parent[w_] = v
                order.append(w_)
    below = {v: (frozenset([v]) if v < n else frozenset()) for v in order}
    for v in reversed(order[1:]):
        below[parent[v]] = below[parent[v]] | below[v]
    out = {}
    for (x, y), w in zip(edges, weights):
        lower = x if parent.get(x) == y else y
        out[_side(below[lower], n)] = float(w)
    assert np.array_equal(D, D.T)
    return AdditiveTree(D, out)


def random_symmetric(n: int, seed: int) -> np.ndarray:
    """Symmetric, zero diagonal, off-diagonal multiples of 2^-20 in (0, 1]: not additive, so some branches come out negative."""
    rng = np.random.default_rng(seed)
    upper = np.triu(rng.integers(1, (1 << 20) + 1, size=(n, n)) / float(1 << 20), 1)
    return upper + upper.T


def all_equal(n: int = 33) -> np.ndarray:
    """Every off-diagonal distance 0.5: every join is decided by the tie rule alone."""
    D = np.full((n, n), 0.5)
    np.fill_diagonal(D, 0.0)
    return D


def duplicated(n: int = 9, seed: int = 5) -> np.ndarray:
    """n genomes of which the last three are copies of the first three: d = 0 pairs."""
    base = random_symmetric(n - 3, seed)
    src = list(range(n - 3)) + [0, 1, 2]
    D = base[np.ix_(src, src)].copy()
    np.fill_diagonal(D, 0.0)
    return D


class Case(NamedTuple):
    name: str
    D: np.ndarray
    edges: dict[frozenset, float] | None  # the generating tree of an additive case


def tiling_sizes() -> list[int]:
    """One below, at and one above each edge of the scan's tiling: the side of a tile (where one scan workgroup
    becomes several) and the lanes of a workgroup (two tiles a side becoming three)."""
    k = kernel_constants()
    edges = sorted({k["kTile"], k["kThreads"], 2 * k["kTile"]})
    return sorted({e + step for e in edges for step in (-1, 0, 1)})


LARGEST = 513
RESTATED_UP_TO = 257


@functools.lru_cache(maxsize=None)
def cases() -> tuple[Case, ...]:
    out = [Case("one", np.zeros((1, 1)), None), Case("two", np.array([[0.0, 0.375], [0.375, 0.0]]), None)]
    for n in (2, 3, 4, 5, 17, 64, 65, 130, LARGEST):
        tree = random_additive_tree(n, 100 + n)
        out.append(Case(f"additive{n}", tree.D, tree.edges))
    for n in sorted({3, 4, 5, *tiling_sizes(), LARGEST}):
        out.append(Case(f"random{n}", random_symmetric(n, 200 + n), None))
    k = kernel_constants()
    tree = random_additive_tree(k["kTile"] + 1, 7)
    out.append(Case(f"additive{k['kTile'] + 1}", tree.D, tree.edges))
    out.append(Case("all_equal33", all_equal(33), None))
    out.append(Case("duplicated9", duplicated(9), None))
    for c in out:
        c.D.setflags(write=False)
    return tuple(out)


def case(name: str) -> Case:
    return next(c for c in cases() if c.name == name)


@functools.lru_cache(maxsize=None)
def restated(name: str) -> Joins:
    """The restatement's table of a case, computed once."""
    return neighbour_joining(case(name).D)


# ---------------------------------------------------------------- ties on more than one tile, and candidates past a workgroup
# Kept out of cases(): these are larger than LARGEST and have references of their own.
def copies(genomes: int, times: int, seed: int) -> np.ndarray:
    """``times`` copies of each of ``genomes`` genomes, copy c of genome g at g + c * genomes: d = 0 between the copies and
    every other distance ``times`` squared times in the matrix."""
    src = np.arange(genomes * times) % genomes
    D = random_symmetric(genomes, seed)[np.ix_(src, src)].copy()
    np.fill_diagonal(D, 0.0)
    return D


# The seeds are chosen for the condition test_tree_host.py states on these inputs (a third of the joins made on more than
# one tile are tied).  With three copies the three pairs of a genome's copies share one score and any seed does; with two
# copies only two joins are made above kTile nodes, the copies of a genome are one pair, and a tie needs a pair of
# different genomes in front: of the seeds 0 .. 11 only 9 has one.
COPIES_SEEDS = {"copies258x86": 4, "copies130x65": 9}


@functools.lru_cache(maxsize=None)
def tie_cases() -> tuple[Case, ...]:
    """Matrices whose joins are decided by the tie rule while more than one scan tile is live: equal scores in different
    tiles, in slots that swap-remove has shuffled."""
    out = (
        Case("all_equal257", all_equal(257), None),
        Case("copies258x86", copies(86, 3, COPIES_SEEDS["copies258x86"]), None),  # three-way ties between the copies of a genome
        Case("copies130x65", copies(65, 2, COPIES_SEEDS["copies130x65"]), None),  # the tile's edge: two tiles, the second two slots wide
    )
    for c in out:
        c.D.setflags(write=False)
    return out


def tie_case(name: str) -> Case:
    return next(c for c in tie_cases() if c.name == name)


@functools.lru_cache(maxsize=None)
def tie_restated(name: str) -> tuple[Joins, tuple[int, ...]]:
    """The restatement's table of a tie case and its tied pairs per join, computed once."""
    tied: list[int] = []
    joins = neighbour_joining(tie_case(name).D, tied)
    return joins, tuple(tied)


def tied_share(tied, n: int) -> tuple[int, int]:
    """``(joins with more than one pair at the smallest score, joins)`` among those made while more than kTile nodes are
    live: join t has n - t."""
    wide = [count for t, count in enumerate(tied) if n - t > kernel_constants()["kTile"]]
    return sum(count > 1 for count in wide), len(wide)


class FarTile(NamedTuple):
    D: np.ndarray
    nt: int  # tiles a side in the first joins: the smallest with nt * nt > kThreads
    first: tuple[tuple[int, int], tuple[int, int]]  # the pairs of joins 0 and 1
    candidate: int  # the index of their tile among the nt * nt candidates the join kernel reduces


@functools.lru_cache(maxsize=None)
def far_tile_case(seed: int = 17) -> FarTile:
    """The smallest matrix at which the join kernel's loop over the candidates takes a second trip, for exactly two
    joins, and whose first two joins are found in a tile that only the second trip reads: four leaves at distance 1.0
    from everything (the largest row sums by far), paired at 2^-20 and 2^-19, all in the diagonal tile nt - 2."""
    k = kernel_constants()
    nt = next(x for x in range(1, 1 << 16) if x * x > k["kThreads"])
    n = (nt - 1) * k["kTile"] + 2
    D = random_symmetric(n, seed)
    top = (nt - 1) * k["kTile"]  # the first slot of the last tile
    first = ((top - 8, top - 3), (top - 18, top - 13))
    for leaf in (*first[0], *first[1]):
        D[leaf, :] = 1.0
        D[:, leaf] = 1.0
    for (a, b), d in zip(first, (2.0**-20, 2.0**-19)):
        D[a, b] = D[b, a] = d
    np.fill_diagonal(D, 0.0)
    D.setflags(write=False)
    return FarTile(D, nt, first, (nt - 2) * nt + (nt - 2))


@functools.lru_cache(maxsize=None)
def far_tile_twin():
    """``pa_nj_host`` of the far-tile case, computed once: the restatement would take a minute at this size."""
    from pyani_plus_amd.engine import nj_tree_host

    return nj_tree_host(far_tile_case().D)


def invalid_matrices() -> list[tuple[str, np.ndarray, tuple[int, int]]]:
    """(what, matrix, the first offending cell in row-major order)."""
    return invalid_distance_matrices(6, 1)
