"""bootstrap-run as DESIGN.md section 7l defines it, restated in numpy with Python integers, and the alignments and
weights the bootstrap tests share.  Written from the contract alone, without looking at how the library computes anything:

* ``fin`` is the splitmix64 finaliser.  ``seeded = fin(seed)``; replicate r has ``base = fin(seeded + r)``; its draw
  t = 0 .. L - 1 hits column ``(fin(base + t) * L) >> 64``; ``w_r[c]`` is the number of hits on column c.
* Per replicate and ordered pair of rows: ``M = sum_c w[c] [q_c == s_c and q_c != '-']`` and
  ``B = sum_c w[c] [q_c != '-' and s_c != '-']``, the diagonal included, so ``B[i, i]`` is row i's weighted residue count.
* ``aln = n_i + n_j - B[i, j]``; ``D[i, j] = 1.0 - M / aln`` (one correctly rounded division, one subtraction), ``missing``
  when ``aln == 0``, 0.0 on the diagonal.
* Each replicate's D goes through neighbour joining (``tests/tree_cases.py``).
* The clade of an edge is the set of leaves on its side away from leaf 0, trivial with fewer than 2 or more than n - 2
  leaves.  Node n + t of the reference tree stands for the edge above it; its support is the number of replicate trees
  that have an edge with the same clade; a trivial clade is in every tree.
"""

from __future__ import annotations

import functools
import re
from typing import NamedTuple

import numpy as np

from tests import tree_cases

GAP = ord("-")
MASK = (1 << 64) - 1


def fin(v: int) -> int:
    z = (v + 0x9E3779B97F4A7C15) & MASK
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & MASK
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & MASK
    return z ^ (z >> 31)


def weights(seed: int, n_cols: int, first: int, count: int) -> np.ndarray:
    """Rows first .. first + count - 1 of the weights of ``seed``, as Python integers in an int64 array."""
    seeded = fin(seed)
    out = np.zeros((count, n_cols), dtype=np.int64)
    for r in range(count):
        base = fin((seeded + first + r) & MASK)
        for t in range(n_cols):
            out[r, (fin((base + t) & MASK) * n_cols) >> 64] += 1
    return out


def counts(rows: np.ndarray, w: np.ndarray) -> tuple[np.ndarray, np.ndarray]:
    """``(M, B)`` of every ordered pair of ``rows`` (n x L bytes) under the weights ``w`` (L integers), int64."""
    rows = np.asarray(rows, dtype=np.uint8)
    w = np.asarray(w, dtype=np.int64)
    residue = rows != GAP
    n = rows.shape[0]
    M, B = np.zeros((n, n), dtype=np.int64), np.zeros((n, n), dtype=np.int64)
    for i in range(n):
        M[i] = ((rows == rows[i]) & residue[i]).astype(np.int64) @ w
        B[i] = (residue & residue[i]).astype(np.int64) @ w
    return M, B


def distances(M: np.ndarray, B: np.ndarray, missing: float = 1.0) -> np.ndarray:
    n = M.shape[0]
    D = np.zeros((n, n), dtype=np.float64)
    for i in range(n):
        for j in range(n):
            if i == j:
                continue
            aln = int(B[i, i]) + int(B[j, j]) - int(B[i, j])
            D[i, j] = float(missing) if aln == 0 else 1.0 - int(M[i, j]) / aln  # int / int is correctly rounded
    return D


# ---------------------------------------------------------------- clades and support
def _below(n: int, child) -> dict[int, frozenset]:
    below = {i: frozenset([i]) for i in range(n)}
    for t in range(len(child)):
        below[n + t] = below[int(child[t][0])] | below[int(child[t][1])]
    return below


def _side(leaves: frozenset, n: int) -> frozenset:
    return frozenset(range(n)) - leaves if 0 in leaves else leaves


def is_trivial(clade: frozenset, n: int) -> bool:
    return not 2 <= len(clade) <= n - 2


def clades(n: int, joins: tree_cases.Joins) -> set[frozenset]:
    """The non-trivial clades of a tree, from its edges as tests/tree_cases.py lists them."""
    edges = tree_cases.joins_bipartitions(n, joins.child, joins.length, joins.last, joins.last_len)
    return {c for c in edges if not is_trivial(c, n)}


def node_clades(n: int, child) -> list[frozenset]:
    """Per join t: the clade of the edge above node n + t.  Whatever that edge leads to, the leaves below the node are one
    of its sides."""
    below = _below(n, child)
    return [_side(below[n + t], n) for t in range(len(child))]


def support(n: int, ref_child, replicate_clades: list[set[frozenset]]) -> list[int]:
    out = []
    for clade in node_clades(n, ref_child):
        out.append(len(replicate_clades) if is_trivial(clade, n) else sum(clade in tree for tree in replicate_clades))
    return out


# ---------------------------------------------------------------- alignments
def alignment(n: int, n_cols: int, seed: int, *, alphabet: bytes = b"ACGT", gaps: float = 0.03, mutate: float = 0.08) -> np.ndarray:
    """n rows of n_cols bytes: a random root, each further row a mutated copy of an earlier one (so that the rows have a
    tree to find), then ``gaps`` of the cells turned to '-'."""
    rng = np.random.default_rng(seed)
    letters = np.frombuffer(alphabet, dtype=np.uint8)
    rows = np.empty((n, n_cols), dtype=np.uint8)
    rows[0] = letters[rng.integers(len(letters), size=n_cols)]
    for i in range(1, n):
        rows[i] = rows[int(rng.integers(i))]
        hit = rng.random(n_cols) < mutate
        rows[i, hit] = letters[rng.integers(len(letters), size=int(hit.sum()))]
    rows[rng.random((n, n_cols)) < gaps] = GAP
    return rows


TIED_ROWS, TIED_COLUMNS, TIED_SEED, TIED_COPIES = 60, 64, 31, 3


def tied_alignment(make=alignment) -> np.ndarray:
    """60 rows of 64 columns stacked three times: 180 rows, more than one scan tile of the joins, whose distances -- ratios
    of small integers, 0 between the copies of a row -- tie in every replicate."""
    return np.tile(make(TIED_ROWS, TIED_COLUMNS, TIED_SEED), (TIED_COPIES, 1))


# the three alignments of the support tests: (rows, columns, seed)
SUPPORT_ALIGNMENTS = ((7, 97, 11), (12, 300, 12), (9, 64, 13))
SUPPORT_REPLICATES = 50


class Restated(NamedTuple):
    rows: np.ndarray
    weights: np.ndarray  # (R, L) int64
    reference: tree_cases.Joins  # the tree of the unit weights
    trees: list  # Joins per replicate
    support: list[int]  # per join of the reference


@functools.lru_cache(maxsize=None)
def restated(n: int, n_cols: int, seed: int, replicates: int = SUPPORT_REPLICATES, boot_seed: int = 0) -> Restated:
    """The whole of the contract on one alignment, computed once."""
    rows = alignment(n, n_cols, seed)
    w = weights(boot_seed, n_cols, 0, replicates)
    reference = tree_cases.neighbour_joining(distances(*counts(rows, np.ones(n_cols, dtype=np.int64))))
    trees = [tree_cases.neighbour_joining(distances(*counts(rows, w[r]))) for r in range(replicates)]
    return Restated(rows, w, reference, trees, support(n, reference.child, [clades(n, t) for t in trees]))


# ---------------------------------------------------------------- the count cases (host twin and device alike)
class CountCase(NamedTuple):
    name: str
    rows: np.ndarray  # n x L bytes
    weights: np.ndarray  # R x L uint8, every row adding up to L


def _alphabet(symbols: int) -> bytes:
    """``symbols`` residue bytes, none of them the gap."""
    return bytes([b for b in range(1, 256) if b != GAP][:symbols])


def _drawn(n_cols: int, count: int, seed: int = 0) -> np.ndarray:
    return weights(seed, n_cols, 0, count).astype(np.uint8)


def _all_on(n_cols: int, column: int) -> np.ndarray:
    w = np.zeros((1, n_cols), dtype=np.uint8)
    w[0, column] = n_cols
    return w


SPLIT_COLUMNS = 4161  # 131 words: with 3 rows and one replicate the device splits them over 3 workgroups, added with atomics
BATCH = 32  # PA_MSA_BOOT_BATCH


@functools.lru_cache(maxsize=None)
def count_cases() -> tuple[CountCase, ...]:
    out = []
    for n in (1, 4, 63, 64, 65, 130):  # the tile's edge, and more than one tile: the mirror runs
        out.append(CountCase(f"rows{n}", alignment(n, 70, 300 + n), _drawn(70, 2, n)))
    for n_cols in (1, 31, 32, 33, 8 * 32, 8 * 32 + 1):  # the seam of a stage through LDS
        out.append(CountCase(f"cols{n_cols}", alignment(5, n_cols, 400 + n_cols), _drawn(n_cols, 3, n_cols)))
    out.append(CountCase("split", alignment(3, SPLIT_COLUMNS, 5), _drawn(SPLIT_COLUMNS, 1, 5)))
    for symbols, bits in ((1, 1), (3, 2), (15, 4), (31, 5), (63, 6), (127, 7), (255 - 1, 8)):  # ACGT, everywhere else, is bits 3
        assert symbols.bit_length() == bits
        out.append(CountCase(f"bits{bits}", alignment(6, 100, 500 + bits, alphabet=_alphabet(symbols), mutate=0.3), _drawn(100, 2, bits)))
    rows = alignment(6, 75, 600)
    rows[1] = GAP
    rows[4] = GAP  # two rows without residues: their pair has no aligned column, whatever the weights
    rows[:, 40] = GAP
    out.append(CountCase("all_gap", rows, _drawn(75, 2, 600)))
    out.append(CountCase("weights_max1", alignment(5, 90, 700), np.ones((1, 90), dtype=np.uint8)))
    heavy = np.zeros((2, 300), dtype=np.uint8)
    heavy[0, 7], heavy[0, 150:195] = 255, 1  # 255 + 45
    heavy[1, 299], heavy[1, 0:45] = 255, 1
    out.append(CountCase("weights_max255", alignment(5, 300, 701), heavy))
    out.append(CountCase("weights_last_column", alignment(5, 75, 702), _all_on(75, 74)))  # column 74: bit 10 of the third word
    out.append(CountCase("batch1", alignment(4, 50, 703), _drawn(50, 1, 703)))
    out.append(CountCase("batch_plus_one", alignment(4, 50, 704), _drawn(50, BATCH + 1, 704)))
    for c in out:
        assert (c.weights.sum(axis=1) == c.rows.shape[1]).all(), c.name
        c.rows.setflags(write=False)
        c.weights.setflags(write=False)
    return tuple(out)


def count_case(name: str) -> CountCase:
    return next(c for c in count_cases() if c.name == name)


# ---------------------------------------------------------------- hand-built counts past a launch's first trip
def stride_cells() -> int:
    """The cells a grid-stride launch covers before its lanes loop: kStrideThreads * kStrideMaxBlocks as
    csrc/pa_launch_geom.h states them."""
    text = (tree_cases.ROOT / "pyani_plus_amd" / "csrc" / "pa_launch_geom.h").read_text()
    found = re.search(r"constexpr uint32_t kStrideThreads = (\d+), kStrideMaxBlocks = (\d+);", text)
    assert found, "kStrideThreads and kStrideMaxBlocks not found in pa_launch_geom.h"
    return int(found.group(1)) * int(found.group(2))


def symmetric_integers(rng, n: int, low: int, high: int) -> np.ndarray:
    """n x n int64 in [low, high], symmetric."""
    upper = np.triu(rng.integers(low, high + 1, size=(n, n)))
    return upper + np.triu(upper, 1).T


class StridedCounts(NamedTuple):
    match: np.ndarray  # R x n x n uint32
    both: np.ndarray
    all_gap: dict[int, tuple[int, int]]  # matrix -> its two rows without a residue


STRIDED_ROWS, STRIDED_REPLICATES = 230, 5


@functools.lru_cache(maxsize=None)
def strided_counts(seed: int = 41) -> StridedCounts:
    """Five 230 x 230 matrices of counts, 264 500 cells in one launch of the distances: the last rows of the last matrix
    are written on the lanes' second trip.  Consistent with the rule: n_i on the diagonal of ``both`` and of ``match``,
    ``both`` <= min(n_i, n_j), ``match`` <= ``both``.  Matrix 1 (first trip) and the last matrix (second trip) have two
    rows without a residue each: their pair has no aligned column."""
    rng = np.random.default_rng(seed)
    n, reps = STRIDED_ROWS, STRIDED_REPLICATES
    all_gap = {1: (3, 7), reps - 1: (n - 7, n - 2)}
    match, both = np.zeros((reps, n, n), dtype=np.int64), np.zeros((reps, n, n), dtype=np.int64)
    for r in range(reps):
        residues = rng.integers(300, 401, size=n)
        for row in all_gap.get(r, ()):
            residues[row] = 0
        both[r] = np.maximum(np.minimum(residues[:, None], residues[None, :]) - symmetric_integers(rng, n, 0, 50), 0)
        match[r] = np.maximum(both[r] - symmetric_integers(rng, n, 0, 40), 0)
        both[r][np.diag_indices(n)] = residues
        match[r][np.diag_indices(n)] = residues
    out = StridedCounts(match.astype(np.uint32), both.astype(np.uint32), all_gap)
    out.match.setflags(write=False)
    out.both.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def restated_counts(name: str) -> tuple[np.ndarray, np.ndarray]:
    """``(M, B)`` of a count case, R x n x n uint32, computed once."""
    c = count_case(name)
    both = [counts(c.rows, c.weights[r]) for r in range(len(c.weights))]
    return np.stack([m for m, _b in both]).astype(np.uint32), np.stack([b for _m, b in both]).astype(np.uint32)
