"""phylo-run as DESIGN.md section 7m defines it, restated with byte loops, Python integers and ``math.log``, and the
alignments, weights and counts the substitution tests share.  Written from the contract alone, without looking at how the
library computes anything; of the package only constants are imported.

* Code: ``A a -> 4``, ``G g -> 5``, ``C c -> 6``, ``T t U u -> 7``, every other byte 0.  Bit 2: a nucleotide; bit 1: the
  class (0 purine, 1 pyrimidine); bit 0: the base within the class.
* Counts of rows i, j under column weights w (all 1 without weights): V = sum of w[c] where both rows hold a nucleotide;
  S = the sum over those columns where the classes are equal and the bases differ; T = the sum where the classes differ.
* Distance: 0.0 for i == j; ``missing`` for V == 0; +0.0 for S + T == 0; p = (S + T) / V;
  jc69: a = 1 - (4 (S + T)) / (3 V), d = -0.75 log a; k80: P = S / V, Q = T / V, a = (1 - 2 P) - Q, b = 1 - 2 Q,
  d = -0.5 log a - 0.25 log b; ``missing`` when a <= 0 or b <= 0 (saturated).  Every operation a double operation of its
  own, in this order; ``math.log`` stands for the rule's logarithm, so a distance with a logarithm is compared within a
  tolerance and everything else bit for bit.
* Per matrix, the unordered pairs that are ``missing`` for V == 0 and those that are for saturation.
"""

from __future__ import annotations

import functools
import math
import re
from typing import NamedTuple

import numpy as np

from pyani_plus_amd._capi import PA_MSA_BOOT_BATCH, PA_SUBST_MODEL_JC69, PA_SUBST_MODEL_K80, PA_SUBST_MODEL_P
from tests import bootstrap_cases, tree_cases
from tests.msa_cases import split_columns

MODELS = {"p": PA_SUBST_MODEL_P, "jc69": PA_SUBST_MODEL_JC69, "k80": PA_SUBST_MODEL_K80}
BATCH = PA_MSA_BOOT_BATCH
# |d - restated d| <= LOG_TOLERANCE * restated d where a logarithm is taken: 4 ulp of the rule's logarithm, 1 of libm's,
# and the roundings of two products and a sum of terms of one sign
LOG_TOLERANCE = 8 * 2.0**-52


def code_table() -> np.ndarray:
    table = np.zeros(256, dtype=np.uint8)
    for letters, code in ((b"Aa", 4), (b"Gg", 5), (b"Cc", 6), (b"TtUu", 7)):
        for byte in letters:
            table[byte] = code
    return table


def counts(rows: np.ndarray, w=None) -> tuple[np.ndarray, np.ndarray, np.ndarray]:
    """``(V, S, T)`` of every ordered pair of ``rows`` (n x L bytes) under the weights ``w`` (L integers; None: ones), int64:
    a loop over the pairs and the columns."""
    table = code_table()
    n, n_cols = rows.shape
    weights = [1] * n_cols if w is None else [int(x) for x in w]
    coded = [[int(table[b]) for b in row] for row in rows]
    V, S, T = (np.zeros((n, n), dtype=np.int64) for _ in range(3))
    for i in range(n):
        for j in range(i, n):
            v = s = t = 0
            for c in range(n_cols):
                a, b = coded[i][c], coded[j][c]
                if a >= 4 and b >= 4:
                    v += weights[c]
                    if (a ^ b) & 2:
                        t += weights[c]
                    elif a != b:
                        s += weights[c]
            V[i, j] = V[j, i] = v
            S[i, j] = S[j, i] = s
            T[i, j] = T[j, i] = t
    return V, S, T


def counts_fast(rows: np.ndarray, w=None) -> tuple[np.ndarray, np.ndarray, np.ndarray]:
    """``counts`` for the larger cases, a row at a time in numpy; ``test_subst_host`` holds the two against each other."""
    coded = code_table()[np.asarray(rows, dtype=np.uint8)].astype(np.int64)
    n, n_cols = coded.shape
    weights = np.ones(n_cols, dtype=np.int64) if w is None else np.asarray(w, dtype=np.int64)
    V, S, T = (np.zeros((n, n), dtype=np.int64) for _ in range(3))
    for i in range(n):
        both = (coded >= 4) & (coded[i] >= 4)
        x = coded ^ coded[i]
        V[i] = both.astype(np.int64) @ weights
        T[i] = (both & ((x & 2) != 0)).astype(np.int64) @ weights
        S[i] = (both & ((x & 2) == 0) & (x != 0)).astype(np.int64) @ weights
    return V, S, T


DEFINED, NO_COLUMNS, SATURATED = 0, 1, 2


def distance(i: int, j: int, v: int, s: int, t: int, model: str, missing: float) -> tuple[float, int, bool]:
    """``(d, why, exact)``: the distance, why it is ``missing`` if it is, and whether no logarithm went into it."""
    if i == j:
        return 0.0, DEFINED, True
    if v == 0:
        return float(missing), NO_COLUMNS, True
    if s + t == 0:
        return 0.0, DEFINED, True
    if model == "p":
        return float(s + t) / float(v), DEFINED, True
    if model == "jc69":
        a = 1.0 - (4.0 * float(s + t)) / (3.0 * float(v))
        if a <= 0:
            return float(missing), SATURATED, True
        return -0.75 * math.log(a), DEFINED, False
    assert model == "k80"
    P, Q = float(s) / float(v), float(t) / float(v)
    a = (1.0 - 2.0 * P) - Q
    b = 1.0 - 2.0 * Q
    if a <= 0 or b <= 0:
        return float(missing), SATURATED, True
    return -0.5 * math.log(a) - 0.25 * math.log(b), DEFINED, False


class Distances(NamedTuple):
    D: np.ndarray  # n x n float64
    exact: np.ndarray  # n x n bool: no logarithm went into the cell
    undefined: tuple[int, int]  # unordered pairs without a column, saturated pairs


def distances(V, S, T, model: str, missing: float) -> Distances:
    n = V.shape[0]
    D, exact = np.zeros((n, n)), np.ones((n, n), dtype=bool)
    none = saturated = 0
    for i in range(n):
        for j in range(n):
            D[i, j], why, exact[i, j] = distance(i, j, int(V[i, j]), int(S[i, j]), int(T[i, j]), model, missing)
            if i < j:
                none += why == NO_COLUMNS
                saturated += why == SATURATED
    return Distances(D, exact, (none, saturated))


def assert_distances(got: np.ndarray, got_undefined, want: Distances, what: str = "") -> None:
    """The bits of the restatement where no logarithm is taken, within ``LOG_TOLERANCE`` of it elsewhere; no -0.0."""
    assert got.shape == want.D.shape, what
    np.testing.assert_array_equal(got[want.exact].view(np.uint64), want.D[want.exact].view(np.uint64), err_msg=what)
    loose = ~want.exact
    assert (np.abs(got[loose] - want.D[loose]) <= LOG_TOLERANCE * want.D[loose]).all(), what
    assert not np.signbit(got).any(), what
    assert tuple(int(x) for x in got_undefined) == want.undefined, what


# ---------------------------------------------------------------- alignments
NUCLEOTIDE_MIX = b"ACGTacgtUuNnRYKMSWBDHV-"  # both cases, U, N, IUPAC letters and the gap


def alignment(n: int, n_cols: int, seed: int, *, alphabet: bytes = b"ACGT", gaps: float = 0.05, mutate: float = 0.15) -> np.ndarray:
    """``bootstrap_cases.alignment`` with another default alphabet's worth of mutation: rows that have a tree to find."""
    return bootstrap_cases.alignment(n, n_cols, seed, alphabet=alphabet, gaps=gaps, mutate=mutate)


def tied_alignment() -> np.ndarray:
    """``bootstrap_cases.tied_alignment`` with this module's rows: 180 rows, every row three times."""
    return bootstrap_cases.tied_alignment(alignment)


class CountCase(NamedTuple):
    name: str
    rows: np.ndarray  # n x L bytes
    weights: np.ndarray | None  # R x L uint8, every row adding up to L; None: the unweighted call


def _drawn(n_cols: int, count: int, seed: int) -> np.ndarray:
    return bootstrap_cases.weights(seed, n_cols, 0, count).astype(np.uint8)


SPLIT_COLUMNS = 4101  # 129 words: with 5 rows (one tile) the device splits them over 3 workgroups, added with atomics
SPLIT_ROWS = 5


def split_of(name: str, compute_units: int):
    """``msa_tile::split_columns`` (as ``tests/msa_cases.py`` restates it) of the launch a case makes first."""
    case = count_case(name)
    n, n_cols = case.rows.shape
    tiles = (n + 63) // 64
    reps = 1 if case.weights is None else min(BATCH, len(case.weights))
    return split_columns(tiles * (tiles + 1) // 2 * reps, (n_cols + 31) // 32, compute_units)


@functools.lru_cache(maxsize=None)
def count_cases() -> tuple[CountCase, ...]:
    out = []
    for n in (1, 2, 63, 64, 65, 130):  # the tile's edge, the padded rows of the last tile, more than one tile: the mirror runs
        rows = alignment(n, 70, 900 + n, alphabet=NUCLEOTIDE_MIX if n <= 2 else b"ACGT")
        out.append(CountCase(f"rows{n}", rows, None))
        out.append(CountCase(f"rows{n}_weighted", rows, _drawn(70, 2, n)))
    for n_cols in (0, 1, 31, 32, 33, 255, 256, 257):  # the word and the 8-word stage
        rows = alignment(5, n_cols, 1000 + n_cols, alphabet=NUCLEOTIDE_MIX, mutate=0.3)
        out.append(CountCase(f"cols{n_cols}", rows, None))
        out.append(CountCase(f"cols{n_cols}_weighted", rows, _drawn(n_cols, 3, n_cols)))
    split = alignment(SPLIT_ROWS, SPLIT_COLUMNS, 7)
    out.append(CountCase("split", split, None))
    out.append(CountCase("split_weighted", split, _drawn(SPLIT_COLUMNS, 1, 7)))
    rows = alignment(5, 300, 1100, alphabet=NUCLEOTIDE_MIX, mutate=0.3)
    out.append(CountCase("weights_nb1", rows, np.ones((1, 300), dtype=np.uint8)))  # must equal the unweighted call
    heavy = np.zeros((2, 300), dtype=np.uint8)
    heavy[0, 7], heavy[0, 150:195] = 255, 1  # 255 + 45: eight weight planes
    heavy[1, 299], heavy[1, 0:45] = 255, 1
    out.append(CountCase("weights_nb8", rows, heavy))
    one = np.zeros((1, 300), dtype=np.uint8)
    one[0, 170] = 255  # a uint8 cannot hold all 300: the mass on two columns, one of them the last
    one[0, 299] = 45
    out.append(CountCase("weights_two_columns", rows, one))
    single = alignment(5, 75, 1101)
    on_one = np.zeros((1, 75), dtype=np.uint8)
    on_one[0, 74] = 75  # all mass on one column: bit 10 of the third word
    out.append(CountCase("weights_one_column", single, on_one))
    few = alignment(4, 50, 1102)
    out.append(CountCase("batch1", few, _drawn(50, 1, 1102)))
    out.append(CountCase("batch3", few, _drawn(50, 3, 1103)))
    out.append(CountCase("batch_plus_one", few, _drawn(50, BATCH + 1, 1104)))
    for c in out:
        if c.weights is not None:
            assert (c.weights.sum(axis=1, dtype=np.int64) == c.rows.shape[1]).all(), c.name
            c.weights.setflags(write=False)
        c.rows.setflags(write=False)
    return tuple(out)


def count_case(name: str) -> CountCase:
    return next(c for c in count_cases() if c.name == name)


@functools.lru_cache(maxsize=None)
def restated_counts(name: str) -> tuple[np.ndarray, np.ndarray, np.ndarray]:
    """``(V, S, T)`` of a count case, R x n x n uint32 (R = 1 without weights), computed once."""
    c = count_case(name)
    each = [counts_fast(c.rows)] if c.weights is None else [counts_fast(c.rows, c.weights[r]) for r in range(len(c.weights))]
    out = tuple(np.stack([x[k] for x in each]).astype(np.uint32) for k in range(3))
    for x in out:
        x.setflags(write=False)
    return out


# ---------------------------------------------------------------- hand-built counts that hit each edge of the rule
def edge_counts() -> tuple[np.ndarray, np.ndarray, np.ndarray]:
    """One 10 x 10 matrix of counts, pair (0, k) the k-th edge; the other cells plain.  uint32 ``[1, 10, 10]`` each."""
    n = 10
    V, S, T = np.full((n, n), 1000, dtype=np.uint32), np.full((n, n), 30, dtype=np.uint32), np.full((n, n), 20, dtype=np.uint32)
    edges = {
        1: (0, 0, 0),  # V == 0: no shared nucleotide column
        2: (1000, 0, 0),  # S + T == 0: +0.0
        3: (1000, 500, 250),  # jc69: a = 1 - 3000 / 3000 = 0 exactly; k80: a = (1 - 1) - 0.25 < 0
        4: (3001, 1250, 1000),  # jc69: a = 1 - 9000 / 9003, just above 0; k80: b = 1 - 2000 / 3001 > 0, a < 0
        5: (1000, 0, 500),  # k80: b = 1 - 1 = 0 exactly, a = 1 - 0.5 > 0; jc69: a = 1/3
        6: (1000, 0, 600),  # k80: b < 0 with a = 0.4 > 0
        7: (8, 3, 2),  # k80: a = (1 - 0.75) - 0.25 = 0 exactly, b = 0.5
        8: (8001, 3000, 2000),  # k80: a = 1/8001 or so, just above 0
    }
    for k, (v, s, t) in edges.items():
        V[0, k] = V[k, 0] = v
        S[0, k] = S[k, 0] = s
        T[0, k] = T[k, 0] = t
    for i in range(n):
        S[i, i] = T[i, i] = 0
    return V[None], S[None], T[None]


# ---------------------------------------------------------------- hand-built counts past a launch's first trip, and tiny matrices
def distance_batch() -> int:
    """The matrices a launch of the distances takes: two 64-bit words each of kSubstUndefined's, as csrc/pa_internal.h
    states that slot."""
    text = (tree_cases.ROOT / "pyani_plus_amd" / "csrc" / "pa_internal.h").read_text()
    found = re.search(r"constexpr ScalarSlot kSubstUndefined\{(\d+), (\d+)\};", text)
    assert found, "kSubstUndefined not found in pa_internal.h"
    return int(found.group(2)) // 4


NO_COLUMN_COUNTS = (0, 0, 0)  # (V, S, T) of a pair without a shared nucleotide column
SATURATED_COUNTS = (1000, 0, 800)  # jc69: a = 1 - 3200 / 3000 < 0; k80: b = 1 - 1.6 < 0; p: 0.8, defined
PLAIN_COUNTS = (1000, 30, 20)


class PlantedCounts(NamedTuple):
    valid: np.ndarray  # R x n x n uint32
    ts: np.ndarray
    tv: np.ndarray
    planted: tuple  # per matrix, ((i, j), kind) with i < j and kind NO_COLUMNS or SATURATED

    def undefined(self, model: str) -> list[list[int]]:
        """Per matrix [pairs without a column, saturated pairs] as planted: nothing saturates under p."""
        return [[sum(kind == NO_COLUMNS for _, kind in of), 0 if model == "p" else sum(kind == SATURATED for _, kind in of)] for of in self.planted]


def _plant(counts, planted) -> PlantedCounts:
    for r, of in enumerate(planted):
        for (i, j), kind in of:
            assert i < j
            for x, value in zip(counts, NO_COLUMN_COUNTS if kind == NO_COLUMNS else SATURATED_COUNTS):
                x[r, i, j] = x[r, j, i] = value
    out = PlantedCounts(*(x.astype(np.uint32) for x in counts), tuple(tuple(of) for of in planted))
    for x in out[:3]:
        x.setflags(write=False)
    return out


STRIDED_ROWS, STRIDED_REPLICATES = 257, 5


@functools.lru_cache(maxsize=None)
def strided_counts(seed: int = 57) -> PlantedCounts:
    """Five 257 x 257 matrices of counts: the first launch of the distances holds four, 264 196 cells, of which the last
    2052 -- rows 249 and up of matrix 3 -- are written on the lanes' second trip, where the wave vote runs again (the last
    wave with four lanes); the second launch holds one.  V in [200, 1000], S and T in [0, 20]: no pair is undefined but
    the planted ones, of which every matrix has another number of each kind; those of matrix 3 in rows 250 and up are
    counted on the second trip."""
    rng = np.random.default_rng(seed)
    n, reps = STRIDED_ROWS, STRIDED_REPLICATES
    valid = np.stack([bootstrap_cases.symmetric_integers(rng, n, 200, 1000) for _ in range(reps)])
    ts = np.stack([bootstrap_cases.symmetric_integers(rng, n, 0, 20) for _ in range(reps)])
    tv = np.stack([bootstrap_cases.symmetric_integers(rng, n, 0, 20) for _ in range(reps)])
    for x in (ts, tv):
        x[:, np.arange(n), np.arange(n)] = 0
    none_first, saturated_first = (1, 2, 3, 1, 5), (2, 4, 1, 3, 6)
    planted = []
    for r in range(reps):  # the first trip: row r and row 20 + r
        of = [((r, 10 + k), NO_COLUMNS) for k in range(none_first[r])] + [((20 + r, 40 + k), SATURATED) for k in range(saturated_first[r])]
        planted.append(of)
    planted[3] += [((n - 7, n - 6), NO_COLUMNS), ((n - 7, n - 1), NO_COLUMNS), ((n - 2, n - 1), NO_COLUMNS)]
    planted[3] += [((n - 6, n - 4), SATURATED), ((n - 3, n - 1), SATURATED)]
    return _plant((valid, ts, tv), planted)


def strided_cells_of(counts: PlantedCounts, first_row: int) -> list[int]:
    """The index within its launch of the cells (i, j) and (j, i) of every pair planted at row ``first_row`` or below."""
    n, batch = counts.valid.shape[1], distance_batch()
    return [
        (r % batch) * n * n + a * n + b
        for r, of in enumerate(counts.planted)
        for (i, j), _kind in of
        if i >= first_row
        for a, b in ((i, j), (j, i))
    ]


@functools.lru_cache(maxsize=None)
def small_counts(n: int) -> PlantedCounts:
    """Matrices so small that a wave spans a whole launch of them, undefined pairs in the matrices that do not lead the
    wave.  n = 3: 27 matrices, every assignment of {defined, no column, saturated} to the pairs (0, 1), (0, 2), (1, 2), the
    kinds of matrix r the digits of r in base 3.  n = 2: nine matrices of one pair, each kind next to each."""
    pairs = [(i, j) for i in range(n) for j in range(i + 1, n)]
    if n == 3:  # noqa: PLR2004
        kinds = [[(r // 3**k) % 3 for k in range(3)] for r in range(27)]
    else:
        assert n == 2  # noqa: PLR2004
        kinds = [[kind] for kind in (DEFINED, DEFINED, NO_COLUMNS, NO_COLUMNS, SATURATED, SATURATED, DEFINED, SATURATED, NO_COLUMNS)]
    counts = [np.full((len(kinds), n, n), value, dtype=np.int64) for value in PLAIN_COUNTS]
    for x in counts[1:]:
        x[:, np.arange(n), np.arange(n)] = 0
    return _plant(counts, [[(pair, kind) for pair, kind in zip(pairs, of) if kind != DEFINED] for of in kinds])


# ---------------------------------------------------------------- the whole pipeline
class Restated(NamedTuple):
    D: Distances
    reference: tree_cases.Joins
    trees: list  # Joins per replicate
    support: list[int]  # per join of the reference; empty without replicates


def assert_same_tree(n: int, got, want, what: str = "") -> None:
    """Two join tables (anything with child, length, last, last_len) are the same unrooted tree: the same edges as
    bipartitions of the leaves, the lengths equal to 1e-9.  Distances that differ in their last bits -- the rule's logarithm
    against ``math.log`` -- may number the joins differently (with three nodes left every pair has the same score but for
    rounding), and do not change the tree."""
    a = tree_cases.joins_bipartitions(n, got.child, got.length, got.last, got.last_len)
    b = tree_cases.joins_bipartitions(n, want.child, want.length, want.last, want.last_len)
    assert set(a) == set(b), what
    for side, length in a.items():
        assert abs(length - b[side]) <= 1e-9 * max(1.0, abs(b[side])), what


def pipeline(rows: np.ndarray, model: str, missing: float, replicates: int = 0, seed: int = 0) -> Restated:
    """Distances, tree and support of ``rows`` from the restatements alone: the draws are ``bootstrap_cases.weights``."""
    n, n_cols = rows.shape
    D = distances(*counts_fast(rows), model, missing)
    reference = tree_cases.neighbour_joining(D.D)
    w = bootstrap_cases.weights(seed, n_cols, 0, replicates)
    trees = [tree_cases.neighbour_joining(distances(*counts_fast(rows, w[r]), model, missing).D) for r in range(replicates)]
    support = bootstrap_cases.support(n, reference.child, [bootstrap_cases.clades(n, t) for t in trees]) if replicates else []
    return Restated(D, reference, trees, support)
