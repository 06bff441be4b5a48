"""The contract of mantel-run-comp restated in numpy, independently of csrc/: the triangle sum with
its 64 accumulators a row, the tree over them and the chains in Python floats; the moments and the cross sum of a
permutation; the permutations of a seed, vectorised over the rows; and the inputs of the tests.  numpy's elementwise
``+``, ``-`` and ``*`` on float64 are single IEEE operations, so the bits below are the contract's."""

from __future__ import annotations

from functools import lru_cache

import numpy as np

from tests.helpers import invalid_distance_matrices

LANES = 64
SIZES = (3, 4, 63, 64, 65, 127, 128, 129, 130, 513)  # the minimum, the edges of one and two strides, rows 62 to 64 either side of a stride
GENERATED = 20  # generated permutations a size, before the reversal and the one with pi[0] = n - 1
_MASK = (1 << 64) - 1


# ------------------------------------------------------------------ the sums
def tri(T: np.ndarray) -> float:
    """The sum of T[i, j], j > i: accumulator j % 64 of row i takes its terms in ascending j from -0.0, the accumulators
    are added as a tree (w = 32 .. 1: a[l] += a[l + w] for l < w), and the rows' sums a[0] are added in ascending i from
    -0.0."""
    n = T.shape[0]
    blocks = -(-n // LANES)
    padded = np.zeros((n, blocks * LANES))
    padded[:, :n] = T
    column = np.arange(blocks * LANES)[None, :]
    live = (column > np.arange(n)[:, None]) & (column < n)
    acc = np.full((n, LANES), -0.0)
    for b in range(blocks):  # one block of 64 columns at a time: accumulator l meets column 64 b + l
        block = slice(LANES * b, LANES * (b + 1))
        acc = np.where(live[:, block], acc + padded[:, block], acc)
    w = LANES // 2
    while w:
        acc[:, :w] = acc[:, :w] + acc[:, w : 2 * w]
        w //= 2
    total = -0.0
    for rho in acc[:, 0].tolist():
        total = total + rho
    return total


def moments(M: np.ndarray) -> tuple[float, float, np.ndarray]:
    """``(mean, ss, the centred matrix)``: mean = tri(M) / (n (n - 1) / 2), ss = tri of the centred squares."""
    n = M.shape[0]
    mean = tri(M) / float(n * (n - 1) // 2)
    centred = M - mean
    return mean, tri(centred * centred), centred


def cross(x: np.ndarray, y: np.ndarray, pi) -> float:
    """tri of x[i, j] * y[pi[i], pi[j]] for the centred matrices x and y."""
    pi = np.asarray(pi, dtype=np.intp)
    return tri(x * y[pi][:, pi])


def restated(X: np.ndarray, Y: np.ndarray, perms) -> tuple[np.ndarray, np.ndarray]:
    """``(stats, cross)`` as ``pa_mantel`` defines them: (mean_x, mean_y, ss_x, ss_y); the identity's sum, then each row's."""
    mean_x, ss_x, x = moments(X)
    mean_y, ss_y, y = moments(Y)
    sums = [cross(x, y, np.arange(len(X)))] + [cross(x, y, pi) for pi in perms]
    return np.array([mean_x, mean_y, ss_x, ss_y]), np.array(sums)


# ------------------------------------------------------------------ the permutations of a seed
def fin(v: np.ndarray) -> np.ndarray:
    """The splitmix64 finaliser on uint64 arrays, mod 2^64."""
    with np.errstate(over="ignore"):
        z = v + np.uint64(0x9E3779B97F4A7C15)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        return z ^ (z >> np.uint64(31))


def permutations(seed: int, n: int, first: int, count: int) -> np.ndarray:
    """Rows ``first .. first + count - 1``: base = fin(fin(seed) + q); from 0 .. n - 1, for t = n - 1 down to 1 swap entries
    t and fin(base + t) mod (t + 1)."""
    q = np.array([(first + r) & _MASK for r in range(count)], dtype=np.uint64)
    with np.errstate(over="ignore"):
        base = fin(fin(np.array([seed], dtype=np.uint64)) + q)
        rows = np.tile(np.arange(n, dtype=np.uint32), (count, 1))
        at = np.arange(count)
        for t in range(n - 1, 0, -1):
            k = (fin(base + np.uint64(t)) % np.uint64(t + 1)).astype(np.intp)
            held = rows[at, t].copy()
            rows[at, t] = rows[at, k]
            rows[at, k] = held
    return rows


# ------------------------------------------------------------------ the inputs
def random_distances(n: int, seed: int) -> np.ndarray:
    """A finite, non-negative, bitwise symmetric matrix with a zero diagonal."""
    a = np.random.default_rng(seed).random((n, n))
    d = a + a.T  # commutative: bitwise symmetric
    np.fill_diagonal(d, 0.0)
    return np.ascontiguousarray(d)


def related_pair(n: int, seed: int) -> tuple[np.ndarray, np.ndarray]:
    """Two distance matrices that agree in part: Y = X + noise."""
    X = random_distances(n, seed)
    Y = X + 0.5 * random_distances(n, seed + 1000)
    return X, np.ascontiguousarray(Y)


def dyadic_distances(n: int, seed: int) -> np.ndarray:
    """Multiples of 2^-10 below 1: every sum of them the tests make is exact."""
    a = np.triu(np.random.default_rng(seed).integers(1, 1024, size=(n, n)), 1)
    return np.ascontiguousarray((a + a.T) / 1024.0)


def checked_permutations(n: int, seed: int) -> np.ndarray:
    """``GENERATED`` generated rows, the reversal, and a row with pi[0] = n - 1 (the rest in order)."""
    return np.vstack([permutations(seed, n, 0, GENERATED), np.arange(n, dtype=np.uint32)[::-1][None, :],
                      np.roll(np.arange(n, dtype=np.uint32), 1)[None, :]])  # fmt: skip



@lru_cache(maxsize=None)
def case(n: int):
    """``(X, Y, perms, restated stats, restated cross)`` of size n, computed once and shared (read-only)."""
    X, Y = related_pair(n, 40 + n)
    perms = checked_permutations(n, 7 + n)
    stats, sums = restated(X, Y, perms)
    for a in (X, Y, perms, stats, sums):
        a.setflags(write=False)
    return X, Y, perms, stats, sums


def invalid_matrices(n: int = 9):
    """``(what, a matrix that breaks the rule, the first offending cell in row-major order)``."""
    return invalid_distance_matrices(n, 5)


def bits(x) -> np.ndarray:
    return np.ascontiguousarray(x, dtype=np.float64).view(np.uint64)
