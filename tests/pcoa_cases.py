"""ordinate-run as it is defined, restated in plain numpy, and the matrices its tests share.  No library import.

The contract (include/pyani_hip.h), restated without looking at how the library computes anything:

* The tall product ``Y = A Q`` (A n x n, Q n x p).  The columns j of a row are cut into chunks of ``kChunk`` (stated in
  ``csrc/pcoa_rule.h``, read here by regex); within chunk b, ``s_b = ((A[i,j0] Q[j0,c] + A[i,j0+1] Q[j0+1,c]) + ...)``
  in ascending j, every product rounded, one accumulator that starts from the first product; ``Y[i,c]`` is the chunk
  sums added in ascending b in the same way.
* The centring of a distance matrix D (finite, >= 0, bitwise symmetric, zero diagonal): ``a = D * D``;
  ``r[i] = (a[i,0] + ... + a[i,n-1]) / n`` in ascending order; ``g = (r[0] + ... + r[n-1]) / n``;
  ``B[i,j] = -0.5 * ((a[i,j] - (r[i] + r[j])) + g)``; ``trace = B[0,0] + B[1,1] + ...``; ``fro2`` the sum over ascending
  i of the rows' sums over ascending j of ``B[i,j] * B[i,j]``.
* The solver's start block ``Q0[i,c] = start_value(i * p + c)``: the splitmix64 finaliser of the index, its top 52 bits
  u mapped to ``((u + 0.5) * 2^-51) - 1`` in (-1, 1).

numpy's elementwise operations are single IEEE operations, each a call of its own.  The reference for the solver is
``numpy.linalg.eigh`` on the whole matrix.
"""

from __future__ import annotations

import functools
import re
from pathlib import Path
from typing import NamedTuple

import numpy as np

from tests.helpers import invalid_distance_matrices

ROOT = Path(__file__).resolve().parent.parent
TOL = 1e-10  # the solver's default stop rule
PHASE1_CAP = 200  # iterations of the unshifted phase, at most
DEFAULT_MAX_ITER = 10000


def kernel_constants() -> dict[str, int]:
    """kChunk as csrc/pcoa_rule.h states it: the columns whose products are added into one accumulator."""
    text = (ROOT / "pyani_plus_amd" / "csrc" / "pcoa_rule.h").read_text()
    found = re.search(r"constexpr int kChunk = (\d+);", text)
    assert found, "kChunk not found in pcoa_rule.h"
    return {"kChunk": int(found.group(1))}


# ---------------------------------------------------------------- the tall product
def mul_tall(A: np.ndarray, Q: np.ndarray, chunk: int | None = None) -> np.ndarray:
    """The contract's order, one numpy operation per IEEE operation, every (i, c) at once."""
    chunk = chunk or kernel_constants()["kChunk"]
    A = np.asarray(A, dtype=np.float64)
    Q = np.asarray(Q, dtype=np.float64)
    n = A.shape[0]
    Y = None
    for j0 in range(0, n, chunk):
        s = A[:, j0 : j0 + 1] * Q[j0][None, :]
        for j in range(j0 + 1, min(j0 + chunk, n)):
            prod = A[:, j : j + 1] * Q[j][None, :]
            s = s + prod
        Y = s if Y is None else Y + s
    return Y


def product_sizes() -> list[int]:
    k = kernel_constants()["kChunk"]
    return sorted({1, 2, 63, 64, 65, k - 1, k, k + 1, 2 * k + 1})


PRODUCT_WIDTHS = (1, 2, 3, 11, 17, 32)


@functools.lru_cache(maxsize=None)
def product_input(n: int, p: int) -> tuple[np.ndarray, np.ndarray]:
    """Random normals scaled by 2^e, e uniform in [-20, 20]: the order of the additions shows in the bits."""
    rng = np.random.default_rng(1000 * n + p)
    A = rng.standard_normal((n, n)) * np.exp2(rng.integers(-20, 21, size=(n, n)))
    Q = rng.standard_normal((n, p)) * np.exp2(rng.integers(-20, 21, size=(n, p)))
    A.setflags(write=False)
    Q.setflags(write=False)
    return A, Q


@functools.lru_cache(maxsize=None)
def product_restated(n: int, p: int) -> np.ndarray:
    out = mul_tall(*product_input(n, p))
    out.setflags(write=False)
    return out


# ---------------------------------------------------------------- the centring
class Centred(NamedTuple):
    B: np.ndarray
    trace: float
    fro2: float


def gower_center(D: np.ndarray) -> Centred:
    D = np.asarray(D, dtype=np.float64)
    n = D.shape[0]
    a = D * D
    r = a[:, 0].copy()
    for j in range(1, n):
        r = r + a[:, j]
    r = r / np.float64(n)
    g = r[0]
    for i in range(1, n):
        g = g + r[i]
    g = g / np.float64(n)
    B = np.float64(-0.5) * ((a - (r[:, None] + r[None, :])) + g)
    trace = B[0, 0]
    for i in range(1, n):
        trace = trace + B[i, i]
    sq = B * B
    rows = sq[:, 0].copy()
    for j in range(1, n):
        rows = rows + sq[:, j]
    fro2 = rows[0]
    for i in range(1, n):
        fro2 = fro2 + rows[i]
    return Centred(B, float(trace), float(fro2))


def random_distances(n: int, seed: int) -> np.ndarray:
    """Symmetric, zero diagonal, off-diagonal uniform in (0, 1]: a distance matrix with no structure."""
    rng = np.random.default_rng(seed)
    upper = np.triu(1.0 - rng.random((n, n)), 1)
    return upper + upper.T


CENTRING_SIZES = (1, 2, 3, 65, 257)


def invalid_matrices() -> list[tuple[str, np.ndarray, tuple[int, int]]]:
    """(what, matrix, the first offending cell in row-major order)."""
    return invalid_distance_matrices(6, 1)


# ---------------------------------------------------------------- the start block
_M64 = (1 << 64) - 1


def start_value(index: int) -> float:
    z = (index + 0x9E3779B97F4A7C15) & _M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & _M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & _M64
    z = z ^ (z >> 31)
    return (float(z >> 12) + 0.5) * 2.0**-51 - 1.0


def start_block(n: int, p: int) -> np.ndarray:
    return np.array([[start_value(i * p + c) for c in range(p)] for i in range(n)], dtype=np.float64)


def block_width(n: int, k: int) -> int:
    return min(n, max(2 * k, k + 8), 32)


# ---------------------------------------------------------------- the solver's cases
class Case(NamedTuple):
    name: str
    B: np.ndarray  # the symmetric matrix the solver is given
    fro2: float
    D: np.ndarray | None  # the distances it was centred from, where there are any


def euclid_points(n: int = 130, dims: int = 4, seed: int = 11) -> np.ndarray:
    """Dyadic coordinates: multiples of 2^-6 in [0, 4)."""
    return np.random.default_rng(seed).integers(0, 256, size=(n, dims)) / 64.0


def pairwise(X: np.ndarray) -> np.ndarray:
    diff = X[:, None, :] - X[None, :, :]
    D = np.sqrt((diff * diff).sum(axis=2))
    D = np.triu(D, 1)
    return D + D.T


def ani_like(n: int = 800, clusters: int = 20, seed: int = 3) -> np.ndarray:
    """Genomes in ``clusters`` groups whose centres lie in three dimensions: distances of the size 1 - ANI takes (up to
    about 0.3 between groups, about 0.01 within one) with symmetric noise, so not Euclidean.  The centres' coordinates
    are centred orthonormal columns scaled by (0.30, 0.18, 0.18): the second and the third axis carry the same
    variation, so the third eigenvalue is comparable to the second and two axes alone cannot be certified."""
    rng = np.random.default_rng(seed)
    spread = rng.standard_normal((clusters, 3))
    centres = np.linalg.qr(spread - spread.mean(axis=0))[0] * np.array([0.30, 0.18, 0.18])
    member = np.arange(n) % clusters
    D = pairwise(centres)[np.ix_(member, member)] + 0.01
    noise = np.triu(rng.uniform(-0.004, 0.004, size=(n, n)), 1)
    D = D + noise + noise.T
    np.fill_diagonal(D, 0.0)
    assert (D >= 0).all()
    return D


def adversarial(n: int = 300, seed: int = 9) -> np.ndarray:
    """A symmetric matrix with the spectrum {10, 9, 8, 1, 0.5, thirty values near -5.5, a small rest}: the thirty
    negative ones outweigh the fourth and fifth in magnitude, so an unshifted iteration would return one of them."""
    rng = np.random.default_rng(seed)
    spectrum = np.concatenate([[10.0, 9.0, 8.0, 1.0, 0.5], -5.5 + 0.02 * rng.standard_normal(30), 0.01 * rng.standard_normal(n - 35)])
    V, _ = np.linalg.qr(rng.standard_normal((n, n)))
    B = (V * spectrum[None, :]) @ V.T
    return 0.5 * (B + B.T)


@functools.lru_cache(maxsize=None)
def cases() -> tuple[Case, ...]:
    out = []
    for name, D in (("euclid130x4", pairwise(euclid_points())), ("ani800", ani_like()), ("noise400", random_distances(400, 21)),
                    ("one", np.zeros((1, 1))), ("two", np.array([[0.0, 0.375], [0.375, 0.0]])), ("random9", random_distances(9, 5)),
                    ("random40", random_distances(40, 6))):
        c = gower_center(D)
        out.append(Case(name, c.B, c.fro2, D))
    B = adversarial()
    out.append(Case("adversarial300", B, float((B * B).sum()), None))
    for c in out:
        c.B.setflags(write=False)
        if c.D is not None:
            c.D.setflags(write=False)
    return tuple(out)


def case(name: str) -> Case:
    return next(c for c in cases() if c.name == name)


# (case, k): every solve the host and the device tests make with the default tolerance and iteration limit; the last one
# asks for the most pairs the solver takes, where the block is as wide as the product allows
SOLVES = (("euclid130x4", 4), ("ani800", 3), ("ani800", 2), ("noise400", 3), ("adversarial300", 4), ("one", 1), ("two", 1), ("two", 2),
          ("random9", 9), ("random40", 24))


@functools.lru_cache(maxsize=None)
def eigh_top(name: str, k: int) -> np.ndarray:
    """The k algebraically largest eigenvalues, descending, by numpy.linalg.eigh on the whole matrix."""
    return np.linalg.eigvalsh(case(name).B)[::-1][:k].copy()


@functools.lru_cache(maxsize=None)
def spectral_scale(name: str) -> float:
    """max |lambda| over the whole spectrum."""
    return float(np.abs(np.linalg.eigvalsh(case(name).B)).max())


def sign_rule_holds(vectors: np.ndarray) -> bool:
    """Every column's entry of largest magnitude, the first such in index order, is positive."""
    return all(v[int(np.argmax(np.abs(v)))] > 0 for v in vectors.T)
