"""Inputs for plot-run's distributions: the families the automatic bin rule is compared on, vectors aimed at the passes
of the radix select, the data and grids of the density cases (the ones of tests/golden/plot_run_dist/cases.json among
them), histogram values on the edges of many bins, and the tolerances.

Used by tests/test_distribution_host.py (no GPU: ``auto_bin_edges``, the host twins, ``rundb.plot_run``),
tests/test_gpu_distribution.py (the kernels) and tests/golden/plot_run_dist/make_plot_run_dist_golden.py (scipy's
densities).  ``TILE`` and ``GRID_SPAN`` restate csrc/dist.hip; when the kernels' change, change them here."""

from __future__ import annotations

import hashlib
import json
import math

import numpy as np

from pyani_plus_amd import _capi, distribution, run_comp
from tests.helpers import GOLDEN
from tests.run_comp_cases import adversarial_values, numpy_hist  # noqa: F401  (the tests import them from here)

TILE = 256  # csrc/dist.hip: elements a workgroup of a grid-stride pass takes per step (kThreads)
GRID_SPAN = 1024 * TILE  # ... and all its workgroups together (kMaxBlocks): longer vectors make the grid stride
CHAIN = _capi.PA_KDE_CHAIN
LDS_BINS = _capi.PA_HIST_WIDE_LDS_BINS

# ---------------------------------------------------------------- the automatic bin rule
EDGE_FAMILIES = ("normal", "ties", "rounded", "equal")
EDGE_SMALL_SIZES = (1, 2, 3, 4, 5, 7, 8)
EDGE_RANDOM_SIZES = tuple(int(n) for n in np.random.default_rng(400).integers(1, 3001, 300))


def edge_values(family: str, n: int, seed: int = 0) -> np.ndarray:
    """``normal``; ``ties``: 70 % of the values are 1.0; ``rounded``: two decimals; ``equal``: one value."""
    rng = np.random.default_rng(1000 * n + EDGE_FAMILIES.index(family) + 7 * seed)
    x = rng.normal(size=n)
    if family == "ties":
        x[rng.random(n) < 0.7] = 1.0  # noqa: PLR2004
    elif family == "rounded":
        x = np.round(x, 2)
    elif family == "equal":
        x = np.full(n, 0.75)
    return x


def edges_from_sorted(x) -> np.ndarray:
    """``auto_bin_edges`` fed from ``numpy.sort``: the path of ``describe`` with the select replaced."""
    s = np.sort(np.asarray(x, dtype=np.float64))
    return distribution.auto_bin_edges(len(s), s[0], s[-1], s[list(distribution.quartile_ranks(len(s)))])


def same_bits(got, want) -> None:
    got, want = np.ascontiguousarray(got, dtype=np.float64), np.ascontiguousarray(want, dtype=np.float64)
    assert got.shape == want.shape, (got.shape, want.shape)
    assert np.array_equal(got.view(np.uint64), want.view(np.uint64))


# ---------------------------------------------------------------- select
SELECT_SIZES = (1, 2, 63, 64, 65, TILE - 1, TILE, TILE + 1, 300_001)  # the last is past GRID_SPAN
SELECT_KINDS = ("equal", "two values", "low byte", "high byte", "special", "nan")
SPECIAL = (-np.inf, -1e300, -1.5, -2.5e-308, -5e-324, -0.0, 0.0, 5e-324, 2.5e-308, 1.5, 1e300, np.inf)


def select_values(kind: str, n: int) -> np.ndarray:
    """``low byte`` / ``high byte``: doubles whose order keys differ in that byte alone (decided by the last or by the
    first pass); ``special``: negatives, both zeros, subnormals and both infinities among normal values; ``nan``: every
    other element NaN."""
    rng = np.random.default_rng(31 * n + SELECT_KINDS.index(kind))
    if kind == "equal":
        return np.full(n, -0.125)
    if kind == "two values":
        return np.where(rng.random(n) < 0.5, 0.25, -3.0)  # noqa: PLR2004
    if kind == "low byte":
        return (np.uint64(0x3FF0000000000000) + rng.integers(0, 256, n).astype(np.uint64)).view(np.float64)
    if kind == "high byte":  # sign and the top seven exponent bits; the other exponent bits are 0, so never inf or NaN
        return ((rng.integers(0, 256, n).astype(np.uint64) << np.uint64(56)) | np.uint64(0x0008000000000000)).view(np.float64)
    if kind == "special":
        x = rng.normal(size=n)
        pick = rng.random(n) < 0.5  # noqa: PLR2004
        x[pick] = np.array(SPECIAL)[rng.integers(0, len(SPECIAL), int(pick.sum()))]
        return x
    assert kind == "nan"
    x = rng.normal(size=n)
    x[1::2] = np.nan
    if n == 1:
        x[0] = 0.5
    return x


def select_rank_sets(n_valid: int) -> list[list[int]]:
    """The first and the last rank; an adjacent pair; a repeated rank; eight ranks at once, unordered."""
    mid = n_valid // 2
    eight = [(k * (n_valid - 1)) // 7 for k in (3, 0, 7, 5, 1, 6, 2, 4)]
    return [[0, n_valid - 1], [max(mid - 1, 0), mid], [mid, mid], eight]


def sorted_valid(x) -> np.ndarray:
    x = np.asarray(x, dtype=np.float64)
    return np.sort(x[~np.isnan(x)])


# ---------------------------------------------------------------- density
KDE_SIZES = (1, 63, 64, 65, CHAIN - 1, CHAIN, CHAIN + 1, 100_003)
KDE_GRIDS = (1, 200, 1024)
RTOL_SCIPY, ATOL_SCIPY = 1e-11, 1e-300  # a plain numpy evaluation of the definition is within 5.2e-14 of gaussian_kde


def device_bound(n: int, n_grid: int) -> float:
    """Device against host twin, relative: the terms are non-negative, so a sum of them is off by at most (additions a
    term passes through) * 2^-53: ``CHAIN`` one after the other, then the tree over the partial sums.  4 * 746 * 2^-53
    covers an argument error of four roundings at the largest exponent that does not underflow, 8 * 2^-53 the two exp
    implementations, the scaling and the twin's own rounding."""
    return (CHAIN + distribution.kde_tree_depth(n, n_grid) + 4 * 746 + 8) * 2.0**-53


def kde_values(kind: str, n: int, seed: int = 0) -> np.ndarray:
    """``identity``: scores shaped like an identity matrix's cells, most near 0.8-1, a share exactly 1.0; ``clusters``:
    two clusters of spread 1e-5 that are 0.2 apart; ``nan``: ``identity`` with every third element NaN."""
    rng = np.random.default_rng(77 * n + 5 * seed + len(kind))
    if kind == "clusters":
        return np.where(np.arange(n) % 2 == 0, 0.4, 0.6) + 1e-5 * rng.normal(size=n)
    x = np.clip(0.9 + 0.05 * rng.normal(size=n), 0.0, 1.0)
    x[rng.random(n) < 0.05] = 1.0  # noqa: PLR2004
    if kind == "nan":
        x[::3] = np.nan
        x[:2] = (0.85, 0.95)  # two values at least
    return x


def scott_bw(x) -> float:
    v = np.asarray(x, dtype=np.float64)
    v = v[~np.isnan(v)]
    return float(np.std(v, ddof=1) * len(v) ** (-1.0 / 5.0))


def kde_grid(x, bw: float, n_grid: int, through_datum: bool = False) -> np.ndarray:
    """seaborn's support grid; ``through_datum`` puts the first value of ``x`` itself on the grid."""
    v = np.asarray(x, dtype=np.float64)
    v = v[~np.isnan(v)]
    grid = np.linspace(v.min() - 3 * bw, v.max() + 3 * bw, n_grid)
    if through_datum:
        grid[np.searchsorted(grid, v[0])] = v[0]  # still ascending
    return grid


def numpy_kde(x, grid, bw: float) -> np.ndarray:
    """Definition 2 with numpy, each grid point's terms added by ``math.fsum`` (exactly rounded)."""
    v = np.asarray(x, dtype=np.float64)
    v = v[~np.isnan(v)]
    norm = 1.0 / (len(v) * bw * math.sqrt(2 * math.pi))
    return np.array([math.fsum(np.exp(-0.5 * ((g - v) / bw) ** 2).tolist()) * norm for g in np.asarray(grid, dtype=np.float64)])


def close(got, want, rtol: float, atol: float = 0.0) -> bool:
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    return got.shape == want.shape and bool(np.all(np.abs(got - want) <= atol + rtol * np.abs(want)))


def worst(got, want) -> float:
    """The largest relative difference, for the messages."""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        rel = np.abs(got - want) / np.abs(want)
    return float(np.nanmax(np.where(want == 0, np.abs(got), rel))) if len(want) else 0.0


# the cases of the golden file: scipy's gaussian_kde on these
GOLDEN_DIR = GOLDEN / "plot_run_dist"


def golden_specs() -> list[dict]:
    specs = [{"name": f"identity-n{n}-g200", "kind": "identity", "n": n, "n_grid": 200} for n in (63, 65, CHAIN - 1, CHAIN + 1, 100_003)]
    specs.append({"name": "identity-n64-g1", "kind": "identity", "n": 64, "n_grid": 1})
    specs.append({"name": f"identity-n{CHAIN}-g1024", "kind": "identity", "n": CHAIN, "n_grid": 1024})
    specs.append({"name": "through-datum-n257-g200", "kind": "identity", "n": 257, "n_grid": 200, "through_datum": True})
    specs.append({"name": "nan-n3000-g200", "kind": "nan", "n": 3000, "n_grid": 200})
    specs.append({"name": "clusters-n1000-g200", "kind": "clusters", "n": 1000, "n_grid": 200, "bw_target": 2e-3})
    return specs


def values_md5(x) -> str:
    return hashlib.md5(np.ascontiguousarray(x, dtype=np.float64).tobytes()).hexdigest()  # noqa: S324


def load_golden() -> list[dict]:
    """The golden cases with ``bw`` and ``density`` as floats (stored as hex, so exactly scipy's)."""
    cases = json.loads((GOLDEN_DIR / "cases.json").read_text())["cases"]
    for case in cases:
        case["bw"] = float.fromhex(case["bw"])
        case["density"] = np.array([float.fromhex(h) for h in case["density"]])
    return cases


def golden_inputs(case: dict) -> tuple[np.ndarray, np.ndarray]:
    """``(values, grid)`` of a golden case, rebuilt from its settings and its stored bandwidth."""
    x = kde_values(case["kind"], case["n"])
    return x, kde_grid(x, case["bw"], case["n_grid"], case.get("through_datum", False))


# ---------------------------------------------------------------- wide histogram
WIDE_BINS = (1, 1024, 1025, 5000, 2**20)
WIDE_BINS_DEVICE = (*WIDE_BINS, LDS_BINS - 1, LDS_BINS, LDS_BINS + 1)


def wide_inputs(bins: int) -> tuple[np.ndarray, np.ndarray]:
    """``(values, edges)``: every edge of ``bins`` uniform bins (the last among them), its two neighbouring doubles, the
    bins' midpoints, NaN, and values outside."""
    rng = np.random.default_rng(bins)
    lo, hi = sorted(rng.random(2) * 4 - 2)
    edges = run_comp.hist_edges(lo, hi, bins)
    values = np.concatenate([adversarial_values(edges), [np.nan, lo - 1.0, hi + 1.0, np.nan]])
    return rng.permutation(values), edges
