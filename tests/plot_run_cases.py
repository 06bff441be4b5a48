"""Inputs of the plot-run golden cases (tests/golden/plot_run/cases.json), rebuilt from the settings each case stores.

Used by the tests and by tests/golden/plot_run/make_plot_run_golden.py, so that both see the same matrices; the md5 in
the case pins them."""

from __future__ import annotations

import hashlib
import json
from pathlib import Path

import numpy as np

from pyani_plus_amd.synth import synth_classify_matrices

GOLDEN = Path(__file__).resolve().parent / "golden"
CASES_FILE = GOLDEN / "plot_run" / "cases.json"


def case_matrix(case: dict) -> np.ndarray:
    """The identity matrix of the case's generator call, NaN cells included, with ``duplicates`` genomes made exact
    copies of others (row and column): genome 3 k + 1 becomes genome 3 k."""
    _labels, ident, _cov = synth_classify_matrices(**case["synth"])
    n = len(ident)
    for k in range(case.get("duplicates", 0)):
        src, dst = (3 * k) % n, (3 * k + 1) % n
        ident[dst, :] = ident[src, :]
        ident[:, dst] = ident[:, src]
    return np.ascontiguousarray(ident)


def filled(case: dict) -> np.ndarray:
    """What is clustered: the case's matrix with its NaN cells replaced by the case's ``na_fill``."""
    x = case_matrix(case)
    x[np.isnan(x)] = case["na_fill"]
    return x


def matrix_md5(matrix: np.ndarray) -> str:
    return hashlib.md5(np.ascontiguousarray(matrix, dtype=np.float64).tobytes()).hexdigest()  # noqa: S324


def load_cases() -> list[dict]:
    return json.loads(CASES_FILE.read_text())["cases"]


def numpy_distances(x: np.ndarray) -> np.ndarray:
    """pdist restated: one column at a time over all pairs, ``acc = acc + d * d`` (two roundings), then ``np.sqrt``."""
    i, j = np.triu_indices(len(x), 1)
    acc = np.zeros(len(i))
    for c in range(x.shape[1]):
        d = x[i, c] - x[j, c]
        acc = acc + d * d
    return np.sqrt(acc)


def distance_inputs(n: int, m: int):
    """(name, matrix) of the three kinds of input: plain, a third of the cells at -5, and duplicated rows."""
    rng = np.random.default_rng([n, m])
    plain = rng.uniform(0.0, 1.0, (n, m))
    yield "plain", plain
    fill = plain.copy()
    fill[rng.random((n, m)) < 0.3] = -5.0
    yield "filled", fill
    dup = np.round(plain, 2)
    for k in range(max(1, n // 8)):
        dup[(3 * k + 1) % n] = dup[(3 * k) % n]
    yield "duplicated", dup


def same_bits(got: np.ndarray, want: np.ndarray) -> None:
    assert got.dtype == want.dtype == np.float64 and got.shape == want.shape
    assert np.array_equal(got.view(np.uint64), want.view(np.uint64))
