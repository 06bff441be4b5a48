"""Shared helpers for the test-suite (reading the golden fixtures)."""

from __future__ import annotations

import csv
import gzip
import hashlib
import json
from pathlib import Path

import numpy as np

GOLDEN = Path(__file__).resolve().parent / "golden"

# fixture set -> (scaled, {md5: fasta file name})
FIXTURE_SETS = {
    "viral_example": (
        300,
        {
            "689d3fd6881db36b5e08329cf23cecdd": "MGV-GENOME-0264574.fas",
            "78975d5144a1cd12e98898d573cf6536": "MGV-GENOME-0266457.fna",
            "5584c7029328dc48d33f95f0a78f7e57": "OP073605.fasta",
        },
    ),
    "bad_alignments": (
        300,
        {
            "689d3fd6881db36b5e08329cf23cecdd": "MGV-GENOME-0264574.fas",
            "a30481565b45f6bbc6ce5260503067e0": "MGV-GENOME-0357962.fna",
        },
    ),
    "bacterial_example": (
        1000,
        {
            "f19cb07198a41a4406a22b2f57a6b5e7": "NC_002696.fasta.gz",
            "073194224aa8c13bebc1d14a3e74a3e7": "NC_010338.fna.gz",
            "9d72a8fb513cf9cc8cc6605a0ad4e837": "NC_011916.fas.gz",
            "9a9e23bfc5a184b8149e07e267d133b0": "NC_014100.fna.gz",
        },
    ),
}


def read_fasta_bytes(path: Path) -> bytes:
    """Decompressed file content (what the reference md5s, utils.py:178-196)."""
    raw = Path(path).read_bytes()
    return gzip.decompress(raw) if raw[:2] == b"\x1f\x8b" else raw


def md5_hex(data: bytes) -> str:
    return hashlib.md5(data).hexdigest()  # noqa: S324


def load_sig(path: Path) -> dict:
    """The single signature object of a sourmash `.sig` JSON fixture."""
    obj = json.loads(Path(path).read_text())
    assert isinstance(obj, list) and len(obj) == 1
    return obj[0]


def sig_mins(path: Path) -> np.ndarray:
    return np.array(load_sig(path)["signatures"][0]["mins"], dtype=np.uint64)


def load_manysearch(path: Path) -> list[dict]:
    with Path(path).open() as handle:
        return list(csv.DictReader(handle))


def invalid_distance_matrices(n: int, seed: int) -> list[tuple[str, np.ndarray, tuple[int, int]]]:
    """``(what, an n x n matrix that breaks the rule of a distance matrix, the first offending cell in row-major order)``.

    The rule: finite, not negative, the bits of its transpose, zero diagonal.  Every matrix breaks it in one way, on a
    random matrix that keeps it; the asymmetric one differs from its transpose by one unit in the last place.
    """
    assert n >= 6
    a = np.random.default_rng(seed).random((n, n))
    base = a + a.T  # commutative: bitwise symmetric
    np.fill_diagonal(base, 0.0)
    out = []
    for what, (i, j), value in (("nan", (n // 4, n // 2 + 1), np.nan), ("negative", (1, 3), -0.25), ("infinite", (0, n - 1), np.inf)):
        d = base.copy()
        d[i, j] = d[j, i] = value
        out.append((what, d, (i, j)))
    d = base.copy()
    d[n // 2, n - 1] = np.nextafter(d[n // 2, n - 1], 2.0)
    out.append(("asymmetric", d, (n // 2, n - 1)))
    d = base.copy()
    d[n - 2, n - 2] = 0.5
    out.append(("diagonal", d, (n - 2, n - 2)))
    return out


def offending_cells(D: np.ndarray) -> tuple[tuple[int, int], int]:
    """The rule of a distance matrix restated on whole arrays: ``(the first cell that breaks it in row-major order, how
    many do)``."""
    d = np.ascontiguousarray(D, dtype=np.float64)
    bad = ~np.isfinite(d) | (d < 0.0) | (d.view(np.uint64) != np.ascontiguousarray(d.T).view(np.uint64)) | (np.eye(len(d), dtype=bool) & (d != 0.0))
    first = int(np.argmax(bad))
    return (first // len(d), first % len(d)), int(bad.sum())


def distance_check_cases() -> list[tuple[str, np.ndarray, tuple[int, int], int]]:
    """``(name, matrix, first offending cell, offending cells)`` at the seams of the device check, whose workgroups take
    256 cells each in row-major order.

    n = 17 has 289 cells, so the second workgroup begins at cell (15, 1) and holds 33: a mirrored pair of negative values
    and a non-zero diagonal cell, once with the first of them in the first workgroup and once with all in the second.
    n = 130: the only asymmetric pair is (129, 0) and (0, 129), the second written, the first reported.
    """
    def base(n: int) -> np.ndarray:
        a = np.random.default_rng(n).random((n, n))
        d = a + a.T
        np.fill_diagonal(d, 0.0)
        return d

    split = base(17)
    split[2, 16] = split[16, 2] = -0.5  # cells 50 and 274
    split[16, 16] = 0.25  # cell 288
    second = base(17)
    second[15, 16] = second[16, 15] = -0.5  # cells 271 and 287
    second[16, 16] = 0.25
    asym = base(130)
    asym[129, 0] = np.nextafter(asym[129, 0], 2.0)
    out = [("n17-both-workgroups", split, (2, 16), 3), ("n17-second-workgroup", second, (15, 16), 3), ("n130-mirrored-cell-first", asym, (0, 129), 2)]
    assert all(offending_cells(d) == (cell, count) for _, d, cell, count in out)
    return out


def distance_refusal(who: str, name: str, cell: tuple[int, int], count: int) -> str:
    """The whole message of the refusal of a distance matrix."""
    return (f"{who}: {name}[{cell[0]},{cell[1]}] is not finite, is negative, differs from its transpose's bits or is a non-zero diagonal cell "
            f"({count} such cells)")  # fmt: skip


def load_matrix_tsv(path: Path) -> tuple[list[str], np.ndarray]:
    """Reference export-run matrix (rows=query, cols=subject); blank -> NaN."""
    with Path(path).open() as handle:
        rows = [line.rstrip("\n").split("\t") for line in handle]
    labels = rows[0][1:]
    mat = np.array([[float(v) if v not in ("", "nan", "NaN") else np.nan for v in r[1:]] for r in rows[1:]])
    return labels, mat
