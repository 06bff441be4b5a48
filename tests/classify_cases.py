"""Inputs of the classify golden cases (tests/golden/classify/cases.json), rebuilt from the settings each case stores.

Used by the tests and by tests/golden/classify/make_classify_golden.py, so that both see the same matrices; the md5 in
the case pins them."""

from __future__ import annotations

import hashlib
import json
from pathlib import Path

import numpy as np

from pyani_plus_amd.synth import synth_classify_matrices

GOLDEN = Path(__file__).resolve().parent / "golden"
CASES_FILE = GOLDEN / "classify" / "cases.json"


def base_matrices(source: dict) -> tuple[list[str], np.ndarray, np.ndarray]:
    """(labels sorted, identity, coverage) of a case's ``source``: a fixture set's matrices or the generator's."""
    if "fixture" in source:
        import pandas as pd

        folder = GOLDEN / source["fixture"] / "matrices"
        frames = []
        for kind in ("identity", "coverage"):
            frame = pd.read_csv(folder / f"{source['method']}_{kind}.tsv", sep="\t", index_col=0).astype(float)
            frames.append(frame.sort_index(axis=0).sort_index(axis=1))
        assert list(frames[0].index) == list(frames[0].columns) == list(frames[1].index) == list(frames[1].columns)
        return [str(x) for x in frames[0].columns], frames[0].to_numpy(dtype=float).copy(), frames[1].to_numpy(dtype=float).copy()
    return synth_classify_matrices(**source["synth"])


def matrices_md5(*mats: np.ndarray) -> str:
    digest = hashlib.md5()  # noqa: S324
    for m in mats:
        digest.update(np.ascontiguousarray(m, dtype=np.float64).tobytes())
    return digest.hexdigest()


def load_cases() -> list[dict]:
    """The cases, their rows unpacked to ``{"members": sorted labels, "raw": [n_nodes, max_cov, min_score, max_score as
    repr or None], "tsv": the reference's first four text fields}``, sorted by members."""
    cases = json.loads(CASES_FILE.read_text())["cases"]
    for case in cases:
        case["rows"] = [{"members": m.split(","), "raw": raw, "tsv": tsv} for m, raw, tsv in case["rows"]]
    return cases
