#!/usr/bin/env python3
"""Generate tests/golden/plot_run/cases.json with scipy (build machine only; no test runs this).

seaborn's ``clustermap``, which the reference's plot-run calls (pyani_plus/plot_run.py:114-147), orders a heatmap with
``scipy.cluster.hierarchy.linkage(rows, method="average", metric="euclidean")`` and the ``leaves`` of
``dendrogram(..., no_plot=True)``.  For every case that is what runs here, on the matrix tests/plot_run_cases.py rebuilds
from the case's settings with its NaN cells filled.  Stored per case: the settings, the md5 of the generated matrix
(before the fill), the number of row distances that equal another one, and scipy's leaves.

    python tests/golden/plot_run/make_plot_run_golden.py      # needs scipy
"""

from __future__ import annotations

import json
import sys
from pathlib import Path

HERE = Path(__file__).resolve().parent
ROOT = HERE.parent.parent.parent


def case_specs() -> list[dict]:
    specs = []

    def add(name, n, seed, na_fill=0, duplicates=0, **synth):
        specs.append({"name": name, "synth": {"n": n, "seed": seed, **synth}, "duplicates": duplicates, "na_fill": na_fill})

    for n in (2, 3, 63, 64, 65, 130, 257, 1000):
        add(f"plain-n{n}", n, 31)
    # two decimals and duplicated genomes: thousands of tied distances, zero distances among them
    for n in (3, 63, 130, 1000):
        add(f"tied-n{n}", n, 32, duplicates=max(1, n // 10), decimals=2)
    # 30 % NaN cells, filled as tANI's are (-5) and as the other scores' are (0)
    for n in (3, 65, 257):
        add(f"nan-fill-5-n{n}", n, 33, na_fill=-5, nan_frac=0.3)
    for n in (64, 130):
        add(f"nan-fill0-n{n}", n, 34, na_fill=0, nan_frac=0.3)
    add("nan-tied-n130", 130, 35, na_fill=-5, duplicates=13, nan_frac=0.3, decimals=2)
    return specs


def main() -> None:
    import numpy as np
    import scipy
    from scipy.cluster.hierarchy import dendrogram, linkage
    from scipy.spatial.distance import pdist

    sys.dont_write_bytecode = True
    sys.path.insert(0, str(ROOT))
    from tests.plot_run_cases import case_matrix, filled, matrix_md5

    cases = []
    for spec in case_specs():
        x = filled(spec)
        n = len(x)
        z = linkage(x, method="average", metric="euclidean")
        d = pdist(x, "euclidean")
        assert np.array_equal(z, linkage(d, method="average"))
        leaves = dendrogram(z, no_plot=True)["leaves"]
        assert sorted(leaves) == list(range(n))
        cases.append({**spec, "md5": matrix_md5(case_matrix(spec)), "tied": int(len(d) - len(np.unique(d))), "leaves": [int(v) for v in leaves]})
    lines = ",\n".join(json.dumps(case, separators=(",", ":")) for case in cases)
    (HERE / "cases.json").write_text('{"scipy":' + json.dumps(scipy.__version__) + ',"cases":[\n' + lines + "\n]}\n")
    print(f"wrote {len(cases)} cases to {HERE / 'cases.json'}")


if __name__ == "__main__":
    main()
