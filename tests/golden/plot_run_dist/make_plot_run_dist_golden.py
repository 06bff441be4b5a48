#!/usr/bin/env python3
"""Generate tests/golden/plot_run_dist/cases.json with scipy (build machine only; no test runs this).

seaborn's ``kdeplot``, which the reference's plot-run calls (pyani_plus/plot_run.py:177), evaluates
``scipy.stats.gaussian_kde(values)`` with Scott's factor on a grid from ``min - 3 bw`` to ``max + 3 bw``.  For every case
of ``tests.distribution_cases.golden_specs`` that is what runs here, on the values and the grid that module rebuilds
from the case's settings.  Stored per case: the settings, the md5 of the generated values, and as hex floats scipy's
bandwidth (the square root of ``kde.covariance``) and its densities.  A case with ``bw_target`` sets the factor so that
the bandwidth comes out near that value instead of Scott's.

    python tests/golden/plot_run_dist/make_plot_run_dist_golden.py      # needs scipy
"""

from __future__ import annotations

import json
import sys
from pathlib import Path

HERE = Path(__file__).resolve().parent
ROOT = HERE.parent.parent.parent


def main() -> None:
    import numpy as np
    import scipy
    from scipy.stats import gaussian_kde

    sys.dont_write_bytecode = True
    sys.path.insert(0, str(ROOT))
    from tests.distribution_cases import golden_specs, kde_grid, kde_values, values_md5

    cases = []
    for spec in golden_specs():
        x = kde_values(spec["kind"], spec["n"])
        v = x[~np.isnan(x)]
        kde = gaussian_kde(v, bw_method=spec["bw_target"] / np.std(v, ddof=1)) if "bw_target" in spec else gaussian_kde(v)
        bw = float(np.sqrt(kde.covariance[0, 0]))
        grid = kde_grid(x, bw, spec["n_grid"], spec.get("through_datum", False))
        density = kde(grid)
        assert density.shape == (spec["n_grid"],) and np.isfinite(density).all()
        cases.append({**spec, "md5": values_md5(x), "bw": bw.hex(), "density": [float(d).hex() for d in density]})
    lines = ",\n".join(json.dumps(case, separators=(",", ":")) for case in cases)
    (HERE / "cases.json").write_text('{"scipy":' + json.dumps(scipy.__version__) + ',"cases":[\n' + lines + "\n]}\n")
    print(f"wrote {len(cases)} cases to {HERE / 'cases.json'}")


if __name__ == "__main__":
    main()
