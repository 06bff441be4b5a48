#!/usr/bin/env python3
"""Time the stages of plot-run's score distributions on generated matrices and write the numbers to
bench_out/dist_bench.json (a benchmark output, not kept in git; DESIGN.md section 7e has the table of the measured run).

    python tools/dist_bench.py device --sizes 1000 10000     # on the GPU machine
    python tools/dist_bench.py host --sizes 1000 10000       # without a GPU: the host twins, numpy and scipy

Each form fills its own section of the output file and leaves the other as it is.  Per size N: an N x N matrix of scores
shaped like an identity matrix (uniform in 0.8 .. 1, the diagonal 1.0, 2 % of the cells NaN), so N^2 cells.  Timed per
stage of ``distribution.describe``:

* ``select_s``: the four order statistics of the automatic bin rule (``pa_select_f64``);
* ``moments_s``: the mean and the squared deviations behind the bandwidth (``pa_moments_f64``);
* ``kde_s``: the density at 200 grid points (``pa_kde_gauss_f64``), N^2 x 200 terms;
* ``histogram_s``: the counts over the automatic bins (``pa_hist_uniform_f64_wide``); ``bins`` is their number;
* ``describe_s``: all of ``distribution.describe``, the range included.

``device``: between two HIP events, the matrix already on the device; the results are compared with the host twins' up to
``--check-max`` genomes.  ``host``: the host twins by a host clock; their density stage only up to ``--host-kde-max``
genomes (it is N^2 x 200 exponentials on one thread), and up to ``--reference-max`` genomes the basis of comparison:
``numpy.histogram_bin_edges(v, "auto")`` (``numpy_bin_edges_s``) and, where scipy imports, ``gaussian_kde(v)`` evaluated
on the same grid (``scipy_gaussian_kde_s``).

Every time is in seconds: the best and the median of ``--repeat`` runs after ``--warmup`` warm-up runs (one run and no
warm-up for host stages over more than 10^7 cells).
"""

from __future__ import annotations

import argparse
import json
import statistics
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

from pyani_plus_amd import distribution, run_comp  # noqa: E402

SEED = 43
NULLS = 0.02


def synth_scores(n: int) -> np.ndarray:
    rng = np.random.default_rng(SEED + n)
    scores = 0.8 + 0.2 * rng.random((n, n))
    np.fill_diagonal(scores, 1.0)
    scores[rng.random((n, n)) < NULLS] = np.nan
    return scores


def host_timed(fn, repeat: int, warmup: int) -> tuple[dict, object]:
    out = None
    for _ in range(warmup):
        out = fn()
    times = []
    for _ in range(repeat):
        t0 = time.perf_counter()
        out = fn()
        times.append(time.perf_counter() - t0)
    return {"best": min(times), "median": statistics.median(times), "runs": repeat}, out


def device_timed(engine, fn, repeat: int, warmup: int) -> tuple[dict, object]:
    t = engine.torch
    out = None
    for _ in range(warmup):
        out = fn()
    times = []
    for _ in range(repeat):
        e0, e1 = t.cuda.Event(enable_timing=True), t.cuda.Event(enable_timing=True)
        e0.record()
        out = fn()
        e1.record()
        e1.synchronize()
        times.append(e0.elapsed_time(e1) / 1e3)
    return {"best": min(times), "median": statistics.median(times), "runs": repeat}, out


def stages(values, engine, timed) -> tuple[dict, distribution.Distribution]:
    """The stages on ``values`` (a host array, or with an ``engine`` a tensor on its device); ``timed(name, fn)`` times
    one and returns its result, or None when the stage is left out."""
    on_device = engine is not None
    row: dict = {}
    lo, hi, n = engine.minmax(values) if on_device else run_comp.minmax_host(values)
    ranks = distribution.quartile_ranks(n)
    stats = timed(row, "select_s", lambda: engine.select(values, ranks) if on_device else distribution.select_host(values, ranks))
    edges = distribution.auto_bin_edges(n, lo, hi, stats)
    row["bins"] = len(edges) - 1
    timed(row, "histogram_s", lambda: engine.hist_uniform_wide(values, edges) if on_device else distribution.hist_uniform_wide_host(values, edges))
    _mean, squares = timed(row, "moments_s", lambda: engine.moments(values) if on_device else distribution.moments_host(values))
    bw = float(np.sqrt(squares / (n - 1)) * n ** (-1.0 / 5.0))
    grid = np.linspace(lo - 3 * bw, hi + 3 * bw, distribution.KDE_GRID)
    timed(row, "kde_s", lambda: engine.kde_gauss(values, grid, bw) if on_device else distribution.kde_gauss_host(values, grid, bw))
    dist = timed(row, "describe_s", lambda: distribution.describe(values, engine))
    return row, dist


def main() -> int:  # noqa: C901, PLR0915
    parser = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    parser.add_argument("what", choices=("device", "host"))
    parser.add_argument("--sizes", type=int, nargs="+", default=[1000, 10000])
    parser.add_argument("--repeat", type=int, default=5)
    parser.add_argument("--warmup", type=int, default=2)
    parser.add_argument("--host-kde-max", type=int, default=1000, help="largest N at which the host twin's density is timed")
    parser.add_argument("--reference-max", type=int, default=1000, help="largest N at which numpy's bin edges and scipy's gaussian_kde are timed")
    parser.add_argument("--check-max", type=int, default=1000, help="largest N at which the device results are compared with the host twins'")
    parser.add_argument("--machine", default=None, help="a line about the machine, kept in the settings")
    parser.add_argument("--out", type=Path, default=ROOT / "bench_out" / "dist_bench.json")
    args = parser.parse_args()
    out = {"settings": {"generator": f"synth_scores(n), seed {SEED}, {NULLS:.0%} NaN cells", "unit": "seconds; best and median of the runs after the warm-up",
                        "repeat": args.repeat, "warmup": args.warmup, "kde_grid": distribution.KDE_GRID}, "sizes": {}}  # fmt: skip
    if args.machine:
        out["settings"]["machine"] = args.machine
    engine = None
    if args.what == "device":
        from pyani_plus_amd.engine import HipEngine

        engine = HipEngine(0)
        info = engine.device_info()
        out["settings"].update(device=info["name"], compute_units=info["compute_units"])
    try:
        for n in args.sizes:
            scores = synth_scores(n)
            cells = n * n
            big = cells > 10**7

            if engine is not None:
                d_scores = engine.torch.from_numpy(scores).to(engine.device)
                engine.sync()

                def timed(row, name, fn):
                    row[name], result = device_timed(engine, fn, args.repeat, args.warmup)
                    return result

                row, dist = stages(d_scores, engine, timed)
                if n <= args.check_max:
                    host = distribution.describe(scores)
                    assert np.array_equal(dist.edges.view(np.uint64), host.edges.view(np.uint64)) and np.array_equal(dist.counts, host.counts), "the histograms differ"
                    worst = float(np.max(np.abs(dist.density - host.density) / host.density))
                    assert worst < 1e-11, f"the densities differ by {worst}"  # noqa: PLR2004
                    row["same_histogram_as_host"], row["density_worst_relative_difference_to_host"] = True, worst
                del d_scores
            else:

                def timed(row, name, fn):
                    if name in {"kde_s", "describe_s"} and n > args.host_kde_max:
                        row[name] = None  # not run: N^2 x 200 exponentials on one thread
                        return None
                    row[name], result = host_timed(fn, 1 if big else args.repeat, 0 if big else 1)
                    return result

                row, _dist = stages(scores, None, timed)
                if n <= args.reference_max:
                    v = scores[~np.isnan(scores)]
                    row["numpy_bin_edges_s"], edges = host_timed(lambda: np.histogram_bin_edges(v, "auto"), args.repeat, 1)
                    assert len(edges) - 1 == row["bins"]
                    try:
                        from scipy.stats import gaussian_kde
                    except ImportError:
                        row["scipy_gaussian_kde_s"] = None
                    else:
                        grid = np.linspace(v.min(), v.max(), distribution.KDE_GRID)
                        row["scipy_gaussian_kde_s"], _density = host_timed(lambda: gaussian_kde(v)(grid), 3, 0)
            row = {"cells": cells, **row}
            out["sizes"][str(n)] = row
            print(f"n={n}: {json.dumps(row)}", flush=True)
            del scores
    finally:
        if engine is not None:
            engine.close()
    data = json.loads(args.out.read_text()) if args.out.is_file() else {}
    data[args.what] = out
    args.out.parent.mkdir(parents=True, exist_ok=True)
    args.out.write_text(json.dumps(data, indent=1) + "\n")
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
