#!/usr/bin/env python3
"""Time the 2-D binning behind plot-run's scatter figures on generated points and write the numbers to
bench_out/scatter_bench.json (a benchmark output, not kept in git; profiles/scatter/scatter_bench.json is the measured
run and DESIGN.md section 7f has its table).

    python tools/scatter_bench.py device      # on the GPU machine
    python tools/scatter_bench.py host        # without a GPU: the host twin and numpy.histogram2d

Each form fills its own section of the output file and leaves the other as it is.  Per case -- ``--points`` points
(10^6 and 10^8), a grid of ``--grids`` cells an axis (256 and 1024), one of three distributions:

* ``uniform``: uniform over the grid, so every cell is hit and neighbours in memory fall into unrelated cells;
* ``one_cell``: every point in one cell, the most contended input there is;
* ``ani``: ``dist_bench.synth_scores`` (identity-like: uniform in 0.8 .. 1, the diagonal 1.0, 2 % NaN) against a
  coverage-like y (uniform in 0.5 .. 1, the diagonal 1.0, 2 % NaN of its own).

``device``: ``HipEngine.bin2d`` between two HIP events with the points already on the device -- the whole call, the
upload of the edges and the copy of the cells back to the host included -- and ``device_gb_per_s``, the effective rate
at 16 bytes a point; the result is compared with the host twin's on every timed input (``same_as_host``).  ``host``:
``scatter.bin2d_host`` and ``numpy.histogram2d`` on the same arrays by a host clock (numpy on the points that are not
NaN, as it refuses NaN), compared with each other.

``--command-size N`` (0: not at all) also times the whole command once on this backend: ``rundb.plot_run`` with
``formats=("tsv",)`` on a generated complete run of N genomes (the ``ani`` matrices), without and with ``scatter=True``,
by a host clock, the read of the run, the clustering and the tables included (``command``).

Every time is in seconds: the best and the median of ``--repeat`` runs after ``--warmup`` warm-up runs (one run and no
warm-up for host stages over more than 10^7 points).
"""

from __future__ import annotations

import argparse
import hashlib
import json
import sys
import tempfile
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tools"))

from dist_bench import NULLS, SEED, device_timed, host_timed, synth_scores  # noqa: E402

from pyani_plus_amd import run_comp, rundb, scatter  # noqa: E402

KINDS = ("uniform", "one_cell", "ani")


def points(kind: str, n: int) -> tuple[np.ndarray, np.ndarray]:
    rng = np.random.default_rng(SEED + n + KINDS.index(kind))
    if kind == "uniform":
        return rng.random(n), rng.random(n)
    if kind == "one_cell":
        return np.full(n, 0.3), np.full(n, 0.7)
    side = int(round(n**0.5))
    assert side * side == n, f"{n} points are not a square matrix"
    y = 0.5 + 0.5 * rng.random((side, side))
    np.fill_diagonal(y, 1.0)
    y[rng.random((side, side)) < NULLS] = np.nan
    return synth_scores(side).reshape(-1), y.reshape(-1)


def edges_for(kind: str, bins: int) -> tuple[np.ndarray, np.ndarray]:
    if kind == "ani":
        return run_comp.hist_edges(0.8, 1.0, bins), run_comp.hist_edges(0.5, 1.0, bins)
    return run_comp.hist_edges(0.0, 1.0, bins), run_comp.hist_edges(0.0, 1.0, bins)


def command_times(n: int, engine) -> dict:
    """``plot_run`` once without and once with ``scatter=True`` on a generated complete run of ``n`` genomes."""
    x, y = (v.reshape(n, n) for v in points("ani", n * n))
    rng = np.random.default_rng(SEED)
    hashes = sorted(hashlib.md5(str(i).encode()).hexdigest() for i in range(n))  # noqa: S324
    value = lambda v: None if np.isnan(v) else float(v)  # noqa: E731
    row: dict = {"genomes": n}
    with tempfile.TemporaryDirectory() as tmp:
        db = Path(tmp) / "run.sqlite"
        conn = rundb.connect_to_db(db)
        for h, length in zip(hashes, rng.integers(10**6, 10**7, n).tolist()):
            rundb.db_genome(conn, Path(f"{h}.fasta"), h, length, h)
        config = rundb.db_configuration(conn, "synthetic", "scatter_bench", "0")
        rundb.add_run(conn, config, "scatter_bench", Path("."), "Done", "generated", {Path(f"g{i}.fasta"): h for i, h in enumerate(hashes)})
        conn.executemany(rundb.INSERT_COMPARISON, ((hashes[i], hashes[j], config.configuration_id, value(x[i, j]), None, None, value(y[i, j]), "", "", "")
                                                   for i in range(n) for j in range(n)))  # fmt: skip
        conn.commit()
        conn.close()
        rundb.plot_run(db, Path(tmp) / "warm", engine=engine)  # fills the run's matrix cache, loads the libraries
        for key, flag in (("plot_run_s", False), ("plot_run_scatter_s", True)):
            t0 = time.perf_counter()
            written = rundb.plot_run(db, Path(tmp) / key, engine=engine, scatter=flag)
            row[key] = time.perf_counter() - t0
            row[key[:-2] + "_files"] = len(written)
    return row


def main() -> int:
    parser = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    parser.add_argument("what", choices=("device", "host"))
    parser.add_argument("--points", type=int, nargs="+", default=[10**6, 10**8])
    parser.add_argument("--grids", type=int, nargs="+", default=[scatter.GRID, scatter.MAX_BINS])
    parser.add_argument("--kinds", nargs="+", choices=KINDS, default=list(KINDS))
    parser.add_argument("--repeat", type=int, default=5)
    parser.add_argument("--warmup", type=int, default=1)
    parser.add_argument("--command-size", type=int, default=1000, help="genomes of the generated run the whole command is timed on (0: not at all)")
    parser.add_argument("--machine", default=None, help="a line about the machine, kept in the settings")
    parser.add_argument("--out", type=Path, default=ROOT / "bench_out" / "scatter_bench.json")
    args = parser.parse_args()
    out = {"settings": {"generator": f"points(kind, n), seed {SEED}; ani: {NULLS:.0%} NaN cells in x and in y", "repeat": args.repeat, "warmup": args.warmup,
                        "unit": "seconds; best and median of the runs after the warm-up", "bytes_per_point": 16}, "cases": {}}  # fmt: skip
    if args.machine:
        out["settings"]["machine"] = args.machine
    engine = None
    if args.what == "device":
        from pyani_plus_amd.engine import HipEngine

        engine = HipEngine(0)
        info = engine.device_info()
        out["settings"].update(device=info["name"], compute_units=info["compute_units"])
    try:
        for n in args.points:
            big = n > 10**7
            for kind in args.kinds:
                x, y = points(kind, n)
                if engine is not None:
                    d_x, d_y = engine.torch.from_numpy(x).to(engine.device), engine.torch.from_numpy(y).to(engine.device)
                    engine.sync()
                for bins in args.grids:
                    xedges, yedges = edges_for(kind, bins)
                    row: dict = {"points": n, "grid": bins, "kind": kind}
                    twin = scatter.bin2d_host(x, y, xedges, yedges)
                    row["counted"] = int(twin[0].sum())
                    row["cells_hit"] = int((twin[0] > 0).sum())
                    if engine is not None:
                        row["device_s"], got = device_timed(engine, lambda: engine.bin2d(d_x, d_y, xedges, yedges), args.repeat, args.warmup)  # noqa: B023
                        assert np.array_equal(got[0], twin[0]) and np.array_equal(got[1], twin[1]), f"device and host twin differ: {row}"
                        row["same_as_host"] = True
                        row["device_gb_per_s"] = 16 * n / row["device_s"]["best"] / 1e9
                    else:
                        row["host_twin_s"], _ = host_timed(lambda: scatter.bin2d_host(x, y, xedges, yedges), 1 if big else args.repeat, 0 if big else 1)  # noqa: B023
                        valid = ~(np.isnan(x) | np.isnan(y))
                        vx, vy = (x, y) if valid.all() else (x[valid], y[valid])
                        row["numpy_histogram2d_s"], (counts, _xe, _ye) = host_timed(lambda: np.histogram2d(vx, vy, bins=(xedges, yedges)), 1 if big else args.repeat, 0 if big else 1)  # noqa: B023
                        assert np.array_equal(counts, twin[0]), f"numpy and host twin differ: {row}"
                        del valid, vx, vy, counts
                    out["cases"][f"{kind}-{n}-{bins}"] = row
                    print(json.dumps(row), flush=True)
                if engine is not None:
                    del d_x, d_y
                del x, y
        if args.command_size:
            out["command"] = command_times(args.command_size, engine)
            print(json.dumps(out["command"]), flush=True)
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
