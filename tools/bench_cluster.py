#!/usr/bin/env python3
"""Time plot-run's clustering on generated matrices and keep the numbers in profiles/cluster/cluster_bench.json.

    python tools/bench_cluster.py device --sizes 1000 4000 10000     # on the GPU machine: every column, and the gate
    python tools/bench_cluster.py host --sizes 1000 2000 4000        # without a GPU: host twin, linkage, scipy

Each form fills its own section of the output file and leaves the other as it is.  Per size, on the identity matrix of ``synth_classify_matrices(n, 31)``: upload of the matrix, the row-distance kernel
(the library's event timer), copy back of the condensed vector, the three together as one wall time, the host twin on
16 threads, the host linkage (both once only above 4000 rows, ``host_runs``), and ``scipy.spatial.distance.pdist`` where scipy is importable (recorded as absent
otherwise; skipped above ``--scipy-max`` rows, where one run takes minutes).  Every time is the best of ``--repeat``
runs after one warm-up, in seconds, and is named so in the file.  The device and host vectors are compared bit for bit.

The gate of DESIGN.md section 7c is read from this file: at n = 4000, ``device_total_s`` against ``host_twin_s``.
"""

from __future__ import annotations

import argparse
import json
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

from pyani_plus_amd import cluster  # noqa: E402
from pyani_plus_amd.synth import synth_classify_matrices  # noqa: E402

SEED = 31
HOST_THREADS = 16


def best_of(fn, repeat: int) -> tuple[float, object]:
    times, out = [], None
    for _ in range(repeat):
        t0 = time.perf_counter()
        out = fn()
        times.append(time.perf_counter() - t0)
    return min(times), out


def device_times(engine, x, repeat: int, row: dict) -> np.ndarray:
    """Upload, kernel (event timer), copy back, and the three as one call, into ``row``; returns the distances."""
    h_x = engine.torch.from_numpy(x)

    def upload():
        d = h_x.to(engine.device)
        engine.sync()
        return d

    def whole():
        return engine.row_distances(x)

    whole()  # warm-up
    row["upload_s"], d_x = best_of(upload, repeat)
    kernel, back = [], []
    for _ in range(repeat):
        engine.prof_reset()
        engine.prof_enable(True)
        d_d = engine.row_distances_device(d_x)
        engine.sync()
        kernel.append(engine.prof_get()["rowdist"][0] / 1e3)
        engine.prof_enable(False)
        t0 = time.perf_counter()
        d_d.cpu().numpy()
        back.append(time.perf_counter() - t0)
        del d_d
    row["kernel_s"], row["copy_back_s"] = min(kernel), min(back)
    row["device_total_s"], got = best_of(whole, repeat)
    return got


def main() -> int:
    parser = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    parser.add_argument("what", choices=("device", "host"))
    parser.add_argument("--sizes", type=int, nargs="+", default=[1000, 4000, 10000])
    parser.add_argument("--repeat", type=int, default=3)
    parser.add_argument("--scipy-max", type=int, default=4000)
    parser.add_argument("--no-host", action="store_true", help="device times only (for a profiler run)")
    parser.add_argument("--out", type=Path, default=ROOT / "profiles" / "cluster" / "cluster_bench.json")
    args = parser.parse_args()
    try:
        from scipy.spatial.distance import pdist
    except ImportError:
        pdist = None
    engine = None
    out = {
        "settings": {
            "generator": f"identity matrix of synth_classify_matrices(n, {SEED})", "unit": f"seconds, best of {args.repeat} after one warm-up",
            "host_threads": HOST_THREADS, "scipy": "absent" if pdist is None else __import__("scipy").__version__,
        },
        "sizes": {},
    }  # fmt: skip
    if args.what == "device":
        from pyani_plus_amd.engine import HipEngine

        engine = HipEngine(0)
        info = engine.device_info()
        out["settings"].update(device=info["name"], compute_units=info["compute_units"])
    try:
        for n in args.sizes:
            _labels, x, _cov = synth_classify_matrices(n, SEED)
            row = {"pairs": n * (n - 1) // 2, "steps": n * (n - 1) // 2 * n}
            got = None
            if engine is not None:
                got = device_times(engine, x, args.repeat, row)
            if not args.no_host:
                cluster.row_distances(x[: min(n, 500)], threads=HOST_THREADS)  # the pool's threads exist
                row["host_runs"] = args.repeat if n <= 4000 else 1  # one run of the largest takes most of a minute
                row["host_twin_s"], want = best_of(lambda: cluster.row_distances(x, threads=HOST_THREADS), row["host_runs"])
                if got is None:
                    got = want
                else:
                    assert np.array_equal(got.view(np.uint64), want.view(np.uint64)), "device and host distances differ"
                    row["same_bits_as_host"] = True
                row["host_linkage_s"], _tree = best_of(lambda: cluster.linkage_average(want, n), row["host_runs"])
                if pdist is None:
                    row["scipy_pdist_s"] = "absent"
                elif n > args.scipy_max:
                    row["scipy_pdist_s"] = f"not run above n = {args.scipy_max}"
                else:
                    row["scipy_pdist_s"], ref = best_of(lambda: pdist(x, "euclidean"), 1)
                    row["scipy_pdist_runs"] = 1
                    assert np.array_equal(got.view(np.uint64), ref.view(np.uint64)), "the distances differ from scipy's"
                    row["same_bits_as_scipy"] = True
            out["sizes"][str(n)] = row
            print(f"n={n}: {row}", flush=True)
        gate = out["sizes"].get("4000")
        if gate and "host_twin_s" in gate and "device_total_s" in gate:
            out["gate"] = {"n": 4000, "device_total_s": gate["device_total_s"], "host_twin_s": gate["host_twin_s"],
                           "passed": gate["device_total_s"] < gate["host_twin_s"], "what": f"best of {args.repeat}; device = upload + kernel + copy back as one call"}  # fmt: skip
            print(f"gate: {out['gate']}", flush=True)
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
