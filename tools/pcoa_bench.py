#!/usr/bin/env python3
"""Time ordinate-run's tall product and eigen-solver on clustered synthetic matrices and keep the numbers in
profiles/pcoa/pcoa_bench.json.

    python tools/pcoa_bench.py device --sizes 1000 10000     # on the GPU machine
    python tools/pcoa_bench.py host --sizes 1000 10000       # the host twins alone, without a GPU
    python tools/pcoa_bench.py eigh --sizes 1000 10000       # numpy.linalg.eigh of the same matrices: what the feature replaces

Per size, on ``clustered_distances(n, seed)`` (genomes in 20 groups whose centres lie in three dimensions, distances of
the size 1 - ANI takes, symmetric noise), centred by ``pa_gower_center_host``, with k = 3 axes and so a block of p = 11
columns:

``device``, the centred matrix resident on the device
* ``product_s``: one ``pa_mul_tall_f64`` (its two launches) between two device events on the context's stream; best of
  ``--repeat`` after one warm-up.  ``product_bytes_per_s`` is n^2 * 8 B over that time: what one pass over the matrix
  moves, not counting the block and the partial sums.  ``fraction_of_hbm`` is that rate over the 6.3 TB/s a streaming
  kernel achieves on an MI355X; ``resident`` says where the matrix was while the product was timed.
* ``centre_s``: ``pa_gower_center`` alone, the same way (the distances resident too).
* ``solve_s``: the whole ``pa_symm_top_eigs`` -- every iteration's upload of Q, product, download of Y and the host
  algebra between -- between two device events (the second recorded when the call returns); ``iterations`` from its
  info.  ``share_outside_product`` is 1 - iterations * product_s / solve_s: the host algebra and the transfers.
* ``same_bits_as_host``: values, vectors, residuals and info against the twin (with ``--no-host`` it is not checked).

``host``
* ``host_product_s`` and ``host_solve_s``: ``pa_mul_tall_f64_host`` and ``pa_symm_top_eigs_host`` on 16 threads, host
  clock, best of ``--repeat`` up to 2000 genomes and run once above.

``eigh``
* ``eigh_s``: ``numpy.linalg.eigh`` of the centred matrix, host clock, run once; ``eigh_threads`` is what the BLAS was
  allowed.  ``max_eigenvalue_difference`` compares its top three with the host twin's.

Each form fills its own section of the output file and leaves the others as they are.
"""

from __future__ import annotations

import argparse
import json
import os
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

from pyani_plus_amd.engine import gower_center_host, mul_tall_host, symm_top_eigs_host  # noqa: E402

SEED = 3
HOST_THREADS = 16
AXES = 3
HBM_ACHIEVABLE = 6.3e12  # bytes per second of a streaming kernel on an MI355X
INFINITY_CACHE = 256 << 20


def clustered_distances(n: int, seed: int, clusters: int = 20) -> np.ndarray:
    rng = np.random.default_rng(seed)
    spread = rng.standard_normal((clusters, 3))
    centres = np.linalg.qr(spread - spread.mean(axis=0))[0] * np.array([0.30, 0.22, 0.15])
    diff = centres[:, None, :] - centres[None, :, :]
    between = np.sqrt((diff * diff).sum(axis=2))
    between = np.triu(between, 1)
    between = between + between.T
    member = np.arange(n) % clusters
    D = between[np.ix_(member, member)] + 0.01
    for i0 in range(0, n, 1000):  # the noise a block of rows at a time: no second n x n temporary
        D[i0 : i0 + 1000] += rng.uniform(-0.004, 0.004, size=(min(1000, n - i0), n))
    D = np.triu(D, 1)
    D = D + D.T
    return D


def block_width(n: int, k: int) -> int:
    return min(n, max(2 * k, k + 8), 32)


def timed(engine, call):
    t = engine.torch
    start, end = t.cuda.Event(enable_timing=True), t.cuda.Event(enable_timing=True)
    engine.sync()
    start.record()
    out = call()
    end.record()
    end.synchronize()
    return start.elapsed_time(end) / 1e3, out


def device_times(engine, D: np.ndarray, B: np.ndarray, fro2: float, repeat: int, row: dict):
    t = engine.torch
    n = len(B)
    p = block_width(n, AXES)
    d_d = t.from_numpy(D).to(engine.device)
    timed(engine, lambda: engine.gower_center_device(d_d))
    row["centre_s"] = min(timed(engine, lambda: engine.gower_center_device(d_d))[0] for _ in range(repeat))
    del d_d
    d_b = t.from_numpy(B).to(engine.device)
    d_q = t.from_numpy(np.random.default_rng(1).uniform(-1.0, 1.0, size=(n, p))).to(engine.device)
    timed(engine, lambda: engine.mul_tall_device(d_b, d_q))
    runs = [timed(engine, lambda: engine.mul_tall_device(d_b, d_q))[0] for _ in range(repeat)]
    row["product_s"] = min(runs)
    row["product_runs_s"] = [round(x, 7) for x in runs]
    row["product_bytes_per_s"] = n * n * 8 / row["product_s"]
    row["fraction_of_hbm"] = row["product_bytes_per_s"] / HBM_ACHIEVABLE
    row["resident"] = (
        f"the {n * n * 8 >> 20} MB matrix had been read by the warm-up and fits the 256 MB Infinity Cache: not streamed from HBM"
        if n * n * 8 <= INFINITY_CACHE
        else f"the {n * n * 8 >> 20} MB matrix exceeds the 256 MB Infinity Cache: every product streams it from HBM"
    )
    timed(engine, lambda: engine.symm_top_eigs(d_b, AXES, fro2))
    solves = [timed(engine, lambda: engine.symm_top_eigs(d_b, AXES, fro2)) for _ in range(repeat)]
    row["solve_s"] = min(s[0] for s in solves)
    got = solves[-1][1]
    row["iterations"], row["phase1_iterations"], row["shift"] = got[3][1], got[3][0], got[3][2]
    row["share_outside_product"] = 1.0 - row["iterations"] * row["product_s"] / row["solve_s"]
    return got


def same_solves(a, b) -> bool:
    return all(np.array_equal(x.view(np.uint64), y.view(np.uint64)) for x, y in zip(a[:3], b[:3])) and a[3] == b[3]


def main() -> int:
    parser = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    parser.add_argument("what", choices=("device", "host", "eigh"))
    parser.add_argument("--sizes", type=int, nargs="+", default=[1000, 10000])
    parser.add_argument("--repeat", type=int, default=5)
    parser.add_argument("--no-host", action="store_true", help="device times only: the solve is not compared with the twin")
    parser.add_argument("--out", type=Path, default=ROOT / "profiles" / "pcoa" / "pcoa_bench.json")
    args = parser.parse_args()
    out = {
        "settings": {"generator": f"clustered_distances(n, {SEED})", "axes": AXES,
                     "unit": f"seconds; best of {args.repeat} after one warm-up unless a row says otherwise", "host_threads": HOST_THREADS,
                     "device_timer": "device events around the library call", "host_timer": "host clock"},
        "sizes": {},
    }  # fmt: skip
    engine = None
    if args.what == "device":
        from pyani_plus_amd.engine import HipEngine

        engine = HipEngine(0)
        info = engine.device_info()
        out["settings"].update(device=info["name"], compute_units=info["compute_units"], hbm_achievable_bytes_per_s=HBM_ACHIEVABLE)
    if args.what == "eigh":
        out["settings"]["eigh_threads"] = os.environ.get("OMP_NUM_THREADS", "not set")
    try:
        for n in args.sizes:
            D = clustered_distances(n, SEED)
            B, _trace, fro2 = gower_center_host(D, HOST_THREADS)
            row: dict = {"block_columns": block_width(n, AXES), "matrix_bytes": n * n * 8}
            print(f"n={n}: matrix ready", flush=True)
            if args.what == "device":
                got = device_times(engine, D, B, fro2, args.repeat, row)
                if not args.no_host:
                    assert same_solves(got, symm_top_eigs_host(B, AXES, fro2, threads=HOST_THREADS)), "device and host solves differ"
                    row["same_bits_as_host"] = True
            elif args.what == "host":
                row["host_runs"] = args.repeat if n <= 2000 else 1
                Q = np.random.default_rng(1).uniform(-1.0, 1.0, size=(n, row["block_columns"]))
                mul_tall_host(B[:200, :200], Q[:200], HOST_THREADS)  # the pool's threads exist
                products, solves = [], []
                for _ in range(row["host_runs"]):
                    t0 = time.perf_counter()
                    mul_tall_host(B, Q, HOST_THREADS)
                    products.append(time.perf_counter() - t0)
                    t0 = time.perf_counter()
                    got = symm_top_eigs_host(B, AXES, fro2, threads=HOST_THREADS)
                    solves.append(time.perf_counter() - t0)
                row.update(host_product_s=min(products), host_solve_s=min(solves), iterations=got[3][1])
            else:
                t0 = time.perf_counter()
                values = np.linalg.eigh(B)[0]
                row["eigh_s"] = time.perf_counter() - t0
                ours = symm_top_eigs_host(B, AXES, fro2, threads=HOST_THREADS)[0]
                row["max_eigenvalue_difference"] = float(np.abs(values[::-1][:AXES] - ours).max())
            out["sizes"][str(n)] = row
            print(f"n={n}: {row}", flush=True)
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
