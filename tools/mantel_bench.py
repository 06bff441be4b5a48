#!/usr/bin/env python3
"""Time mantel-run-comp's cross sums on clustered synthetic distance pairs and keep the numbers in
profiles/mantel/mantel_bench.json.

    python tools/mantel_bench.py --size 1000 --permutations 9999                            # on the GPU machine
    python tools/mantel_bench.py --size 10000 --permutations 999 --numpy-permutations 10

Per size, X = ``clustered_distances(n, seed)`` (tools/pcoa_bench.py: genomes in 20 groups, distances of the size 1 - ANI
takes) and Y = the same groups seen with other noise, the permutations those of seed 1:

* ``device_s``: one ``HipEngine.mantel`` -- the host check of the permutations and their inverses, the uploads of every
  batch, the check of the matrices, the moments, the cross and chain kernels of every batch and the read-back -- with the
  matrices resident on the device, between two device events on the context's stream; best of ``--repeat`` after one
  warm-up.  ``device_terms_per_s`` is (permutations + 1) n (n - 1) / 2 products over that time.
* ``twin_s``: ``pa_mantel_host`` of the same call on 16 threads, host clock; best of ``--repeat`` up to 2000 genomes, run
  once above.  ``same_bits``: the device's stats and cross sums against the twin's, bit for bit.
* ``numpy_s``: the plain loop ``X[iu] @ Y[p][:, p][iu]`` on the same host, host clock, over ``--numpy-permutations``
  permutations (default: all of them) and scaled to the full count; ``numpy_extrapolated_from`` says from how many.
  ``numpy_max_difference`` compares its centred cross sums with the twin's over the permutations it ran.

A size fills its own entry of the output file and leaves the others as they are.
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
sys.path.insert(0, str(ROOT / "tools"))

from pcoa_bench import clustered_distances, timed  # noqa: E402

from pyani_plus_amd.engine import mantel_host, mantel_permutations  # noqa: E402

SEED = 3
PERMUTATION_SEED = 1
HOST_THREADS = 16


def distance_pair(n: int) -> tuple[np.ndarray, np.ndarray]:
    """Two runs of the same genomes: the same groups, independent noise."""
    X = clustered_distances(n, SEED)
    rng = np.random.default_rng(SEED + 1)
    Y = X.copy()
    for i0 in range(0, n, 1000):
        Y[i0 : i0 + 1000] += rng.uniform(0.0, 0.008, size=(min(1000, n - i0), n))
    Y = np.triu(Y, 1)
    return X, Y + Y.T


def main() -> int:
    parser = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    parser.add_argument("--size", type=int, required=True)
    parser.add_argument("--permutations", type=int, required=True)
    parser.add_argument("--numpy-permutations", type=int, default=None)
    parser.add_argument("--repeat", type=int, default=5)
    parser.add_argument("--out", type=Path, default=ROOT / "profiles" / "mantel" / "mantel_bench.json")
    args = parser.parse_args()
    from pyani_plus_amd.engine import HipEngine

    n, count = args.size, args.permutations
    X, Y = distance_pair(n)
    perms = mantel_permutations(PERMUTATION_SEED, n, 0, count)
    terms = (count + 1) * n * (n - 1) // 2
    row: dict = {"permutations": count, "matrix_bytes": n * n * 8, "products": terms}
    print(f"n={n}: matrices ready", flush=True)
    engine = HipEngine(0)
    try:
        t = engine.torch
        d_x, d_y = t.from_numpy(X).to(engine.device), t.from_numpy(Y).to(engine.device)
        timed(engine, lambda: engine.mantel(d_x, d_y, perms))
        runs = [timed(engine, lambda: engine.mantel(d_x, d_y, perms)) for _ in range(args.repeat)]
        info = engine.device_info()
    finally:
        engine.close()
    row["device_runs_s"] = [round(r[0], 6) for r in runs]
    row["device_s"] = min(r[0] for r in runs)
    row["device_terms_per_s"] = terms / row["device_s"]
    got = runs[-1][1]
    print(f"n={n}: device {row['device_s']:.4f} s", flush=True)
    mantel_host(X[:200, :200], Y[:200, :200], perms[:0, :200], HOST_THREADS)  # the pool's threads exist
    row["twin_runs"] = args.repeat if n <= 2000 else 1
    twins = []
    for _ in range(row["twin_runs"]):
        t0 = time.perf_counter()
        want = mantel_host(X, Y, perms, HOST_THREADS)
        twins.append(time.perf_counter() - t0)
    row["twin_s"] = min(twins)
    row["same_bits"] = bool(all(np.array_equal(a.view(np.uint64), b.view(np.uint64)) for a, b in zip(got, want)))
    print(f"n={n}: twin {row['twin_s']:.3f} s, same bits {row['same_bits']}", flush=True)
    ran = count if args.numpy_permutations is None else min(count, args.numpy_permutations)
    iu = np.triu_indices(n, 1)
    t0 = time.perf_counter()
    x = X[iu] - X[iu].mean()
    y_mean = Y[iu].mean()
    sums = np.array([x @ (Y[p][:, p][iu] - y_mean) for p in perms[:ran].astype(np.intp)])
    spent = time.perf_counter() - t0
    row["numpy_s"] = spent * (count / ran) if ran else None
    row["numpy_extrapolated_from"] = None if ran == count else ran
    row["numpy_max_difference"] = float(np.abs(sums - want[1][1 : 1 + ran]).max()) if ran else None
    row["speedup_over_twin"] = row["twin_s"] / row["device_s"]
    row["speedup_over_numpy"] = row["numpy_s"] / row["device_s"] if ran else None
    print(f"n={n}: {row}", flush=True)
    data = json.loads(args.out.read_text()) if args.out.is_file() else {}
    data.setdefault("settings", {}).update(
        generator=f"clustered_distances(n, {SEED}) and the same groups with other noise; permutations of seed {PERMUTATION_SEED}",
        unit=f"seconds; device: best of {args.repeat} after one warm-up, device events around the library call; host legs: host clock",
        host_threads=HOST_THREADS, device=info["name"], compute_units=info["compute_units"])  # fmt: skip
    data.setdefault("sizes", {})[str(n)] = row
    args.out.parent.mkdir(parents=True, exist_ok=True)
    args.out.write_text(json.dumps(data, indent=1) + "\n")
    return 0 if row["same_bits"] else 1


if __name__ == "__main__":
    raise SystemExit(main())
