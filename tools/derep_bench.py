#!/usr/bin/env python3
"""Time dereplicate-run's three calls on clustered synthetic identities and keep the numbers in
profiles/derep/derep_bench.json.

    python tools/derep_bench.py --size 1000        # on the GPU machine
    python tools/derep_bench.py --size 10000

Per size, the scores are ``1 - clustered_distances(n, seed)`` (tools/pcoa_bench.py: genomes in 20 groups, distances of the
size 1 - ANI takes), the coverages all 1, and ``--min-identity`` lies inside the noise of a group, so that a genome is
adjacent to a few members of its group and the graph falls into many small pieces.  Per mode (greedy, cover):

* ``adjacency_s``, ``select_s``, ``assign_s``: ``HipEngine.derep_adjacency_device``, ``derep_select_device`` and
  ``derep_assign_device`` with the matrices (and then the bit matrix) resident on the device, each between two device
  events on the context's stream; ``device_s``: the three in a row between two events.  Best of ``--repeat`` after one
  warm-up.  ``rounds`` and ``representatives`` are what the selection reports.
* ``twin_s``: the three host twins in a row on 16 threads, host clock; best of ``--repeat`` up to 2000 genomes, run once
  above; ``twin_select_s`` is the selection's share (one thread: the sequential rule).  ``same_bits``: the device's
  representatives, assignment and scores against the twin's.

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

from pyani_plus_amd.engine import derep_adjacency_host, derep_assign_host, derep_select_host  # noqa: E402

SEED = 3
HOST_THREADS = 16
MODES = ("greedy", "cover")


def main() -> int:
    parser = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    parser.add_argument("--size", type=int, required=True)
    parser.add_argument("--min-identity", type=float, default=0.9939)
    parser.add_argument("--repeat", type=int, default=5)
    parser.add_argument("--out", type=Path, default=ROOT / "profiles" / "derep" / "derep_bench.json")
    args = parser.parse_args()
    from pyani_plus_amd.engine import HipEngine

    n = args.size
    S = 1.0 - clustered_distances(n, SEED)
    np.fill_diagonal(S, 1.0)
    C = np.ones((n, n))
    options = {"score_edges": "mean", "coverage_edges": "min", "min_score": args.min_identity, "cov_min": 0.5}
    row: dict = {"min_identity": args.min_identity, "matrix_bytes": n * n * 8, "bit_matrix_bytes": n * ((n + 63) // 64) * 8, "modes": {}}
    print(f"n={n}: matrices ready", flush=True)
    engine = HipEngine(0)
    got = {}
    try:
        t = engine.torch
        d_s, d_c = t.from_numpy(S).to(engine.device), t.from_numpy(C).to(engine.device)

        def whole(mode: str):
            bits = engine.derep_adjacency_device(d_s, d_c, **options)
            is_rep, n_reps, rounds = engine.derep_select_device(bits, n, mode)
            rep, score = engine.derep_assign_device(d_s, bits, is_rep, score_edges="mean")
            return bits, is_rep, n_reps, rounds, rep, score

        for mode in MODES:
            bits, is_rep, n_reps, rounds, rep, score = timed(engine, lambda: whole(mode))[1]  # noqa: B023  the warm-up
            legs = {
                "adjacency_s": lambda: engine.derep_adjacency_device(d_s, d_c, **options),
                "select_s": lambda: engine.derep_select_device(bits, n, mode),  # noqa: B023
                "assign_s": lambda: engine.derep_assign_device(d_s, bits, is_rep, score_edges="mean"),  # noqa: B023
                "device_s": lambda: whole(mode),  # noqa: B023
            }
            entry: dict = {"rounds": rounds, "representatives": n_reps}
            for name, call in legs.items():
                runs = [timed(engine, call)[0] for _ in range(args.repeat)]
                entry[name] = min(runs)
                entry[name.replace("_s", "_runs_s")] = [round(r, 6) for r in runs]
            row["modes"][mode] = entry
            got[mode] = (is_rep.cpu().numpy(), rep.cpu().numpy().view(np.uint32), score.cpu().numpy())
            print(f"n={n} {mode}: device {entry['device_s']:.4f} s, {rounds} rounds, {n_reps} representatives", flush=True)
        info = engine.device_info()
    finally:
        engine.close()
    derep_adjacency_host(S[:200, :200], C[:200, :200], threads=HOST_THREADS, **options)  # the pool's threads exist
    twin_runs = args.repeat if n <= 2000 else 1
    ok = True
    for mode in MODES:
        entry = row["modes"][mode]
        entry["twin_runs"] = twin_runs
        totals, selects = [], []
        for _ in range(twin_runs):
            t0 = time.perf_counter()
            h_bits = derep_adjacency_host(S, C, threads=HOST_THREADS, **options)
            t1 = time.perf_counter()
            h_is_rep, _count = derep_select_host(h_bits, n, mode)
            t2 = time.perf_counter()
            h_rep, h_score = derep_assign_host(S, h_bits, h_is_rep, score_edges="mean", threads=HOST_THREADS)
            totals.append(time.perf_counter() - t0)
            selects.append(t2 - t1)
        entry["twin_s"], entry["twin_select_s"] = min(totals), min(selects)
        is_rep, rep, score = got[mode]
        entry["same_bits"] = bool(np.array_equal(is_rep, h_is_rep) and np.array_equal(rep, h_rep) and np.array_equal(score.view(np.uint64), h_score.view(np.uint64)))
        entry["speedup_over_twin"] = entry["twin_s"] / entry["device_s"]
        ok = ok and entry["same_bits"]
        print(f"n={n} {mode}: twin {entry['twin_s']:.3f} s (selection {entry['twin_select_s']:.3f} s), same bits {entry['same_bits']}", flush=True)
    data = json.loads(args.out.read_text()) if args.out.is_file() else {}
    data.setdefault("settings", {}).update(
        generator=f"scores 1 - clustered_distances(n, {SEED}), coverages 1; mean score edges, min coverage edges, cov_min 0.5",
        unit=f"seconds; device: best of {args.repeat} after one warm-up, device events around the calls; host legs: host clock",
        host_threads=HOST_THREADS, device=info["name"], compute_units=info["compute_units"])  # fmt: skip
    data.setdefault("sizes", {})[str(n)] = row
    args.out.parent.mkdir(parents=True, exist_ok=True)
    args.out.write_text(json.dumps(data, indent=1) + "\n")
    return 0 if ok else 1


if __name__ == "__main__":
    raise SystemExit(main())
