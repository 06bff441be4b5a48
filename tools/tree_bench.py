#!/usr/bin/env python3
"""Time tree-run's neighbour joining on random additive matrices and keep the numbers in profiles/tree/tree_bench.json.

    python tools/tree_bench.py device --sizes 1000 10000     # on the GPU machine
    python tools/tree_bench.py host --sizes 1000 10000       # the host twin alone, without a GPU

Per size, on ``additive_matrix(n, seed)`` (a random rooted binary tree over n leaves, every branch a multiple of 2^-10,
so the distances are exact):

* ``device_s``: ``pa_nj`` alone -- the check, the row sums, the 3 (n - 2) launches of the joins and the two read-backs --
  between two device events on the context's stream, the matrix already on the device (the call overwrites it, so each
  run gets a fresh copy made before the first event); best of ``--repeat`` after one warm-up;
* ``upload_s``: the host matrix to the device, host clock around a synchronised copy, best of ``--repeat``;
* ``share_scan``, ``share_join``, ``share_update``: the three per-join kernels' shares of their summed event time, from
  one further run with the library's event timer on, which times every stride-th join (at most 512 of them);
* ``host_twin_s``: ``pa_nj_host`` on 16 threads, host clock; best of ``--repeat`` up to 2000 leaves, run once above;
* ``same_bits_as_host``: the device's join table against the twin's, bit for bit.

``pairs`` is the number of pair scores the joins need, the sum of m (m - 1) / 2 for m = n .. 3, and ``scan_bytes`` eight
times that: what the scans read.  ``device_pairs_per_s`` is pairs over ``device_s``, a whole-call rate, not a kernel's.
Each form fills its own section of the output file and leaves the other as it is.
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

from pyani_plus_amd.engine import nj_tree_host  # noqa: E402

SEED = 17
HOST_THREADS = 16


def additive_matrix(n: int, seed: int) -> np.ndarray:
    """Leaf distances of a random rooted binary tree: the leaves of a node are a range of indices, split at a random
    point; d(i, j) = depth[i] + depth[j] - 2 depth[their last common node], depths sums of multiples of 2^-10 in (0, 1]."""
    rng = np.random.default_rng(seed)
    D = np.zeros((n, n), dtype=np.float64)
    leaf_depth = np.zeros(n)
    inner: list[tuple[int, int, int, float]] = []  # (lo, mid, hi, depth of the node)
    stack = [(0, n, 0.0)]
    while stack:
        lo, hi, depth = stack.pop()
        if hi - lo == 1:
            leaf_depth[lo] = depth
            continue
        mid = int(rng.integers(lo + 1, hi))
        inner.append((lo, mid, hi, depth))
        for a, b in ((lo, mid), (mid, hi)):
            stack.append((a, b, depth + int(rng.integers(1, 1025)) / 1024.0))
    for lo, mid, hi, depth in inner:
        block = (leaf_depth[lo:mid, None] + leaf_depth[None, mid:hi]) - 2.0 * depth
        D[lo:mid, mid:hi] = block
        D[mid:hi, lo:mid] = block.T
    return D


def pair_scores(n: int) -> int:
    return sum(m * (m - 1) // 2 for m in range(3, n + 1))


def same_tables(a, b) -> bool:
    return (np.array_equal(a[0], b[0]) and np.array_equal(a[1].view(np.uint64), b[1].view(np.uint64)) and np.array_equal(a[2], b[2])
            and np.float64(a[3]).view(np.uint64) == np.float64(b[3]).view(np.uint64))  # fmt: skip


def device_times(engine, D: np.ndarray, repeat: int, row: dict):
    t = engine.torch
    h = t.from_numpy(D)
    uploads = []
    for _ in range(repeat):
        t0 = time.perf_counter()
        d = h.to(engine.device)
        engine.sync()
        uploads.append(time.perf_counter() - t0)
    row["upload_s"] = min(uploads)
    n = len(D)
    from pyani_plus_amd.engine import _nj_outputs

    def one_call():
        work = d.clone()
        out = _nj_outputs(n)
        start, end = t.cuda.Event(enable_timing=True), t.cuda.Event(enable_timing=True)
        engine.sync()
        start.record()
        engine._check(engine.lib.pa_nj(engine.ctx, work.data_ptr(), n, *(a.ctypes.data for a in out)), "pa_nj")  # noqa: SLF001
        end.record()
        end.synchronize()
        return start.elapsed_time(end) / 1e3, (out[0], out[1], out[2], float(out[3][0]))

    one_call()  # warm-up
    runs = [one_call() for _ in range(repeat)]
    row["device_s"] = min(r[0] for r in runs)
    row["device_runs_s"] = [round(r[0], 6) for r in runs]
    row["device_pairs_per_s"] = row["pairs"] / row["device_s"]
    engine.prof_reset()
    engine.prof_enable(True)
    try:
        one_call()
        prof = engine.prof_get()
    finally:
        engine.prof_enable(False)
    phases = {k: prof[f"nj_{k}"][0] for k in ("scan", "join", "update")}
    total = sum(phases.values())
    row["timed_joins"] = prof["nj_scan"][1]
    for k, ms in phases.items():
        row[f"share_{k}"] = ms / total if total else None
    return runs[-1][1]


def main() -> int:
    parser = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    parser.add_argument("what", choices=("device", "host"))
    parser.add_argument("--sizes", type=int, nargs="+", default=[1000, 10000])
    parser.add_argument("--repeat", type=int, default=5)
    parser.add_argument("--no-host", action="store_true", help="device times only")
    parser.add_argument("--out", type=Path, default=ROOT / "profiles" / "tree" / "tree_bench.json")
    args = parser.parse_args()
    out = {
        "settings": {"generator": f"additive_matrix(n, {SEED})", "unit": f"seconds; best of {args.repeat} after one warm-up unless a row says otherwise",
                     "host_threads": HOST_THREADS, "device_timer": "device events around pa_nj", "host_timer": "host clock"},
        "sizes": {},
    }  # fmt: skip
    engine = None
    if args.what == "device":
        from pyani_plus_amd.engine import HipEngine

        engine = HipEngine(0)
        info = engine.device_info()
        out["settings"].update(device=info["name"], compute_units=info["compute_units"])
    try:
        for n in args.sizes:
            D = additive_matrix(n, SEED)
            row = {"joins": n - 2, "launches": 3 * (n - 2) + 3, "pairs": pair_scores(n), "scan_bytes": 8 * pair_scores(n)}
            got = device_times(engine, D, args.repeat, row) if engine is not None else None
            if not args.no_host:
                nj_tree_host(D[:200, :200], HOST_THREADS)  # the pool's threads exist
                row["host_runs"] = args.repeat if n <= 2000 else 1
                times = []
                for _ in range(row["host_runs"]):
                    t0 = time.perf_counter()
                    want = nj_tree_host(D, HOST_THREADS)
                    times.append(time.perf_counter() - t0)
                row["host_twin_s"] = min(times)
                if got is not None:
                    assert same_tables(got, want), "device and host join tables differ"
                    row["same_bits_as_host"] = True
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
