#!/usr/bin/env python3
"""Time search-run's device walk on synthetic sketches and keep the numbers in profiles/search/search_bench.json.

    python tools/search_bench.py --subjects 10000 --queries 1000 --replaced     # on the GPU machine
    python tools/search_bench.py --subjects 10000 --queries 10000
    python tools/search_bench.py --subjects 100000 --queries 10000

The sketches are ``synth.synth_sketches_torch`` (about 5 000 hashes each, 40 species, made on the device: no genome is
hashed), the queries first and the subjects after them in one CSR, resident on the device, as ``search.search`` lays
them out.  One walk is what ``search.search`` does: per tile of 2 048 subjects one ``pair_counts`` of all queries
against it and one accumulating ``best_hits_device`` (rank identity, ``--top`` 5), then the copy of the three M x top
arrays to the host.

* ``pair_counts_s``, ``best_hits_s``: the sums over a walk's tiles of the time between two device events around each
  call; ``copy_s``: the final copy, between two events; ``walk_s``: a whole walk between two events, no event inside.
  Each the best of ``--repeat`` walks after one warm-up walk; the runs are kept beside the best.
* ``--replaced`` (run once, host clock unless said otherwise): what ``pa_best_hits`` replaces, in the same process on
  the same sketches -- ``counts_d2h_s`` the copy of the M x N counts to the host (a tile at a time, as they are made;
  the time of the copies alone), ``ani_host_s`` ``engine.ani_host`` on them with 16 threads, ``argpartition_s``
  ``numpy.argpartition`` of the identities for the top -- and ``same_hits``: the device's lists against
  ``best_hits_host`` on the copied counts.

A pair of sizes fills its own entry of the output file and leaves the others as they are.
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

from pcoa_bench import timed  # noqa: E402

from pyani_plus_amd.engine import ani_host, best_hits_host  # noqa: E402
from pyani_plus_amd.methods.sourmash_hip import DEVICE_TILE_COLUMNS  # noqa: E402
from pyani_plus_amd.synth import synth_sketches_torch  # noqa: E402

K, HOST_THREADS, RANK = 31, 16, "identity"


def main() -> int:  # noqa: PLR0915
    parser = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    parser.add_argument("--subjects", type=int, required=True)
    parser.add_argument("--queries", type=int, required=True)
    parser.add_argument("--top", type=int, default=5)
    parser.add_argument("--repeat", type=int, default=5)
    parser.add_argument("--replaced", action="store_true", help="also time, once, what pa_best_hits replaces")
    parser.add_argument("--out", type=Path, default=ROOT / "profiles" / "search" / "search_bench.json")
    args = parser.parse_args()
    from pyani_plus_amd.engine import HipEngine

    n, m, top = args.subjects, args.queries, args.top
    engine = HipEngine(0)
    try:
        t = engine.torch
        sketches = synth_sketches_torch(engine, m + n)
        sizes = sketches.sizes()
        d_sizes = t.from_numpy(sizes.astype(np.uint32).view(np.int32)).to(engine.device)
        d_q, d_s = d_sizes[:m], d_sizes[m:]
        tiles = [(s0, min(s0 + DEVICE_TILE_COLUMNS, n)) for s0 in range(0, n, DEVICE_TILE_COLUMNS)]
        print(f"N={n} M={m}: {sketches.total} hashes on the device, {len(tiles)} tiles", flush=True)

        def walk(clock=None):
            """One walk; ``clock``: the dict that receives the legs' seconds (an event pair around each call)."""
            state = None
            for s0, s1 in tiles:
                if clock is None:
                    state = engine.best_hits_device(engine.pair_counts(sketches, (0, m), (m + s0, m + s1)), d_q, d_s[s0:s1], s0, RANK, top, state)
                    continue
                seconds, counts = timed(engine, lambda: engine.pair_counts(sketches, (0, m), (m + s0, m + s1)))  # noqa: B023
                clock["pair_counts_s"] += seconds
                seconds, state = timed(engine, lambda: engine.best_hits_device(counts, d_q, d_s[s0:s1], s0, RANK, top, state))  # noqa: B023
                clock["best_hits_s"] += seconds
            if clock is None:
                return [x.cpu() for x in state]
            clock["copy_s"], host = timed(engine, lambda: [x.cpu() for x in state])
            return host

        lists = [x.numpy().view(np.uint32) for x in walk()]  # the warm-up
        runs: dict = {"pair_counts_s": [], "best_hits_s": [], "copy_s": [], "walk_s": []}
        for _ in range(args.repeat):
            clock = {"pair_counts_s": 0.0, "best_hits_s": 0.0, "copy_s": 0.0}
            walk(clock)
            for name, seconds in clock.items():
                runs[name].append(seconds)
            runs["walk_s"].append(timed(engine, walk)[0])
        row: dict = {"subjects": n, "queries": m, "top": top, "rank": RANK, "tiles": len(tiles), "hashes": int(sketches.total),
                     "counts_bytes": m * n * 4, "lists_bytes": 3 * m * top * 4,
                     "queries_with_a_full_list": int((lists[0][:, top - 1] != 0xFFFFFFFF).sum())}  # fmt: skip
        for name, values in runs.items():
            row[name] = min(values)
            row[name.replace("_s", "_runs_s")] = [round(v, 6) for v in values]
        print(f"N={n} M={m}: walk {row['walk_s']:.4f} s (pair_counts {row['pair_counts_s']:.4f}, best_hits {row['best_hits_s']:.4f}, copy {row['copy_s']:.6f})",
              flush=True)
        if args.replaced:
            counts = np.empty((m, n), dtype=np.uint32)
            d2h = 0.0
            for s0, s1 in tiles:
                tile = engine.pair_counts(sketches, (0, m), (m + s0, m + s1))
                engine.sync()
                t0 = time.perf_counter()
                counts[:, s0:s1] = tile.cpu().numpy().view(np.uint32)
                d2h += time.perf_counter() - t0
            ani_host(counts[:64], sizes[:64], sizes[m:], K, threads=HOST_THREADS)  # the pool's threads exist
            t0 = time.perf_counter()
            identity, _cov, _null = ani_host(counts, sizes[:m], sizes[m:], K, threads=HOST_THREADS)
            t1 = time.perf_counter()
            picked = np.argpartition(-np.nan_to_num(identity, nan=-1.0), top - 1, axis=1)[:, :top]
            t2 = time.perf_counter()
            twin = best_hits_host(counts, sizes[:m], sizes[m:], 0, RANK, top, threads=HOST_THREADS)
            t3 = time.perf_counter()
            row["replaced"] = {"runs": 1, "counts_d2h_s": d2h, "ani_host_s": t1 - t0, "ani_host_threads": HOST_THREADS, "argpartition_s": t2 - t1,
                               "best_hits_host_s": t3 - t2, "same_hits": bool(all(np.array_equal(a, b) for a, b in zip(lists, twin))),
                               "argpartition_picks": int(picked.size)}  # fmt: skip
            print(f"N={n} M={m}: replaced: d2h {d2h:.4f} s, ani_host {t1 - t0:.4f} s, argpartition {t2 - t1:.4f} s; same hits {row['replaced']['same_hits']}",
                  flush=True)
        info = engine.device_info()
    finally:
        engine.close()
    data = json.loads(args.out.read_text()) if args.out.is_file() else {}
    data.setdefault("settings", {}).update(
        generator="synth.synth_sketches_torch: 4 500 to 5 500 hashes a sketch, 40 species, queries first; k = 31",
        unit=f"seconds; device legs: best of {args.repeat} walks after one warm-up walk, device events around the calls; replaced legs: host clock, run once",
        device=info["name"], compute_units=info["compute_units"])  # fmt: skip
    data.setdefault("sizes", {})[f"{n}x{m}"] = row
    args.out.parent.mkdir(parents=True, exist_ok=True)
    args.out.write_text(json.dumps(data, indent=1) + "\n")
    return 0 if row.get("replaced", {}).get("same_hits", True) else 1


if __name__ == "__main__":
    raise SystemExit(main())
