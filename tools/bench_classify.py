#!/usr/bin/env python3
"""Time classify on generated matrices (two species, cov_min 0.1: the graph is complete) and keep the numbers in
profiles/classify/classify_bench.json.

    python tools/bench_classify.py reference --reference-path DIR --sizes 200 400   # the reference's functions, CPU
    python tools/bench_classify.py host --sizes 200 400 1000 4000                   # this project without a GPU
    python tools/bench_classify.py device --sizes 200 400 1000 4000 10000           # this project on the GPU

Each form fills its own section of the output file and leaves the others as they are.  The device form splits a run
into upload of the two matrices ("load"), edge build and edge sort (the library's event timers), copy back, clique
pass and TSV, and times numpy's stable argsort of the same scores beside the sort stage.  Times are the median of
``--repeat`` runs after one warm-up, in seconds.
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

from pyani_plus_amd import classify as cl  # noqa: E402
from pyani_plus_amd.synth import synth_classify_matrices  # noqa: E402

COV_MIN = 0.1
SEED = 31


def matrices(n: int):
    return synth_classify_matrices(n, SEED, groups=2)


def median_of(fn, repeat: int) -> tuple[float, object]:
    times, out = [], None
    for _ in range(repeat):
        t0 = time.perf_counter()
        out = fn()
        times.append(time.perf_counter() - t0)
    return statistics.median(times), out


def bench_reference(path: Path, sizes: list[int]) -> dict:
    import contextlib
    import io

    import pandas as pd

    sys.dont_write_bytecode = True
    sys.path.append(str(path))
    import networkx as nx
    from pyani_plus import classify as ref

    out = {}
    for n in sizes:
        labels, ident, cov = matrices(n)
        f_ident, f_cov = pd.DataFrame(ident, index=labels, columns=labels), pd.DataFrame(cov, index=labels, columns=labels)
        t0 = time.perf_counter()
        graph = ref.construct_graph(f_cov, f_ident, ref.AGG_FUNCS["min"], ref.AGG_FUNCS["mean"], COV_MIN)
        t1 = time.perf_counter()
        initial = ref.find_initial_cliques(graph) if len(list(nx.connected_components(graph))) != 1 else []
        with contextlib.redirect_stdout(io.StringIO()), contextlib.redirect_stderr(io.StringIO()):
            recursive = ref.find_cliques_recursively(graph)
        unique = ref.get_unique_cliques(initial, recursive)
        t2 = time.perf_counter()
        out[str(n)] = {"construct_graph_s": t1 - t0, "cliques_s": t2 - t1, "total_s": t2 - t0, "rows": len(unique), "runs": 1}
        print(f"reference n={n}: {out[str(n)]}", flush=True)
    return out


def finish(labels, edges, repeat: int) -> dict:
    t_cliques, rows = median_of(lambda: cl.cliques_from_edges(labels, *edges), repeat)
    t_tsv, text = median_of(lambda: cl.classify_tsv(rows), repeat)
    return {"clique_pass_s": t_cliques, "tsv_s": t_tsv, "rows": len(rows), "tsv_bytes": len(text)}


def bench_host(sizes: list[int], repeat: int) -> dict:
    out = {}
    for n in sizes:
        labels, ident, cov = matrices(n)
        t_edges, edges = median_of(lambda: cl.edges_host(ident, cov, cov_min=COV_MIN), repeat)
        row = {"edges": len(edges[0]), "edges_host_s": t_edges, **finish(labels, edges, repeat)}
        row["total_s"] = row["edges_host_s"] + row["clique_pass_s"] + row["tsv_s"]
        out[str(n)] = row
        print(f"host n={n}: {row}", flush=True)
    return out


def bench_device(sizes: list[int], repeat: int) -> dict:
    from pyani_plus_amd.engine import HipEngine

    engine = HipEngine(0)
    t = engine.torch
    out = {"device": engine.device_info()["name"]}
    try:
        for n in sizes:
            labels, ident, cov = matrices(n)
            h_ident, h_cov = t.from_numpy(ident), t.from_numpy(cov)

            def upload():
                d = h_ident.to(engine.device), h_cov.to(engine.device)
                engine.sync()
                return d

            engine.classify_edges_device(*upload(), cov_min=COV_MIN)  # warm-up: the workspaces grow once
            t_load, (d_ident, d_cov) = median_of(upload, repeat)
            build, sort, wall, back = [], [], [], []
            edges = None
            for _ in range(repeat):
                engine.prof_reset()
                engine.prof_enable(True)
                t0 = time.perf_counter()
                d_edges = engine.classify_edges_device(d_ident, d_cov, cov_min=COV_MIN)
                engine.sync()
                t1 = time.perf_counter()
                prof = engine.prof_get()
                engine.prof_enable(False)
                t2 = time.perf_counter()
                edges = tuple(x.cpu().numpy() for x in d_edges)
                t3 = time.perf_counter()
                build.append(prof["cls_edges"][0] / 1e3)
                sort.append(prof["cls_sort"][0] / 1e3)
                wall.append(t1 - t0)
                back.append(t3 - t2)
                del d_edges
            edges = (edges[0].view(np.uint32), edges[1].view(np.uint32), edges[2], edges[3])
            scores = np.ascontiguousarray(cl.edges_host(ident, cov, cov_min=COV_MIN)[2]) if n <= 1000 else None
            if scores is not None:
                assert np.array_equal(scores, edges[2]), "device and host edge lists differ"
            unsorted = np.random.default_rng(0).permutation(edges[2])
            t_argsort, _ = median_of(lambda: np.argsort(unsorted, kind="stable"), max(1, min(repeat, 3)))
            row = {"edges": len(edges[0]), "load_s": t_load, "edge_build_s": statistics.median(build), "edge_sort_s": statistics.median(sort),
                   "edges_call_wall_s": statistics.median(wall), "copy_back_s": statistics.median(back), **finish(labels, edges, repeat),
                   "numpy_stable_argsort_s": t_argsort}  # fmt: skip
            row["total_s"] = row["load_s"] + row["edges_call_wall_s"] + row["copy_back_s"] + row["clique_pass_s"] + row["tsv_s"]
            out[str(n)] = row
            print(f"device n={n}: {row}", flush=True)
            del d_ident, d_cov
    finally:
        engine.close()
    return out


def main() -> int:
    parser = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    parser.add_argument("what", choices=("reference", "host", "device"))
    parser.add_argument("--sizes", type=int, nargs="+", default=[200, 400])
    parser.add_argument("--repeat", type=int, default=3)
    parser.add_argument("--reference-path", type=Path, default=None)
    parser.add_argument("--out", type=Path, default=ROOT / "profiles" / "classify" / "classify_bench.json")
    args = parser.parse_args()
    if args.what == "reference":
        if args.reference_path is None:
            parser.error("--reference-path is needed")
        section = bench_reference(args.reference_path, args.sizes)
    elif args.what == "host":
        section = bench_host(args.sizes, args.repeat)
    else:
        section = bench_device(args.sizes, args.repeat)
    data = json.loads(args.out.read_text()) if args.out.is_file() else {}
    data.setdefault("settings", {"generator": "synth_classify_matrices(n, 31, groups=2)", "cov_min": COV_MIN, "coverage_edges": "min",
                                 "score_edges": "mean", "unit": "seconds, median of the runs"})
    data[args.what] = section
    args.out.parent.mkdir(parents=True, exist_ok=True)
    args.out.write_text(json.dumps(data, indent=1) + "\n")
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
