#!/usr/bin/env python3
"""Time plot-run-comp's join and histograms on generated runs and keep the numbers in profiles/runcomp/runcomp_bench.json.

    python tools/runcomp_bench.py device --sizes 1000 10000     # on the GPU machine: every column
    python tools/runcomp_bench.py host --sizes 1000             # without a GPU: host twins, dictionaries, phases

Each form fills its own section of the output file and leaves the other as it is.  Per size N: a reference run with all
N^2 comparisons (2 % of them NULL) and another run over the same genomes, row by row, with its own 2 % of NULLs.  Timed:

* ``device_resident_s``: the join plus the three ranges and histograms (``pa_runcomp_join``, 2 x ``pa_minmax_f64``,
  2 x ``pa_hist_uniform_f64`` per other run, and the reference run's range and histogram) between two HIP events, every
  input already on the device; ``device_resident_columns_s`` is the same with the other run column by column;
* ``device_with_upload_s``: a host clock around the upload of q, s and y, the same work and the copy back of the three
  joined arrays, ending in a synchronise (the reference matrix is uploaded once per command, ``upload_ref_s``);
* ``host_twin_s``: ``run_comp.compare`` without an engine;
* ``dict_join_s`` (N = 1000 only): the reference's method, two dictionaries keyed by (query_hash, subject_hash) tuples
  and two list comprehensions, without its ORM and without its histograms.

``phases`` (at ``--phase-size``, default 1000): ``rundb.plot_run_comp``'s parts on a database with two such runs, by a
host clock: the SQLite read of both runs, join plus histograms, the table write, and the whole command.

Every time is in seconds: the best and the median of ``--repeat`` runs after ``--warmup`` warm-up runs (one run and no
warm-up for the host twins at 10^8 rows, ``host_runs``).  The device and host results are compared bit for bit.
"""

from __future__ import annotations

import argparse
import hashlib
import json
import statistics
import sys
import tempfile
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

from pyani_plus_amd import reports, run_comp, rundb  # noqa: E402

SEED = 41
NULLS = 0.02


def synth_runs(n: int):
    """``(ref, q, s, y)``: the reference run's matrix and the other run row by row over the same genomes."""
    rng = np.random.default_rng(SEED + n)
    ref = 0.8 + 0.2 * rng.random((n, n))
    np.fill_diagonal(ref, 1.0)
    y = np.clip(ref + rng.normal(0.0, 0.004, (n, n)), 0.0, 1.0).reshape(-1)
    ref[rng.random((n, n)) < NULLS] = np.nan
    y[rng.random(n * n) < NULLS] = np.nan
    index = np.arange(n, dtype=np.uint32)
    return ref, np.repeat(index, n), np.tile(index, n), y


def timed(fn, repeat: int, warmup: int) -> tuple[dict, object]:
    out = None
    for _ in range(warmup):
        out = fn()
    times = []
    for _ in range(repeat):
        t0 = time.perf_counter()
        out = fn()
        times.append(time.perf_counter() - t0)
    return {"best": min(times), "median": statistics.median(times), "runs": repeat}, out


def same(a, b) -> bool:
    return all(np.array_equal(getattr(a, k).view(np.uint64), getattr(b, k).view(np.uint64)) for k in ("x", "y", "d")) and all(
        getattr(a, k) == getattr(b, k) for k in ("x_range", "y_range", "d_range")
    ) and all(np.array_equal(getattr(a, k), getattr(b, k)) for k in ("x_counts", "y_counts", "d_counts"))


def device_times(engine, ref, q, s, y, repeat: int, warmup: int, row: dict):
    t = engine.torch
    n = len(ref)

    def upload_ref():
        d = t.from_numpy(ref).to(engine.device)
        engine.sync()
        return d

    row["upload_ref_s"], d_ref = timed(upload_ref, repeat, 1)
    as_i32 = lambda a: t.from_numpy(a.view(np.int32))  # noqa: E731
    h_q, h_s, h_y = as_i32(q), as_i32(s), t.from_numpy(y)
    d_q, d_s, d_y = h_q.to(engine.device), h_s.to(engine.device), h_y.to(engine.device)
    # column by column: the same comparisons in the order of a run written subject by subject
    order = t.arange(n * n, device=engine.device).reshape(n, n).T.reshape(-1)
    columns = (d_q[order].contiguous(), d_s[order].contiguous(), d_y[order].contiguous())
    del order

    def resident(dq, ds, dy):
        def work():
            run_comp.range_and_counts(d_ref, engine)
            d_x, d_yy, d_d = engine.run_join_device(d_ref, dq, ds, dy)
            run_comp.range_and_counts(d_yy, engine)
            run_comp.range_and_counts(d_d, engine)
            return d_x

        for _ in range(warmup):
            work()
        times = []
        for _ in range(repeat):
            e0, e1 = t.cuda.Event(enable_timing=True), t.cuda.Event(enable_timing=True)
            e0.record()
            work()
            e1.record()
            e1.synchronize()
            times.append(e0.elapsed_time(e1) / 1e3)
        return {"best": min(times), "median": statistics.median(times), "runs": repeat}

    row["device_resident_s"] = resident(d_q, d_s, d_y)
    row["device_resident_columns_s"] = resident(*columns)
    del columns, d_q, d_s, d_y

    def with_upload():
        comp = run_comp.compare(d_ref, h_q.to(engine.device), h_s.to(engine.device), h_y.to(engine.device), engine)
        engine.sync()
        return comp

    row["device_with_upload_s"], comp = timed(with_upload, repeat, warmup)
    return comp


def dict_join_seconds(ref, q, s, y, repeat: int) -> dict:
    """The reference's method on the same runs: rows of (query_hash, subject_hash, identity) as its ORM yields them are
    made outside the clock; the two dictionaries and the two lists are inside."""
    hashes = [hashlib.md5(str(i).encode()).hexdigest() for i in range(len(ref))]  # noqa: S324
    ref_rows = [(hashes[i], hashes[j], None if np.isnan(v) else float(v)) for i, row in enumerate(ref) for j, v in enumerate(row)]
    other_rows = [(hashes[a], hashes[b], None if np.isnan(v) else float(v)) for a, b, v in zip(q.tolist(), s.tolist(), y.tolist())]

    def join():
        reference = {(a, b): v for a, b, v in ref_rows if v is not None}
        other = {(a, b): v for a, b, v in other_rows if v is not None and (a, b) in reference}
        x_values = [reference[pair] for pair in other]
        return x_values, list(other.values())

    out, (xs, ys) = timed(join, repeat, 0)
    out["rows_in_common"] = len(xs)
    assert len(xs) == len(ys)
    return out


def make_database(path: Path, ref, q, s, y) -> None:
    """Two runs of the method ``synthetic`` over ``len(ref)`` genomes: run 1 holds ``ref``, run 2 the rows q, s, y."""
    n = len(ref)
    hashes = sorted(hashlib.md5(str(i).encode()).hexdigest() for i in range(n))  # noqa: S324
    conn = rundb.connect_to_db(path)
    fasta = {Path(f"g{i}.fasta"): h for i, h in enumerate(hashes)}
    for h in hashes:
        rundb.db_genome(conn, Path(f"{h}.fasta"), h, 1000, h)
    value = lambda v: None if np.isnan(v) else float(v)  # noqa: E731
    for name, rows in (("reference", ((i, j, ref[i, j]) for i in range(n) for j in range(n))), ("other", zip(q.tolist(), s.tolist(), y.tolist()))):
        config = rundb.db_configuration(conn, "synthetic", name, "0")
        rundb.add_run(conn, config, "runcomp_bench", Path("."), "Done", name, fasta)
        conn.executemany(rundb.INSERT_COMPARISON, ((hashes[a], hashes[b], config.configuration_id, value(v), None, None, value(v), "", "", "") for a, b, v in rows))
        conn.commit()
    conn.close()


def phase_times(n: int, engine, repeat: int) -> dict:
    ref, q, s, y = synth_runs(n)
    out: dict = {"n": n, "rows_per_run": n * n}
    with tempfile.TemporaryDirectory() as tmp:
        db = Path(tmp) / "runs.sqlite"
        t0 = time.perf_counter()
        make_database(db, ref, q, s, y)
        out["make_database_s"] = time.perf_counter() - t0
        conn = rundb.connect_to_db(db)
        runs = [rundb.load_run(conn, 1), rundb.load_run(conn, 2)]
        hashes = sorted(a.genome_hash for a in runs[0].fasta_hashes)
        conn.execute("CREATE TEMP TABLE run_comp_ref (genome_hash VARCHAR NOT NULL PRIMARY KEY, idx INTEGER NOT NULL)")
        conn.executemany("INSERT INTO temp.run_comp_ref VALUES (?, ?)", zip(hashes, range(n)))
        out["sqlite_read_both_runs_s"], columns = timed(lambda: [reports._run_comparison_columns(conn, run) for run in runs], repeat, 1)  # noqa: SLF001
        conn.close()
        (rq, rs, ry), (oq, os_, oy) = columns
        matrix = np.full((n, n), np.nan)
        matrix[rq, rs] = ry
        assert np.array_equal(np.isnan(matrix), np.isnan(ref)) and np.array_equal(oq, q) and np.array_equal(os_, s)
        out["join_and_histograms_host_s"], comp = timed(lambda: run_comp.compare(matrix, oq, os_, oy), repeat, 1)
        if engine is not None:
            out["join_and_histograms_device_with_upload_s"], on_device = timed(lambda: run_comp.compare(matrix, oq, os_, oy, engine), repeat, 1)
            assert same(on_device, comp), "device and host results differ"
        out["table_write_s"], _none = timed(lambda: run_comp.write_pairs_tsv(Path(tmp) / "pairs.tsv", "#reference\tother", comp.x, comp.y), repeat, 1)
        out["table_bytes"] = (Path(tmp) / "pairs.tsv").stat().st_size
        out["plot_run_comp_host_s"], written = timed(lambda: rundb.plot_run_comp(db, Path(tmp) / "out", "1,2"), repeat, 1)
        if engine is not None:
            out["plot_run_comp_device_s"], again = timed(lambda: rundb.plot_run_comp(db, Path(tmp) / "dev", "1,2", engine=engine), repeat, 1)
            assert written[0].read_bytes() == again[0].read_bytes(), "the tables differ"
            out["same_bytes_with_device"] = True
    return out


def main() -> int:
    parser = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    parser.add_argument("what", choices=("device", "host"))
    parser.add_argument("--sizes", type=int, nargs="+", default=[1000, 10000])
    parser.add_argument("--repeat", type=int, default=5)
    parser.add_argument("--warmup", type=int, default=2)
    parser.add_argument("--phase-size", type=int, default=1000, help="genomes of the database of the phase timings (0: none)")
    parser.add_argument("--dict-max", type=int, default=1000, help="largest N at which the dictionary join is timed")
    parser.add_argument("--machine", default=None, help="a line about the machine, kept in the settings")
    parser.add_argument("--out", type=Path, default=ROOT / "profiles" / "runcomp" / "runcomp_bench.json")
    args = parser.parse_args()
    out = {"settings": {"generator": f"synth_runs(n), seed {SEED}, {NULLS:.0%} NULLs in each run", "unit": "seconds; best and median of the runs after the warm-up",
                        "repeat": args.repeat, "warmup": args.warmup}, "sizes": {}}  # fmt: skip
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
            ref, q, s, y = synth_runs(n)
            row: dict = {"rows": n * n}
            big = n * n > 10**7
            row["host_twin_s"], host = timed(lambda: run_comp.compare(ref, q, s, y), 1 if big else args.repeat, 0 if big else 1)
            row["rows_in_common"] = len(host.x)
            if engine is not None:
                device = device_times(engine, ref, q, s, y, args.repeat, args.warmup, row)
                assert same(device, host), "device and host results differ"
                row["same_bits_as_host"] = True
                del device
            if n <= args.dict_max:
                row["dict_join_s"] = dict_join_seconds(ref, q, s, y, 3)
                assert row["dict_join_s"]["rows_in_common"] == len(host.x)
            out["sizes"][str(n)] = row
            print(f"n={n}: {json.dumps(row)}", flush=True)
            del ref, q, s, y, host
        if args.phase_size:
            out["phases"] = phase_times(args.phase_size, engine, 3)
            print(f"phases: {json.dumps(out['phases'])}", flush=True)
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
