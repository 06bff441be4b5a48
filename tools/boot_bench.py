#!/usr/bin/env python3
"""Time bootstrap-run's steps on synthetic alignments and keep the numbers in profiles/boot/boot_bench.json.

    python tools/boot_bench.py --rows 1000 --columns 1000000                  # on the GPU machine
    python tools/boot_bench.py --rows 10000 --columns 100000 --no-twin
    python tools/boot_bench.py --rows 1000 --columns 100000 --command 100     # also the whole command, 100 replicates

Per size the alignment is ``synth.synth_msa_rows(rows, columns, seed=7)``, packed and resident on the device, and the
weights are those of seed 1.  Device legs: device events around the library call on the context's stream, best of
``--repeat`` after one warm-up, divided by the replicates of the call where it holds several:

* ``weighted_counts_s``: one ``HipEngine.msa_boot_counts`` over ``--replicates`` replicates -- the host check of the
  weights, their upload, the slicing into planes, the pair kernel and the mirror -- per replicate;
  ``weighted_kernels_s`` is the same call's device phase alone (``pa_prof_get``: the events around its launches);
* ``pair_counts_s``: the unweighted ``pa_msa_pair_counts`` (symmetric) on the same planes, the yardstick;
  ``ratio`` is weighted_kernels_s over it, ``model_ratio`` the instruction count (b + 2 + 6 nb) / (b + 4);
* ``distances_s``: ``msa_boot_distances`` per replicate;  ``nj_s``: one ``pa_nj`` of a replicate's matrix;
* ``twin_counts_s``: ``pa_msa_boot_counts_host`` of one replicate on 16 threads, host clock, run once, and
  ``same_counts``: the device's integers of that replicate against it;
* ``command_s`` (with ``--command R``): the whole ``bootstrap_run`` with the engine and R replicates on a run made of
  this alignment, host clock, once; ``command_host_s`` the same without the engine when ``--command-host`` is given.

A size fills its own entry of the output file and leaves the others as they are.
"""

from __future__ import annotations

import argparse
import json
import logging
import sys
import tempfile
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tools"))

from pcoa_bench import timed  # noqa: E402

from pyani_plus_amd import engine as engine_mod  # noqa: E402
from pyani_plus_amd.synth import synth_msa_rows  # noqa: E402

ALIGNMENT_SEED = 7
WEIGHT_SEED = 1
HOST_THREADS = 16


def loaded(rows: np.ndarray) -> engine_mod.LoadedMSA:
    n, length = rows.shape
    stride = max(32, (length + 31) // 32 * 32)
    padded = np.full((n, stride), engine_mod.GAP, dtype=np.uint8)
    padded[:, :length] = rows
    hist = np.bincount(rows.ravel(), minlength=256).astype(np.uint64)
    return engine_mod.LoadedMSA("", [f"g{i:05d}".encode() for i in range(n)], np.full(n, length, np.uint64), hist, padded, length)


def whole_command(rows: np.ndarray, replicates: int, engine, host_too: bool, row: dict) -> None:
    """A run of this alignment in a temporary database, then ``bootstrap_run`` on it."""
    from pyani_plus_amd import rundb

    logging.getLogger("pyani_plus_amd").setLevel(logging.WARNING)
    with tempfile.TemporaryDirectory() as tmp:
        tmp = Path(tmp)
        fasta = tmp / "genomes"
        fasta.mkdir()
        names = [f"g{i:05d}" for i in range(len(rows))]
        for name, r in zip(names, rows):
            (fasta / f"{name}.fasta").write_bytes(b">" + name.encode() + b"\n" + bytes(r[r != engine_mod.GAP]) + b"\n")
        aln = tmp / "synthetic.aln.fasta"
        with aln.open("wb") as handle:
            for name, r in zip(names, rows):
                handle.write(b">" + name.encode() + b"\n" + bytes(r) + b"\n")
        db = tmp / "runs.sqlite"
        t0 = time.perf_counter()
        assert rundb.run_external_alignment_hip(fasta, db, alignment=aln, temp=tmp / "t", engine=engine).status == "Done"
        row["run_s"] = time.perf_counter() - t0
        t0 = time.perf_counter()
        device = rundb.bootstrap_run(db, tmp / "device", replicates=replicates, seed=WEIGHT_SEED, engine=engine)
        row["command_s"] = time.perf_counter() - t0
        row["command_replicates"] = replicates
        if host_too:
            t0 = time.perf_counter()
            host = rundb.bootstrap_run(db, tmp / "host", replicates=replicates, seed=WEIGHT_SEED)
            row["command_host_s"] = time.perf_counter() - t0
            row["command_same_bytes"] = all(a.read_bytes() == b.read_bytes() for a, b in zip(device, host))


def main() -> int:
    parser = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    parser.add_argument("--rows", type=int, required=True)
    parser.add_argument("--columns", type=int, required=True)
    parser.add_argument("--replicates", type=int, default=8, help="replicates of the timed call (at least --repeat + 1: each pa_nj run uses one up)")
    parser.add_argument("--repeat", type=int, default=5)
    parser.add_argument("--no-twin", action="store_true")
    parser.add_argument("--no-nj", action="store_true")
    parser.add_argument("--command", type=int, default=0, metavar="R")
    parser.add_argument("--command-host", action="store_true")
    parser.add_argument("--out", type=Path, default=ROOT / "profiles" / "boot" / "boot_bench.json")
    args = parser.parse_args()
    from pyani_plus_amd.engine import HipEngine

    n, n_cols, reps = args.rows, args.columns, max(args.replicates, args.repeat + 1)
    rows = synth_msa_rows(n, n_cols, seed=ALIGNMENT_SEED)
    msa = loaded(rows)
    weights = engine_mod.msa_boot_weights(WEIGHT_SEED, n_cols, 0, reps)
    nb = int(weights.max()).bit_length()
    row: dict = {"rows": n, "columns": n_cols, "replicates_per_call": reps, "weight_planes": nb, "max_weight": int(weights.max())}
    print(f"{n} x {n_cols}: alignment and weights ready, {nb} weight planes", flush=True)
    engine = HipEngine(0)
    try:
        dm = engine.msa_upload(msa)
        b = dm.bits
        row["code_bits"] = b
        row["model_ratio"] = (b + 2 + 6 * nb) / (b + 4)
        timed(engine, lambda: engine.msa_pair_counts(dm, symmetric=True))
        runs = [timed(engine, lambda: engine.msa_pair_counts(dm, symmetric=True))[0] for _ in range(args.repeat)]
        row["pair_counts_runs_s"] = [round(x, 6) for x in runs]
        row["pair_counts_s"] = min(runs)
        timed(engine, lambda: engine.msa_boot_counts(dm, weights))
        engine.prof_enable(True)
        runs, phases = [], []
        for _ in range(args.repeat):
            engine.prof_reset()
            spent, (match, both) = timed(engine, lambda: engine.msa_boot_counts(dm, weights))
            runs.append(spent / reps)
            phases.append(engine.prof_get()["msa_boot"][0] / 1e3 / reps)
        engine.prof_enable(False)
        row["weighted_counts_runs_s"] = [round(x, 6) for x in runs]
        row["weighted_counts_s"] = min(runs)
        row["weighted_kernels_s"] = min(phases)
        row["ratio"] = row["weighted_kernels_s"] / row["pair_counts_s"]
        print(f"{n} x {n_cols}: pair counts {row['pair_counts_s']:.5f} s, weighted {row['weighted_counts_s']:.5f} s a replicate "
              f"(kernels {row['weighted_kernels_s']:.5f} s): ratio {row['ratio']:.2f}, model {row['model_ratio']:.2f}", flush=True)  # fmt: skip
        timed(engine, lambda: engine.msa_boot_distances(match, both))
        runs = [timed(engine, lambda: engine.msa_boot_distances(match, both)) for _ in range(args.repeat)]
        row["distances_s"] = min(r[0] for r in runs) / reps
        distances = runs[-1][1]
        del runs
        first = (match[0].cpu().numpy().view(np.uint32), both[0].cpu().numpy().view(np.uint32))
        del match, both
        if not args.no_nj:
            timed(engine, lambda: engine.nj_tree_inplace(distances[reps - 1]))
            runs = [timed(engine, lambda r=r: engine.nj_tree_inplace(distances[r]))[0] for r in range(args.repeat)]
            row["nj_runs_s"] = [round(x, 6) for x in runs]
            row["nj_s"] = min(runs)
            print(f"{n} x {n_cols}: distances {row['distances_s']:.6f} s, pa_nj {row['nj_s']:.4f} s", flush=True)
        del distances
        if not args.no_twin:
            engine_mod.msa_boot_counts_host(msa.rows[:8], min(n_cols, 64), np.ones((1, min(n_cols, 64)), dtype=np.uint8), HOST_THREADS)  # the pool's threads exist
            t0 = time.perf_counter()
            want = engine_mod.msa_boot_counts_host(msa.rows, n_cols, weights[:1], HOST_THREADS)
            row["twin_counts_s"] = time.perf_counter() - t0
            row["same_counts"] = bool(np.array_equal(first[0], want[0][0]) and np.array_equal(first[1], want[1][0]))
            print(f"{n} x {n_cols}: twin {row['twin_counts_s']:.2f} s a replicate, same counts {row['same_counts']}", flush=True)
        if args.command:
            whole_command(rows, args.command, engine, args.command_host, row)
            print(f"{n} x {n_cols}: command with {args.command} replicates {row['command_s']:.2f} s", flush=True)
        info = engine.device_info()
    finally:
        engine.close()
    data = json.loads(args.out.read_text()) if args.out.is_file() else {}
    data.setdefault("settings", {}).update(
        generator=f"synth_msa_rows(rows, columns, seed={ALIGNMENT_SEED}); weights of seed {WEIGHT_SEED}",
        unit=f"seconds; device legs: best of {args.repeat} after one warm-up, device events around the library call, per replicate; host legs: host clock, once",
        host_threads=HOST_THREADS, device=info["name"], compute_units=info["compute_units"])  # fmt: skip
    data.setdefault("sizes", {})[f"{n}x{n_cols}"] = row
    args.out.parent.mkdir(parents=True, exist_ok=True)
    args.out.write_text(json.dumps(data, indent=1) + "\n")
    return 0 if row.get("same_counts", True) and row.get("command_same_bytes", True) else 1


if __name__ == "__main__":
    raise SystemExit(main())
