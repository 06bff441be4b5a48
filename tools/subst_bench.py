#!/usr/bin/env python3
"""Time phylo-run's steps on synthetic alignments and keep the numbers in profiles/subst/subst_bench.json.

    python tools/subst_bench.py --rows 1000 --columns 1000000                  # on the GPU machine
    python tools/subst_bench.py --rows 10000 --columns 100000 --no-twin
    python tools/subst_bench.py --rows 1000 --columns 100000 --command 100     # also the whole command, 100 replicates

Per size the alignment is ``synth.synth_msa_rows(rows, columns, seed=7)``, packed with the nucleotide code (3 bits, four
planes a word) and resident on the device; the weights are those of seed 1.  Every comparison is taken in this one
process, on the same planes.  Device legs: the device phase of the library call (``pa_prof_get``: the events around its
launches on the context's stream), best of ``--repeat`` after one warm-up, divided by the replicates of the call where it
holds several:

* ``pair_counts_s``: ``pa_msa_pair_counts`` (symmetric), the yardstick of the unweighted call; ``subst_counts_s``:
  ``pa_msa_subst_counts`` without weights; ``unweighted_ratio`` the second over the first, ``unweighted_model`` the
  instruction count 7 : (b + 4);
* ``boot_counts_s``: ``pa_msa_boot_counts`` over ``--replicates`` replicates, the yardstick of the weighted call, per
  replicate; ``subst_boot_counts_s``: ``pa_msa_subst_counts`` with the same weights; ``weighted_ratio`` and
  ``weighted_model`` (4 + 9 nb) : (b + 2 + 6 nb);
* ``*_runs_s``: the repetitions, whose spread is what a ratio may be off by;
* ``distances_s``: ``pa_subst_distances`` (K80) per matrix, once after a warm-up (device events around the call);
* ``twin_counts_s``, ``twin_distances_s``: the host twins on 16 threads, one replicate, host clock, once, and
  ``same_counts`` / ``same_distances``: the device's results of that replicate against them;
* ``command_s`` (with ``--command R``): the whole ``phylo_run`` with the engine and R replicates on a run made of this
  alignment, host clock, once.

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

from boot_bench import ALIGNMENT_SEED, HOST_THREADS, WEIGHT_SEED, loaded  # noqa: E402
from pcoa_bench import timed  # noqa: E402

from pyani_plus_amd import engine as engine_mod  # noqa: E402
from pyani_plus_amd.synth import synth_msa_rows  # noqa: E402

MODEL = "k80"


def phase_runs(engine, call, phase: str, repeat: int, per: int) -> list[float]:
    """The device phase ``phase`` of ``call()``, in seconds per ``per``, ``repeat`` times after one warm-up."""
    call()
    engine.prof_enable(True)
    runs = []
    for _ in range(repeat):
        engine.prof_reset()
        call()
        engine.sync()
        runs.append(engine.prof_get()[phase][0] / 1e3 / per)
    engine.prof_enable(False)
    return runs


def whole_command(rows: np.ndarray, replicates: int, engine, row: dict) -> None:
    """A run of this alignment in a temporary database, then ``phylo_run`` on it."""
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
        rundb.phylo_run(db, tmp / "device", model=MODEL, replicates=replicates, seed=WEIGHT_SEED, engine=engine)
        row["command_s"] = time.perf_counter() - t0
        row["command_replicates"] = replicates


def main() -> int:
    parser = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    parser.add_argument("--rows", type=int, required=True)
    parser.add_argument("--columns", type=int, required=True)
    parser.add_argument("--replicates", type=int, default=8, help="replicates of the timed weighted calls")
    parser.add_argument("--repeat", type=int, default=5)
    parser.add_argument("--no-twin", action="store_true")
    parser.add_argument("--command", type=int, default=0, metavar="R")
    parser.add_argument("--out", type=Path, default=ROOT / "profiles" / "subst" / "subst_bench.json")
    args = parser.parse_args()
    from pyani_plus_amd.engine import HipEngine

    n, n_cols, reps = args.rows, args.columns, args.replicates
    rows = synth_msa_rows(n, n_cols, seed=ALIGNMENT_SEED)
    msa = loaded(rows)
    weights = engine_mod.msa_boot_weights(WEIGHT_SEED, n_cols, 0, reps)
    nb = int(weights.max()).bit_length()
    row: dict = {"rows": n, "columns": n_cols, "replicates_per_call": reps, "weight_planes": nb, "max_weight": int(weights.max())}
    print(f"{n} x {n_cols}: alignment and weights ready, {nb} weight planes", flush=True)
    engine = HipEngine(0)
    try:
        dm = engine.msa_subst_upload(msa)
        b = dm.bits
        row["code_bits"] = b
        row["unweighted_model"] = 7 / (b + 4)
        row["weighted_model"] = (4 + 9 * nb) / (b + 2 + 6 * nb)
        for key, call, phase, per in (
            ("pair_counts", lambda: engine.msa_pair_counts(dm, symmetric=True), "msa_pairs", 1),
            ("subst_counts", lambda: engine.msa_subst_counts(dm), "msa_pairs", 1),
            ("boot_counts", lambda: engine.msa_boot_counts(dm, weights), "msa_boot", reps),
            ("subst_boot_counts", lambda: engine.msa_subst_counts(dm, weights), "msa_pairs", reps),
        ):
            runs = phase_runs(engine, call, phase, args.repeat, per)
            row[f"{key}_runs_s"] = [round(x, 7) for x in runs]
            row[f"{key}_s"] = min(runs)
        row["unweighted_ratio"] = row["subst_counts_s"] / row["pair_counts_s"]
        row["weighted_ratio"] = row["subst_boot_counts_s"] / row["boot_counts_s"]
        print(f"{n} x {n_cols}: unweighted {row['subst_counts_s']:.5f} s against {row['pair_counts_s']:.5f} s: ratio {row['unweighted_ratio']:.3f}, "
              f"model {row['unweighted_model']:.3f}; weighted {row['subst_boot_counts_s']:.5f} s against {row['boot_counts_s']:.5f} s a replicate: "
              f"ratio {row['weighted_ratio']:.3f}, model {row['weighted_model']:.3f}", flush=True)  # fmt: skip
        counts = engine.msa_subst_counts(dm, weights[:1])
        timed(engine, lambda: engine.subst_distances(*counts, MODEL))
        row["distances_s"], (distances, undefined) = timed(engine, lambda: engine.subst_distances(*counts, MODEL))
        row["undefined"] = [int(x) for x in undefined[0]]
        print(f"{n} x {n_cols}: distances {row['distances_s']:.6f} s, undefined pairs {row['undefined']}", flush=True)
        if not args.no_twin:
            small = min(n_cols, 64)
            engine_mod.msa_subst_counts_host(msa.rows[:8], small, np.ones((1, small), dtype=np.uint8), HOST_THREADS)  # the pool's threads exist
            t0 = time.perf_counter()
            want = engine_mod.msa_subst_counts_host(msa.rows, n_cols, weights[:1], HOST_THREADS)
            row["twin_counts_s"] = time.perf_counter() - t0
            row["same_counts"] = all(bool(np.array_equal(a.cpu().numpy().view(np.uint32), w)) for a, w in zip(counts, want))
            t0 = time.perf_counter()
            twin, twin_undefined = engine_mod.subst_distances_host(*want, MODEL, threads=HOST_THREADS)
            row["twin_distances_s"] = time.perf_counter() - t0
            row["same_distances"] = bool(np.array_equal(distances.cpu().numpy().view(np.uint64), twin.view(np.uint64)) and
                                         np.array_equal(undefined, twin_undefined))  # fmt: skip
            print(f"{n} x {n_cols}: twin counts {row['twin_counts_s']:.2f} s a replicate, same {row['same_counts']}; twin distances "
                  f"{row['twin_distances_s']:.3f} s, same {row['same_distances']}", flush=True)  # fmt: skip
        del counts, distances
        if args.command:
            whole_command(rows, args.command, engine, row)
            print(f"{n} x {n_cols}: command with {args.command} replicates {row['command_s']:.2f} s", flush=True)
        info = engine.device_info()
    finally:
        engine.close()
    data = json.loads(args.out.read_text()) if args.out.is_file() else {}
    data.setdefault("settings", {}).update(
        generator=f"synth_msa_rows(rows, columns, seed={ALIGNMENT_SEED}); weights of seed {WEIGHT_SEED}; model {MODEL}",
        unit=f"seconds; counts: the call's device phase, best of {args.repeat} after one warm-up, per replicate; distances: device events, once; host legs: host clock, once",
        host_threads=HOST_THREADS, device=info["name"], compute_units=info["compute_units"])  # fmt: skip
    data.setdefault("sizes", {})[f"{n}x{n_cols}"] = row
    args.out.parent.mkdir(parents=True, exist_ok=True)
    args.out.write_text(json.dumps(data, indent=1) + "\n")
    return 0 if row.get("same_counts", True) and row.get("same_distances", True) else 1


if __name__ == "__main__":
    raise SystemExit(main())
