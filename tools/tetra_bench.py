#!/usr/bin/env python3
"""Time the TETRA-hip steps on generated genomes and keep the numbers in profiles/tetra/tetra_bench.json.

    python tools/tetra_bench.py                       # on the GPU machine: 1 000 genomes of 5 Mb, arena resident

What is measured (device times with device events on the engine's stream, the best of ``--repeat`` runs after one
warm-up; host times are wall seconds):

* ``pa_tetra_counts`` on the whole arena, beside the k-mer hash kernel (k = 31, scaled = 1000) on the same arena in the
  same run -- the yardstick: it reads the same bytes --, beside the kernel's direct-counting form (both forms in the
  tools build), and beside ``pa_tetra_counts_host`` on 16 threads, which is run once on the first ``--host-genomes``
  genomes (its time scales with the residues) and compared with the device's counts;
* ``pa_tetra_corr`` on the unit rows of the arena's genomes (N = 1 000) and on 10 000 generated unit rows, beside
  ``pa_tetra_corr_host`` on 16 threads, the results compared bit for bit;
* the whole ``tetra`` command (``rundb.run_tetra_hip``) on the first ``--command-genomes`` genomes written out as FASTA
  files, on the device and on the host, with its phases.

DESIGN.md section 7g quotes this file."""

from __future__ import annotations

import argparse
import json
import os
import sys
import tempfile
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

from pyani_plus_amd import _capi, rundb  # noqa: E402
from pyani_plus_amd.engine import HipEngine, tetra_correlations_host, tetra_counts_host, tetra_zscores  # noqa: E402
from pyani_plus_amd.synth import arena_to_ascii, device_arena_to_host, synth_arena_torch  # noqa: E402

HOST_THREADS = 16


def event_ms(engine, fn, repeat: int) -> tuple[float, object]:
    """Best device time of ``fn`` in milliseconds (events on the current stream) after one warm-up, and its last result."""
    t = engine.torch
    out = fn()
    t.cuda.synchronize(engine.device)
    best = float("inf")
    for _ in range(repeat):
        e0, e1 = t.cuda.Event(enable_timing=True), t.cuda.Event(enable_timing=True)
        e0.record()
        out = fn()
        e1.record()
        t.cuda.synchronize(engine.device)
        best = min(best, e0.elapsed_time(e1))
    return best, out


def main() -> int:
    parser = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    parser.add_argument("--genomes", type=int, default=1000)
    parser.add_argument("--length", type=int, default=5_000_000)
    parser.add_argument("--species", type=int, default=40)
    parser.add_argument("--repeat", type=int, default=5)
    parser.add_argument("--host-genomes", type=int, default=100)
    parser.add_argument("--command-genomes", type=int, default=100)
    parser.add_argument("--corr-sizes", type=int, nargs="*", default=[1000, 10000])
    parser.add_argument("--out", type=Path, default=ROOT / "profiles" / "tetra" / "tetra_bench.json")
    args = parser.parse_args()

    engine = HipEngine(0)
    t = engine.torch
    info = engine.device_info()
    n = args.genomes
    arena = synth_arena_torch(engine, n, args.length, n_species=args.species)
    result: dict = {
        "settings": {
            "generator": f"synth_arena_torch({n}, {args.length}, n_species={args.species})", "arena_bases": arena.arena_bases,
            "unit": f"device: milliseconds between device events, best of {args.repeat} after one warm-up; host: wall seconds",
            "host_threads": HOST_THREADS, "device": info["name"], "compute_units": info["compute_units"],
        }  # fmt: skip
    }

    # ---- counts beside the k-mer hash kernel
    dirty = engine.arena_dirty(arena)
    gs = np.ascontiguousarray(arena.genome_start, dtype=np.uint64)
    counts_dev = t.empty((n, _capi.PA_TETRA_BINS), dtype=t.int64, device=engine.device)

    def count():
        engine._check(  # noqa: SLF001 - the library call alone, without the copy back
            engine.lib.pa_tetra_counts(engine.ctx, arena.packed.data_ptr(), arena.mask.data_ptr(), dirty.data_ptr(), arena.arena_bases,
                                       gs.ctypes.data, n, counts_dev.data_ptr()),
            "pa_tetra_counts",
        )  # fmt: skip

    counts_ms, _ = event_ms(engine, count, args.repeat)
    counts = counts_dev.cpu().numpy().view(np.uint64)
    engine.sketch(arena, 31, 1000)  # warm-up
    hash_ms = float("inf")
    engine.prof_enable(True)
    for _ in range(args.repeat):
        engine.prof_reset()
        engine.sketch(arena, 31, 1000)
        hash_ms = min(hash_ms, engine.prof_get()["kmer_hash"][0])
    engine.prof_enable(False)
    packed_bytes = arena.arena_bases // 4
    result["counts"] = {
        "pa_tetra_counts_ms": counts_ms, "kmer_hash_kernel_ms": hash_ms, "counts_over_hash": counts_ms / hash_ms,
        "packed_bytes": packed_bytes, "packed_GB_per_s": packed_bytes / counts_ms / 1e6,
        "windows_counted": int(counts[:, :256].sum()),
    }  # fmt: skip
    # the two forms of the kernel (one update per start and derived tri- and dinucleotides, or three updates per start),
    # both in the tools build, where PA_TETRA_DIRECT selects the second
    tools_engine = HipEngine(0, tools=True)

    def count_tools():
        tools_engine._check(  # noqa: SLF001
            tools_engine.lib.pa_tetra_counts(tools_engine.ctx, arena.packed.data_ptr(), arena.mask.data_ptr(), dirty.data_ptr(), arena.arena_bases,
                                             gs.ctypes.data, n, counts_dev.data_ptr()),
            "pa_tetra_counts",
        )  # fmt: skip

    forms = {}
    for form, value in (("derived", "0"), ("direct", "1")):
        os.environ["PA_TETRA_DIRECT"] = value
        forms[f"{form}_ms"], _ = event_ms(tools_engine, count_tools, args.repeat)
        forms[f"{form}_same_counts"] = bool(np.array_equal(counts_dev.cpu().numpy().view(np.uint64), counts))
    os.environ.pop("PA_TETRA_DIRECT")
    tools_engine.close()
    result["counts"]["forms"] = forms
    n_host = min(args.host_genomes, n)
    host_arena = device_arena_to_host(arena, list(range(max(n_host, min(args.command_genomes, n)))), args.length)
    sub = type(host_arena)(host_arena.packed[: int(host_arena.genome_start[n_host]) // 16], host_arena.mask[: int(host_arena.genome_start[n_host]) // 32],
                           host_arena.genome_start[: n_host + 1])  # fmt: skip
    t0 = time.perf_counter()
    counts_host = tetra_counts_host(sub, threads=HOST_THREADS)
    host_s = time.perf_counter() - t0
    result["counts"].update({
        "host_genomes": n_host, "host_twin_s": host_s, "host_twin_s_scaled_to_arena": host_s * n / max(n_host, 1),
        "same_counts_as_host": bool(np.array_equal(counts_host, counts[:n_host])),
    })  # fmt: skip

    # ---- correlations
    _z, unit = tetra_zscores(counts)
    result["corr"] = {}
    rng = np.random.default_rng(7)
    for size in args.corr_sizes:
        if size == n:
            rows, source = unit, "the arena's genomes"
        else:
            rows = rng.standard_normal((size, _capi.PA_TETRA_WORDS))
            rows -= rows.mean(axis=1, keepdims=True)
            rows /= np.sqrt((rows * rows).sum(axis=1, keepdims=True))
            source = "generated unit rows (normal, centred, normalised)"
        d_rows = engine._f64_on_device(rows)  # noqa: SLF001
        ms, d_out = event_ms(engine, lambda d_rows=d_rows: engine.tetra_correlations_device(d_rows), args.repeat)
        got = d_out.cpu().numpy()
        del d_out
        t0 = time.perf_counter()
        want = tetra_correlations_host(rows, threads=HOST_THREADS)
        host_s = time.perf_counter() - t0
        pairs = size * (size + 1) // 2
        result["corr"][str(size)] = {
            "rows": source, "pa_tetra_corr_ms": ms, "pairs_evaluated": pairs, "multiply_adds": pairs * _capi.PA_TETRA_WORDS,
            "GFLOP_per_s": 2 * pairs * _capi.PA_TETRA_WORDS / ms / 1e6, "host_twin_s": host_s,
            "same_bits_as_host": bool(np.array_equal(got.view(np.uint64), want.view(np.uint64))),
        }  # fmt: skip
        del got, want

    # ---- the whole command
    n_cmd = min(args.command_genomes, n)
    with tempfile.TemporaryDirectory(prefix="tetra_bench_") as tmp:
        fasta_dir = Path(tmp) / "fasta"
        fasta_dir.mkdir()
        for g in range(n_cmd):
            (fasta_dir / f"g{g:04d}.fasta").write_bytes(b">g%d\n" % g + arena_to_ascii(host_arena, g) + b"\n")
        command = {"genomes": n_cmd, "residues": n_cmd * args.length}
        for label, eng in (("device", engine), ("host", None)):
            timings: dict = {}
            t0 = time.perf_counter()
            run = rundb.run_tetra_hip(fasta_dir, Path(tmp) / f"{label}.db", cache=Path(tmp) / f"cache_{label}", temp=Path(tmp) / f"tmp_{label}",
                                      engine=eng, timings=timings)  # fmt: skip
            command[f"{label}_s"] = time.perf_counter() - t0
            command[f"{label}_phases_s"] = timings
            assert run.status == "Done"
        result["command"] = command
    engine.close()
    args.out.parent.mkdir(parents=True, exist_ok=True)
    args.out.write_text(json.dumps(result, indent=1) + "\n")
    print(json.dumps(result))
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
