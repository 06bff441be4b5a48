"""external-alignment-hip timings on synthetic alignments.

    python tools/bench_msa.py [--configs A,B,C] [--reps 3] [--out profiles/msa_bench.json]

Per configuration: the FASTA file is written to a temporary directory, then timed
  load     pa_msa_load (md5 on its own thread beside the parallel parse) + rows copied out; md5 alone (hashlib) shown apart
  upload   rows -> device + pack kernel (msa_upload)
  pairs    the symmetric pair-count call (msa_pair_counts), best of --reps
  metrics  (M, B, n) -> the five numbers for every ordered pair, host thread pool
and the kernel times of the library's own event timers (phases msa_pack, msa_pairs).  The model bound of the pair kernel
is pairs(j >= i) x ceil(L / 32) x (b + 4) VALU lane-ops at 256 CU x 4 SIMD x 32 lanes x 2.4 GHz."""

from __future__ import annotations

import argparse
import hashlib
import json
import sys
import tempfile
import time
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

from pyani_plus_amd.engine import HipEngine, load_msa, msa_code_table, msa_metrics  # noqa: E402
from pyani_plus_amd.synth import msa_fasta_bytes, synth_msa_rows  # noqa: E402

CONFIGS = {
    "A": dict(n=10_000, length=29_903, opts=dict(divergence=0.01, gap_runs=2e-5, n_runs=5e-5)),
    "B": dict(n=1_000, length=2_000_000, opts=dict(divergence=0.01, gap_runs=1e-5, n_runs=1e-5)),
    "C": dict(n=2_000, length=30_000, opts=dict(divergence=0.03, gap_runs=1e-4, n_runs=5e-5, iupac=0.005, lower=0.01)),
}
PEAK_LANE_OPS = 256 * 4 * 32 * 2.4e9


def bench(engine: HipEngine, name: str, cfg: dict, reps: int, tmp: Path) -> dict:
    t0 = time.perf_counter()
    rows = synth_msa_rows(cfg["n"], cfg["length"], seed=ord(name), **cfg["opts"])
    path = tmp / f"{name}.fasta"
    path.write_bytes(msa_fasta_bytes([f"g{i:05d}" for i in range(cfg["n"])], rows, seed=1))
    del rows
    synth_s = time.perf_counter() - t0
    t0 = time.perf_counter()
    md5_alone = hashlib.md5(path.read_bytes()).hexdigest()
    md5_s = time.perf_counter() - t0
    t0 = time.perf_counter()
    msa = load_msa(path)
    load_s = time.perf_counter() - t0
    assert msa.md5 == md5_alone
    _code, bits = msa_code_table(msa.histogram)
    torch = engine.torch
    engine.prof_enable(True)
    engine.prof_reset()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    dm = engine.msa_upload(msa)
    torch.cuda.synchronize()
    upload_s = time.perf_counter() - t0
    pack_ms = engine.prof_get()["msa_pack"][0]
    pair_s, kernel_ms = [], []
    for _ in range(reps):
        engine.prof_reset()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        m, b = engine.msa_pair_counts(dm, symmetric=True)
        torch.cuda.synchronize()
        pair_s.append(time.perf_counter() - t0)
        kernel_ms.append(engine.prof_get()["msa_pairs"][0])
        if _ < reps - 1:
            del m, b
    t0 = time.perf_counter()
    m_h, b_h = m.cpu().numpy().view(np.uint32), b.cpu().numpy().view(np.uint32)
    d2h_s = time.perf_counter() - t0
    n_res = dm.nongap.cpu().numpy().view(np.uint32)[: msa.n_rows].astype(np.uint64)
    t0 = time.perf_counter()
    step = max(1, 10_000_000 // msa.n_rows)
    for r0 in range(0, msa.n_rows, step):
        r1 = min(msa.n_rows, r0 + step)
        msa_metrics(m_h[r0:r1], b_h[r0:r1], n_res[r0:r1, None], n_res[None, :])
    metrics_s = time.perf_counter() - t0
    engine.prof_enable(False)
    n, words = msa.n_rows, (msa.n_cols + 31) // 32
    tri = n * (n + 1) // 2
    model_ms = tri * words * (bits + 4) / PEAK_LANE_OPS * 1e3
    best_kernel = min(kernel_ms)
    out = {
        "config": name, "rows": n, "columns": msa.n_cols, "bits": bits, "file_bytes": path.stat().st_size,
        "synth_and_write_s": round(synth_s, 3), "md5_alone_s": round(md5_s, 3), "load_s (md5 beside parse)": round(load_s, 3),
        "upload_and_pack_s": round(upload_s, 4), "pack_kernel_ms": round(pack_ms, 3),
        "pairs_call_ms": [round(x * 1e3, 3) for x in pair_s], "pairs_kernel_ms": [round(x, 3) for x in kernel_ms],
        "pairs_model_ms": round(model_ms, 3), "fraction_of_model": round(model_ms / best_kernel, 3),
        "device_step_ordered_pairs_per_s": round(n * n / (upload_s + min(pair_s)), 1),
        "counts_to_host_s": round(d2h_s, 3), "metrics_all_ordered_pairs_s": round(metrics_s, 3),
        "file_to_metrics_s": round(load_s + upload_s + min(pair_s) + d2h_s + metrics_s, 3),
    }
    print(json.dumps(out), flush=True)
    path.unlink()
    return out


def main() -> None:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--configs", default="A,B,C")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", type=Path, default=None)
    args = ap.parse_args()
    engine = HipEngine(0)
    results = []
    with tempfile.TemporaryDirectory() as tmp:
        for name in args.configs.split(","):
            results.append(bench(engine, name, CONFIGS[name], args.reps, Path(tmp)))
    engine.close()
    if args.out:
        args.out.parent.mkdir(parents=True, exist_ok=True)
        args.out.write_text(json.dumps({"device": "MI355X", "results": results}, indent=1) + "\n")


if __name__ == "__main__":
    main()
