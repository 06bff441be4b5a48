"""Lean harness for the rocprofv3 --pmc passes of bootstrap-run's weighted pair kernel and its unweighted yardstick: two
calls of each on one synthetic alignment, no other kernels of ours beside them.  Usage on the GPU machine, one counter
group a process:
    rocprofv3 --pmc SQ_INSTS_VALU SQ_ACTIVE_INST_VALU SQ_WAVE_CYCLES SQ_BUSY_CYCLES GRBM_GUI_ACTIVE \
        --kernel-include-regex pairs_kernel --kernel-trace --output-format csv -d out/sq_valu -- python3 tools/boot_pmc.py [rows] [columns] [replicates]
``tools/pmc_summary.py out msa_boot_pairs_kernel`` (and ``... msa_pairs_kernel``) then prints the mean of each counter per dispatch.
"""
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
sys.path.insert(0, str(Path(__file__).resolve().parent))
from boot_bench import ALIGNMENT_SEED, WEIGHT_SEED, loaded  # noqa: E402

from pyani_plus_amd.engine import HipEngine, msa_boot_weights  # noqa: E402
from pyani_plus_amd.synth import synth_msa_rows  # noqa: E402

n = int(sys.argv[1]) if len(sys.argv) > 1 else 1000
n_cols = int(sys.argv[2]) if len(sys.argv) > 2 else 100000
reps = int(sys.argv[3]) if len(sys.argv) > 3 else 8
msa = loaded(synth_msa_rows(n, n_cols, seed=ALIGNMENT_SEED))
weights = msa_boot_weights(WEIGHT_SEED, n_cols, 0, reps)
eng = HipEngine(0)
dm = eng.msa_upload(msa)
for _ in range(2):
    match, both = eng.msa_boot_counts(dm, weights)
    plain = eng.msa_pair_counts(dm, symmetric=True)
eng.sync()
print("rows", n, "columns", n_cols, "replicates", reps, "weight planes", int(weights.max()).bit_length(), "code bits", dm.bits)
eng.close()
