"""Lean harness for the rocprofv3 --pmc passes of mantel-run-comp's cross kernel: two calls of one device batch each,
no other kernels but the call's own.  Usage on the GPU machine, one counter group a process and no tracing beside it:
    rocprofv3 --pmc SQ_LDS_BANK_CONFLICT SQ_LDS_IDX_ACTIVE --kernel-include-regex mantel_cross_kernel \
        --output-format csv -d out/lds -- python3 tools/mantel_pmc.py [n_genomes] [permutations]
``tools/pmc_summary.py out mantel_cross`` then prints the mean of each counter per dispatch.
"""
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
sys.path.insert(0, str(Path(__file__).resolve().parent))
from mantel_bench import PERMUTATION_SEED, distance_pair  # noqa: E402

from pyani_plus_amd.engine import HipEngine, mantel_permutations  # noqa: E402

n = int(sys.argv[1]) if len(sys.argv) > 1 else 1000
count = int(sys.argv[2]) if len(sys.argv) > 2 else 255
X, Y = distance_pair(n)
perms = mantel_permutations(PERMUTATION_SEED, n, 0, count)
eng = HipEngine(0)
t = eng.torch
d_x, d_y = t.from_numpy(X).to(eng.device), t.from_numpy(Y).to(eng.device)
for _ in range(2):
    stats, cross = eng.mantel(d_x, d_y, perms)
print("genomes", n, "permutations", count, "observed cross sum", cross[0])
eng.close()
