#!/bin/bash
# The host twins of plot-run's distributions under AddressSanitizer + UBSan (a stand-alone CPU program).
#   bash tests/tools/sanitize/run_dist.sh [trials]
set -eu
HERE=$(cd "$(dirname "$0")" && pwd)
ROOT=$(cd "$HERE/../../.." && pwd)
OUT=${TMPDIR:-/tmp}/pa_sanitize_dist.$$
mkdir -p "$OUT"
TRIALS=${1:-2000}
FLAGS="-O1 -g -std=c++17 -ffp-contract=off -fsanitize=address,undefined -fno-omit-frame-pointer -fno-sanitize-recover=undefined"
g++ $FLAGS -I"$ROOT/include" -o "$OUT/dist_host" "$HERE/dist_host.cpp"
"$OUT/dist_host" "$TRIALS"
rm -rf "$OUT"
echo "sanitizer runs clean"
