#!/bin/bash
# The host twin of plot-run's scatter figures under AddressSanitizer + UBSan (a stand-alone CPU program).
#   bash tests/tools/sanitize/run_scatter.sh [trials]
set -eu
HERE=$(cd "$(dirname "$0")" && pwd)
ROOT=$(cd "$HERE/../../.." && pwd)
OUT=${TMPDIR:-/tmp}/pa_sanitize_scatter.$$
mkdir -p "$OUT"
TRIALS=${1:-2000}
FLAGS="-O1 -g -std=c++17 -ffp-contract=off -Wno-unknown-pragmas -fsanitize=address,undefined -fno-omit-frame-pointer -fno-sanitize-recover=undefined"
g++ $FLAGS -I"$ROOT/include" -o "$OUT/scatter_host" "$HERE/scatter_host.cpp"
"$OUT/scatter_host" "$TRIALS"
rm -rf "$OUT"
echo "sanitizer runs clean"
