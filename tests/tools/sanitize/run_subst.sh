#!/bin/bash
# The host side of phylo-run under AddressSanitizer + UBSan (a stand-alone CPU program).
#   bash tests/tools/sanitize/run_subst.sh [trials]
set -eu
HERE=$(cd "$(dirname "$0")" && pwd)
ROOT=$(cd "$HERE/../../.." && pwd)
OUT=${TMPDIR:-/tmp}/pa_sanitize_subst.$$
mkdir -p "$OUT"
TRIALS=${1:-300}
FLAGS="-O1 -g -std=c++17 -ffp-contract=off -fsanitize=address,undefined -fno-omit-frame-pointer -fno-sanitize-recover=undefined"
g++ $FLAGS -I"$ROOT/include" -o "$OUT/subst_host" "$HERE/subst_host.cpp" -lpthread
"$OUT/subst_host" "$TRIALS"
rm -rf "$OUT"
echo "sanitizer runs clean"
