#!/bin/bash
# The workspace carver's offsets, alignments and refusals under AddressSanitizer + UBSan (a stand-alone CPU program; the
# header it tests needs no HIP runtime).
#   bash tests/tools/sanitize/run_carve.sh
set -eu
HERE=$(cd "$(dirname "$0")" && pwd)
OUT=${TMPDIR:-/tmp}/pa_sanitize_carve.$$
mkdir -p "$OUT"
FLAGS="-O1 -g -std=c++17 -Wall -Wextra -fsanitize=address,undefined -fno-omit-frame-pointer -fno-sanitize-recover=undefined"
g++ $FLAGS -o "$OUT/carve" "$HERE/carve.cpp"
"$OUT/carve"
rm -rf "$OUT"
echo "sanitizer runs clean"
