#!/bin/bash
# The kernel launcher's grid arithmetic, limit checks and value dispatch under AddressSanitizer + UBSan (a stand-alone CPU
# program; the header it tests needs no HIP runtime).
#   bash tests/tools/sanitize/run_launch_geom.sh
set -eu
HERE=$(cd "$(dirname "$0")" && pwd)
OUT=${TMPDIR:-/tmp}/pa_sanitize_launch_geom.$$
mkdir -p "$OUT"
FLAGS="-O1 -g -std=c++17 -Wall -Wextra -fsanitize=address,undefined -fno-omit-frame-pointer -fno-sanitize-recover=undefined"
g++ $FLAGS -o "$OUT/launch_geom" "$HERE/launch_geom.cpp"
"$OUT/launch_geom"
rm -rf "$OUT"
echo "sanitizer runs clean"
