#!/bin/bash
# tools/asan/run_soft_pack.sh: the packed soft-bit hand-over's pure functions (openlte_amd/csrc/soft_pack.h, a header that compiles without HIP)
# built with g++ -fsanitize=address,undefined and checked against scalar statements of the format and of the staged copy (soft_pack_driver.cc).  CPU only.
set -e
cd "$(dirname "$0")/../.."
OUT=${TMPDIR:-/tmp}/mi_lte_asan_soft_pack
g++ -std=c++17 -O2 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined -fno-omit-frame-pointer -Wall tools/asan/soft_pack_driver.cc -o $OUT
ASAN_OPTIONS=detect_leaks=1 $OUT "$@"
