#!/bin/bash
# tools/asan/run_turbo_signs.sh: the sign-bit hand-over of the turbo trellis kernels (openlte_amd/csrc/turbo_swar.h: the sign words'
# layout and helpers, traceback_entry) built with g++ -fsanitize=address,undefined and checked against the byte form it replaces (turbo_signs_driver.cc).  CPU only.
set -e
cd "$(dirname "$0")/../.."
OUT=${TMPDIR:-/tmp}/mi_lte_asan_turbo_signs
g++ -std=c++17 -O2 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined -fno-omit-frame-pointer -Wall tools/asan/turbo_signs_driver.cc -o $OUT
ASAN_OPTIONS=detect_leaks=1 $OUT "$@"
