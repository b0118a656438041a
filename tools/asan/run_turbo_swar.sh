#!/bin/bash
# tools/asan/run_turbo_swar.sh: the byte-parallel helpers of the turbo glue kernels (openlte_amd/csrc/turbo_swar.h, a header that compiles without
# HIP) built with g++ -fsanitize=address,undefined and checked against a scalar restatement of the reference's steps (turbo_swar_driver.cc).  CPU only.
set -e
cd "$(dirname "$0")/../.."
OUT=${TMPDIR:-/tmp}/mi_lte_asan_turbo_swar
g++ -std=c++17 -O2 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined -fno-omit-frame-pointer -Wall tools/asan/turbo_swar_driver.cc -o $OUT
ASAN_OPTIONS=detect_leaks=1 $OUT "$@"
