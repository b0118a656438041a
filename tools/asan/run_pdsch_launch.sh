#!/bin/bash
# tools/asan/run_pdsch_launch.sh [query file]: the PDSCH demodulators' launch rule (openlte_amd/csrc/pdsch_launch.h, pure host code) built with
# g++ -fsanitize=address,undefined and asked query by query (pdsch_launch_driver.cc; queries from the file or from stdin).  CPU only.
set -e
cd "$(dirname "$0")/../.."
OUT=${TMPDIR:-/tmp}/mi_lte_asan_pdsch_launch
g++ -std=c++17 -O2 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined -fno-omit-frame-pointer -Wall tools/asan/pdsch_launch_driver.cc -o $OUT
ASAN_OPTIONS=detect_leaks=1 $OUT "$@"
