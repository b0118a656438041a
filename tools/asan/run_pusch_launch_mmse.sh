#!/bin/bash
# tools/asan/run_pusch_launch_mmse.sh [query file]: run_pusch_launch.sh for the driver's eight-field form (--mmse: the queries carry the plan's
# equaliser behind threads_override), built with g++ -fsanitize=address,undefined and asked query by query.  CPU only.
set -e
cd "$(dirname "$0")/../.."
OUT=${TMPDIR:-/tmp}/mi_lte_asan_pusch_launch_mmse
g++ -std=c++17 -O2 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined -fno-omit-frame-pointer -Wall tools/asan/pusch_launch_driver.cc -o $OUT
ASAN_OPTIONS=detect_leaks=1 $OUT --mmse "$@"
