#!/bin/bash
# tools/asan/run_turbo_plan.sh [random lists] [group file ...]: the merged turbo decode's layout planner (turbo_plan.cc, pure host code) built with
# g++ -fsanitize=address,undefined and checked against a replay of the kernels' index expressions (turbo_plan_driver.cc).  CPU only.
set -e
cd "$(dirname "$0")/../.."
OUT=${TMPDIR:-/tmp}/mi_lte_asan_turbo_plan
g++ -std=c++17 -O2 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined -fno-omit-frame-pointer -Wall -Iinclude tools/asan/turbo_plan_driver.cc \
    openlte_amd/csrc/turbo_plan.cc -o $OUT
ASAN_OPTIONS=detect_leaks=1 $OUT "$@"
