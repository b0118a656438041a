#!/bin/bash
# tools/asan/run_rm_geom.sh: the turbo rate-matching geometry (openlte_amd/csrc/rm_geom.h, a header that compiles without HIP) built with
# g++ -fsanitize=address,undefined and held to the transmitter's walk of the circular buffer (tx::rate_match_turbo; the sources tx.cc needs
# are tools/asan/run.sh's) at every block size and rank table and on a grid of soft-buffer sizes (rm_geom_driver.cc).  CPU only.
set -e
cd "$(dirname "$0")/../.."
OUT=${TMPDIR:-/tmp}/mi_lte_asan_rm_geom
g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined -fno-omit-frame-pointer -Wall -Iinclude tools/asan/rm_geom_driver.cc \
    openlte_amd/csrc/tx.cc openlte_amd/csrc/tx_ctrl.cc openlte_amd/csrc/tx_ul.cc openlte_amd/csrc/sched.cc openlte_amd/csrc/synth.cc openlte_amd/csrc/ul_rs.cc openlte_amd/csrc/pdcch_geom.cc -o $OUT
ASAN_OPTIONS=detect_leaks=1 $OUT "$@"
