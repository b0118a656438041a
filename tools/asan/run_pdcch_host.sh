#!/bin/bash
# tools/asan/run_pdcch_host.sh: the PDCCH host arithmetic (dci.cc, pdcch_geom.cc, pdcch_synth.cc and the transmit-side files whose coding steps they call) built
# with g++ -fsanitize=address,undefined and walked by pdcch_host_driver.cc, which also checks round trips and index ranges itself.  CPU only.
set -e
cd "$(dirname "$0")/../.."
OUT=${TMPDIR:-/tmp}/mi_lte_asan_pdcch_host
g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined -fno-omit-frame-pointer -Wall -Iinclude tools/asan/pdcch_host_driver.cc \
    openlte_amd/csrc/dci.cc openlte_amd/csrc/pdcch_geom.cc openlte_amd/csrc/pdcch_synth.cc openlte_amd/csrc/tx.cc openlte_amd/csrc/sched.cc openlte_amd/csrc/synth.cc -o $OUT
ASAN_OPTIONS=detect_leaks=1 $OUT
