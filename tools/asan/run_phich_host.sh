#!/bin/bash
# tools/asan/run_phich_host.sh: the PHICH host arithmetic (phich_geom.cc, with pdcch_geom.cc whose REG numbering it calls) built with
# g++ -fsanitize=address,undefined and walked by phich_host_driver.cc over the entry points' whole argument ranges.  CPU only.
set -e
cd "$(dirname "$0")/../.."
OUT=${TMPDIR:-/tmp}/mi_lte_asan_phich_host
g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined -fno-omit-frame-pointer -Wall -Iinclude tools/asan/phich_host_driver.cc \
    openlte_amd/csrc/phich_geom.cc openlte_amd/csrc/pdcch_geom.cc -o $OUT
ASAN_OPTIONS=detect_leaks=1 $OUT
