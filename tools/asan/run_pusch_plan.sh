#!/bin/bash
# tools/asan/run_pusch_plan.sh [query file]: the host half of the PUSCH plans and of the 3GPP transport-block mode (openlte_amd/csrc/pusch_plan.cc,
# dlsch3_layout.cc, plan_arith.cc, ulsch_host.cc and what they call -- pure host code, no HIP library) built with g++ -fsanitize=address,undefined
# and asked query by query (pusch_plan_driver.cc; queries from the file or from stdin).  CPU only.  NOSAN=1: the same build without the
# sanitizers, for a query whose plan has hundreds of thousands of allocations.
set -e
cd "$(dirname "$0")/../.."
OUT=${TMPDIR:-/tmp}/mi_lte_asan_pusch_plan${NOSAN:+_nosan}
SAN="-fsanitize=address,undefined -fno-sanitize-recover=undefined"
[ -z "$NOSAN" ] || SAN=""
g++ -std=c++17 -O2 -g $SAN -fno-omit-frame-pointer -Wall -Iinclude tools/asan/pusch_plan_driver.cc \
    openlte_amd/csrc/pusch_plan.cc openlte_amd/csrc/dlsch3_layout.cc openlte_amd/csrc/plan_arith.cc openlte_amd/csrc/ulsch_host.cc \
    openlte_amd/csrc/synth.cc openlte_amd/csrc/ul_rs.cc -o $OUT
ASAN_OPTIONS=detect_leaks=1 $OUT "$@"
