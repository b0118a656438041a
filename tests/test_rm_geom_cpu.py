"""The turbo rate-matching geometry every un-matching kernel gathers by (openlte_amd/csrc/rm_geom.h: K_mimo, the soft-buffer rule, RmGeom and
the index of the reference-mode rank tables) on the CPU: tools/asan/rm_geom_driver.cc holds it to the transmitter's own walk of the circular
buffer (tx::rate_match_turbo) under g++ -fsanitize=address,undefined.  No GPU, nothing loaded into Python."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_rm_geom_against_the_transmitter_under_address_and_undefined_behaviour_sanitizers():
    """With E = 2 Nnn + 37 (two laps and a partial one): every d element with a rank is what e[rank], e[rank + Nnn], .. carry in the
    transmitter's output, every e index below E is claimed exactly once, and an element outside N_cb claims none -- (a) at all 188 block sizes
    times the 12 rank tables through rm_combo / rm_combo_geom, termination rows included; (b) through rm_soft_buffer for K in {40, 48, 512,
    1008, 2048, 3136, 6144} x C in {1, 2, 5, 13} x N_soft in {250368, 1237248, 3667200, 40000, 3000} x M_dl_harq in {1, 4, 8} x tx_mode in
    {1, 3} x rv 0..3 (N_cb down to 14).  No case skipped, none differing, no sanitizer report."""
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    r = subprocess.run(["bash", os.path.join(ROOT, "tools", "asan", "run_rm_geom.sh")], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0 and "ERROR" not in r.stderr and "runtime error" not in r.stderr, (r.stdout + r.stderr)[-3000:]
    assert "MISMATCH" not in r.stdout, r.stdout[-2000:]
    m = re.search(r"rm geom driver: (\d+) sizes, (\d+) table cases \((\d+) limited, (\d+) comparisons\), (\d+) grid cases \((\d+) limited, "
                  r"(\d+) comparisons, smallest N_cb (\d+)\), (\d+) skipped, (\d+) differing", r.stdout)
    assert m, r.stdout[-1000:]
    sizes, table, lim_a, cmp_a, grid, lim_b, cmp_b, min_ncb, skipped, differing = map(int, m.groups())
    assert (sizes, table, grid, skipped, differing) == (188, 2256, 3360, 0, 0), r.stdout[-1000:]
    # both rules exercised: limited buffers in either part, and every e index of every case compared (sum of E over the cases)
    assert lim_a == 60 and lim_b == 1048 and min_ncb == 14 and cmp_a == 25531896 and cmp_b == 24138656, r.stdout[-1000:]
