"""The byte-parallel helpers of the turbo glue kernels (openlte_amd/csrc/turbo_swar.h) on the CPU: tools/asan/turbo_swar_driver.cc checks them
against a scalar restatement of the reference's steps under g++ -fsanitize=address,undefined.  No GPU, nothing loaded into Python."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_swar_helpers_under_address_and_undefined_behaviour_sanitizers():
    """Every (a, b) of soft_xor / Step 3 / Step 11 and every (A, B, G) of Step 10 in [-127, 127] (16.6 M triples), four per word with unlike
    neighbours; whole blocks with halo through the feedback, Steps 3, 10, 11 and the two nine-bit sums the way perm and vote walk a unit:
    random values, blocks full of 0 and +-1, saturated ones, the first unit's +127 preset, last units of eight valid values with junk
    behind them.  No mismatch, no sanitizer report."""
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    r = subprocess.run(["bash", os.path.join(ROOT, "tools", "asan", "run_turbo_swar.sh")], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0 and "ERROR" not in r.stderr and "runtime error" not in r.stderr, (r.stdout + r.stderr)[-3000:]
    assert "MISMATCH" not in r.stdout and " 0 mismatches" in r.stdout, r.stdout[-2000:]
    checked = int(r.stdout.split("turbo swar driver: ")[1].split()[0])
    assert checked >= 255 ** 3 + 3 * 255 * 255, r.stdout[-1000:]  # the exhaustive parts ran in full
