"""The sign-bit hand-over between the trellis kernels and perm / vote (turbo_swar.h) as a stand-alone CPU program under the address and
undefined-behaviour sanitizers (tools/asan/turbo_signs_driver.cc, run as a subprocess; nothing is loaded into this interpreter)."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_sign_bit_helpers_under_address_and_undefined_behaviour_sanitizers():
    """joined_from_bits against joined_from (every nibble x byte position x magnitude, a million random words, magnitude 0 under a set sign
    bit), the sign bits of all 2048 traceback table entries against the byte masks of the entry function they replace, and the pack-and-
    expand round trip of 64-step blocks (full, and last blocks of 8, 40 and 56 steps) against the step-by-step traceback.  No mismatch, no
    sanitizer report."""
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    r = subprocess.run(["bash", os.path.join(ROOT, "tools", "asan", "run_turbo_signs.sh")], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "ERROR" not in r.stderr and "runtime error" not in r.stderr, (r.stdout + r.stderr)[-3000:]
    assert "MISMATCH" not in r.stdout and " 0 mismatches" in r.stdout, r.stdout[-2000:]
    checked = int(r.stdout.split("turbo signs driver: ")[1].split()[0])
    assert checked >= 16 * 4 * 128 + 1000000 + 5 * 2048, r.stdout[-1000:]  # the exhaustive parts ran in full
