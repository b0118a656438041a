"""The packed soft-bit hand-over between PDSCH demodulation and turbo prep (openlte_amd/csrc/soft_pack.h) on the CPU: tools/asan/soft_pack_driver.cc
restates the demodulator's packing loop and prep's two staging loops around the header's functions and checks them against scalar statements of
the format under g++ -fsanitize=address,undefined.  No GPU, nothing loaded into Python."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_soft_pack_under_address_and_undefined_behaviour_sanitizers():
    """Every nibble's four bytes; pack then expand for Q_m = 4 and 6 at every length of 1..300 symbols and around multiples of 32 and 128 bits up
    to the longest allocation (all-clear, all-set and random masks, junk behind the last symbol): bit n of the slot is soft bit n, every dword is
    written once and none behind the last, the tail bits are 0; the staged copy is the byte form's with zeros from E to the next 16-byte boundary,
    whole and lap by lap from arbitrary lap starts, on blocks of exactly the size the kernels may touch.  No mismatch, no sanitizer report."""
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    r = subprocess.run(["bash", os.path.join(ROOT, "tools", "asan", "run_soft_pack.sh")], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0 and "ERROR" not in r.stderr and "runtime error" not in r.stderr, (r.stdout + r.stderr)[-3000:]
    assert "MISMATCH" not in r.stdout and " 0 mismatches" in r.stdout, r.stdout[-2000:]
    assert int(r.stdout.split("soft pack driver: ")[1].split()[0]) >= 10 ** 6, r.stdout[-1000:]
