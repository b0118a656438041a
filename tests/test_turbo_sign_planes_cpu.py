"""The layout of the trellis kernels' sign words -- per code block, by plane (turbo_swar.h, "the trellis kernels' sign words") -- checked by
the stand-alone CPU driver tools/asan/turbo_signs_driver.cc, built with plain g++ -fsanitize=address,undefined and run as a subprocess
(nothing is loaded into this interpreter)."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_sign_plane_layout_under_address_and_undefined_behaviour_sanitizers():
    """The driver's fourth part: the bit map is a permutation of the 32 positions and is the definition (step 4 w + b -> bit 8 b + w);
    packing the lock-step kernel's way (traceback_entry values in traceback order, an accumulator per byte pair) equals packing the
    state-parallel kernel's way (a step-ordered 64-bit mask) for 100 000 masks; and expanding a unit at every position u % 4 = 0..3 the way
    perm and vote do equals the step-by-step traceback's joined bytes -- the halo across a word and across a 64-step block, the first unit's
    preset, magnitude 0 under a set sign bit, last blocks of 8, 40 and 56 steps.  No mismatch, no sanitizer report."""
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    r = subprocess.run(["bash", os.path.join(ROOT, "tools", "asan", "run_turbo_signs.sh")], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "ERROR" not in r.stderr and "runtime error" not in r.stderr, (r.stdout + r.stderr)[-3000:]
    assert "MISMATCH" not in r.stdout and " 0 mismatches" in r.stdout, r.stdout[-2000:]
    m = re.search(r"sign planes: units per position u % 4: (\d+) (\d+) (\d+) (\d+); halo across a word (\d+), across a block (\d+), preset (\d+); "
                  r"magnitude 0 under a set sign (\d+)", r.stdout)
    assert m, r.stdout[-1000:]
    assert all(int(v) > 0 for v in m.groups()), m.group(0)  # every case of the expansion occurred
    checked = int(r.stdout.split("turbo signs driver: ")[1].split()[0])
    # part 1 (exhaustive + random), part 2, part 3's words (4000 blocks x 8 units x >= 4 words) and part 4's 100 000 masks x 3 checks
    assert checked >= 16 * 4 * 128 + 1000000 + 5 * 2048 + 4000 * 8 * 4 + 3 * 100000, r.stdout[-1000:]
