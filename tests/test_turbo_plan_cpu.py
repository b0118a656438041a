"""The merged turbo decode's layout planner (openlte_amd/csrc/turbo_plan.cc) on the CPU: tools/asan/turbo_plan_driver.cc plans group lists and
replays the kernels' index expressions against the tables, under g++ -fsanitize=address,undefined.  No GPU, nothing loaded into Python."""
import os
import shutil
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N_RANDOM = 3000
N_FIXED = 188 * 6 + 187 * 36 + 2  # every size alone and every neighbouring pair with 1, 63, 64, 65, 4096, 4097 code blocks each; all sizes with 1 and 64


def bench_group_lists():
    """bench.py's two PDSCH batches of 65 536 subframes as the planner sees them: (K, code blocks, first slot, longest allocation's soft bits)
    per block size, ascending.  W4: eight 12-PRB and one 4-PRB 64QAM allocation per subframe (8192 and 1024 tiles); chain-mixed: the
    allocation lists of ChainMixedWorkload.draw_lists, unit i carrying list i mod 192."""
    if ROOT not in sys.path:
        sys.path.insert(0, ROOT)
    import bench
    per_prb = lambda cfi, mod: ((14 - cfi) * 12 - 6) * (2, 4, 6)[mod - 1]
    n = 65536
    w4 = {1064 + 24: (n, 4 * per_prb(2, 3)), 3240 + 24: (8 * n, 12 * per_prb(2, 3))}
    lists = bench.ChainMixedWorkload.draw_lists(bench.ChainMixedWorkload.N_UNIQUE, 0)
    mixed = {}
    for u, (_sf, _cell, cfi, lst) in enumerate(lists):
        times = n // len(lists) + (u < n % len(lists))
        for (mod, tbs, _p0, n_prb, _rnti, _rv) in lst:
            cnt, e = mixed.get(tbs + 24, (0, 0))
            mixed[tbs + 24] = (cnt + times, max(e, n_prb * per_prb(cfi, mod)))
    out = []
    for sizes in (w4, mixed):
        rows, base = [], 0
        for K in sorted(sizes):
            rows.append((K, sizes[K][0], base, sizes[K][1]))
            base += sizes[K][0]
        out.append(rows)
    return out


def test_merged_decode_plan_under_address_and_undefined_behaviour_sanitizers(tmp_path):
    """Every block size alone, neighbouring pairs around the tile and map granularities, all 188 sizes at once, the benchmark's W4 and mixed
    batches (the mixed one takes the dealt launch order) and 3000 seeded random lists: every code block, tile, tile pair and trellis is
    reached exactly once by the replayed prep / vote, perm, trellis and state-parallel launches, sizes keep to their own scratch, the
    descriptor kernel's bisection finds every slot's size, unsorted / empty / over-long lists are refused; no sanitizer report."""
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    w4, mixed = bench_group_lists()
    files = []
    for name, rows in (("w4", w4), ("chain_mixed", mixed)):
        files.append(str(tmp_path / ("groups_%s.txt" % name)))
        with open(files[-1], "w") as f:
            f.writelines("%d %d %d %d\n" % r for r in rows)
    assert [(r[1] + 63) // 64 for r in w4] == [1024, 8192] and len(mixed) >= 8 and sum((r[1] + 63) // 64 for r in mixed) >= 4 * 512
    r = subprocess.run(["bash", os.path.join(ROOT, "tools", "asan", "run_turbo_plan.sh"), str(N_RANDOM)] + files, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0 and "ERROR" not in r.stderr and "runtime error" not in r.stderr, (r.stdout + r.stderr)[-3000:]
    assert "turbo plan driver: %d plans checked" % (N_FIXED + 2 + N_RANDOM) in r.stdout, r.stdout[-1000:]
    dealt = int(r.stdout.split("plans checked, ")[1].split()[0])
    assert dealt >= 100, r.stdout[-1000:]  # the launch order's branch is exercised, not merely present
