#!/usr/bin/env python3
"""One timing of k_pucch2_decode (PUCCH formats 2 / 2a / 2b, mi_lte_pucch2_decode_run) at 65 536 resources, A = 1, 4 and 13 information bits,
next to k_pucch_decode (formats 1 / 1a / 1b, mi_lte_pucch_decode_run) on the same resource count and the same grids, in one process.  The
figures are kernel times -- the HIP events the library puts round each launch (mi_lte_profile_*) -- so the staging copies of either call
are left out; medians over repeated calls, alternating, inside a time limit of the tool's own.  A = 1 runs one coset of the search, A = 13
all 128: their difference is what the exhaustive search costs.  No target: the numbers are what is recorded.

    python tools/pucch2_timing.py [--resources 65536] [--steps 20] [--warmup 2] [--time-limit 120] [--out profiles/pucch2_timing.txt]
Prints one JSON line last (and writes it to --out with a header)."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import openlte_amd as m  # noqa: E402
from openlte_amd.lib import PucchRes  # noqa: E402

N_RB_UL, CELL, N_UNITS = 100, 17, 16


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--resources", type=int, default=65536)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--time-limit", type=float, default=120.0, help="seconds for the timed loop; it ends early (after at least 3 steps) when they are used up")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    n, rng = args.resources, np.random.default_rng(1)
    ul = m.UlCfg(0, 0, 0, 0, 0)
    L = m.load_library()
    # 16 units: eight format-2 UEs each (n2 over two blocks and the mixed one) at 10 dB; the format-1 decoder reads the same grids
    n2s, sfs = [0, 5, 11, 12, 17, 23, 24, 30], [u % 10 for u in range(N_UNITS)]
    tabs, tab_of, grids = [], {}, np.zeros((N_UNITS, 2, 16, 1200), np.float32)
    for u in range(N_UNITS):
        for i, n2 in enumerate(n2s):
            if (sfs[u], n2) not in tab_of:
                tab_of[(sfs[u], n2)] = len(tabs)
                tabs.append(m.pucch2_table(ul, CELL, sfs[u], N_RB_UL, n2, 2, 3, 0x100 + i))
            g = m.pucch2_modulate(tabs[tab_of[(sfs[u], n2)]], i % 3, m.pucch2_encode(13, rng.integers(0, 2, 13)), [i & 1, (i >> 1) & 1])
            grids[u, :, :14] += g
    grids[:, :, :14] += (10 ** (-10 / 20) / np.sqrt(2) * rng.standard_normal((N_UNITS, 2, 14, 1200))).astype(np.float32)
    ctx = m.Context(0)
    d_sub = ctx.to_device(grids)
    d_out = ctx.alloc(64 * n)
    res = {A: (m.Pucch2Res * n)(*[m.Pucch2Res(r % N_UNITS, r % 3, tab_of[(sfs[r % N_UNITS], n2s[(r // N_UNITS) % len(n2s)])], A) for r in range(n)]) for A in (1, 4, 13)}
    tarr = (m.Pucch2Tab * len(tabs))(*tabs)
    # the yardstick: format 1 / 1a / 1b resources N_1_p = 0 .. 3, the tables of their subframe
    t1 = np.zeros((N_UNITS, 4, 352), np.float32)
    for u in range(N_UNITS):
        for n1 in range(4):
            assert L.mi_lte_ul_pucch_tables(C.byref(ul), CELL, sfs[u], n1, 0, 1, 1, C.c_void_p(t1[u, n1].ctypes.data)) == 0
    res1 = (PucchRes * n)(*[PucchRes(r % N_UNITS, r % 3, (r // N_UNITS) % 4) for r in range(n)])
    tab1 = np.ascontiguousarray(t1[np.arange(n) % N_UNITS, (np.arange(n) // N_UNITS) % 4]).reshape(-1)
    bits1, nb1, rc1 = np.zeros(2 * n, np.uint8), np.zeros(n, np.uint32), np.zeros(n, np.uint32)

    def run2(A):
        ctx._check(L.mi_lte_pucch2_decode_run(ctx.h, N_RB_UL, d_sub.ptr, N_UNITS, res[A], n, tarr, len(tabs), d_out.ptr))
        ctx.sync()

    def run1():
        ctx._check(L.mi_lte_pucch_decode_run(ctx.h, N_RB_UL, 1, d_sub.ptr, res1, tab1, n, bits1, nb1, rc1))

    runs = [("pucch2_A1", "k_pucch2_decode", lambda: run2(1)), ("pucch2_A4", "k_pucch2_decode", lambda: run2(4)),
            ("pucch2_A13", "k_pucch2_decode", lambda: run2(13)), ("pucch1", "k_pucch_decode", run1)]
    for _ in range(args.warmup):
        for _, _, f in runs:
            f()
    ms = {name: [] for name, _, _ in runs}
    t0, steps = time.monotonic(), 0
    ctx.profile(True)
    while steps < args.steps and (steps < 3 or time.monotonic() - t0 < args.time_limit):
        for name, kernel, f in runs:  # alternating, one call of each per step
            ctx._check(L.mi_lte_profile_reset(ctx.h))
            f()
            ms[name].append(ctx.profile_report()[kernel][1])
        steps += 1
    ctx.profile(False)
    rec = np.frombuffer(d_out.download(np.uint8, 64 * n).tobytes(), np.dtype(m.Pucch2Result))  # (the last pucch2 call: A = 13)
    med = {k: float(np.median(v)) for k, v in ms.items()}
    out = {"workload": "pucch2_timing", "resources": n, "units": N_UNITS, "n_rb_ul": N_RB_UL, "n_tab": len(tabs), "steps": steps, "warmup": args.warmup,
           "kernel_ms": {k: round(v, 4) for k, v in med.items()}, "kernel_ms_range": {k: [round(min(v), 4), round(max(v), 4)] for k, v in ms.items()},
           "ns_per_resource": {k: round(1e6 * v / n, 2) for k, v in med.items()},
           "search_share_A13": round((med["pucch2_A13"] - med["pucch2_A1"]) / med["pucch2_A13"], 3),
           "pucch2_A13_over_pucch1": round(med["pucch2_A13"] / med["pucch1"], 3), "pucch2_A4_over_pucch1": round(med["pucch2_A4"] / med["pucch1"], 3),
           "decided_A13": int((rec["A"] == 13).sum()), "build_id": L.mi_lte_build_id().decode(), "device": ctx.device_name}
    print("k_pucch2_decode %.2f (A = 1) / %.2f (A = 4) / %.2f (A = 13) ns a resource against k_pucch_decode's %.2f; the search is %.0f %% of the A = 13 kernel"
          % (out["ns_per_resource"]["pucch2_A1"], out["ns_per_resource"]["pucch2_A4"], out["ns_per_resource"]["pucch2_A13"], out["ns_per_resource"]["pucch1"],
             100 * out["search_share_A13"]))
    line = json.dumps(out)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write("# tools/pucch2_timing.py --resources %d --steps %d --warmup %d on one MI355X (gfx950)\n" % (n, args.steps, args.warmup))
            f.write("# kernel_ms: medians of the event-bracketed kernel time of one call (staging copies left out), calls alternating.  pucch2_A*:\n")
            f.write("# k_pucch2_decode with A information bits (2^A words searched per wavefront); pucch1: k_pucch_decode, formats 1 / 1a / 1b, on the\n")
            f.write("# same grids and resource count.  search_share_A13 = (A13 - A1) / A13: what the 127 further cosets of the search cost.  No target.\n")
            f.write(line + "\n")
    for b in (d_sub, d_out):
        b.free()
    ctx.close()
    return 0 if out["decided_A13"] == n else 1


if __name__ == "__main__":
    sys.exit(main())
