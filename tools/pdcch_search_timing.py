#!/usr/bin/env python3
"""One timing of the blind PDCCH search (mi_lte_pdcch_search_run) next to the common-search-space receiver (mi_lte_pdcch_decode_run with
MI_LTE_PDCCH_PER_PORT_ESTIMATES) on the same grids in one process: 20 MHz, 2 ports, CFI 3, two DCI sizes, 4 096 subframes.  The grids are
`--unique` synthesised control regions (three C-RNTI DCIs each at L = 1 / 2 / 4 in their own search spaces plus one SI-RNTI format-1A-sized
DCI at L = 4 in the common one), repeated over the units.  Both calls are whole calls: launches, the wait and the results' way to the host.
No target: the two numbers and their ratio are what is recorded.

    python tools/pdcch_search_timing.py [--units 4096] [--steps 10] [--warmup 2] [--out profiles/pdcch_search_timing.txt]
Prints one JSON line last (and writes it to --out with a header)."""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import openlte_amd as m  # noqa: E402
from openlte_amd import synth  # noqa: E402

SIZES = (28, 43)  # format 1A / 0 at 20 MHz, and a format-2-sized payload


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--units", type=int, default=4096)
    ap.add_argument("--unique", type=int, default=16)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    n, nu, cell = args.units, args.unique, 17
    cfg = m.DlCfg(2048, 100, 2, 0)
    n_cce = m.load_library().mi_lte_get_n_cce(100, 13, 3, 2)
    rng = np.random.default_rng(1)
    sfs_u, recs, rntis = [u % 10 for u in range(nu)], [], [0xFFFF]
    for u in range(nu):
        lst, used = [(0xFFFF, 4, 0, SIZES[0], int(rng.integers(0, 1 << SIZES[0])))], {0, 1, 2, 3}
        for L in (1, 2, 4):
            for _ in range(50):
                rnti = int(rng.integers(0x3D, 0xFFF4))
                cce = m.pdcch_search_space(rnti, sfs_u[u], n_cce, L)[0]
                if not used & set(range(cce, cce + L)):
                    used |= set(range(cce, cce + L))
                    lst.append((rnti, L, cce, SIZES[L % 2], int(rng.integers(0, 1 << SIZES[L % 2]))))
                    rntis.append(rnti)
                    break
        recs.append(lst)
    g = synth.ctrl_grids_dci(cfg, sfs_u, [cell] * nu, [3] * nu, recs, snr_db=15.0, seed=3)
    ctx = m.Context(0)
    reps = -(-n // nu)
    d_g = ctx.to_device(np.ascontiguousarray(np.tile(g, (reps, 1, 1, 1))[:n]))
    d_sf, d_cell = ctx.to_device(np.asarray([sfs_u[u % nu] for u in range(n)], np.uint32)), ctx.to_device(np.full(n, cell, np.uint32))
    search = ctx.pdcch_search_plan(cfg, [cell], SIZES, rntis)
    common = ctx.pdcch_plan(cfg, [cell], 1.0, per_port_estimates=True)

    def run_search():
        return search.search_raw(d_g, d_sf, d_cell, n)

    def run_common():
        return common.decode_raw(d_g, d_sf, d_cell, n)

    for _ in range(args.warmup):
        run_search()
        run_common()
    ctx.sync()
    t_s, t_c = [], []
    for _ in range(args.steps):  # alternating, one call of each per step
        ctx.timer_start()
        run_search()
        t_s.append(ctx.timer_stop())
        ctx.timer_start()
        run_common()
        t_c.append(ctx.timer_stop())
    cfi, ncce, nf, found = run_search()
    sent_found = sum(1 for u in range(nu) for r in recs[u] if r in {found[16 * u + k].as_tuple()[:5] for k in range(min(int(nf[u]), 16))})
    ctx.profile(True)
    run_search()
    ctx.sync()
    split = {k: round(ms, 4) for k, (nl, ms) in sorted(ctx.profile_report().items(), key=lambda kv: -kv[1][1])}
    ctx.profile(False)
    ms_s, ms_c = float(np.median(t_s)), float(np.median(t_c))
    res = {"workload": "pdcch_search", "units": n, "unique": nu, "n_rb": 100, "n_ant": 2, "cfi": 3, "n_cce": int(ncce[0]), "sizes": list(SIZES), "n_rnti": len(rntis),
           "pairs_per_unit": int((ncce[0] // 8 + ncce[0] // 4 + ncce[0] // 2 + ncce[0]) * len(SIZES)), "steps": args.steps, "warmup": args.warmup,
           "search_ms": round(ms_s, 3), "common_ms": round(ms_c, 3), "search_us_per_subframe": round(1e3 * ms_s / n, 4),
           "common_us_per_subframe": round(1e3 * ms_c / n, 4), "search_over_common": round(ms_s / ms_c, 3),
           "search_ms_range": [round(min(t_s), 3), round(max(t_s), 3)], "common_ms_range": [round(min(t_c), 3), round(max(t_c), 3)],
           "search_kernel_ms": split, "cfi_ok": int((cfi == 3).sum()), "sent_found": sent_found, "sent": sum(len(r) for r in recs), "device": ctx.device_name}
    print("search %.4f us / subframe against the common-search-space receiver's %.4f (x %.2f)"
          % (res["search_us_per_subframe"], res["common_us_per_subframe"], res["search_over_common"]))
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write("# tools/pdcch_search_timing.py --units %d --steps %d --warmup %d on one MI355X (gfx950)\n" % (n, args.steps, args.warmup))
            f.write("# search_*: mi_lte_pdcch_search_run (every CCE-aligned candidate at L = 8, 4, 2, 1 x two DCI sizes); common_*: mi_lte_pdcch_decode_run\n")
            f.write("# (six common-search-space candidates x formats 1A, 1C) on the same grids, whole calls, alternating, medians.  No target.\n")
            f.write(line + "\n")
    for b in (d_g, d_sf, d_cell):
        b.free()
    search.close()
    common.close()
    ctx.close()
    return 0 if sent_found == sum(len(r) for r in recs) and (cfi == 3).all() else 1


if __name__ == "__main__":
    sys.exit(main())
