#!/usr/bin/env python3
"""One timing of k_phich_decode (mi_lte_phich_decode_run) at 4 096 units of 100 RB with N_g = 2 -- 25 groups, 300 gathered elements and 200
records a unit, the largest case -- for cells of 1, 2 and 4 ports, next to k_pdcch_decode (mi_lte_pdcch_decode_run, each port's own
estimate) on the same device subframes in the same process, for scale.  The subframes are the synthesiser's control regions (PCFICH, two
DCIs, smooth channels, noisy estimates at 10 dB) with every PHICH group filled by the float64 modulator of tests/phich_model.py through the
same estimates; 16 distinct units repeated over the batch, which is resident in HBM (0.3 / 0.5 / 0.8 MB a unit of which a decoder touches a
few KB).  The figures are kernel times -- the HIP events the library puts round each launch (mi_lte_profile_*) -- medians over repeated
calls, alternating, inside a time limit of the tool's own.  No target: the numbers are what is recorded.

    python tools/phich_timing.py [--units 4096] [--steps 20] [--warmup 2] [--time-limit 120] [--out profiles/phich_timing.txt]
Prints one JSON line last (and writes it to --out with a header)."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import openlte_amd as m  # noqa: E402
from openlte_amd import synth  # noqa: E402
import phich_model as pm  # noqa: E402

N_RB, N_G, BLOCK = 100, 2.0, 16


def host_block(n_ant, rng):
    """(grids float32 [16, 2 + 2 n_ant, 16, 1200], cells, subframes, present, hi)"""
    n_grp = pm.n_group(N_RB, 2)

    def clean(cell):  # the reference's REG numbering lets a PHICH REG land on a PCFICH REG in some cells: not those
        regs = [r for grp in range(n_grp) for r in pm.group_regs(N_RB, cell, grp)]
        return len(set(regs)) == len(regs) and not set(regs) & {int(x + 0.5) for x in pm.pcfich_reg_numbers(N_RB, cell)}
    cells, sfs = [c for c in ((37 * u + 5) % 504 for u in range(504)) if clean(c)][:BLOCK], [u % 10 for u in range(BLOCK)]
    cfg = m.DlCfg(2048, N_RB, n_ant, 0)
    g = synth.ctrl_grids(cfg, sfs, cells, [2] * BLOCK, [[(0xFFFF, 5, 4, 2, 0), (0xFFFE, 3, 3, 10, 0)]] * BLOCK, phich_res=N_G, snr_db=10.0, seed=7 + n_ant)
    present, hi = pm.random_pattern(rng, BLOCK, n_grp)
    for u in range(BLOCK):
        h = g[u, 2:2 + n_ant, 0].astype(np.float64) + 1j * g[u, 2 + n_ant:, 0]
        s = pm.scramble_signs(sfs[u], cells[u])
        for grp in range(n_grp):
            k = pm.group_res(N_RB, cells[u], grp)
            y = (h[:, k] * pm.modulate_group(n_ant, grp, present[u, grp], hi[u, grp], s)).sum(0)
            g[u, 0, 0, k], g[u, 1, 0, k] = y.real, y.imag  # (the synthesiser leaves the PHICH elements to noise: written over)
    return g, cells, sfs, present, hi


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--units", type=int, default=4096)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--time-limit", type=float, default=120.0, help="seconds for the timed loops; each ends early (after at least 3 steps) when its share is used up")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    n = (args.units + BLOCK - 1) // BLOCK * BLOCK
    rng = np.random.default_rng(1)
    ctx = m.Context(0)
    L = ctx.L
    out = {"workload": "phich_timing", "units": n, "n_rb_dl": N_RB, "n_g": N_G, "n_group": pm.n_group(N_RB, 2), "steps": {}, "warmup": args.warmup, "kernel_ms": {},
           "kernel_ms_range": {}, "us_per_4096_units": {}, "phich_over_pdcch": {}, "wrong_hi": {}, "pdcch_dcis_found": {}}
    for n_ant in (1, 2, 4):
        g, cells, sfs, present, hi = host_block(n_ant, rng)
        cfg = m.DlCfg(2048, N_RB, n_ant, 0)
        d_sub = ctx.alloc(n * g[0].nbytes)
        for b in range(n // BLOCK):
            d_sub.upload(g, b * g.nbytes)
        d_sf, d_cell = ctx.to_device(np.tile(np.asarray(sfs, np.uint32), n // BLOCK)), ctx.to_device(np.tile(np.asarray(cells, np.uint32), n // BLOCK))
        ph = ctx.phich_plan(cfg, sorted(set(cells)), phich_res=N_G)
        pd = ctx.pdcch_plan(cfg, sorted(set(cells)), phich_res=N_G, per_port_estimates=True)
        d_out = ctx.alloc(ph.out_bytes(n))

        def run_phich():
            ph.decode_dev(d_sub, d_sf, d_cell, n, d_out=d_out)
            ctx.sync()

        def run_pdcch():
            return pd.decode_raw(d_sub, d_sf, d_cell, n)

        runs = [("phich_%dport" % n_ant, "k_phich_decode", run_phich), ("pdcch_%dport" % n_ant, "k_pdcch_decode", run_pdcch)]
        for _ in range(args.warmup):
            for _, _, f in runs:
                f()
        ms = {name: [] for name, _, _ in runs}
        t0, steps = time.monotonic(), 0
        ctx.profile(True)
        while steps < args.steps and (steps < 3 or time.monotonic() - t0 < args.time_limit / 3):
            for name, kernel, f in runs:  # alternating, one call of each per step
                ctx._check(L.mi_lte_profile_reset(ctx.h))
                f()
                ms[name].append(ctx.profile_report()[kernel][1])
            steps += 1
        ctx.profile(False)
        rec = d_out.download(np.uint8, ph.out_bytes(n)).view(np.dtype(m.PhichResult)).reshape(n // BLOCK, BLOCK, -1, 8)
        on = np.broadcast_to(present == 1, rec["hi"].shape)
        n_dci = run_pdcch()[3]
        for name, v in ms.items():
            out["kernel_ms"][name] = round(float(np.median(v)), 4)
            out["kernel_ms_range"][name] = [round(min(v), 4), round(max(v), 4)]
            out["us_per_4096_units"][name] = round(1e3 * float(np.median(v)) * 4096 / n, 2)
        out["steps"]["%dport" % n_ant] = steps
        out["phich_over_pdcch"]["%dport" % n_ant] = round(float(np.median(ms["phich_%dport" % n_ant]) / np.median(ms["pdcch_%dport" % n_ant])), 4)
        out["wrong_hi"]["%dport" % n_ant] = int((rec["hi"][on] != np.broadcast_to(hi, rec["hi"].shape)[on]).sum())
        out["pdcch_dcis_found"]["%dport" % n_ant] = int(n_dci.sum())
        print("%d port(s): k_phich_decode %.1f us per 4 096 units, k_pdcch_decode %.1f us on the same subframes: x %.3f"
              % (n_ant, out["us_per_4096_units"]["phich_%dport" % n_ant], out["us_per_4096_units"]["pdcch_%dport" % n_ant], out["phich_over_pdcch"]["%dport" % n_ant]))
        ph.close()
        pd.close()
        for b in (d_sub, d_sf, d_cell, d_out):
            b.free()
    out["build_id"], out["device"] = L.mi_lte_build_id().decode(), ctx.device_name
    line = json.dumps(out)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write("# tools/phich_timing.py --units %d --steps %d --warmup %d on one MI355X (gfx950)\n" % (n, args.steps, args.warmup))
            f.write("# kernel_ms: medians of the event-bracketed kernel time of one call over all units, calls alternating; kernel_ms_range: smallest and\n")
            f.write("# largest.  phich_*: k_phich_decode, 100 RB, N_g = 2 (25 groups, 200 records a unit); pdcch_*: k_pdcch_decode on the same device\n")
            f.write("# subframes (each port's own estimate).  wrong_hi: decisions on sent indicators that differ from what was sent.  No target.\n")
            f.write(line + "\n")
    ctx.close()
    return 0 if not any(out["wrong_hi"].values()) else 1


if __name__ == "__main__":
    sys.exit(main())
