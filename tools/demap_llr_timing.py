#!/usr/bin/env python3
"""What the max-log soft-decision demapper costs: k_pdsch_demod_llr (MI_LTE_DEMAP_MAXLOG, automatic and fixed gain) next to k_pdsch_demod, the
default demapper, on the same 3GPP plan -- W4 (8 x 12 PRB + 1 x 4 PRB, 64QAM, 100 RB) over --units subframes, the planes of 16 synthesised
units tiled -- in one process, the three alternating.  The figures are kernel times: the HIP events the library puts round each launch
(mi_lte_profile_*), medians over --steps runs of the whole plan inside a time limit of the tool's own.  --parent-pkg DIR (a directory that holds
the `openlte_amd` package of the parent commit with its built library) times k_pdsch_demod of that library on the same input in a child
process started by the same call: the yardstick the comparison is against.  No target: the numbers are what is recorded.

    python tools/demap_llr_timing.py [--units 1024] [--steps 20] [--warmup 2] [--time-limit 120] [--parent-pkg DIR] [--out profiles/demap_llr_timing.txt]
Prints one JSON line last (and writes it to --out with a header)."""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N_SOFT, CFI, SEED_UNITS = 1237248, 2, 16


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--units", type=int, default=1024)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--time-limit", type=float, default=120.0, help="seconds for the timed loop; it ends early (after at least 3 steps) when they are used up")
    ap.add_argument("--parent-pkg", default=None)
    ap.add_argument("--pkg", default=None, help="(the child of --parent-pkg) import openlte_amd from here and time the default demapper alone")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    sys.path.insert(0, args.pkg or ROOT)
    import openlte_amd as m
    from openlte_amd import synth
    ref_only = args.pkg is not None
    n = args.units
    cfg = m.DlCfg(2048, 100, 1, 0)

    def w4(u):
        return [m.make_alloc(u, 3, 3240 if a < 8 else 1064, list(range(a * 12, a * 12 + 12)) if a < 8 else list(range(96, 100)), 0x100 + a) for a in range(9)]

    sfs16, cells16 = [u % 10 for u in range(SEED_UNITS)], [(31 * u + 7) % 504 for u in range(SEED_UNITS)]
    iq, _ = synth.dl_units_3gpp(cfg, sfs16, cells16, [a for u in range(SEED_UNITS) for a in w4(u)], 9, N_SOFT, n_pdcch_symbs=CFI, snr_db=15.0,
                                max_delay=4, seed=77)
    ctx = m.Context(0)
    d_iq, d_start = ctx.to_device(iq.reshape(-1, 2)), ctx.to_device((np.arange(SEED_UNITS) * iq.shape[1]).astype(np.uint64))
    d_sf16, d_cell16 = ctx.to_device(np.asarray(sfs16, np.uint32)), ctx.to_device(np.asarray(cells16, np.uint32))
    d_sub16 = ctx.alloc(SEED_UNITS * ctx.subframe_floats(1) * 4)
    ctx.dl_frontend_dev(cfg, d_iq, None, d_start, d_sf16, d_cell16, SEED_UNITS, d_sub16)
    planes = d_sub16.download(np.float32).reshape(SEED_UNITS, -1)
    for b in (d_iq, d_start, d_sf16, d_cell16, d_sub16):
        b.free()
    reps = (n + SEED_UNITS - 1) // SEED_UNITS
    d_sub = ctx.to_device(np.tile(planes, (reps, 1))[:n])
    sfs, cells = (sfs16 * reps)[:n], (cells16 * reps)[:n]
    d_sf, d_cell = ctx.to_device(np.asarray(sfs, np.uint32)), ctx.to_device(np.asarray(cells, np.uint32))
    plan = ctx.pdsch_plan_3gpp(cfg, CFI, [a for u in range(n) for a in w4(u)], N_SOFT)
    d_out, d_st = ctx.alloc(plan.n_alloc * plan.out_stride), ctx.alloc(4 * plan.n_alloc)

    def run(mode, gain):
        if not ref_only:
            plan.set_demapper(mode, gain)
        plan.run_dev(d_sub, d_sf, d_cell, d_out, d_st)
        ctx.sync()

    if ref_only:
        runs = [("ref", "k_pdsch_demod", lambda: run(0, 0.0))]
    else:
        run(m.DEMAP_MAXLOG, 0.0)
        fixed = float(plan.llr_gain().mean())
        runs = [("ref", "k_pdsch_demod", lambda: run(m.DEMAP_REF, 0.0)), ("maxlog_auto", "k_pdsch_demod_llr", lambda: run(m.DEMAP_MAXLOG, 0.0)),
                ("maxlog_fixed", "k_pdsch_demod_llr", lambda: run(m.DEMAP_MAXLOG, fixed))]
    for _ in range(args.warmup):
        for _, _, f in runs:
            f()
    ms = {name: [] for name, _, _ in runs}
    ok = {}
    t0, steps = time.monotonic(), 0
    ctx.profile(True)
    while steps < args.steps and (steps < 3 or time.monotonic() - t0 < args.time_limit):
        for name, kernel, f in runs:  # alternating, one run of each per step
            ctx._check(ctx.L.mi_lte_profile_reset(ctx.h))
            f()
            ms[name].append(ctx.profile_report()[kernel][1])
            ok[name] = int((d_st.download(np.int32) == 0).sum())
        steps += 1
    ctx.profile(False)
    med = {k: float(np.median(v)) for k, v in ms.items()}
    n_re = 100 * (12 * (14 - CFI) - 6)  # resource elements per unit (a subframe without PBCH / sync signals)
    out = {"workload": "demap_llr_timing", "units": n, "allocations": plan.n_alloc, "steps": steps, "warmup": args.warmup,
           "kernel_ms": {k: round(v, 4) for k, v in med.items()}, "kernel_ms_range": {k: [round(min(v), 4), round(max(v), 4)] for k, v in ms.items()},
           "ns_per_allocation": {k: round(1e6 * v / plan.n_alloc, 2) for k, v in med.items()}, "decoded": ok,
           "plane_GBps": {k: round(n * n_re * 16 / (v * 1e6), 1) for k, v in med.items()},
           "build_id": m.load_library().mi_lte_build_id().decode(), "device": ctx.device_name}
    if not ref_only:
        out["maxlog_auto_over_ref"] = round(med["maxlog_auto"] / med["ref"], 3)
        out["maxlog_fixed_over_ref"] = round(med["maxlog_fixed"] / med["ref"], 3)
    for b in (d_sub, d_sf, d_cell, d_out, d_st):
        b.free()
    plan.close()
    ctx.close()
    if args.parent_pkg:
        child = subprocess.run([sys.executable, os.path.abspath(__file__), "--pkg", args.parent_pkg, "--units", str(n), "--steps", str(args.steps),
                                "--warmup", str(args.warmup), "--time-limit", str(args.time_limit)], capture_output=True, text=True, timeout=600)
        if child.returncode != 0:
            print(child.stdout[-2000:], child.stderr[-2000:])
            return 1
        parent = json.loads(child.stdout.strip().splitlines()[-1])
        out["parent_library"] = {k: parent[k] for k in ("kernel_ms", "kernel_ms_range", "build_id", "decoded")}
        pm = parent["kernel_ms"]["ref"]
        out["ref_over_parent_ref"] = round(med["ref"] / pm, 3)
        out["maxlog_auto_over_parent_ref"] = round(med["maxlog_auto"] / pm, 3)
        out["maxlog_fixed_over_parent_ref"] = round(med["maxlog_fixed"] / pm, 3)
    line = json.dumps(out)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write("# tools/demap_llr_timing.py --units %d --steps %d --warmup %d%s on one MI355X (gfx950)\n"
                    % (n, args.steps, args.warmup, " --parent-pkg <the parent commit's package>" if args.parent_pkg else ""))
            f.write("# kernel_ms: medians of the event-bracketed kernel time of one plan run (W4: 9 allocations per unit, 64QAM), runs alternating.\n")
            f.write("# ref: k_pdsch_demod, the default demapper; maxlog_auto / maxlog_fixed: k_pdsch_demod_llr with the automatic gain (a first sweep over the\n")
            f.write("# estimate planes for the mean channel power) and with a fixed one.  parent_library: k_pdsch_demod of the parent commit's library on the\n")
            f.write("# same input, in a child process of the same call.  plane_GBps: 16 bytes per resource element over the kernel time.  No target.\n")
            f.write(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
