#!/usr/bin/env python3
"""What the 3GPP PUSCH plans' max-log soft-decision demapper costs: k_pusch_demod_llr (MI_LTE_DEMAP_MAXLOG, automatic and fixed gain, symbol tap
off) next to k_pusch_demod<.., SPEC = true>, the default demapper, on the same 3GPP plan, in one process, the three alternating.  Shapes, all
on a 100-RB cell over --units subframes (the planes of 16 synthesised units tiled): W5's (16 UEs x 6 PRB per subframe; the 192-thread
instantiation, all twelve symbols side by side) as QPSK, the workload's modulation, and as 64QAM, and one 96-PRB 64QAM allocation per
subframe (256 threads, two symbols at a time).  The figures are kernel times: the HIP events the library puts round each launch
(mi_lte_profile_*), medians over --steps runs of the whole plan inside a time limit of the tool's own.  --parent-pkg DIR (a directory that
holds the `openlte_amd` package of the parent commit with its built library) times k_pusch_demod of that library on the same input in a
child process started by the same call: the yardstick the comparison is against.  No target: the numbers are what is recorded.

    python tools/pusch_llr_timing.py [--units 2048] [--steps 20] [--warmup 2] [--time-limit 60] [--parent-pkg DIR] [--out profiles/pusch_llr_timing.txt]
Prints one JSON line last (and writes it to --out with a header)."""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED_UNITS, ULC = 16, (3, 0, 0, 2, 5)
# name -> (mod_type, I_TBS, N_prb, allocations per subframe)
SHAPES = {"w5_qpsk": (1, 5, 6, 16), "w5_64qam": (3, 22, 6, 16), "prb96_64qam": (3, 22, 96, 1)}


def time_shape(m, synth, ctx, name, n, args, ref_only):
    mod, itbs, n_prb, per = SHAPES[name]
    cfg, ul = m.DlCfg(2048, 100, 1, 0), m.UlCfg(*ULC)
    size = int(m.load_library().mi_lte_tbs(itbs, n_prb))

    def allocs(u):
        return [m.make_alloc(u, mod, size, list(range(n_prb * a, n_prb * a + n_prb)), 0x100 + a) for a in range(per)]

    sfs16, cell = [u % 10 for u in range(SEED_UNITS)], 17
    iq, _ = synth.ul_units_3gpp(cfg, ul, sfs16, [cell] * SEED_UNITS, [a for u in range(SEED_UNITS) for a in allocs(u)], per, snr_db=15.0, max_delay=3, seed=77)
    planes, d16 = ctx.ul_frontend(cfg, iq.reshape(-1, 2), np.arange(SEED_UNITS) * iq.shape[1], keep=True)
    d16.free()
    reps = (n + SEED_UNITS - 1) // SEED_UNITS
    d_sub = ctx.to_device(np.tile(planes.reshape(SEED_UNITS, -1), (reps, 1))[:n])
    plan = ctx.pusch_plan_3gpp(cfg, ul, (sfs16 * reps)[:n], [cell] * n, [a for u in range(n) for a in allocs(u)])
    d_out, d_st = ctx.alloc(plan.n_alloc * plan.out_stride), ctx.alloc(4 * plan.n_alloc)

    def run(mode, gain):
        if not ref_only:
            plan.set_demapper(mode, gain)
        plan.run_dev(d_sub, d_out, d_st)
        ctx.sync()

    if ref_only:
        runs = [("ref", "k_pusch_demod", lambda: run(0, 0.0))]
    else:
        run(m.DEMAP_MAXLOG, 0.0)
        fixed = float(np.median(plan.llr_gain()))
        runs = [("ref", "k_pusch_demod", lambda: run(m.DEMAP_REF, 0.0)), ("maxlog_auto", "k_pusch_demod_llr", lambda: run(m.DEMAP_MAXLOG, 0.0)),
                ("maxlog_fixed", "k_pusch_demod_llr", lambda: run(m.DEMAP_MAXLOG, fixed))]
    for _ in range(args.warmup):
        for _, _, f in runs:
            f()
    ms = {k: [] for k, _, _ in runs}
    ok = {}
    t0, steps = time.monotonic(), 0
    ctx.profile(True)
    while steps < args.steps and (steps < 3 or time.monotonic() - t0 < args.time_limit):
        for k, kernel, f in runs:  # alternating, one run of each per step
            ctx._check(ctx.L.mi_lte_profile_reset(ctx.h))
            f()
            ms[k].append(ctx.profile_report()[kernel][1])
            ok[k] = int((d_st.download(np.int32) == 0).sum())
        steps += 1
    ctx.profile(False)
    med = {k: float(np.median(v)) for k, v in ms.items()}
    out = {"units": n, "allocations": plan.n_alloc, "N_prb": n_prb, "mod_type": mod, "tbs": size, "steps": steps,
           "kernel_ms": {k: round(v, 4) for k, v in med.items()}, "kernel_ms_range": {k: [round(min(v), 4), round(max(v), 4)] for k, v in ms.items()},
           "ns_per_allocation": {k: round(1e6 * v / plan.n_alloc, 2) for k, v in med.items()}, "decoded": ok}
    for b in (d_sub, d_out, d_st):
        b.free()
    plan.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--units", type=int, default=2048)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--time-limit", type=float, default=60.0, help="seconds per shape for the timed loop; it ends early (after at least 3 steps) when they are used up")
    ap.add_argument("--parent-pkg", default=None)
    ap.add_argument("--pkg", default=None, help="(the child of --parent-pkg) import openlte_amd from here and time the default demapper alone")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    sys.path.insert(0, args.pkg or ROOT)
    import openlte_amd as m
    from openlte_amd import synth
    ref_only = args.pkg is not None
    ctx = m.Context(0)
    out = {"workload": "pusch_llr_timing", "warmup": args.warmup, "shapes": {name: time_shape(m, synth, ctx, name, args.units, args, ref_only) for name in SHAPES},
           "build_id": m.load_library().mi_lte_build_id().decode(), "device": ctx.device_name}
    ctx.close()
    if args.parent_pkg:
        child = subprocess.run([sys.executable, os.path.abspath(__file__), "--pkg", args.parent_pkg, "--units", str(args.units), "--steps", str(args.steps),
                                "--warmup", str(args.warmup), "--time-limit", str(args.time_limit)], capture_output=True, text=True, timeout=600)
        if child.returncode != 0:
            print(child.stdout[-2000:], child.stderr[-2000:])
            return 1
        parent = json.loads(child.stdout.strip().splitlines()[-1])
        out["parent_library"] = {"build_id": parent["build_id"], "shapes": {name: {k: s[k] for k in ("kernel_ms", "kernel_ms_range", "decoded")} for name, s in parent["shapes"].items()}}
        for name, s in out["shapes"].items():
            pm = parent["shapes"][name]["kernel_ms"]["ref"]
            s["over_parent_ref"] = {k: round(v / pm, 3) for k, v in s["kernel_ms"].items()}
    line = json.dumps(out)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write("# tools/pusch_llr_timing.py --units %d --steps %d --warmup %d%s on one MI355X (gfx950)\n"
                    % (args.units, args.steps, args.warmup, " --parent-pkg <the parent commit's package>" if args.parent_pkg else ""))
            f.write("# kernel_ms: medians of the event-bracketed kernel time of one plan run, runs alternating.  ref: k_pusch_demod<.., SPEC = true>, the default\n")
            f.write("# demapper; maxlog_auto / maxlog_fixed: k_pusch_demod_llr with the automatic gain and with a fixed one (both run the rho pass), tap off.\n")
            f.write("# parent_library: k_pusch_demod of the parent commit's library on the same input, in a child process of the same call; over_parent_ref:\n")
            f.write("# this library's three kernels over it.  No target.\n")
            f.write(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
