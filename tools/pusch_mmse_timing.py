#!/usr/bin/env python3
"""What MMSE equalisation on the 3GPP PUSCH plans costs, by the method of tools/pusch_rxdiv_timing.py and on its shapes.  In the calling
process one 3GPP plan per shape runs k_pusch_demod (the default demapper), k_pusch_demod_llr under the automatic and the noise-referenced
gain, k_pusch_demod_llr_rx on two antennas under both gains, and k_pusch_demod_llr_mmse on one and on two antennas, the seven alternating;
event-bracketed kernel times (mi_lte_profile_*), medians over --steps runs.  `mmse1_over_noise` / `mmse2_over_noise`: the MMSE launch over
the noise-on launch of the same n_rx in the same loop, reported without a bound.
--parent-pkg DIR (a directory that holds the `openlte_amd` package of the parent commit with its built library) compares the two libraries
on the five launches the parent has too: --parent-runs times over, a child process times this library's and then a child process the
parent library's on the same input, all started by the same call, each under a time limit of its own (timeout -k 10); the first child that
fails ends the tool.  `within_parent_spread`: the median of this library's child runs lies at or under the slowest of the parent's own
runs, per shape and kernel and for all of them -- the parent's spread is the measurement's own noise.

    python tools/pusch_mmse_timing.py [--units 2048] [--steps 20] [--warmup 2] [--parent-pkg DIR] [--parent-runs 5] [--out profiles/pusch_mmse_timing.txt]
Prints one JSON line last (and writes it to --out with a header)."""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from pusch_llr_timing import SEED_UNITS, SHAPES, ULC  # noqa: E402

N_ANT = 2
SHARED = ("ref", "maxlog_auto", "maxlog_noise", "rx2_auto", "rx2_noise")  # what the parent library launches too


def time_shape(m, synth, ctx, name, n, args, child):
    mod, itbs, n_prb, per = SHAPES[name]
    cfg, ul = m.DlCfg(2048, 100, 1, 0), m.UlCfg(*ULC)
    size = int(m.load_library().mi_lte_tbs(itbs, n_prb))

    def allocs(u):
        return [m.make_alloc(u, mod, size, list(range(n_prb * a, n_prb * a + n_prb)), 0x100 + a) for a in range(per)]

    sfs16, cell = [u % 10 for u in range(SEED_UNITS)], 17
    seed_allocs = [a for u in range(SEED_UNITS) for a in allocs(u)]
    # two antenna captures of the same sixteen units; antenna 0 serves the single-antenna launches
    iq, _ = synth.ul_units_3gpp_rx(cfg, ul, sfs16, [cell] * SEED_UNITS, seed_allocs, per, N_ANT, seed=77, snr_db=15.0, max_delay=3)
    planes, d16 = ctx.ul_frontend(cfg, iq.reshape(-1, 2), np.arange(iq.shape[0]) * iq.shape[1], keep=True)
    d16.free()
    reps = (n + SEED_UNITS - 1) // SEED_UNITS
    planes = planes.reshape(-1, SEED_UNITS, planes[0].size)
    d_sub = ctx.to_device(np.concatenate([np.tile(p, (reps, 1))[:n] for p in planes]))  # antenna-major, ant_stride = n
    plan = ctx.pusch_plan_3gpp(cfg, ul, (sfs16 * reps)[:n], [cell] * n, [a for u in range(n) for a in allocs(u)])
    d_out, d_st = ctx.alloc(plan.n_alloc * plan.out_stride), ctx.alloc(4 * plan.n_alloc)

    def run(mode, noise, n_rx=1, mmse=False):
        plan.set_demapper(mode, 0.0)
        plan.set_llr_noise(noise)
        plan.set_rx_antennas(n_rx, n)
        if not child:
            plan.set_equaliser(m.EQ_MMSE if mmse else m.EQ_ZF)
        plan.run_dev(d_sub, d_out, d_st)
        ctx.sync()

    runs = [("ref", "k_pusch_demod", lambda: run(m.DEMAP_REF, 0.0)), ("maxlog_auto", "k_pusch_demod_llr", lambda: run(m.DEMAP_MAXLOG, 0.0)),
            ("maxlog_noise", "k_pusch_demod_llr", lambda: run(m.DEMAP_MAXLOG, 8.0)),
            ("rx2_auto", "k_pusch_demod_llr_rx", lambda: run(m.DEMAP_MAXLOG, 0.0, 2)), ("rx2_noise", "k_pusch_demod_llr_rx", lambda: run(m.DEMAP_MAXLOG, 8.0, 2))]
    if not child:
        runs.append(("mmse1", "k_pusch_demod_llr_mmse", lambda: run(m.DEMAP_MAXLOG, 8.0, 1, True)))
        runs.append(("mmse2", "k_pusch_demod_llr_mmse", lambda: run(m.DEMAP_MAXLOG, 8.0, 2, True)))
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
    out = {"units": n, "allocations": plan.n_alloc, "N_prb": n_prb, "mod_type": mod, "tbs": size, "steps": steps,
           "kernel_ms": {k: round(float(np.median(v)), 4) for k, v in ms.items()},
           "kernel_ms_range": {k: [round(min(v), 4), round(max(v), 4)] for k, v in ms.items()}, "decoded": ok}
    for k, base in (("mmse1", "maxlog_noise"), ("mmse2", "rx2_noise")):
        out[k + "_over_noise"] = round(out["kernel_ms"][k] / out["kernel_ms"][base], 4) if k in ms else None
    for b in (d_sub, d_out, d_st):
        b.free()
    plan.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--units", type=int, default=2048)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--time-limit", type=float, default=40.0, help="seconds per shape for the timed loop; it ends early (after at least 3 steps) when they are used up")
    ap.add_argument("--parent-pkg", default=None)
    ap.add_argument("--parent-runs", type=int, default=5)
    ap.add_argument("--pkg", default=None, help="(the child of --parent-pkg) import openlte_amd from here and time the launches both libraries have")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    sys.path.insert(0, args.pkg or ROOT)
    import openlte_amd as m
    from openlte_amd import synth
    ctx = m.Context(0)
    out = {"workload": "pusch_mmse_timing", "warmup": args.warmup,
           "shapes": {name: time_shape(m, synth, ctx, name, args.units, args, args.pkg is not None) for name in SHAPES},
           "build_id": m.load_library().mi_lte_build_id().decode(), "device": ctx.device_name}
    ctx.close()
    if args.parent_pkg:
        def child(pkg):
            c = subprocess.run(["timeout", "-k", "10", "280", sys.executable, os.path.abspath(__file__), "--pkg", pkg, "--units", str(args.units), "--steps", str(args.steps),
                                "--warmup", str(args.warmup), "--time-limit", str(args.time_limit)], capture_output=True, text=True, timeout=300)
            if c.returncode != 0:
                print(c.stdout[-2000:], c.stderr[-2000:])
                sys.exit(1)
            return json.loads(c.stdout.strip().splitlines()[-1])

        ours, parents = [], []
        for i in range(args.parent_runs):  # alternating, so that neither library has the warmer or the cooler device
            ours.append(child(ROOT))
            parents.append(child(args.parent_pkg))
            print("# pair %d of %d done" % (i + 1, args.parent_runs), flush=True)
        out["parent_library"] = {"build_id": parents[0]["build_id"]}
        within = True
        for name, s in out["shapes"].items():
            s["vs_parent"] = {}
            for k in SHARED:
                pv, ov = [p["shapes"][name]["kernel_ms"][k] for p in parents], [o["shapes"][name]["kernel_ms"][k] for o in ours]
                spread, ok = (max(pv) - min(pv)) / float(np.mean(pv)), float(np.median(ov)) <= max(pv)
                s["vs_parent"][k] = {"this_ms": [round(v, 4) for v in ov], "parent_ms": [round(v, 4) for v in pv], "parent_spread": round(spread, 4),
                                     "ratio": round(float(np.median(ov)) / float(np.median(pv)), 4), "within_parent_spread": bool(ok)}
                within = within and ok
        out["within_parent_spread"] = bool(within)
    line = json.dumps(out)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write("# tools/pusch_mmse_timing.py --units %d --steps %d --warmup %d%s on one MI355X (gfx950)\n"
                    % (args.units, args.steps, args.warmup, " --parent-pkg <the parent commit's package> --parent-runs %d" % args.parent_runs if args.parent_pkg else ""))
            f.write("# kernel_ms: medians of the event-bracketed kernel time of one plan run, runs alternating.  ref: k_pusch_demod<.., SPEC = true>; maxlog_auto /\n")
            f.write("# maxlog_noise: the single-antenna k_pusch_demod_llr under the automatic / the noise-referenced gain; rx2_auto / rx2_noise: k_pusch_demod_llr_rx on\n")
            f.write("# two antennas; mmse1 / mmse2: k_pusch_demod_llr_mmse on one / two antennas; mmse<n>_over_noise: over the noise-on launch of the same n_rx, no bound.\n")
            f.write("# vs_parent: the five launches both libraries have, of this library (this_ms) and of the parent commit's (parent_ms), each figure one child process\n")
            f.write("# of the same call, the libraries alternating; ratio: median over median; parent_spread: the parent runs' max - min over their mean;\n")
            f.write("# within_parent_spread: this library's median is no slower than the slowest parent run.\n")
            f.write(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
