#!/usr/bin/env python3
"""What the CRS noise estimate and the noise-referenced gain of the 3GPP PDSCH plans cost, by the method of tools/pusch_noise_timing.py:
k_pdsch_demod (the default demapper) and k_pdsch_demod_llr under the automatic gain and under the noise-referenced one
(mi_lte_pdsch_plan_set_llr_noise, with its k_dl_crs_noise over the plan's units) on one 3GPP plan -- W4 (8 x 12 PRB + 1 x 4 PRB, 64QAM,
100 RB) over --units subframes, the planes of 16 synthesised units tiled -- in one process, the three alternating; event-bracketed kernel
times (mi_lte_profile_*), medians over --steps runs.  Then k_dl_crs_noise alone (mi_lte_dl_crs_noise_run) over --noise-units units at 100 RB on
one port and on two (the same y planes in the two-port layout: the kernel reads nothing else).
--parent-pkg DIR (a directory that holds the `openlte_amd` package of the parent commit with its built library) compares the two libraries
by one method: --parent-runs times over, a child process times this library's k_pdsch_demod and k_pdsch_demod_llr (automatic gain, the
setter off: the two kernels the parent has too, alternating) and then a child process times the parent library's on the same input, all
started by the same call.  The margin is the spread of the parent's own repeated runs -- `within_parent_spread` says whether the median of
this library's child runs lies at or under the slowest of the parent's, per kernel and for both.  The rest is reported, not gated.

    python tools/pdsch_noise_timing.py [--units 1024] [--noise-units 4096] [--steps 20] [--warmup 2] [--parent-pkg DIR] [--parent-runs 5] [--out profiles/pdsch_noise_timing.txt]
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


def timed(ctx, runs, args):
    """runs: (key, [kernel names], callable).  Alternating, one run of each per step; ms[key][kernel] = the event-bracketed times"""
    for _ in range(args.warmup):
        for _, _, f in runs:
            f()
    ms = {k: {kn: [] for kn in kernels} for k, kernels, _ in runs}
    t0, steps = time.monotonic(), 0
    ctx.profile(True)
    while steps < args.steps and (steps < 3 or time.monotonic() - t0 < args.time_limit):
        for k, kernels, f in runs:
            ctx._check(ctx.L.mi_lte_profile_reset(ctx.h))
            f()
            rep = ctx.profile_report()
            for kn in kernels:
                ms[k][kn].append(rep[kn][1])
        steps += 1
    ctx.profile(False)
    return ms, steps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--units", type=int, default=1024)
    ap.add_argument("--noise-units", type=int, default=4096)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--time-limit", type=float, default=60.0, help="seconds per timed loop; it ends early (after at least 3 steps) when they are used up")
    ap.add_argument("--parent-pkg", default=None)
    ap.add_argument("--parent-runs", type=int, default=5)
    ap.add_argument("--pkg", default=None, help="(the child of --parent-pkg) import openlte_amd from here and time the two kernels that library has")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    sys.path.insert(0, args.pkg or ROOT)
    import openlte_amd as m
    from openlte_amd import synth
    child_run = args.pkg is not None
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
    planes = d_sub16.download(np.float32).reshape(SEED_UNITS, 4, 16, 1200)
    for b in (d_iq, d_start, d_sf16, d_cell16, d_sub16):
        b.free()

    def tiled(block, n_units):
        """n_units units on the device, the 16-unit block repeated"""
        d = ctx.alloc(n_units * block[0].nbytes)
        for u0 in range(0, n_units, SEED_UNITS):
            d.upload(np.ascontiguousarray(block[:min(SEED_UNITS, n_units - u0)]), offset=u0 * block[0].nbytes)
        return d

    reps = (n + SEED_UNITS - 1) // SEED_UNITS
    d_sub = tiled(planes, n)
    d_sf, d_cell = ctx.to_device(np.asarray((sfs16 * reps)[:n], np.uint32)), ctx.to_device(np.asarray((cells16 * reps)[:n], np.uint32))
    plan = ctx.pdsch_plan_3gpp(cfg, CFI, [a for u in range(n) for a in w4(u)], N_SOFT)
    d_out, d_st = ctx.alloc(plan.n_alloc * plan.out_stride), ctx.alloc(4 * plan.n_alloc)
    ok = {}

    def run(key, mode, noise):
        plan.set_demapper(mode, 0.0)
        if not child_run:
            plan.set_llr_noise(noise)
        plan.run_dev(d_sub, d_sf, d_cell, d_out, d_st)
        ctx.sync()
        ok[key] = int((d_st.download(np.int32) == 0).sum())

    runs = [("ref", ["k_pdsch_demod"], lambda: run("ref", m.DEMAP_REF, 0.0)), ("maxlog_auto", ["k_pdsch_demod_llr"], lambda: run("maxlog_auto", m.DEMAP_MAXLOG, 0.0))]
    if not child_run:
        runs.append(("maxlog_noise", ["k_pdsch_demod_llr", "k_dl_crs_noise"], lambda: run("maxlog_noise", m.DEMAP_MAXLOG, 8.0)))
    ms, steps = timed(ctx, runs, args)
    first = {k: v[kernels[0]] for (k, kernels, _), v in zip(runs, ms.values())}
    out = {"workload": "pdsch_noise_timing", "units": n, "allocations": plan.n_alloc, "steps": steps, "warmup": args.warmup,
           "kernel_ms": {k: round(float(np.median(v)), 4) for k, v in first.items()},
           "kernel_ms_range": {k: [round(min(v), 4), round(max(v), 4)] for k, v in first.items()}, "decoded": dict(ok)}
    for b in (d_sub, d_sf, d_cell, d_out, d_st):
        b.free()
    plan.close()
    if not child_run:
        v = ms["maxlog_noise"]["k_dl_crs_noise"]
        out["plan_crs_noise_ms"] = round(float(np.median(v)), 4)
        out["plan_crs_noise_ms_range"] = [round(min(v), 4), round(max(v), 4)]
        out["noise_over_auto"] = round(out["kernel_ms"]["maxlog_noise"] / out["kernel_ms"]["maxlog_auto"], 4)
        out["noise_with_estimate_over_auto"] = round((out["kernel_ms"]["maxlog_noise"] + out["plan_crs_noise_ms"]) / out["kernel_ms"]["maxlog_auto"], 4)
        # the estimator alone: --noise-units units at 100 RB, one port and two
        nu = args.noise_units
        reps = (nu + SEED_UNITS - 1) // SEED_UNITS
        d_sf, d_cell = ctx.to_device(np.asarray((sfs16 * reps)[:nu], np.uint32)), ctx.to_device(np.asarray((cells16 * reps)[:nu], np.uint32))
        d_s2 = ctx.alloc(4 * nu)
        out["crs_noise"] = {"units": nu}
        for n_ant in (1, 2):
            block = np.zeros((SEED_UNITS, 2 + 2 * n_ant, 16, 1200), np.float32)
            block[:, :2] = planes[:, :2]
            d_sub = tiled(block, nu)
            c = m.DlCfg(2048, 100, n_ant, 0)

            def alone():
                ctx.dl_crs_noise_dev(c, d_sub, d_sf, d_cell, nu, d_s2)
                ctx.sync()

            t, _ = timed(ctx, [("alone", ["k_dl_crs_noise"], alone)], args)
            v = t["alone"]["k_dl_crs_noise"]
            s2 = d_s2.download(np.float32)
            out["crs_noise"]["%d_port" % n_ant] = {"kernel_ms": round(float(np.median(v)), 4), "kernel_ms_range": [round(min(v), 4), round(max(v), 4)],
                                                   "ns_per_unit": round(1e6 * float(np.median(v)) / nu, 2),
                                                   "y_plane_GBps": round(nu * 4 * n_ant * 200 * 8 / (float(np.median(v)) * 1e6), 1),
                                                   "sigma2_mean": float(s2.mean())}
            d_sub.free()
        for b in (d_sf, d_cell, d_s2):
            b.free()
    out["build_id"], out["device"] = m.load_library().mi_lte_build_id().decode(), ctx.device_name
    ctx.close()
    if args.parent_pkg:
        def child(pkg):
            c = subprocess.run([sys.executable, os.path.abspath(__file__), "--pkg", pkg, "--units", str(n), "--steps", str(args.steps),
                                "--warmup", str(args.warmup), "--time-limit", str(args.time_limit)], capture_output=True, text=True, timeout=300)
            if c.returncode != 0:
                print(c.stdout[-2000:], c.stderr[-2000:])
                sys.exit(1)
            return json.loads(c.stdout.strip().splitlines()[-1])

        ours, parents = [], []
        for _ in range(args.parent_runs):  # alternating, so that neither library has the warmer or the cooler device
            ours.append(child(ROOT))
            parents.append(child(args.parent_pkg))
        out["parent_library"] = {"build_id": parents[0]["build_id"]}
        out["vs_parent"], within = {}, True
        for k in ("ref", "maxlog_auto"):
            pv, ov = [p["kernel_ms"][k] for p in parents], [o["kernel_ms"][k] for o in ours]
            spread, ok_k = (max(pv) - min(pv)) / float(np.mean(pv)), float(np.median(ov)) <= max(pv)
            out["vs_parent"][k] = {"this_ms": [round(v, 4) for v in ov], "parent_ms": [round(v, 4) for v in pv], "parent_spread": round(spread, 4),
                                   "ratio": round(float(np.median(ov)) / float(np.median(pv)), 4), "within_parent_spread": bool(ok_k)}
            within = within and ok_k
        out["within_parent_spread"] = bool(within)
    line = json.dumps(out)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write("# tools/pdsch_noise_timing.py --units %d --noise-units %d --steps %d --warmup %d%s on one MI355X (gfx950)\n"
                    % (n, args.noise_units, args.steps, args.warmup, " --parent-pkg <the parent commit's package> --parent-runs %d" % args.parent_runs if args.parent_pkg else ""))
            f.write("# kernel_ms: medians of the event-bracketed kernel time of one plan run (W4: 9 allocations per unit, 64QAM, 100 RB), runs alternating.  ref:\n")
            f.write("# k_pdsch_demod; maxlog_auto: k_pdsch_demod_llr<1>, automatic gain, the setter off; maxlog_noise: k_pdsch_demod_llr<1, PdschLlrNoise> with\n")
            f.write("# g = 8 / sigma2, and plan_crs_noise_ms the k_dl_crs_noise launch of that run over the plan's units.  crs_noise: mi_lte_dl_crs_noise_run alone.\n")
            f.write("# vs_parent: ref and maxlog_auto of this library (this_ms) and of the parent commit's (parent_ms), each figure one child process of the\n")
            f.write("# same call timing those two kernels alone, the libraries alternating; ratio: median over median; parent_spread: the parent runs' max - min\n")
            f.write("# over their mean; within_parent_spread: this library's median is no slower than the slowest parent run.  The rest is reported, no bound.\n")
            f.write(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
