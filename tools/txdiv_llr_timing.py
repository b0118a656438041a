#!/usr/bin/env python3
"""What the transmit-diversity work costs, in kernel times (the HIP events the library puts round each launch, mi_lte_profile_*), on the timing
shape of tools/demap_llr_timing.py: W4 (8 x 12 PRB + 1 x 4 PRB, 64QAM, 100 RB) over --units subframes (4096: 36 864 allocations), the planes
of 16 synthesised units tiled.
(a) Against the parent commit's library (--parent-pkg DIR, a directory that holds the parent's `openlte_amd` package with its built library), in
    child processes of this call that alternate between the two libraries, --rounds each: k_pdsch_demod and k_pdsch_demod_llr on the
    single-port cell and, where the parent has the two-port plan, k_pdsch_demod<false> and k_pdsch_demod_llr<2> (labelled k_pdsch_demod_llr_txd)
    on the two-port cell.  Gate, for every key both libraries measured: every child's median of this library is no slower than the slowest
    single run of the parent's -- the parent's own spread is the margin, since the code is meant to do the same work.
(b) The two-port cell of the same shape: k_pdsch_demod_llr_txd (automatic gain) next to k_pdsch_demod<false>, the default demapper of the
    same plan, and next to the single-port k_pdsch_demod_llr, per symbol.  Reported.

    python tools/txdiv_llr_timing.py --parent-pkg DIR [--units 4096] [--steps 8] [--rounds 3] [--out profiles/txdiv_llr_timing.txt]
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


def measure(pkg, n, steps, warmup, time_limit):
    """One process, one library: the kernel times of its single-port plan and, where the library has them, of its two-port plan"""
    sys.path.insert(0, pkg)
    import openlte_amd as m
    from openlte_amd import synth
    ctx = m.Context(0)
    has_txd = hasattr(ctx, "pdsch_plan_3gpp_txdiv")
    sfs16, cells16 = [u % 10 for u in range(SEED_UNITS)], [(31 * u + 7) % 504 for u in range(SEED_UNITS)]
    reps = (n + SEED_UNITS - 1) // SEED_UNITS
    sfs, cells = (sfs16 * reps)[:n], (cells16 * reps)[:n]
    out = {"build_id": m.load_library().mi_lte_build_id().decode(), "device": ctx.device_name, "kernel_ms": {}, "kernel_ms_range": {}, "symbols": {}}

    def w4(u, txm):
        return [m.make_alloc(u, 3, 3240 if a < 8 else 1064, list(range(a * 12, a * 12 + 12)) if a < 8 else list(range(96, 100)), 0x100 + a, tx_mode=txm)
                for a in range(9)]

    for n_ant in (1, 2) if has_txd else (1,):
        cfg, txm = m.DlCfg(2048, 100, n_ant, 0), 1 if n_ant == 1 else 2
        seed_allocs = [a for u in range(SEED_UNITS) for a in w4(u, txm)]
        gen = synth.dl_units_3gpp if n_ant == 1 else synth.dl_units_3gpp_txdiv
        iq, _ = gen(cfg, sfs16, cells16, seed_allocs, 9, N_SOFT, n_pdcch_symbs=CFI, snr_db=15.0, max_delay=4, seed=77)
        d_iq, d_start = ctx.to_device(iq.reshape(-1, 2)), ctx.to_device((np.arange(SEED_UNITS) * iq.shape[1]).astype(np.uint64))
        d_sf16, d_cell16 = ctx.to_device(np.asarray(sfs16, np.uint32)), ctx.to_device(np.asarray(cells16, np.uint32))
        d_sub16 = ctx.alloc(SEED_UNITS * ctx.subframe_floats(n_ant) * 4)
        ctx.dl_frontend_dev(cfg, d_iq, None, d_start, d_sf16, d_cell16, SEED_UNITS, d_sub16)
        planes = d_sub16.download(np.float32).reshape(SEED_UNITS, -1)
        for b in (d_iq, d_start, d_sf16, d_cell16, d_sub16):
            b.free()
        d_sub = ctx.to_device(np.tile(planes, (reps, 1))[:n])
        d_sf, d_cell = ctx.to_device(np.asarray(sfs, np.uint32)), ctx.to_device(np.asarray(cells, np.uint32))
        allocs = [a for u in range(n) for a in w4(u, txm)]
        plan = ctx.pdsch_plan_3gpp(cfg, CFI, allocs, N_SOFT) if n_ant == 1 else ctx.pdsch_plan_3gpp_txdiv(cfg, CFI, allocs, N_SOFT)
        d_out, d_st = ctx.alloc(plan.n_alloc * plan.out_stride), ctx.alloc(4 * plan.n_alloc)

        def run(mode):
            plan.set_demapper(mode, 0.0)
            plan.run_dev(d_sub, d_sf, d_cell, d_out, d_st)
            ctx.sync()

        tag = "p%d_" % n_ant
        runs = [(tag + "ref", "k_pdsch_demod", m.DEMAP_REF), (tag + "maxlog", "k_pdsch_demod_llr" if n_ant == 1 else "k_pdsch_demod_llr_txd", m.DEMAP_MAXLOG)]
        for _ in range(warmup):
            for _, _, mode in runs:
                run(mode)
        ms = {name: [] for name, _, _ in runs}
        t0, k = time.monotonic(), 0
        ctx.profile(True)
        while k < steps and (k < 3 or time.monotonic() - t0 < time_limit):
            for name, kernel, mode in runs:  # alternating, one run of each per step
                ctx._check(ctx.L.mi_lte_profile_reset(ctx.h))
                run(mode)
                ms[name].append(ctx.profile_report()[kernel][1])
            k += 1
        ctx.profile(False)
        plan.set_demapper(m.DEMAP_REF, 0.0)
        plan.run_dev(d_sub, d_sf, d_cell, d_out, d_st)
        ctx.sync()
        out["symbols"][tag[:-1]] = int(sum(len(plan.soft_bits(a)) for a in range(9 * SEED_UNITS)) // 6 * (n / SEED_UNITS))
        for name in ms:
            out["kernel_ms"][name] = round(float(np.median(ms[name])), 4)
            out["kernel_ms_range"][name] = [round(min(ms[name]), 4), round(max(ms[name]), 4)]
        for b in (d_sub, d_sf, d_cell, d_out, d_st):
            b.free()
        plan.close()
    out["steps"] = k
    ctx.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--units", type=int, default=4096)
    ap.add_argument("--steps", type=int, default=8)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--time-limit", type=float, default=60.0, help="seconds for a child's timed loop; it ends early (after at least 3 steps) when they are used up")
    ap.add_argument("--parent-pkg", default=None)
    ap.add_argument("--child", default=None, help="(internal) measure the library of the package in this directory and print one JSON line")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.child:
        print(json.dumps(measure(args.child, args.units, args.steps, args.warmup, args.time_limit)))
        return 0
    libs = [("this", ROOT)] + ([("parent", args.parent_pkg)] if args.parent_pkg else [])
    res = {name: [] for name, _ in libs}
    for _ in range(args.rounds):
        for name, pkg in libs:  # alternating child processes: one library each, no GPU work in this process
            child = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", pkg, "--units", str(args.units), "--steps", str(args.steps),
                                    "--warmup", str(args.warmup), "--time-limit", str(args.time_limit)], capture_output=True, text=True, timeout=900)
            if child.returncode != 0:
                print(child.stdout[-2000:], child.stderr[-2000:])
                return 1
            res[name].append(json.loads(child.stdout.strip().splitlines()[-1]))
    this = res["this"]
    out = {"workload": "txdiv_llr_timing", "units": args.units, "allocations": 9 * args.units, "steps": this[0]["steps"], "rounds": args.rounds,
           "this": {"build_id": this[0]["build_id"], "kernel_ms": [r["kernel_ms"] for r in this], "kernel_ms_range": [r["kernel_ms_range"] for r in this]},
           "device": this[0]["device"]}
    ok = True
    if args.parent_pkg:
        par = res["parent"]
        out["parent"] = {"build_id": par[0]["build_id"], "kernel_ms": [r["kernel_ms"] for r in par], "kernel_ms_range": [r["kernel_ms_range"] for r in par]}
        gate = {}
        for k in (k for k in this[0]["kernel_ms"] if all(k in r["kernel_ms"] for r in par)):  # every key both libraries measured
            slowest_parent_run = max(r["kernel_ms_range"][k][1] for r in par)
            worst_median = max(r["kernel_ms"][k] for r in this)
            gate[k] = {"this_worst_median_ms": worst_median, "parent_median_ms": float(np.median([r["kernel_ms"][k] for r in par])),
                       "parent_slowest_run_ms": slowest_parent_run, "ok": bool(worst_median <= slowest_parent_run)}
            ok = ok and gate[k]["ok"]
        out["parent_gate"] = gate
    med = {k: float(np.median([r["kernel_ms"][k] for r in this])) for k in this[0]["kernel_ms"]}
    sym = this[0]["symbols"]
    out["ns_per_symbol"] = {"k_pdsch_demod_llr_txd": round(1e6 * med["p2_maxlog"] / sym["p2"], 4), "k_pdsch_demod<false>": round(1e6 * med["p2_ref"] / sym["p2"], 4),
                            "k_pdsch_demod_llr": round(1e6 * med["p1_maxlog"] / sym["p1"], 4), "k_pdsch_demod<true>": round(1e6 * med["p1_ref"] / sym["p1"], 4)}
    out["symbols"] = sym
    out["txd_over_demod_false"] = round(med["p2_maxlog"] / med["p2_ref"], 3)
    out["txd_over_llr_per_symbol"] = round(out["ns_per_symbol"]["k_pdsch_demod_llr_txd"] / out["ns_per_symbol"]["k_pdsch_demod_llr"], 3)
    line = json.dumps(out)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write("# tools/txdiv_llr_timing.py --units %d --steps %d --warmup %d --rounds %d%s on one MI355X (gfx950)\n"
                    % (args.units, args.steps, args.warmup, args.rounds, " --parent-pkg <the parent commit's package>" if args.parent_pkg else ""))
            f.write("# kernel_ms: per child process, the median of the event-bracketed kernel time of one plan run (W4: 9 allocations per unit, 64QAM).\n")
            f.write("# p1_ref / p1_maxlog: k_pdsch_demod<true> / k_pdsch_demod_llr on the single-port cell; p2_ref / p2_maxlog: k_pdsch_demod<false> /\n")
            f.write("# k_pdsch_demod_llr_txd on the two-port cell.  parent_gate: per key both libraries measured, this library's worst child median against the\n")
            f.write("# slowest single run of the parent commit's library, child processes alternating.  ns_per_symbol: kernel time over the plan's modulation symbols.\n")
            f.write(line + "\n")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
