#!/usr/bin/env python3
"""HARQ soft combining on the 3GPP PUSCH plans at full load: 2 048 uplink subframe units of a 100-RB cell, one 96-PRB 64QAM allocation each
(the size of Table 7.1.7.2.1-1's column 96 at I_TBS 22, BCJR x 8, exact interleaver), with a pool of one soft buffer per unit.

After one HARQ run with NEW_DATA (the first transmission), the plain plan run (mi_lte_pusch_decode_run) and the HARQ run of a further
transmission (mi_lte_pusch_decode_run_harq without NEW_DATA: every buffer read, combined and written back) are timed alternately, one run
each per step, in one process; then one profiled run of each gives the per-kernel split.  Reported, not gated (the downlink's figure:
profiles/harq_bench.txt).

    python tools/pusch_harq_bench.py [--units 2048] [--steps 10] [--warmup 2] [--out profiles/pusch_harq_bench.txt]
Prints one JSON line last (and writes it to --out with a header)."""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import openlte_amd as m  # noqa: E402
from openlte_amd import synth  # noqa: E402

N_PRB, MOD, ITBS, ULC = 96, 3, 22, (3, 0, 0, 2, 5)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--units", type=int, default=2048)
    ap.add_argument("--unique", type=int, default=10, help="distinct synthesised subframes (subframe numbers 0..9), repeated over the units")
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=None, help="also write the JSON line (with a header) to this file")
    args = ap.parse_args()
    ctx = m.Context(0)
    cfg, ul = m.DlCfg(2048, 100, 1, 0), m.UlCfg(*ULC)
    size = int(m.load_library().mi_lte_tbs(ITBS, N_PRB))
    lay = m.ulsch_layout(size, 144 * N_PRB * 6, 6)
    nu, n, cell = args.unique, args.units, 17
    sfs_u = list(range(nu))
    allocs_u = [m.make_alloc(i, MOD, size, list(range(2, 2 + N_PRB)), 0x100 + i) for i in range(nu)]
    iq, tx = synth.ul_units_3gpp(cfg, ul, sfs_u, [cell] * nu, allocs_u, 1, snr_db=30.0, max_delay=3, seed=11)
    planes, d_u = ctx.ul_frontend(cfg, iq.reshape(-1, 2), np.arange(nu) * iq.shape[1], keep=True)
    d_u.free()
    reps = (n + nu - 1) // nu
    d_sub = ctx.to_device(np.tile(planes.reshape(nu, -1), (reps, 1))[:n])
    allocs = [m.make_alloc(u, MOD, size, list(range(2, 2 + N_PRB)), 0x100 + u % nu) for u in range(n)]
    plan = ctx.pusch_plan_3gpp(cfg, ul, [sfs_u[u % nu] for u in range(n)], [cell] * n, allocs)
    pool = ctx.harq_pool(n, size)
    d_out, d_st = ctx.alloc(n * plan.out_stride), ctx.alloc(4 * n)
    d_out_h, d_st_h = ctx.alloc(n * plan.out_stride), ctx.alloc(4 * n)
    first, again = m.harq_binds(n, range(n), True), m.harq_binds(n, range(n), False)

    def plain():
        plan.run_dev(d_sub, d_out, d_st)

    def harq():
        plan.run_harq_dev(pool, again, d_sub, d_out_h, d_st_h)

    plan.run_harq_dev(pool, first, d_sub, d_out_h, d_st_h)  # the first transmission fills every buffer
    for _ in range(args.warmup):
        plain()
        harq()
    ctx.sync()
    t_plain, t_harq = [], []
    for _ in range(args.steps):  # alternating, one run of each per step
        ctx.timer_start()
        plain()
        t_plain.append(ctx.timer_stop())
        ctx.timer_start()
        harq()
        t_harq.append(ctx.timer_stop())
    st, st_h = d_st.download(np.int32), d_st_h.download(np.int32)
    bits, bits_h = d_out.download(np.uint8).reshape(n, plan.out_stride), d_out_h.download(np.uint8).reshape(n, plan.out_stride)
    tx_ok = all((bits_h[u, :size] == tx[u % nu, 0, :size]).all() for u in range(nu))
    n_tx = pool.state(0)["n_tx"]

    def split(fn):
        ctx.profile(True)
        fn()
        ctx.sync()
        out = {k: round(ms, 4) for k, (nl, ms) in sorted(ctx.profile_report().items(), key=lambda kv: -kv[1][1])}
        ctx.profile(False)
        return out

    split_plain, split_harq = split(plain), split(harq)
    ms_plain, ms_harq = float(np.median(t_plain)), float(np.median(t_harq))
    info = n * size
    res = {"workload": "pusch_harq3gpp", "units": n, "N_prb": N_PRB, "mod_type": MOD, "tbs": size, "code_blocks": n * lay["C"], "K": lay["K"],
           "decoder": "bcjr x8, exact interleaver", "n_buf": n, "pool_bytes": n * pool.buffer_bytes, "steps": args.steps, "warmup": args.warmup,
           "plain_ms": round(ms_plain, 3), "harq_ms": round(ms_harq, 3), "plain_ms_range": [round(min(t_plain), 3), round(max(t_plain), 3)],
           "harq_ms_range": [round(min(t_harq), 3), round(max(t_harq), 3)], "plain_info_gbit_per_s": round(info / ms_plain / 1e6, 3),
           "harq_info_gbit_per_s": round(info / ms_harq / 1e6, 3), "harq_rate_vs_plain": round(ms_plain / ms_harq, 4),
           "harq_kernels_ms": round(sum(v for k, v in split_harq.items() if k.startswith("k_harq_")), 4), "plain_kernel_ms": split_plain,
           "harq_kernel_ms": split_harq, "status_ok_plain": int((st == 0).sum()), "status_ok_harq": int((st_h == 0).sum()),
           "harq_rows_equal_plain": bool((bits == bits_h).all()), "distinct_units_equal_tx": bool(tx_ok), "buffer0_n_tx_after_timing": n_tx,
           "build_id": m.load_library().mi_lte_build_id().decode(), "device": ctx.device_name}
    print("HARQ run %.3f ms against the plain run's %.3f ms (%.1f %% of its rate)" % (ms_harq, ms_plain, 100 * res["harq_rate_vs_plain"]))
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write("# tools/pusch_harq_bench.py --units %d --steps %d --warmup %d on one MI355X (gfx950)\n" % (n, args.steps, args.warmup))
            f.write("# %d uplink units, one %d-PRB 64QAM grant of tbs %d (%d code blocks) each, with %d HARQ buffers (%.2f GB); plain_ms: the plain\n"
                    % (n, N_PRB, size, lay["C"], n, n * pool.buffer_bytes / 1e9))
            f.write("# plan run, harq_ms: the HARQ run of a further transmission (every buffer combined), alternating, medians; *_kernel_ms: one\n")
            f.write("# profiled run of each (mi_lte_profile_*), ms per kernel.  Reported, not gated.\n")
            f.write(line + "\n")
    for b in (d_sub, d_out, d_st, d_out_h, d_st_h):
        b.free()
    pool.close()
    plan.close()
    ctx.close()
    return 0 if (st == 0).all() and (st_h == 0).all() and tx_ok else 1


if __name__ == "__main__":
    sys.exit(main())
