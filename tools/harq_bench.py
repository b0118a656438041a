#!/usr/bin/env python3
"""HARQ soft combining in the 3GPP transport-block mode at full load: tools/dlsch3gpp_bench.py's batch (2 048 subframe units of a 20 MHz
single-port cell, one 100-PRB 64QAM allocation of TBS 75 376 each: 13 code blocks of K = 5824, CFI 1, BCJR x 8, exact interleaver) with a
pool of 2 048 soft buffers, one per unit (mi_lte_harq_buffer_bytes(75376) = 454 584 bytes each, 0.93 GB).

After one HARQ run with NEW_DATA (the first transmission), the plain plan run (mi_lte_pdsch_decode_run) and the HARQ run of a further
transmission (mi_lte_pdsch_decode_run_harq without NEW_DATA: every buffer read, combined and written back) are timed alternately, one run
each per step, in one process; then one profiled run of each gives the per-kernel split.

    python tools/harq_bench.py [--units 2048] [--steps 10] [--warmup 2] [--n-soft 1237248] [--out profiles/harq_bench.txt]
Prints one JSON line last (and writes it to --out with a header)."""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import openlte_amd as m  # noqa: E402
from openlte_amd import synth  # noqa: E402

TBS = 75376


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--units", type=int, default=2048)
    ap.add_argument("--unique", type=int, default=10, help="distinct synthesised subframes (subframe numbers 0..9), repeated over the units")
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--n-soft", type=int, default=1237248)
    ap.add_argument("--out", default=None, help="also write the JSON line (with a header) to this file")
    args = ap.parse_args()
    ctx = m.Context(0)
    cfg = m.DlCfg(2048, 100, 1, m.IQ_I8)
    nu, n = args.unique, args.units
    sfs_u, cells_u = list(range(nu)), [(17 * i + 3) % 504 for i in range(nu)]
    allocs_u = [m.make_alloc(i, 3, TBS, list(range(100)), 0x100 + i) for i in range(nu)]
    iq, tx = synth.dl_units_3gpp(cfg, sfs_u, cells_u, allocs_u, 1, args.n_soft, n_pdcch_symbs=1, snr_db=30.0, max_delay=4, seed=11)
    ul = iq.shape[1]
    sfs, cells = [sfs_u[u % nu] for u in range(n)], [cells_u[u % nu] for u in range(n)]
    allocs = [m.make_alloc(u, 3, TBS, list(range(100)), 0x100 + u % nu) for u in range(n)]
    d_iq = ctx.to_device(iq.reshape(-1, 2))
    d_start = ctx.to_device(((np.arange(n) % nu) * ul).astype(np.uint64))
    d_sf, d_cell = ctx.to_device(np.asarray(sfs, np.uint32)), ctx.to_device(np.asarray(cells, np.uint32))
    d_sub = ctx.alloc(n * ctx.subframe_floats(1) * 4)
    ctx.dl_frontend_dev(cfg, d_iq, None, d_start, d_sf, d_cell, n, d_sub)
    plan = ctx.pdsch_plan_3gpp(cfg, 1, allocs, args.n_soft)
    pool = ctx.harq_pool(n, TBS)
    d_out, d_st = ctx.alloc(n * plan.out_stride), ctx.alloc(4 * n)
    d_out_h, d_st_h = ctx.alloc(n * plan.out_stride), ctx.alloc(4 * n)
    first, again = m.harq_binds(n, range(n), True), m.harq_binds(n, range(n), False)

    def plain():
        plan.run_dev(d_sub, d_sf, d_cell, d_out, d_st)

    def harq():
        plan.run_harq_dev(pool, again, d_sub, d_sf, d_cell, d_out_h, d_st_h)

    plan.run_harq_dev(pool, first, d_sub, d_sf, d_cell, d_out_h, d_st_h)  # the first transmission fills every buffer
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
    tx_ok = all((bits_h[u, :TBS] == tx[u % nu, 0, :TBS]).all() for u in range(nu))
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
    harq_kernels_ms = round(sum(v for k, v in split_harq.items() if k.startswith("k_harq_")), 4)
    info = n * TBS
    res = {"workload": "harq3gpp", "units": n, "tbs": TBS, "code_blocks": n * 13, "K": 5824, "decoder": "bcjr x8, exact interleaver",
           "n_soft": args.n_soft, "n_buf": n, "pool_bytes": n * pool.buffer_bytes, "steps": args.steps, "warmup": args.warmup,
           "plain_ms": round(ms_plain, 3), "harq_ms": round(ms_harq, 3), "plain_ms_range": [round(min(t_plain), 3), round(max(t_plain), 3)],
           "harq_ms_range": [round(min(t_harq), 3), round(max(t_harq), 3)], "plain_info_gbit_per_s": round(info / ms_plain / 1e6, 3),
           "harq_info_gbit_per_s": round(info / ms_harq / 1e6, 3), "harq_rate_vs_plain": round(ms_plain / ms_harq, 4),
           "harq_kernels_ms": harq_kernels_ms, "target_rate_vs_plain": 0.95, "target_harq_kernels_ms": 2.0,
           "meets_targets": bool(ms_plain / ms_harq >= 0.95 and harq_kernels_ms <= 2.0), "plain_kernel_ms": split_plain, "harq_kernel_ms": split_harq,
           "status_ok_plain": int((st == 0).sum()), "status_ok_harq": int((st_h == 0).sum()), "harq_rows_equal_plain": bool((bits == bits_h).all()),
           "distinct_units_equal_tx": bool(tx_ok), "buffer0_n_tx_after_timing": n_tx, "device": ctx.device_name}
    print("HARQ run %.3f ms against the plain run's %.3f ms (%.1f %% of its rate); k_harq_* %.3f ms"
          % (ms_harq, ms_plain, 100 * res["harq_rate_vs_plain"], harq_kernels_ms))
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write("# tools/harq_bench.py --steps %d --warmup %d on one MI355X (gfx950)\n" % (args.steps, args.warmup))
            f.write("# tools/dlsch3gpp_bench.py's batch (%d units, one 13-block TBS 75 376 grant each) with %d HARQ buffers (%.2f GB); plain_ms: the\n"
                    % (n, n, n * pool.buffer_bytes / 1e9))
            f.write("# plain plan run, harq_ms: the HARQ run of a further transmission (every buffer combined), alternating, medians;\n")
            f.write("# *_kernel_ms: one profiled run of each (mi_lte_profile_*), ms per kernel.  Targets: >= 95 % of the plain rate, k_harq_* <= 2 ms.\n")
            f.write(line + "\n")
    for b in (d_iq, d_start, d_sf, d_cell, d_sub, d_out, d_st, d_out_h, d_st_h):
        b.free()
    pool.close()
    plan.close()
    ctx.close()
    return 0 if (st == 0).all() and (st_h == 0).all() and tx_ok else 1


if __name__ == "__main__":
    sys.exit(main())
