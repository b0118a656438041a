#!/usr/bin/env python3
"""The PDSCH plans' 3GPP transport-block mode at full load: 2 048 subframe units of a 20 MHz single-port cell, each with one 100-PRB 64QAM
allocation of TBS 75 376 (13 code blocks of K = 5824: 26 624 blocks), CFI 1, BCJR x 8 with the exact interleaver.  Reports the plan's run
(demodulation + rate un-matching + decode + finish; the front end runs once before) in ms and information Gbit/s, the per-kernel split, and
next to it mi_lte_turbo_decode_batch BCJR x 8 on the same 26 624 rate-un-matched blocks (the plan's cb_soft tap): the decode alone.

    python tools/dlsch3gpp_bench.py [--units 2048] [--steps 10] [--warmup 2] [--n-soft 1237248]
Prints one JSON line last."""
import argparse
import ctypes as C
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
    d_start = ctx.to_device(((np.arange(n) % nu) * ul).astype(np.uint64))  # unit u reads the capture of distinct subframe u % unique
    d_sf, d_cell = ctx.to_device(np.asarray(sfs, np.uint32)), ctx.to_device(np.asarray(cells, np.uint32))
    d_sub = ctx.alloc(n * ctx.subframe_floats(1) * 4)
    ctx.dl_frontend_dev(cfg, d_iq, None, d_start, d_sf, d_cell, n, d_sub)
    plan = ctx.pdsch_plan_3gpp(cfg, 1, allocs, args.n_soft)
    d_out, d_st = ctx.alloc(n * plan.out_stride), ctx.alloc(4 * n)

    def timed(fn):
        for _ in range(args.warmup):
            fn()
        ctx.sync()
        ctx.timer_start()
        for _ in range(args.steps):
            fn()
        return ctx.timer_stop() / args.steps

    ms_plan = timed(lambda: plan.run_dev(d_sub, d_sf, d_cell, d_out, d_st))
    st = d_st.download(np.int32)
    bits = d_out.download(np.uint8).reshape(n, plan.out_stride)
    tx_ok = all((bits[u, :TBS] == tx[u % nu, 0, :TBS]).all() for u in range(nu))
    ctx.profile(True)
    plan.run_dev(d_sub, d_sf, d_cell, d_out, d_st)
    ctx.sync()
    split = {k: round(ms, 4) for k, (nl, ms) in sorted(ctx.profile_report().items(), key=lambda kv: -kv[1][1])}
    ctx.profile(False)

    # the same blocks through mi_lte_turbo_decode_batch (one block size: the plan's blocks are contiguous from allocation 0's)
    p, nc, K = C.c_void_p(), C.c_uint32(), C.c_uint32()
    ctx._check(ctx.L.mi_lte_pdsch_plan_cb_soft(plan.h, 0, C.byref(p), C.byref(nc), C.byref(K)))
    n_cb = n * nc.value
    d_c = ctx.alloc(n_cb * K.value)
    ms_dec = timed(lambda: ctx._check(ctx.L.mi_lte_turbo_decode_batch(ctx.h, p, m.SOFT_I8, K.value, n_cb, m.TURBO_BCJR, 8, 1, d_c.ptr)))
    info = n * TBS
    res = {"workload": "dlsch3gpp", "units": n, "tbs": TBS, "code_blocks": n_cb, "K": K.value, "decoder": "bcjr x8, exact interleaver", "n_soft": args.n_soft,
           "steps": args.steps, "warmup": args.warmup, "plan_ms": round(ms_plan, 3), "plan_info_gbit_per_s": round(info / ms_plan / 1e6, 3),
           "decode_batch_ms": round(ms_dec, 3), "decode_batch_info_gbit_per_s": round(info / ms_dec / 1e6, 3),
           "plan_rate_vs_decode_batch": round(ms_dec / ms_plan, 4), "plan_kernel_ms": split,
           "status_ok": int((st == 0).sum()), "distinct_units_equal_tx": bool(tx_ok), "device": ctx.device_name}
    print("3GPP plan: %.3f ms per run of %d units (%.2f Gbit/s information), decode_batch alone %.3f ms (%.2f Gbit/s): %.1f %%"
          % (ms_plan, n, res["plan_info_gbit_per_s"], ms_dec, res["decode_batch_info_gbit_per_s"], 100 * res["plan_rate_vs_decode_batch"]))
    print(json.dumps(res))
    plan.close()
    ctx.close()
    return 0 if (st == 0).all() and tx_ok else 1


if __name__ == "__main__":
    sys.exit(main())
