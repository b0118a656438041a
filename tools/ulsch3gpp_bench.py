#!/usr/bin/env python3
"""The PUSCH plans' 3GPP transport-block mode at full load: 2 048 uplink subframe units of a 20 MHz cell, each with one 99-PRB 64QAM grant of
TBS 73 712 (13 code blocks of K = 5696: 26 624 blocks), BCJR x 8 with the exact interleaver.  Reports the plan's run (demodulation + rate
un-matching + decode + finish; the front end runs once before) in ms and information Gbit/s, the per-kernel split, next to it
mi_lte_turbo_decode_batch BCJR x 8 on the same 26 624 rate-un-matched blocks (the plan's cb_soft tap): the decode alone -- and k_pusch_demod's
time in both variants from the same process: the 3GPP plan's and a reference-mode plan's over the same grids with one-block QPSK transport
blocks on the same 99 PRB (the reference-mode envelope; the demodulator's work does not depend on the transport block).

    python tools/ulsch3gpp_bench.py [--units 2048] [--steps 10] [--warmup 2] [--uci | --cqi]
--uci: the same grants with control information multiplexed on them (HARQ-ACK O = 1, Q' = 48; RI O = 2, Q' = 24; 600 coded CQI bits): the run of a
plan of mi_lte_pusch_plan_create_3gpp_uci against a plain 3GPP plan of the same build on the same subframes (alternated; the plain plan rate
un-matches over the wrong G and fails its CRCs there, which costs it nothing: the decoders run a fixed eight iterations), the per-kernel split with
k_ulsch_uci_gather and k_ulsch_uci_decide next to k_dl3_rm_i8, and the gather's bytes per second (every soft byte once in and once out).
--cqi: the --uci grants with real CQI reports in the 600 coded bits (mi_lte_cqi_encode: O = 11, the block code, on the even subframes, O = 64,
CRC8 and the convolutional code, on the odd ones) and the plan decoding them (mi_lte_pusch_plan_set_cqi_decode): the run with decoding off,
with every allocation decoded as O = 11 and with every allocation as O = 64, alternated (the kernel's work does not depend on what was sent),
k_ulsch_cqi_decode's own time in both, and the records of a run with each allocation's own O against the sent reports.
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

TBS, N_PRB = 73712, 99


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--units", type=int, default=2048)
    ap.add_argument("--unique", type=int, default=10, help="distinct synthesised subframes (subframe numbers 0..9), repeated over the units")
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--uci", action="store_true", help="the control-information leg (see above)")
    ap.add_argument("--cqi", action="store_true", help="the CQI decoding leg (see above)")
    args = ap.parse_args()
    cqi_leg_on, args.uci = args.cqi, args.uci or args.cqi
    ctx = m.Context(0)
    cfg, ul = m.DlCfg(2048, 100, 1, m.IQ_I8), m.UlCfg(3, 0, 0, 2, 1)
    nu, n, cell = args.unique, args.units, 42
    prbs = list(range(N_PRB))
    sfs_u = list(range(nu))
    ctl = m.UlschUci(1, 2, 48, 24, 600) if args.uci else None
    ack, ri = [[u & 1] for u in range(nu)], [[(u >> 1) & 1, u & 1] for u in range(nu)]
    cqi = np.random.default_rng(5).integers(0, 2, (nu, 600)).astype(np.uint8)
    cqi_O = [11 if u % 2 == 0 else 64 for u in range(nu)]
    cqi_o = [np.random.default_rng(50 + u).integers(0, 2, cqi_O[u]).astype(np.uint8) for u in range(nu)]
    if cqi_leg_on:
        cqi = np.stack([m.cqi_encode(cqi_O[u], cqi_o[u], 600) for u in range(nu)])
    iq, tx = synth.ul_units_3gpp(cfg, ul, sfs_u, [cell] * nu, [m.make_alloc(i, 3, TBS, prbs, 0x100 + i) for i in range(nu)], 1, snr_db=30.0,
                                 max_delay=3, seed=11, **(dict(uci=[ctl] * nu, ack=ack, ri=ri, cqi=cqi) if args.uci else {}))
    ulen = iq.shape[1]
    sfs = [sfs_u[u % nu] for u in range(n)]
    d_iq = ctx.to_device(iq.reshape(-1, 2))
    d_start = ctx.to_device(((np.arange(n) % nu) * ulen).astype(np.uint64))  # unit u reads the capture of distinct subframe u % unique
    d_sub = ctx.alloc(n * ctx.ul_subframe_floats() * 4)
    ctx.ul_frontend_dev(cfg, d_iq, None, d_start, n, d_sub)
    plan = ctx.pusch_plan_3gpp(cfg, ul, sfs, [cell] * n, [m.make_alloc(u, 3, TBS, prbs, 0x100 + u % nu) for u in range(n)])
    # the same grids, the same 99 PRB and 64QAM de-mapping through the reference-mode demodulator: a one-block transport block (its decode fails, which
    # is not what is timed)
    plan_ref = ctx.pusch_plan(cfg, ul, sfs, [cell] * n, [m.make_alloc(u, 3, 6120, prbs, 0x100 + u % nu) for u in range(n)])
    d_out, d_st = ctx.alloc(n * plan.out_stride), ctx.alloc(4 * n)

    def timed(fn):
        for _ in range(args.warmup):
            fn()
        ctx.sync()
        ctx.timer_start()
        for _ in range(args.steps):
            fn()
        return ctx.timer_stop() / args.steps

    if cqi_leg_on:
        plan_ref.close()
        plan.close()
        return cqi_leg(ctx, args, cfg, ul, sfs, cell, prbs, ctl, cqi_O, cqi_o, tx, d_sub, timed, d_out, d_st)
    if args.uci:
        plan_ref.close()
        return uci_leg(ctx, args, cfg, ul, sfs, cell, prbs, ctl, ack, ri, cqi, tx, d_sub, plan, timed, d_out, d_st)

    def profiled(p):
        ctx.profile(True)
        p.run_dev(d_sub, d_out, d_st)
        ctx.sync()
        rep = {k: round(ms, 4) for k, (nl, ms) in sorted(ctx.profile_report().items(), key=lambda kv: -kv[1][1])}
        ctx.profile(False)
        return rep

    ms_plan = timed(lambda: plan.run_dev(d_sub, d_out, d_st))
    st = d_st.download(np.int32)
    bits = d_out.download(np.uint8).reshape(n, plan.out_stride)
    tx_ok = all((bits[u, :TBS] == tx[u % nu, 0, :TBS]).all() for u in range(nu))
    split = profiled(plan)
    demod_ms = {"3gpp": [], "reference": []}
    for _ in range(3):  # alternated
        demod_ms["3gpp"].append(profiled(plan)["k_pusch_demod"])
        demod_ms["reference"].append(profiled(plan_ref)["k_pusch_demod"])

    p, nc, K = C.c_void_p(), C.c_uint32(), C.c_uint32()
    ctx._check(ctx.L.mi_lte_pusch_plan_cb_soft(plan.h, 0, C.byref(p), C.byref(nc), C.byref(K)))
    n_cb = n * nc.value
    d_c = ctx.alloc(n_cb * K.value)
    ms_dec = timed(lambda: ctx._check(ctx.L.mi_lte_turbo_decode_batch(ctx.h, p, m.SOFT_I8, K.value, n_cb, m.TURBO_BCJR, 8, 1, d_c.ptr)))
    info = n * TBS
    res = {"workload": "ulsch3gpp", "units": n, "tbs": TBS, "n_prb": N_PRB, "code_blocks": n_cb, "K": K.value, "decoder": "bcjr x8, exact interleaver",
           "steps": args.steps, "warmup": args.warmup, "plan_ms": round(ms_plan, 3), "plan_info_gbit_per_s": round(info / ms_plan / 1e6, 3),
           "decode_batch_ms": round(ms_dec, 3), "decode_batch_info_gbit_per_s": round(info / ms_dec / 1e6, 3),
           "plan_rate_vs_decode_batch": round(ms_dec / ms_plan, 4), "plan_kernel_ms": split, "k_pusch_demod_ms": demod_ms,
           "status_ok": int((st == 0).sum()), "distinct_units_equal_tx": bool(tx_ok), "device": ctx.device_name}
    print("3GPP PUSCH plan: %.3f ms per run of %d units (%.2f Gbit/s information), decode_batch alone %.3f ms (%.2f Gbit/s): %.1f %%"
          % (ms_plan, n, res["plan_info_gbit_per_s"], ms_dec, res["decode_batch_info_gbit_per_s"], 100 * res["plan_rate_vs_decode_batch"]))
    print("k_pusch_demod, ms per run: 3GPP variant %s, reference variant %s" % (demod_ms["3gpp"], demod_ms["reference"]))
    print(json.dumps(res))
    plan.close()
    plan_ref.close()
    ctx.close()
    return 0 if (st == 0).all() and tx_ok else 1


def uci_leg(ctx, args, cfg, ul, sfs, cell, prbs, ctl, ack, ri, cqi, tx, d_sub, plan, timed, d_out, d_st):
    n, nu = args.units, args.unique
    plan_uci = ctx.pusch_plan_3gpp(cfg, ul, sfs, [cell] * n, [m.make_alloc(u, 3, TBS, prbs, 0x100 + u % nu) for u in range(n)], uci=[ctl] * n)
    ms = {"uci": [], "plain": []}
    for _ in range(3):  # alternated
        ms["uci"].append(round(timed(lambda: plan_uci.run_dev(d_sub, d_out, d_st)), 3))
        ms["plain"].append(round(timed(lambda: plan.run_dev(d_sub, d_out, d_st)), 3))
    plan_uci.run_dev(d_sub, d_out, d_st)
    st = d_st.download(np.int32)
    bits = d_out.download(np.uint8).reshape(n, plan.out_stride)
    rec = plan_uci.uci_results()
    tx_ok = all((bits[u, :TBS] == tx[u % nu, 0, :TBS]).all() for u in range(nu))
    ctl_ok = all(rec[u]["ack"][:1] == ack[u % nu] and rec[u]["ri"] == ri[u % nu] for u in range(n))
    cq = plan_uci.cqi_soft(0)
    cqi_ok = bool((((cq < 0) == (cqi[0] == 1)) | (cq == 0)).all())
    ctx.profile(True)
    plan_uci.run_dev(d_sub, d_out, d_st)
    ctx.sync()
    split = {k: round(v[1], 4) for k, v in sorted(ctx.profile_report().items(), key=lambda kv: -kv[1][1])}
    ctx.profile(False)
    run_bytes = m.ulsch_uci_G(N_PRB, 6, ctl) + ctl.Q_cqi
    gather_tb_s = 2.0 * n * run_bytes / (split["k_ulsch_uci_gather"] * 1e-3) / 1e12
    res = {"workload": "ulsch3gpp_uci", "units": n, "tbs": TBS, "n_prb": N_PRB, "uci": {"O_ack": 1, "Qp_ack": 48, "O_ri": 2, "Qp_ri": 24, "Q_cqi": 600},
           "steps": args.steps, "warmup": args.warmup, "plan_uci_ms": ms["uci"], "plan_plain_ms": ms["plain"],
           "uci_over_plain": round(min(ms["uci"]) / min(ms["plain"]), 4), "plan_kernel_ms": split, "gather_bytes_in_plus_out": 2 * n * run_bytes,
           "gather_tb_per_s": round(gather_tb_s, 3), "status_ok": int((st == 0).sum()), "distinct_units_equal_tx": bool(tx_ok),
           "control_bits_equal_tx": bool(ctl_ok), "cqi_signs_equal_tx": cqi_ok, "device": ctx.device_name}
    print("3GPP PUSCH plan with control information: %s ms per run of %d units, plain plan on the same subframes %s ms" % (ms["uci"], n, ms["plain"]))
    print("k_ulsch_uci_gather %.4f ms (%.2f TB/s in + out), k_ulsch_uci_decide %.4f ms, k_dl3_rm_i8 %.4f ms"
          % (split["k_ulsch_uci_gather"], gather_tb_s, split["k_ulsch_uci_decide"], split["k_dl3_rm_i8"]))
    print(json.dumps(res))
    plan_uci.close()
    plan.close()
    ctx.close()
    return 0 if (st == 0).all() and tx_ok and ctl_ok and cqi_ok else 1


def cqi_leg(ctx, args, cfg, ul, sfs, cell, prbs, ctl, cqi_O, cqi_o, tx, d_sub, timed, d_out, d_st):
    n, nu = args.units, args.unique
    plan = ctx.pusch_plan_3gpp(cfg, ul, sfs, [cell] * n, [m.make_alloc(u, 3, TBS, prbs, 0x100 + u % nu) for u in range(n)], uci=[ctl] * n)
    legs = {"off": None, "O11": [11] * n, "O64": [64] * n}
    ms, kernel_ms = {k: [] for k in legs}, {}
    for _ in range(3):  # alternated
        for k, O_list in legs.items():
            plan.set_cqi_decode(O_list)
            ms[k].append(round(timed(lambda: plan.run_dev(d_sub, d_out, d_st)), 3))
    for k, O_list in legs.items():
        plan.set_cqi_decode(O_list)
        plan.run_dev(d_sub, d_out, d_st)
        ctx.profile(True)
        plan.run_dev(d_sub, d_out, d_st)
        ctx.sync()
        rep = ctx.profile_report()
        ctx.profile(False)
        kernel_ms[k] = {name: round(rep[name][1], 4) for name in ("k_ulsch_uci_gather", "k_ulsch_uci_decide", "k_ulsch_cqi_decode") if name in rep}
    plan.set_cqi_decode([cqi_O[u % nu] for u in range(n)])
    plan.run_dev(d_sub, d_out, d_st)
    st = d_st.download(np.int32)
    bits = d_out.download(np.uint8).reshape(n, plan.out_stride)
    rec = plan.cqi_results()
    tx_ok = all((bits[u, :TBS] == tx[u % nu, 0, :TBS]).all() for u in range(nu))

    def sent(u):
        O, words = cqi_O[u % nu], [0, 0, 0, 0]
        for i, b in enumerate(cqi_o[u % nu]):
            words[i >> 5] |= int(b) << (i & 31)
        return (O, m.CQI_NO_CRC if O <= 11 else m.CQI_CRC_OK, words)

    cqi_ok = all((rec[u]["O"], rec[u]["crc"], rec[u]["bits"]) == sent(u) for u in range(n))
    res = {"workload": "ulsch3gpp_cqi", "units": n, "tbs": TBS, "n_prb": N_PRB, "uci": {"O_ack": 1, "Qp_ack": 48, "O_ri": 2, "Qp_ri": 24, "Q_cqi": 600},
           "steps": args.steps, "warmup": args.warmup, "plan_ms": ms, "on_minus_off_ms": {k: round(min(ms[k]) - min(ms["off"]), 3) for k in ("O11", "O64")},
           "kernel_ms": kernel_ms, "status_ok": int((st == 0).sum()), "distinct_units_equal_tx": bool(tx_ok), "cqi_reports_equal_tx": bool(cqi_ok),
           "record_0": rec[0], "record_1": rec[1], "device": ctx.device_name}
    print("3GPP PUSCH plan with control information, ms per run of %d units: CQI decoding off %s, O = 11 %s, O = 64 %s" % (n, ms["off"], ms["O11"], ms["O64"]))
    print("k_ulsch_cqi_decode: O = 11 %.4f ms, O = 64 %.4f ms; k_ulsch_uci_gather %.4f ms"
          % (kernel_ms["O11"]["k_ulsch_cqi_decode"], kernel_ms["O64"]["k_ulsch_cqi_decode"], kernel_ms["off"]["k_ulsch_uci_gather"]))
    print(json.dumps(res))
    plan.close()
    ctx.close()
    return 0 if (st == 0).all() and tx_ok and cqi_ok else 1


if __name__ == "__main__":
    sys.exit(main())
