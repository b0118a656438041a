#!/usr/bin/env python3
"""What MI_LTE_DEMAP_MAXLOG buys on a transmit-diversity plan (mi_lte_pdsch_plan_create_3gpp_txdiv, k_pdsch_demod_llr_txd) over the default
demapper, the reference's combiner with its sqrt(a0^2 + a1^2) normaliser and hard 16QAM / 64QAM decisions.  Two ports, a 25-RB cell, one code
block per transport block at code rate about 0.5: 64QAM on 14 PRB and 16QAM on 20 PRB with every port's gain drawn from 0.5 .. 1.5 (the two
ports of a unit differ by up to 9.5 dB, where the default normaliser is biased), and the same two classes with both ports at unit gain; over
synth.dl_units_3gpp_txdiv(..., max_delay=4); --blocks transport blocks (one per unit: its own cell, subframe, payload, channel and noise) per
point, 1 dB steps.  Per point: the share of blocks decoded (status 0 and the payload equal to the transmitted one) under BCJR x 8 with the
default demapper and with MAXLOG under the automatic gain.  The SNR at 50 % block error is interpolated between the two points round it;
`gap_db` is the default demapper's minus MAXLOG's.

    python tools/txdiv_llr_sweep.py [--blocks 16] [--snr-lo 0] [--snr-hi 26] [--out profiles/txdiv_llr_sweep.txt]
Prints one JSON line last (and writes the table and the line to --out)."""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import openlte_amd as m  # noqa: E402
from openlte_amd import synth  # noqa: E402

N_RB, FFT, CFI, N_SOFT, N_ANT = 25, 512, 2, 1237248, 2
# name -> (mod_type, N_prb, code rate, the synthesiser's range of per-port gains)
CLASSES = {"64qam_r0.5": (3, 14, 0.5, (0.5, 1.5)), "16qam_r0.5": (2, 20, 0.5, (0.5, 1.5)), "64qam_r0.5_flat": (3, 14, 0.5, (1.0, 1.0)),
           "16qam_r0.5_flat": (2, 20, 0.5, (1.0, 1.0))}
SEED0 = 3000


def tbs_for_rate(mod, n_prb, rate=0.5):
    """The one-block size of Table 7.1.7.2.1-1's column n_prb whose tbs + 24 is nearest rate * G (G of a two-port subframe without PBCH / sync
    signals: 8 resource elements per PRB in the three CRS symbols behind the control region, 12 in the other nine)."""
    G = n_prb * (12 * (14 - CFI) - 12) * {1: 2, 2: 4, 3: 6}[mod]
    L = m.load_library()
    sizes = sorted({int(L.mi_lte_tbs(i, n_prb)) for i in range(27)})
    return min((s for s in sizes if s + 24 <= 6144), key=lambda s: abs(s + 24 - rate * G)), G


def class_units(name, n_blocks):
    """(subframes, cells, allocations) of a class: one transport block per unit, never subframe 0 or 5."""
    mod, n_prb, rate, _ = CLASSES[name]
    size, _ = tbs_for_rate(mod, n_prb, rate)
    sfs = [(1, 2, 3, 4, 6, 7, 8, 9)[u % 8] for u in range(n_blocks)]
    cells = [(37 * u + 11) % 504 for u in range(n_blocks)]
    allocs = [m.make_alloc(u, mod, size, list(range((3 * u) % (N_RB - n_prb + 1), (3 * u) % (N_RB - n_prb + 1) + n_prb)), 0x300 + u, tx_mode=2)
              for u in range(n_blocks)]
    return sfs, cells, allocs


def point_seed(name, snr_db):
    return SEED0 + 100 * list(CLASSES).index(name) + int(round(snr_db))


class Point:
    """One (class, SNR) point on the device: the units through the front end, one transmit-diversity plan over them."""

    def __init__(self, ctx, name, snr_db, n_blocks):
        self.ctx, self.cfg = ctx, m.DlCfg(FFT, N_RB, N_ANT, 0)
        self.sfs, self.cells, self.allocs = class_units(name, n_blocks)
        iq, self.tx = synth.dl_units_3gpp_txdiv(self.cfg, self.sfs, self.cells, self.allocs, 1, N_SOFT, n_pdcch_symbs=CFI, gain=CLASSES[name][3],
                                                snr_db=snr_db, max_delay=4, seed=point_seed(name, snr_db))
        n, ul = n_blocks, iq.shape[1]
        d_iq, d_start = ctx.to_device(iq.reshape(-1, 2)), ctx.to_device((np.arange(n) * ul).astype(np.uint64))
        self.d_sf, self.d_cell = ctx.to_device(np.asarray(self.sfs, np.uint32)), ctx.to_device(np.asarray(self.cells, np.uint32))
        self.d_sub = ctx.alloc(n * ctx.subframe_floats(N_ANT) * 4)
        ctx.dl_frontend_dev(self.cfg, d_iq, None, d_start, self.d_sf, self.d_cell, n, self.d_sub)
        for b in (d_iq, d_start):
            b.free()
        self.plan = ctx.pdsch_plan_3gpp_txdiv(self.cfg, CFI, self.allocs, N_SOFT)

    def decoded(self, mode, gain=0.0):
        """bool [n_blocks]: status 0 and the payload equal to the transmitted one"""
        self.plan.set_demapper(mode, gain)
        st, bits = self.plan.run(self.d_sub, self.sfs, self.cells)
        return np.array([st[a] == 0 and (bits[a] == self.tx[a, 0, :al.tbs]).all() for a, al in enumerate(self.allocs)])

    def close(self):
        self.plan.close()
        for b in (self.d_sub, self.d_sf, self.d_cell):
            b.free()


def snr_at_half(snrs, share):
    """The SNR at which the decoded share first reaches 0.5 for good (linear between the last point under it and the next), or None."""
    below = [i for i, s in enumerate(share) if s < 0.5]
    if not below:
        return float(snrs[0])
    i = below[-1]
    if i + 1 >= len(snrs):
        return None
    return float(snrs[i] + (0.5 - share[i]) / (share[i + 1] - share[i]) * (snrs[i + 1] - snrs[i]))


def value_point(snrs, table, blocks):
    """The rule of the value tests: a class and SNR where MAXLOG decodes every block there and 1 dB below and the default demapper none there
    and 1 dB above ("window"); without one, the first point of the largest difference in decoded blocks ("largest_difference")."""
    for name in table:
        ref, ml = table[name]["ref"], table[name]["maxlog"]
        for i in range(1, len(snrs) - 1):
            if ml[i] == 1 and ml[i - 1] == 1 and ref[i] == 0 and ref[i + 1] == 0:
                return {"rule": "window", "class": name, "snr_db": snrs[i]}
    best = max(((table[n]["maxlog"][i] - table[n]["ref"][i], -k, -i) for k, n in enumerate(table) for i in range(len(snrs))))
    name, i = list(table)[-best[1]], -best[2]
    return {"rule": "largest_difference", "class": name, "snr_db": snrs[i], "maxlog_blocks": int(round(table[name]["maxlog"][i] * blocks)),
            "ref_blocks": int(round(table[name]["ref"][i] * blocks))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=16)
    ap.add_argument("--snr-lo", type=int, default=0)
    ap.add_argument("--snr-hi", type=int, default=26)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    snrs = list(range(args.snr_lo, args.snr_hi + 1))
    ctx = m.Context(0)
    cols = ["ref", "maxlog"]
    table = {name: {c: [] for c in cols} for name in CLASSES}
    for name in CLASSES:
        for snr in snrs:
            p = Point(ctx, name, float(snr), args.blocks)
            table[name]["ref"].append(float(p.decoded(m.DEMAP_REF).mean()))
            table[name]["maxlog"].append(float(p.decoded(m.DEMAP_MAXLOG).mean()))
            p.close()
    half = {name: {c: snr_at_half(snrs, table[name][c]) for c in cols} for name in CLASSES}
    gap = {n: (None if half[n]["ref"] is None or half[n]["maxlog"] is None else round(half[n]["ref"] - half[n]["maxlog"], 2)) for n in CLASSES}
    sizes = {n: {"mod_type": CLASSES[n][0], "N_prb": CLASSES[n][1], "tbs": tbs_for_rate(*CLASSES[n][:3])[0], "G": tbs_for_rate(*CLASSES[n][:3])[1],
                 "port_gain": list(CLASSES[n][3])} for n in CLASSES}
    for n in CLASSES:
        sizes[n]["code_rate"] = round((sizes[n]["tbs"] + 24) / sizes[n]["G"], 3)
    out = {"workload": "txdiv_llr_sweep", "n_rb_dl": N_RB, "n_ant": N_ANT, "cfi": CFI, "blocks_per_point": args.blocks, "max_delay": 4, "decoder": "BCJR x 8",
           "classes": sizes, "snr_db": snrs, "decoded_share": table, "snr_db_at_half": half, "gap_db": gap, "value_point": value_point(snrs, table, args.blocks),
           "auto_T": m.DEMAP_AUTO_T, "build_id": m.load_library().mi_lte_build_id().decode(), "device": ctx.device_name}
    lines = ["# tools/txdiv_llr_sweep.py --blocks %d --snr-lo %d --snr-hi %d on one MI355X (gfx950)" % (args.blocks, args.snr_lo, args.snr_hi),
             "# share of transport blocks decoded per SNR point on a two-port transmit-diversity plan; ref: the default demapper (the reference's",
             "# combiner and normaliser, hard 16QAM / 64QAM decisions), maxlog: MI_LTE_DEMAP_MAXLOG under the automatic gain (T = %d)." % m.DEMAP_AUTO_T,
             "# snr_db_at_half: the interpolated SNR of 50 % block error; gap_db: ref minus maxlog, what the soft decisions buy.",
             "# value_point: where tests/test_txdiv_gpu.py takes its value test from."]
    for name in CLASSES:
        lines.append("# %s (mod_type %d, %d PRB, tbs %d, G %d, code rate %.3f, port gain %.1f .. %.1f)"
                     % (name, sizes[name]["mod_type"], sizes[name]["N_prb"], sizes[name]["tbs"], sizes[name]["G"], sizes[name]["code_rate"],
                        CLASSES[name][3][0], CLASSES[name][3][1]))
        lines.append("#  SNR  " + "  ".join("%6s" % c for c in cols))
        for i, snr in enumerate(snrs):
            lines.append("# %4d  " % snr + "  ".join("%6.2f" % table[name][c][i] for c in cols))
        lines.append("#  50%   " + "  ".join("%6s" % ("-" if half[name][c] is None else "%.1f" % half[name][c]) for c in cols))
    print("\n".join(lines))
    line = json.dumps(out)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n" + line + "\n")
    ctx.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
