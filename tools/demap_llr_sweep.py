#!/usr/bin/env python3
"""What the max-log soft-decision demapper of the 3GPP PDSCH plans (mi_lte_pdsch_plan_set_demapper, MI_LTE_DEMAP_MAXLOG) buys, in dB, and the
sweep its automatic gain's constant T (MI_LTE_DEMAP_AUTO_T) is chosen by.  Two traffic classes in a 25-RB cell, one code block each, code rate
about 0.5: 64QAM on 14 PRB and 16QAM on 20 PRB (and two for the tests, at one channel gain for every unit: the first again, and the same
transport block at code rate 0.33), over synth.dl_units_3gpp(..., max_delay=4); --blocks transport blocks (one per unit: its own
cell, subframe, payload, channel and noise) per point, 1 dB steps.  Per point: the share of blocks decoded (status 0 and the payload equal to
the transmitted one) under BCJR x 8 with (a) the default demapper and (b) MAXLOG under the automatic gain at T in {8, 16, 24, 32, 48} (the
library's MI_LTE_DEMAP_AUTO_T environment variable, a tuning aid, stands in for the header's constant).  The SNR at 50 % block error is
interpolated between the two points round it; `gap_db` is (a) minus (b).

    python tools/demap_llr_sweep.py [--blocks 16] [--snr-lo 2] [--snr-hi 30] [--out profiles/demap_llr_sweep.txt]
Prints one JSON line last (and writes the table and the line to --out)."""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import openlte_amd as m  # noqa: E402
from openlte_amd import synth  # noqa: E402

N_RB, FFT, CFI, N_SOFT = 25, 512, 2, 1237248
T_SET = (8, 16, 24, 32, 48)
# name -> (mod_type, N_prb, code rate, the synthesiser's range of channel gains).  The first two are the classes T is chosen on: every unit draws
# its gain from 0.5 .. 1.5, 9.5 dB between the weakest and the strongest block, which is what spreads their curves over some 8 dB.
# The _flat classes have every unit at gain 1, so that a point's blocks differ in payload, cell, delay, phase and noise alone and the curve is
# the code's own waterfall: 64qam_r0.5_flat is the first class again, 64qam_r0.33_flat the same transport block on 22 PRB.  The tests
# (tests/test_demap_llr_gpu.py) take their HARQ and value points from them.
CLASSES = {"64qam_r0.5": (3, 14, 0.5, (0.5, 1.5)), "16qam_r0.5": (2, 20, 0.5, (0.5, 1.5)), "64qam_r0.5_flat": (3, 14, 0.5, (1.0, 1.0)),
           "64qam_r0.33_flat": (3, 22, 0.33, (1.0, 1.0))}
T_CLASSES = ("64qam_r0.5", "16qam_r0.5")
SEED0 = 1000


def tbs_for_rate(mod, n_prb, rate=0.5):
    """The one-block size of Table 7.1.7.2.1-1's column n_prb whose tbs + 24 is nearest rate * G (G of a subframe without PBCH / sync signals)."""
    G = n_prb * (12 * (14 - CFI) - 6) * {1: 2, 2: 4, 3: 6}[mod]
    L = m.load_library()
    sizes = sorted({int(L.mi_lte_tbs(i, n_prb)) for i in range(27)})
    return min((s for s in sizes if s + 24 <= 6144), key=lambda s: abs(s + 24 - rate * G)), G


def class_units(name, n_blocks):
    """(subframes, cells, allocations) of a class: one transport block per unit, never subframe 0 or 5."""
    mod, n_prb, rate, _ = CLASSES[name]
    size, _ = tbs_for_rate(mod, n_prb, rate)
    sfs = [(1, 2, 3, 4, 6, 7, 8, 9)[u % 8] for u in range(n_blocks)]
    cells = [(37 * u + 11) % 504 for u in range(n_blocks)]
    allocs = [m.make_alloc(u, mod, size, list(range((3 * u) % (N_RB - n_prb + 1), (3 * u) % (N_RB - n_prb + 1) + n_prb)), 0x300 + u) for u in range(n_blocks)]
    return sfs, cells, allocs


def point_seed(name, snr_db):
    return SEED0 + 100 * list(CLASSES).index(name) + int(round(snr_db))


class Point:
    """One (class, SNR) point on the device: the units through the front end, one 3GPP plan over them."""

    def __init__(self, ctx, name, snr_db, n_blocks):
        self.ctx, self.cfg = ctx, m.DlCfg(FFT, N_RB, 1, 0)
        self.sfs, self.cells, self.allocs = class_units(name, n_blocks)
        iq, self.tx = synth.dl_units_3gpp(self.cfg, self.sfs, self.cells, self.allocs, 1, N_SOFT, n_pdcch_symbs=CFI, gain=CLASSES[name][3], snr_db=snr_db,
                                          max_delay=4, seed=point_seed(name, snr_db))
        n, ul = n_blocks, iq.shape[1]
        d_iq, d_start = ctx.to_device(iq.reshape(-1, 2)), ctx.to_device((np.arange(n) * ul).astype(np.uint64))
        d_sf, d_cell = ctx.to_device(np.asarray(self.sfs, np.uint32)), ctx.to_device(np.asarray(self.cells, np.uint32))
        self.d_sub = ctx.alloc(n * ctx.subframe_floats(1) * 4)
        ctx.dl_frontend_dev(self.cfg, d_iq, None, d_start, d_sf, d_cell, n, self.d_sub)
        for b in (d_iq, d_start, d_sf, d_cell):
            b.free()
        self.plan = ctx.pdsch_plan_3gpp(self.cfg, CFI, self.allocs, N_SOFT)

    def decoded(self, mode, gain=0.0):
        """bool [n_blocks]: status 0 and the payload equal to the transmitted one"""
        self.plan.set_demapper(mode, gain)
        st, bits = self.plan.run(self.d_sub, self.sfs, self.cells)
        return np.array([st[a] == 0 and (bits[a] == self.tx[a, 0, :al.tbs]).all() for a, al in enumerate(self.allocs)])

    def close(self):
        self.plan.close()
        self.d_sub.free()


def snr_at_half(snrs, share):
    """The SNR at which the decoded share first reaches 0.5 for good (linear between the last point under it and the next), or None."""
    below = [i for i, s in enumerate(share) if s < 0.5]
    if not below:
        return float(snrs[0])
    i = below[-1]
    if i + 1 >= len(snrs):
        return None
    return float(snrs[i] + (0.5 - share[i]) / (share[i + 1] - share[i]) * (snrs[i + 1] - snrs[i]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=16)
    ap.add_argument("--snr-lo", type=int, default=2)
    ap.add_argument("--snr-hi", type=int, default=30)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    snrs = list(range(args.snr_lo, args.snr_hi + 1))
    ctx = m.Context(0)
    cols = ["ref"] + ["T%d" % t for t in T_SET]
    table = {name: {c: [] for c in cols} for name in CLASSES}
    for name in CLASSES:
        for snr in snrs:
            p = Point(ctx, name, float(snr), args.blocks)
            table[name]["ref"].append(float(p.decoded(m.DEMAP_REF).mean()))
            for t in T_SET:
                os.environ["MI_LTE_DEMAP_AUTO_T"] = str(t)
                table[name]["T%d" % t].append(float(p.decoded(m.DEMAP_MAXLOG).mean()))
            os.environ.pop("MI_LTE_DEMAP_AUTO_T")
            p.close()
    half = {name: {c: snr_at_half(snrs, table[name][c]) for c in cols} for name in CLASSES}
    # T: the most transport blocks decoded over every point of the two rate-0.5 classes; among equals the smallest, which leaves the most
    # room under the +-127 clamp for the sums of rate un-matching and HARQ combining
    total = {t: sum(sum(table[n]["T%d" % t]) for n in T_CLASSES) * args.blocks for t in T_SET}
    best = min(T_SET, key=lambda t: (-round(total[t]), t))
    gap = {n: (None if half[n]["ref"] is None or half[n]["T%d" % best] is None else round(half[n]["ref"] - half[n]["T%d" % best], 2)) for n in CLASSES}
    sizes = {n: {"mod_type": CLASSES[n][0], "N_prb": CLASSES[n][1], "tbs": tbs_for_rate(*CLASSES[n][:3])[0], "G": tbs_for_rate(*CLASSES[n][:3])[1],
                 "channel_gain": list(CLASSES[n][3])} for n in CLASSES}
    for n in CLASSES:
        sizes[n]["code_rate"] = round((sizes[n]["tbs"] + 24) / sizes[n]["G"], 3)
    out = {"workload": "demap_llr_sweep", "n_rb_dl": N_RB, "cfi": CFI, "blocks_per_point": args.blocks, "max_delay": 4, "decoder": "BCJR x 8", "classes": sizes,
           "snr_db": snrs, "decoded_share": table, "snr_db_at_half": half, "blocks_decoded_r0.5": {"T%d" % t: int(round(total[t])) for t in T_SET}, "best_T": best, "header_T": m.DEMAP_AUTO_T, "gap_db": gap,
           "build_id": m.load_library().mi_lte_build_id().decode(), "device": ctx.device_name}
    lines = ["# tools/demap_llr_sweep.py --blocks %d --snr-lo %d --snr-hi %d on one MI355X (gfx950)" % (args.blocks, args.snr_lo, args.snr_hi),
             "# share of transport blocks decoded per SNR point; ref: the default demapper, T<n>: MI_LTE_DEMAP_MAXLOG under the automatic gain with T = n.",
             "# snr_db_at_half: the interpolated SNR of 50 % block error; gap_db: ref minus MAXLOG at best_T, what the soft decisions buy.",
             "# best_T: the T with the most blocks decoded over the two rate-0.5 classes (%s), the smallest among equals."
             % ", ".join("T%d: %d" % (t, round(total[t])) for t in T_SET)]
    for name in CLASSES:
        lines.append("# %s (mod_type %d, %d PRB, tbs %d, G %d, code rate %.3f, channel gain %.1f .. %.1f)"
                     % (name, sizes[name]["mod_type"], sizes[name]["N_prb"], sizes[name]["tbs"], sizes[name]["G"], sizes[name]["code_rate"],
                        CLASSES[name][3][0], CLASSES[name][3][1]))
        lines.append("#  SNR  " + "  ".join("%5s" % c for c in cols))
        for i, snr in enumerate(snrs):
            lines.append("# %4d  " % snr + "  ".join("%5.2f" % table[name][c][i] for c in cols))
        lines.append("#  50%   " + "  ".join("%5s" % ("-" if half[name][c] is None else "%.1f" % half[name][c]) for c in cols))
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
