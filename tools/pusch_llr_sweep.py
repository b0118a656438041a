#!/usr/bin/env python3
"""What the max-log soft-decision demapper of the 3GPP PUSCH plans (mi_lte_pusch_plan_set_demapper, MI_LTE_DEMAP_MAXLOG) buys on the uplink, in
dB, and the check of the automatic gain's constant T (MI_LTE_DEMAP_AUTO_T, chosen on the downlink by tools/demap_llr_sweep.py) against the
same set of candidates.  Traffic classes in a 25-RB cell, one code block each: 16QAM on 20 PRB and 64QAM on 14 PRB at code rate about 0.5, and
a 64QAM transport block on 22 PRB (code rate 0.30) -- each once with every unit's channel gain drawn from the synthesiser's
0.5 .. 1.5 and once at unit gain (`_flat`: the code's own waterfall) -- and further unit-gain classes the tests' value point is looked for
in: 64QAM at code rates 0.15 .. 0.75, two classes of two code blocks on 24 PRB and two of seven and five code blocks on 96 PRB of a 100-RB
cell.  All over
synth.ul_units_3gpp(..., max_delay=3); --blocks transport blocks (one per unit: its own cell, subframe, payload, channel and noise) per
point, 1 dB steps.  Per point: the share of blocks decoded (status 0 and the payload equal to the transmitted one) under BCJR x 8 with (a)
the default demapper and (b) MAXLOG under the automatic gain at T in demap_llr_sweep.T_SET (the library's MI_LTE_DEMAP_AUTO_T environment
variable, a tuning aid, stands in for the header's constant).  The SNR at 50 % block error is interpolated between the two points round
it; `gap_db` is (a) minus (b) at the header's T.  `keep_header_T`: no other T of the set is more than 0.2 dB better at 50 % block error in
both rate-0.5 classes with the spread of gains.

    python tools/pusch_llr_sweep.py [--blocks 16] [--snr-lo 0] [--snr-hi 26] [--out profiles/pusch_llr_sweep.txt]
Prints one JSON line last (and writes the table and the line to --out)."""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import openlte_amd as m  # noqa: E402
from openlte_amd import synth  # noqa: E402
from demap_llr_sweep import T_SET, snr_at_half  # noqa: E402

N_RB, FFT, ULC = 25, 512, (3, 0, 0, 2, 1)
SPREAD, FLAT = (0.5, 1.5), (1.0, 1.0)
# name -> (mod_type, N_prb, code rate, the synthesiser's range of channel gains)
CLASSES = {"16qam_r0.5": (2, 20, 0.5, SPREAD), "64qam_r0.5": (3, 14, 0.5, SPREAD), "64qam_r0.33": (3, 22, 0.33, SPREAD),
           "16qam_r0.5_flat": (2, 20, 0.5, FLAT), "64qam_r0.5_flat": (3, 14, 0.5, FLAT), "64qam_r0.33_flat": (3, 22, 0.33, FLAT),
           "64qam_r0.25_flat": (3, 24, 0.25, FLAT), "64qam_r0.2_flat": (3, 24, 0.2, FLAT), "64qam_r0.15_flat": (3, 24, 0.15, FLAT),
           "64qam_r0.6_flat": (3, 10, 0.6, FLAT), "64qam_r0.67_flat": (3, 10, 0.67, FLAT), "64qam_r0.75_flat": (3, 8, 0.75, FLAT),
           "64qam_r0.5_flat_2cb": (3, 24, 0.5, FLAT), "16qam_r0.5_flat_2cb": (2, 24, 0.5, FLAT),
           "64qam_r0.5_flat_100rb": (3, 96, 0.5, FLAT), "64qam_r0.33_flat_100rb": (3, 96, 0.33, FLAT),
           "64qam_r0.4_flat_100rb": (3, 96, 0.4, FLAT), "64qam_r0.25_flat_100rb": (3, 96, 0.25, FLAT), "64qam_r0.2_flat_100rb": (3, 96, 0.2, FLAT),
           "64qam_r0.15_flat_100rb": (3, 96, 0.15, FLAT), "16qam_r0.33_flat_100rb": (2, 96, 0.33, FLAT), "16qam_r0.2_flat_100rb": (2, 96, 0.2, FLAT)}
# 24 PRB at code rate 0.5: transport blocks of two code blocks; 96 PRB of a 100-RB cell: seven and five (every block has to pass: a steeper curve)
MULTI_BLOCK = tuple(n for n in CLASSES if n.endswith(("_2cb", "_100rb")))


def cell_of(name):
    """(N_rb_ul, FFT size) of a class's cell"""
    return (100, 2048) if name.endswith("_100rb") else (N_RB, FFT)
T_CLASSES = ("16qam_r0.5", "64qam_r0.5")
SEED0 = 3000


def tbs_for_rate(mod, n_prb, rate=0.5, one_block=True):
    """The size of Table 7.1.7.2.1-1's column n_prb (one code block unless told otherwise) whose tbs + 24 is nearest rate * G, G = 144 N_prb Q_m."""
    G = 144 * n_prb * {1: 2, 2: 4, 3: 6}[mod]
    L = m.load_library()
    sizes = sorted({int(L.mi_lte_tbs(i, n_prb)) for i in range(27)})
    return min((s for s in sizes if s + 24 <= 6144 or not one_block), key=lambda s: abs(s + 24 - rate * G)), G


def class_tbs(name):
    return tbs_for_rate(*CLASSES[name][:3], one_block=name not in MULTI_BLOCK)


def class_units(name, n_blocks):
    """(subframes, cells, allocations) of a class: one transport block per unit."""
    mod, n_prb, rate, _ = CLASSES[name]
    size, _ = class_tbs(name)
    sfs = [u % 10 for u in range(n_blocks)]
    cells = [(37 * u + 11) % 504 for u in range(n_blocks)]
    n_rb = cell_of(name)[0]
    allocs = [m.make_alloc(u, mod, size, list(range((3 * u) % (n_rb - n_prb), (3 * u) % (n_rb - n_prb) + n_prb)), 0x300 + u) for u in range(n_blocks)]
    return sfs, cells, allocs


def point_seed(name, snr_db):
    return SEED0 + 100 * list(CLASSES).index(name) + int(round(snr_db))


class Point:
    """One (class, SNR) point on the device: the units through the uplink front end, one 3GPP plan over them."""

    def __init__(self, ctx, name, snr_db, n_blocks):
        self.ctx, self.cfg, self.ul = ctx, m.DlCfg(cell_of(name)[1], cell_of(name)[0], 1, 0), m.UlCfg(*ULC)
        self.sfs, self.cells, self.allocs = class_units(name, n_blocks)
        iq, self.tx = synth.ul_units_3gpp(self.cfg, self.ul, self.sfs, self.cells, self.allocs, 1, gain=CLASSES[name][3], max_delay=3, snr_db=snr_db,
                                          peak=100.0, seed=point_seed(name, snr_db))
        _, self.d_sub = ctx.ul_frontend(self.cfg, iq.reshape(-1, 2), np.arange(n_blocks) * iq.shape[1], keep=True)
        self.plan = ctx.pusch_plan_3gpp(self.cfg, self.ul, self.sfs, self.cells, self.allocs)

    def decoded(self, mode, gain=0.0):
        """bool [n_blocks]: status 0 and the payload equal to the transmitted one"""
        self.plan.set_demapper(mode, gain)
        st, bits = self.plan.run(self.d_sub)
        return np.array([st[a] == 0 and (bits[a] == self.tx[a, 0, :al.tbs]).all() for a, al in enumerate(self.allocs)])

    def close(self):
        self.plan.close()
        self.d_sub.free()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=16)
    ap.add_argument("--snr-lo", type=int, default=0)
    ap.add_argument("--snr-hi", type=int, default=26)
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
        print("# %s done" % name, flush=True)
    half = {name: {c: snr_at_half(snrs, table[name][c]) for c in cols} for name in CLASSES}
    head = "T%d" % m.DEMAP_AUTO_T
    total = {t: sum(sum(table[n]["T%d" % t]) for n in T_CLASSES) * args.blocks for t in T_SET}

    def better(t, n):  # dB by which T = t beats the header's T at 50 % block error in class n (None: a curve without a crossing)
        a, b = half[n][head], half[n]["T%d" % t]
        return None if a is None or b is None else a - b

    wins = [t for t in T_SET if t != m.DEMAP_AUTO_T and all(better(t, n) is not None and better(t, n) > 0.2 for n in T_CLASSES)]
    gap = {n: (None if half[n]["ref"] is None or half[n][head] is None else round(half[n]["ref"] - half[n][head], 2)) for n in CLASSES}
    sizes = {n: {"mod_type": CLASSES[n][0], "N_prb": CLASSES[n][1], "tbs": class_tbs(n)[0], "G": class_tbs(n)[1],
                 "channel_gain": list(CLASSES[n][3])} for n in CLASSES}
    for n in CLASSES:
        sizes[n]["code_rate"] = round((sizes[n]["tbs"] + 24) / sizes[n]["G"], 3)
    out = {"workload": "pusch_llr_sweep", "n_rb_ul": N_RB, "blocks_per_point": args.blocks, "max_delay": 3, "decoder": "BCJR x 8", "classes": sizes,
           "snr_db": snrs, "decoded_share": table, "snr_db_at_half": half, "blocks_decoded_r0.5": {"T%d" % t: int(round(total[t])) for t in T_SET},
           "header_T": m.DEMAP_AUTO_T, "T_better_by_more_than_0.2_dB_in_both": wins, "keep_header_T": not wins, "gap_db": gap,
           "build_id": m.load_library().mi_lte_build_id().decode(), "device": ctx.device_name}
    lines = ["# tools/pusch_llr_sweep.py --blocks %d --snr-lo %d --snr-hi %d on one MI355X (gfx950)" % (args.blocks, args.snr_lo, args.snr_hi),
             "# share of transport blocks decoded per SNR point; ref: the default demapper, T<n>: MI_LTE_DEMAP_MAXLOG under the automatic gain with T = n.",
             "# snr_db_at_half: the interpolated SNR of 50 %% block error; gap_db: ref minus MAXLOG at the header's T = %d, what the soft decisions buy." % m.DEMAP_AUTO_T,
             "# blocks decoded over the two rate-0.5 classes with the spread of gains (%s); T more than 0.2 dB better than the header's in both at 50 %% block error: %s."
             % (", ".join("T%d: %d" % (t, round(total[t])) for t in T_SET), wins or "none")]
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
