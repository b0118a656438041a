#!/usr/bin/env python3
"""What the noise-referenced LLR gain of the 3GPP PUSCH plans (mi_lte_pusch_plan_set_llr_noise) buys HARQ combining on the uplink
(mi_lte_pusch_decode_run_harq), and which `scale` to recommend.  Every transport block is sent twice with the same payload, rv 0 then rv 2,
each transmission with its own subframe, seed, channel phase, delay and noise (synth.ul_units_3gpp(..., gain=(1, 1), max_delay=3)), and
both are combined in a pool buffer; a block counts when the second run returns status 0 and the transmitted payload.  Classes:

  16qam_25prb_plus8db    16QAM on 25 PRB of a 50-RB cell, first-transmission code rate about 0.75 (one code block short of three); the
                         second transmission 8 dB above the first
  64qam_then_qpsk        the same SNR for both; 64QAM on 12 PRB of a 25-RB cell at code rate about 0.75, the retransmission QPSK on 24 PRB
  16qam_96prb_plus8db    the first class with six code blocks on 96 PRB of a 100-RB cell (the size of the column with C = 6 nearest 0.75)

Modes: R the default demapper, A MAXLOG under the automatic gain, N<s> MAXLOG under the noise-referenced gain with scale s in SCALES.
BCJR x 8, --blocks transport blocks (one per unit) per point, 1 dB steps of the first transmission's SNR.  The recommended scale is the one
that decodes the most blocks over all classes and points (ties: the smaller).  `windows`: per class and scale the points p at which N
decodes every block at p and p - 1 and A none at p and p + 1 (the rule of DESIGN.md section 8's value tests); `largest_difference`: per
class the point where N at the recommended scale leads A by the most blocks.

    python tools/pusch_harq_sweep.py [--blocks 16] [--snr-lo -6] [--snr-hi 16] [--out profiles/pusch_harq_sweep.txt]
Prints one JSON line last (and writes the table and the line to --out)."""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import openlte_amd as m  # noqa: E402
from openlte_amd import synth  # noqa: E402

ULC = (3, 0, 0, 2, 1)
FFT = {25: 512, 50: 1024, 100: 2048}
SCALES = (4, 8, 16)
MODES = ("R", "A") + tuple("N%d" % s for s in SCALES)
QM = {1: 2, 2: 4, 3: 6}
# name -> (N_rb_ul, (mod_type, N_prb) of the first transmission, (mod_type, N_prb, dB over the first) of the second, code rate, code blocks or None)
CLASSES = {"16qam_25prb_plus8db": (50, (2, 25), (2, 25, 8.0), 0.75, None),
           "64qam_then_qpsk": (25, (3, 12), (1, 24, 0.0), 0.75, None),
           "16qam_96prb_plus8db": (100, (2, 96), (2, 96, 8.0), 0.75, 6)}
SEED0 = 7000


def class_tbs(name):
    """(tbs, G of the first transmission): the size of the first transmission's column of Table 7.1.7.2.1-1 (with the class's number of code
    blocks, where it names one) whose tbs + 24 is nearest rate * G"""
    _, (mod, n_prb), _, rate, n_cb = CLASSES[name]
    G = 144 * n_prb * QM[mod]
    L = m.load_library()
    sizes = sorted({int(L.mi_lte_tbs(i, n_prb)) for i in range(27)})
    if n_cb is not None:
        sizes = [s for s in sizes if m.ulsch_layout(s, 0, 2)["C"] == n_cb]
    return min(sizes, key=lambda s: abs(s + 24 - rate * G)), G


def point_seed(name, snr_db):
    return SEED0 + 200 * list(CLASSES).index(name) + 2 * (int(round(snr_db)) + 50)


class Point:
    """One (class, SNR of the first transmission) point on the device: both transmissions through the uplink front end, a 3GPP plan over each
    and a pool with one buffer per transport block."""

    def __init__(self, ctx, name, snr_db, n_blocks):
        n_rb, first, second, _, _ = CLASSES[name]
        self.ctx, self.cfg, self.ul, self.n = ctx, m.DlCfg(FFT[n_rb], n_rb, 1, 0), m.UlCfg(*ULC), n_blocks
        size, _ = class_tbs(name)
        self.cells = [(37 * u + 11) % 504 for u in range(n_blocks)]
        self.tx, self.d_sub, self.plans = None, [], []
        for k, (mod, n_prb, rv, off) in enumerate(((first[0], first[1], 0, 0.0), (second[0], second[1], 2, second[2]))):
            sfs = [(u + 4 * k) % 10 for u in range(n_blocks)]
            allocs = [m.make_alloc(u, mod, size, list(range((3 * u) % (n_rb - n_prb), (3 * u) % (n_rb - n_prb) + n_prb)), 0x300 + u, rv_idx=rv)
                      for u in range(n_blocks)]
            iq, tx = synth.ul_units_3gpp(self.cfg, self.ul, sfs, self.cells, allocs, 1, gain=(1.0, 1.0), max_delay=3, snr_db=snr_db + off, peak=100.0,
                                         seed=point_seed(name, snr_db) + k, payload=self.tx)
            self.tx = tx
            self.d_sub.append(ctx.ul_frontend(self.cfg, iq.reshape(-1, 2), np.arange(n_blocks) * iq.shape[1], keep=True)[1])
            self.plans.append(ctx.pusch_plan_3gpp(self.cfg, self.ul, sfs, self.cells, allocs))
        self.size = size
        self.pool = ctx.harq_pool(n_blocks, max_tbs=size)

    def decoded(self, mode):
        """bool [n_blocks] after the second transmission: status 0 and the payload equal to the transmitted one.  mode: one of MODES"""
        st = bits = None
        for k, (plan, d_sub) in enumerate(zip(self.plans, self.d_sub)):
            plan.set_demapper(m.DEMAP_REF if mode == "R" else m.DEMAP_MAXLOG, 0.0)
            plan.set_llr_noise(float(mode[1:]) if mode[0] == "N" else 0.0)
            d_out, d_st = self.ctx.alloc(self.n * plan.out_stride), self.ctx.alloc(4 * self.n)
            d_out.zero()
            plan.run_harq_dev(self.pool, m.harq_binds(self.n, list(range(self.n)), k == 0), d_sub, d_out, d_st)
            st, bits = d_st.download(np.int32), d_out.download(np.uint8).reshape(self.n, plan.out_stride)
            d_out.free()
            d_st.free()
        return np.array([st[a] == 0 and (bits[a, :self.size] == self.tx[a, 0, :self.size]).all() for a in range(self.n)])

    def close(self):
        for p in self.plans:
            p.close()
        for d in self.d_sub:
            d.free()
        self.pool.close()


def windows(snrs, n_col, a_col, n_blocks):
    """the points p with N = all at p - 1 and p, A = 0 at p and p + 1"""
    return [snrs[i] for i in range(1, len(snrs) - 1) if n_col[i - 1] == n_col[i] == n_blocks and a_col[i] == a_col[i + 1] == 0]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=16)
    ap.add_argument("--snr-lo", type=int, default=-6)
    ap.add_argument("--snr-hi", type=int, default=16)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    snrs = list(range(args.snr_lo, args.snr_hi + 1))
    ctx = m.Context(0)
    table = {name: {c: [] for c in MODES} for name in CLASSES}
    for name in CLASSES:
        for snr in snrs:
            p = Point(ctx, name, float(snr), args.blocks)
            for c in MODES:
                table[name][c].append(int(p.decoded(c).sum()))
            p.close()
        print("# %s done" % name, flush=True)
    total = {s: sum(sum(table[n]["N%d" % s]) for n in CLASSES) for s in SCALES}
    best = min(SCALES, key=lambda s: (-total[s], s))
    win = {n: {"N%d" % s: windows(snrs, table[n]["N%d" % s], table[n]["A"], args.blocks) for s in SCALES} for n in CLASSES}
    diff = {}
    for n in CLASSES:
        d = [x - y for x, y in zip(table[n]["N%d" % best], table[n]["A"])]
        i = int(np.argmax(d))
        diff[n] = {"snr_db": snrs[i], "N": table[n]["N%d" % best][i], "A": table[n]["A"][i], "R": table[n]["R"][i]}
    sizes = {}
    for n in CLASSES:
        size, G = class_tbs(n)
        sizes[n] = {"n_rb_ul": CLASSES[n][0], "first": list(CLASSES[n][1]), "second": list(CLASSES[n][2]), "tbs": size, "G_first": G,
                    "code_rate_first": round((size + 24) / G, 3), "code_blocks": m.ulsch_layout(size, 0, 2)["C"], "seed_of_point": "%d + 200 * class index + 2 * (snr_db + 50) + transmission" % SEED0}
    out = {"workload": "pusch_harq_sweep", "blocks_per_point": args.blocks, "max_delay": 3, "channel_gain": [1.0, 1.0], "decoder": "BCJR x 8",
           "rv": [0, 2], "classes": sizes, "snr_db": snrs, "blocks_decoded": table, "blocks_decoded_per_scale": {"N%d" % s: total[s] for s in SCALES},
           "recommended_scale": best, "windows": win, "largest_difference": diff, "build_id": m.load_library().mi_lte_build_id().decode(),
           "device": ctx.device_name}
    lines = ["# tools/pusch_harq_sweep.py --blocks %d --snr-lo %d --snr-hi %d on one MI355X (gfx950)" % (args.blocks, args.snr_lo, args.snr_hi),
             "# transport blocks (of %d) decoded after two combined transmissions, rv 0 then rv 2, per SNR of the first transmission." % args.blocks,
             "# R: the default demapper; A: MAXLOG, automatic gain; N<s>: MAXLOG, noise-referenced gain with scale s.",
             "# blocks decoded over all classes and points: %s; recommended scale: %d." % (", ".join("N%d: %d" % (s, total[s]) for s in SCALES), best)]
    for n in CLASSES:
        lines.append("# %s (%d-RB cell; first: mod_type %d on %d PRB; second: mod_type %d on %d PRB, %+g dB; tbs %d, %d code blocks, code rate of the first %.3f)"
                     % (n, sizes[n]["n_rb_ul"], *CLASSES[n][1], *CLASSES[n][2], sizes[n]["tbs"], sizes[n]["code_blocks"], sizes[n]["code_rate_first"]))
        lines.append("#  SNR  " + "  ".join("%4s" % c for c in MODES))
        for i, snr in enumerate(snrs):
            lines.append("# %4d  " % snr + "  ".join("%4d" % table[n][c][i] for c in MODES))
        lines.append("#  windows (N all at p - 1 and p, A none at p and p + 1): " + ", ".join("%s: %s" % (c, w or "none") for c, w in win[n].items()))
        lines.append("#  largest difference N%d - A: %s" % (best, diff[n]))
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
