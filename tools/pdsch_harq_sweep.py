#!/usr/bin/env python3
"""What the noise-referenced LLR gain of the 3GPP PDSCH plans (mi_lte_pdsch_plan_set_llr_noise: g = scale / sigma2 of the CRS noise estimate)
buys HARQ combining on the downlink (mi_lte_pdsch_decode_run_harq).  Every transport block is sent twice with the same payload, rv 0 then
rv 2, each transmission with its own subframe, seed, channel phase, delay and noise (synth.dl_units_3gpp(..., gain=(1, 1), max_delay=4)), and
both are combined in a pool buffer; a block counts when the second run returns status 0 and the transmitted payload.  Classes:

  16qam_25prb_plus8db       16QAM on 25 PRB of a 50-RB single-port cell, two code blocks, first-transmission code rate about 0.75; the second
                            transmission 8 dB above the first
  64qam_then_qpsk           the same SNR for both; 64QAM on 12 PRB of a 25-RB cell at code rate about 0.75, the retransmission QPSK on 24 PRB
  16qam_25prb_plus8db_txd2  the first class (the same transport block size) on a two-port cell in transmit diversity

Modes: R the default demapper, A MAXLOG under the automatic gain, N<s> MAXLOG under the noise-referenced gain with scale s in SCALES.
BCJR x 8, --blocks transport blocks (one per unit) per point, 1 dB steps of the first transmission's SNR.  `windows`: per class and scale the
points p at which N decodes every block at p and p - 1 and A none at p and p + 1; `largest_difference`: per class the first point where N8
leads A by the most blocks.

    python tools/pdsch_harq_sweep.py [--blocks 16] [--snr-lo -4] [--snr-hi 14] [--out profiles/pdsch_harq_sweep.txt]
Prints one JSON line last (and writes the table and the line to --out)."""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import openlte_amd as m  # noqa: E402
from openlte_amd import synth  # noqa: E402

FFT = {25: 512, 50: 1024}
CFI, N_SOFT = 2, 1237248
SCALES = (4, 8, 16)
MODES = ("R", "A") + tuple("N%d" % s for s in SCALES)
QM = {1: 2, 2: 4, 3: 6}
# name -> (N_rb_dl, N_ant, (mod_type, N_prb) of the first transmission, (mod_type, N_prb, dB over the first) of the second, code rate, code blocks or None)
CLASSES = {"16qam_25prb_plus8db": (50, 1, (2, 25), (2, 25, 8.0), 0.75, 2),
           "64qam_then_qpsk": (25, 1, (3, 12), (1, 24, 0.0), 0.75, None),
           "16qam_25prb_plus8db_txd2": (50, 2, (2, 25), (2, 25, 8.0), 0.75, 2)}
SUBFRAMES = (1, 2, 3, 4, 6, 7, 8, 9)  # never 0 or 5: G is the same for every unit
SEED0 = 9000


def class_tbs(name):
    """(tbs, G of the first transmission on a single-port cell): the size of the first transmission's column of Table 7.1.7.2.1-1 (with the
    class's number of code blocks, where it names one) whose tbs + 24 is nearest rate * G.  The two-port class takes the single-port size."""
    _, _, (mod, n_prb), _, rate, n_cb = CLASSES[name]
    G = n_prb * (12 * (14 - CFI) - 6) * QM[mod]
    L = m.load_library()
    sizes = sorted({int(L.mi_lte_tbs(i, n_prb)) for i in range(27)})
    if n_cb is not None:
        sizes = [s for s in sizes if m.dlsch_layout(s, 0, 2, 1, 0, N_SOFT, 8)["C"] == n_cb]
    return min(sizes, key=lambda s: abs(s + 24 - rate * G)), G


def point_seed(name, snr_db):
    return SEED0 + 200 * list(CLASSES).index(name) + 2 * (int(round(snr_db)) + 50)


class Point:
    """One (class, SNR of the first transmission) point on the device: both transmissions through the front end, a 3GPP plan over each and a
    pool with one buffer per transport block."""

    def __init__(self, ctx, name, snr_db, n_blocks):
        n_rb, n_ant, first, second, _, _ = CLASSES[name]
        self.ctx, self.cfg, self.n, self.n_ant = ctx, m.DlCfg(FFT[n_rb], n_rb, n_ant, 0), n_blocks, n_ant
        self.size, _ = class_tbs(name)
        self.cells = [(37 * u + 11) % 504 for u in range(n_blocks)]
        self.tx, self.units, self.plans = None, [], []
        make_units = synth.dl_units_3gpp if n_ant == 1 else synth.dl_units_3gpp_txdiv
        make_plan = ctx.pdsch_plan_3gpp if n_ant == 1 else ctx.pdsch_plan_3gpp_txdiv
        for k, (mod, n_prb, rv, off) in enumerate(((first[0], first[1], 0, 0.0), (second[0], second[1], 2, second[2]))):
            sfs = [SUBFRAMES[(u + 3 * k) % 8] for u in range(n_blocks)]
            allocs = [m.make_alloc(u, mod, self.size, list(range((3 * u) % (n_rb - n_prb + 1), (3 * u) % (n_rb - n_prb + 1) + n_prb)), 0x300 + u, rv_idx=rv,
                                   tx_mode=1 if n_ant == 1 else 2) for u in range(n_blocks)]
            iq, self.tx = make_units(self.cfg, sfs, self.cells, allocs, 1, N_SOFT, n_pdcch_symbs=CFI, gain=(1.0, 1.0), max_delay=4, snr_db=snr_db + off,
                                     seed=point_seed(name, snr_db) + k, payload=self.tx)
            d_iq, d_start = ctx.to_device(iq.reshape(-1, 2)), ctx.to_device((np.arange(n_blocks) * iq.shape[1]).astype(np.uint64))
            d_sf, d_cell = ctx.to_device(np.asarray(sfs, np.uint32)), ctx.to_device(np.asarray(self.cells, np.uint32))
            d_sub = ctx.alloc(n_blocks * ctx.subframe_floats(n_ant) * 4)
            ctx.dl_frontend_dev(self.cfg, d_iq, None, d_start, d_sf, d_cell, n_blocks, d_sub)
            d_iq.free()
            d_start.free()
            self.units.append((d_sub, d_sf, d_cell))
            self.plans.append(make_plan(self.cfg, CFI, allocs, N_SOFT))
        self.pool = ctx.harq_pool(n_blocks, max_tbs=self.size)

    def decoded(self, mode):
        """bool [n_blocks] after the second transmission: status 0 and the payload equal to the transmitted one.  mode: one of MODES"""
        st = bits = None
        for k, (plan, (d_sub, d_sf, d_cell)) in enumerate(zip(self.plans, self.units)):
            plan.set_demapper(m.DEMAP_REF if mode == "R" else m.DEMAP_MAXLOG, 0.0)
            plan.set_llr_noise(float(mode[1:]) if mode[0] == "N" else 0.0)
            d_out, d_st = self.ctx.alloc(self.n * plan.out_stride), self.ctx.alloc(4 * self.n)
            d_out.zero()
            plan.run_harq_dev(self.pool, m.harq_binds(self.n, list(range(self.n)), k == 0), d_sub, d_sf, d_cell, d_out, d_st)
            st, bits = d_st.download(np.int32), d_out.download(np.uint8).reshape(self.n, plan.out_stride)
            d_out.free()
            d_st.free()
        return np.array([st[a] == 0 and (bits[a, :self.size] == self.tx[a, 0, :self.size]).all() for a in range(self.n)])

    def noise(self):
        """float32 [2, n_blocks]: the sigma2 taps of the two plans' last noise-on runs"""
        return np.stack([p.llr_noise() for p in self.plans])

    def close(self):
        for p in self.plans:
            p.close()
        for bufs in self.units:
            for b in bufs:
                b.free()
        self.pool.close()


def windows(snrs, n_col, a_col, n_blocks):
    """the points p with N = all at p - 1 and p, A = 0 at p and p + 1"""
    return [snrs[i] for i in range(1, len(snrs) - 1) if n_col[i - 1] == n_col[i] == n_blocks and a_col[i] == a_col[i + 1] == 0]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=16)
    ap.add_argument("--snr-lo", type=int, default=-4)
    ap.add_argument("--snr-hi", type=int, default=14)
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
    win = {n: {"N%d" % s: windows(snrs, table[n]["N%d" % s], table[n]["A"], args.blocks) for s in SCALES} for n in CLASSES}
    diff = {}
    for n in CLASSES:
        d = [x - y for x, y in zip(table[n]["N8"], table[n]["A"])]
        i = int(np.argmax(d))
        diff[n] = {"snr_db": snrs[i], "N8": table[n]["N8"][i], "A": table[n]["A"][i], "R": table[n]["R"][i]}
    sizes = {}
    for n in CLASSES:
        size, G = class_tbs(n)
        sizes[n] = {"n_rb_dl": CLASSES[n][0], "n_ant": CLASSES[n][1], "first": list(CLASSES[n][2]), "second": list(CLASSES[n][3]), "tbs": size,
                    "G_first_single_port": G, "code_rate_first_single_port": round((size + 24) / G, 3), "code_blocks": m.dlsch_layout(size, 0, 2, 1, 0, N_SOFT, 8)["C"],
                    "seed_of_point": "%d + 200 * class index + 2 * (snr_db + 50) + transmission" % SEED0}
    out = {"workload": "pdsch_harq_sweep", "blocks_per_point": args.blocks, "cfi": CFI, "max_delay": 4, "channel_gain": [1.0, 1.0], "decoder": "BCJR x 8",
           "rv": [0, 2], "classes": sizes, "snr_db": snrs, "blocks_decoded": table, "blocks_decoded_per_scale": {"N%d" % s: total[s] for s in SCALES},
           "windows": win, "largest_difference": diff, "build_id": m.load_library().mi_lte_build_id().decode(), "device": ctx.device_name}
    lines = ["# tools/pdsch_harq_sweep.py --blocks %d --snr-lo %d --snr-hi %d on one MI355X (gfx950)" % (args.blocks, args.snr_lo, args.snr_hi),
             "# transport blocks (of %d) decoded after two combined transmissions, rv 0 then rv 2, per SNR of the first transmission." % args.blocks,
             "# R: the default demapper; A: MAXLOG, automatic gain; N<s>: MAXLOG, noise-referenced gain with scale s.",
             "# blocks decoded over all classes and points: %s." % ", ".join("N%d: %d" % (s, total[s]) for s in SCALES)]
    for n in CLASSES:
        lines.append("# %s (%d-RB cell, %d port(s); first: mod_type %d on %d PRB; second: mod_type %d on %d PRB, %+g dB; tbs %d, %d code blocks, single-port code rate of the first %.3f)"
                     % (n, sizes[n]["n_rb_dl"], sizes[n]["n_ant"], *CLASSES[n][2], *CLASSES[n][3], sizes[n]["tbs"], sizes[n]["code_blocks"], sizes[n]["code_rate_first_single_port"]))
        lines.append("#  SNR  " + "  ".join("%4s" % c for c in MODES))
        for i, snr in enumerate(snrs):
            lines.append("# %4d  " % snr + "  ".join("%4d" % table[n][c][i] for c in MODES))
        lines.append("#  windows (N all at p - 1 and p, A none at p and p + 1): " + ", ".join("%s: %s" % (c, w or "none") for c, w in win[n].items()))
        lines.append("#  largest difference N8 - A (the first such point): %s" % diff[n])
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
