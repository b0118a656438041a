#!/usr/bin/env python3
"""What receive-antenna combining on the 3GPP PUSCH plans (mi_lte_pusch_plan_set_rx_antennas) buys, in dB.  Traffic classes in a 25-RB cell,
one code block each, at code rate about 0.5: tools/pusch_llr_sweep.py's 16QAM on 20 PRB and 64QAM on 14 PRB, and 64QAM on 6 PRB -- each
once with every antenna's channel gain drawn from the synthesiser's 0.5 .. 1.5 and once at unit gain (`_flat`).  Four antenna captures of
every transport block (synth.ul_units_3gpp_rx: one payload; gain, phase, delay up to 3 samples and noise of equal power per antenna);
--blocks transport blocks per point (one per unit: its own cell, subframe, payload and channels), 1 dB steps, SNR per antenna at unit gain.
Per point the share of blocks decoded (status 0 and the payload equal to the transmitted one) under BCJR x 8 and MAXLOG:
  ant0, ant1   one antenna alone (n_rx = 1, automatic gain)
  rx2, rx2n    antennas 0 and 1 combined, automatic gain / noise-referenced gain at scale 8
  rx4          all four combined, automatic gain
`gain_db`: the SNR at 50 % block error (interpolated) of ant0 minus that of rx2 and of rx4.  `value`: the first point p of the first
class where rx2 decodes every block at p - 1 and p and each antenna alone none at p and p + 1 (DESIGN section 8's window rule), or, where
no class has one, the first point of the largest difference rx2 - max(ant0, ant1).

    python tools/pusch_rxdiv_sweep.py [--blocks 16] [--snr-lo -4] [--snr-hi 18] [--out profiles/pusch_rxdiv_sweep.txt]
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
from demap_llr_sweep import snr_at_half  # noqa: E402
from pusch_llr_sweep import FFT, FLAT, N_RB, SPREAD, ULC, tbs_for_rate  # noqa: E402

# name -> (mod_type, N_prb, code rate, the synthesiser's range of channel gains per antenna)
CLASSES = {"16qam_r0.5": (2, 20, 0.5, SPREAD), "64qam_r0.5": (3, 14, 0.5, SPREAD), "64qam_r0.5_6prb": (3, 6, 0.5, SPREAD),
           "16qam_r0.5_flat": (2, 20, 0.5, FLAT), "64qam_r0.5_flat": (3, 14, 0.5, FLAT), "64qam_r0.5_6prb_flat": (3, 6, 0.5, FLAT)}
MODES = ("ant0", "ant1", "rx2", "rx2n", "rx4")
N_ANT = 4
SEED0 = 7000


def class_units(name, n_blocks):
    mod, n_prb, rate, _ = CLASSES[name]
    size, _ = tbs_for_rate(mod, n_prb, rate)
    sfs = [u % 10 for u in range(n_blocks)]
    cells = [(37 * u + 11) % 504 for u in range(n_blocks)]
    allocs = [m.make_alloc(u, mod, size, list(range((3 * u) % (N_RB - n_prb), (3 * u) % (N_RB - n_prb) + n_prb)), 0x300 + u) for u in range(n_blocks)]
    return sfs, cells, allocs


def point_seed(name, snr_db):
    return SEED0 + 100 * list(CLASSES).index(name) + int(round(snr_db)) + 50


class Antenna:
    """the subframes of one antenna of a point's device buffer, as a run's d_subframes"""

    def __init__(self, buf, byte_offset):
        self.ptr = buf.ptr + byte_offset


class Point:
    """One (class, SNR) point on the device: four antenna captures of every unit through one front-end call, one 3GPP plan over the units."""

    def __init__(self, ctx, name, snr_db, n_blocks):
        self.ctx, self.cfg, self.ul, self.n = ctx, m.DlCfg(FFT, N_RB, 1, 0), m.UlCfg(*ULC), n_blocks
        self.sfs, self.cells, self.allocs = class_units(name, n_blocks)
        iq, self.tx = synth.ul_units_3gpp_rx(self.cfg, self.ul, self.sfs, self.cells, self.allocs, 1, N_ANT, seed=point_seed(name, snr_db),
                                             gain=CLASSES[name][3], max_delay=3, snr_db=snr_db, peak=100.0)
        _, self.d_sub = ctx.ul_frontend(self.cfg, iq.reshape(-1, 2), np.arange(iq.shape[0]) * iq.shape[1], keep=True)
        self.plan = ctx.pusch_plan_3gpp(self.cfg, self.ul, self.sfs, self.cells, self.allocs)
        self.plan.set_demapper(m.DEMAP_MAXLOG, 0.0)

    def decoded(self, mode):
        """bool [n_blocks]: status 0 and the payload equal to the transmitted one"""
        n_rx = {"ant0": 1, "ant1": 1, "rx2": 2, "rx2n": 2, "rx4": 4}[mode]
        self.plan.set_rx_antennas(n_rx, self.n)
        self.plan.set_llr_noise(8.0 if mode == "rx2n" else 0.0)
        first = Antenna(self.d_sub, (self.n * self.ctx.ul_subframe_floats() * 4) if mode == "ant1" else 0)
        st, bits = self.plan.run(first)
        return np.array([st[a] == 0 and (bits[a] == self.tx[a, 0, :al.tbs]).all() for a, al in enumerate(self.allocs)])

    def close(self):
        self.plan.close()
        self.d_sub.free()


def value_point(snrs, table, n_blocks):
    """the window rule, then the fallback: (kind, class, snr, counts)"""
    def cnt(name, mode, i):
        return int(round(table[name][mode][i] * n_blocks))
    for name in table:
        for i in range(1, len(snrs) - 1):
            if (cnt(name, "rx2", i - 1) == cnt(name, "rx2", i) == n_blocks
                    and all(cnt(name, a, j) == 0 for a in ("ant0", "ant1") for j in (i, i + 1))):
                return {"kind": "window", "class": name, "snr_db": snrs[i], "rx2": [n_blocks, n_blocks], "ant0": [0, 0], "ant1": [0, 0]}
    best = None
    for name in table:
        for i in range(len(snrs)):
            d = cnt(name, "rx2", i) - max(cnt(name, "ant0", i), cnt(name, "ant1", i))
            if best is None or d > best[0]:
                best = (d, name, i)
    d, name, i = best
    return {"kind": "largest difference", "class": name, "snr_db": snrs[i], "rx2": cnt(name, "rx2", i), "ant0": cnt(name, "ant0", i), "ant1": cnt(name, "ant1", i)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=16)
    ap.add_argument("--snr-lo", type=int, default=-4)
    ap.add_argument("--snr-hi", type=int, default=18)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    snrs = list(range(args.snr_lo, args.snr_hi + 1))
    ctx = m.Context(0)
    table = {name: {c: [] for c in MODES} for name in CLASSES}
    for name in CLASSES:
        for snr in snrs:
            p = Point(ctx, name, float(snr), args.blocks)
            for mode in MODES:
                table[name][mode].append(float(p.decoded(mode).mean()))
            p.close()
        print("# %s done" % name, flush=True)
    half = {name: {c: snr_at_half(snrs, table[name][c]) for c in MODES} for name in CLASSES}

    def gain(name, mode):
        a, b = half[name]["ant0"], half[name][mode]
        return None if a is None or b is None else round(a - b, 2)

    sizes = {}
    for n, (mod, n_prb, rate, g) in CLASSES.items():
        size, G = tbs_for_rate(mod, n_prb, rate)
        sizes[n] = {"mod_type": mod, "N_prb": n_prb, "tbs": size, "G": G, "code_rate": round((size + 24) / G, 3), "channel_gain": list(g)}
    value = value_point(snrs, table, args.blocks)
    out = {"workload": "pusch_rxdiv_sweep", "n_rb_ul": N_RB, "blocks_per_point": args.blocks, "max_delay": 3, "decoder": "BCJR x 8", "classes": sizes,
           "snr_db": snrs, "decoded_share": table, "snr_db_at_half": half, "gain_db": {n: {k: gain(n, k) for k in ("rx2", "rx2n", "rx4")} for n in CLASSES},
           "value": value, "build_id": m.load_library().mi_lte_build_id().decode(), "device": ctx.device_name}
    lines = ["# tools/pusch_rxdiv_sweep.py --blocks %d --snr-lo %d --snr-hi %d on one MI355X (gfx950)" % (args.blocks, args.snr_lo, args.snr_hi),
             "# share of transport blocks decoded per SNR point (per antenna, at unit gain); ant0 / ant1: one antenna alone, rx2 / rx2n: two combined under",
             "# the automatic / the noise-referenced gain (scale 8), rx4: four combined.  All MI_LTE_DEMAP_MAXLOG, BCJR x 8.",
             "# gain_db: SNR at 50 % block error of ant0 minus that of the combined mode.  value: " + json.dumps(value)]
    for name in CLASSES:
        s = sizes[name]
        lines.append("# %s (mod_type %d, %d PRB, tbs %d, G %d, code rate %.3f, channel gain %.1f .. %.1f): gain rx2 %s dB, rx2n %s dB, rx4 %s dB"
                     % (name, s["mod_type"], s["N_prb"], s["tbs"], s["G"], s["code_rate"], s["channel_gain"][0], s["channel_gain"][1],
                        gain(name, "rx2"), gain(name, "rx2n"), gain(name, "rx4")))
        lines.append("#  SNR  " + "  ".join("%5s" % c for c in MODES))
        for i, snr in enumerate(snrs):
            lines.append("# %4d  " % snr + "  ".join("%5.2f" % table[name][c][i] for c in MODES))
        lines.append("#  50%   " + "  ".join("%5s" % ("-" if half[name][c] is None else "%.1f" % half[name][c]) for c in MODES))
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
