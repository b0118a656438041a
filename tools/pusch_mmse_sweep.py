#!/usr/bin/env python3
"""What MMSE equalisation on the 3GPP PUSCH plans (mi_lte_pusch_plan_set_equaliser) buys, in dB, by the method of pusch_rxdiv_sweep.py.
Traffic classes in a 25-RB cell (N_fft 512), one code block each, at code rate about 0.5: 16QAM on 20 PRB and 64QAM on 14 PRB, each through
three channels of the multipath synthesiser (synth.ul_units_3gpp_rx(..., paths=)) at unit gain -- `flat` (one path), `a0.5` and `a1.0` (a
second path 4 samples late at 0.5 of and at the first one's amplitude; every antenna its own phases) -- and on one and on two antennas.
--blocks transport blocks per point (one per unit: its own cell, subframe, payload and channels), 1 dB steps, SNR per antenna.  Per point
the share of blocks decoded (status 0 and the payload equal to the transmitted one) under BCJR x 8, MAXLOG and the noise-referenced gain at
scale 8 on the same captures:
  zf    the zero-forcing equaliser (MI_LTE_EQ_ZF)
  mmse  MI_LTE_EQ_MMSE
`gain_db`: the SNR at 50 % block error (interpolated) of zf minus that of mmse.  `value`: the first point p of the first curve where mmse
decodes every block at p - 1 and p and zf none at p and p + 1 (DESIGN section 8's window rule), or, where no curve has one, the first point
of the largest difference mmse - zf.

    python tools/pusch_mmse_sweep.py [--blocks 16] [--snr-lo 0] [--snr-hi 34] [--out profiles/pusch_mmse_sweep.txt]
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
from pusch_llr_sweep import FFT, FLAT, N_RB, ULC, tbs_for_rate  # noqa: E402

TRAFFIC = {"16qam_r0.5": (2, 20, 0.5), "64qam_r0.5": (3, 14, 0.5)}          # name -> (mod_type, N_prb, code rate)
CHANNELS = {"flat": ([0], [1.0]), "a0.5": ([0, 4], [1.0, 0.5]), "a1.0": ([0, 4], [1.0, 1.0])}  # name -> (delays, amplitudes)
CLASSES = ["%s_%s_rx%d" % (t, c, n) for t in TRAFFIC for c in CHANNELS for n in (1, 2)]
MODES = ("zf", "mmse")
SEED0 = 9000


def parts(name):
    t, c, n = name.rsplit("_", 2)
    return t, c, int(n[2:])


def class_units(name, n_blocks):
    mod, n_prb, rate = TRAFFIC[parts(name)[0]]
    size, _ = tbs_for_rate(mod, n_prb, rate)
    sfs = [u % 10 for u in range(n_blocks)]
    cells = [(37 * u + 11) % 504 for u in range(n_blocks)]
    allocs = [m.make_alloc(u, mod, size, list(range((3 * u) % (N_RB - n_prb), (3 * u) % (N_RB - n_prb) + n_prb)), 0x300 + u) for u in range(n_blocks)]
    return sfs, cells, allocs


def point_seed(name, snr_db):
    return SEED0 + 100 * CLASSES.index(name) + int(round(snr_db)) + 50


class Point:
    """One (class, SNR) point on the device: the class's antenna captures of every unit through one front-end call, one 3GPP plan over the
    units with MAXLOG and the noise-referenced gain at scale 8."""

    def __init__(self, ctx, name, snr_db, n_blocks):
        _, chan, n_rx = parts(name)
        self.ctx, self.cfg, self.ul, self.n = ctx, m.DlCfg(FFT, N_RB, 1, 0), m.UlCfg(*ULC), n_blocks
        self.sfs, self.cells, self.allocs = class_units(name, n_blocks)
        iq, self.tx = synth.ul_units_3gpp_rx(self.cfg, self.ul, self.sfs, self.cells, self.allocs, 1, n_rx, seed=point_seed(name, snr_db),
                                             gain=FLAT, max_delay=3, snr_db=snr_db, peak=100.0, paths=CHANNELS[chan])
        _, self.d_sub = ctx.ul_frontend(self.cfg, iq.reshape(-1, 2), np.arange(iq.shape[0]) * iq.shape[1], keep=True)
        self.plan = ctx.pusch_plan_3gpp(self.cfg, self.ul, self.sfs, self.cells, self.allocs)
        self.plan.set_demapper(m.DEMAP_MAXLOG, 0.0)
        self.plan.set_llr_noise(8.0)
        self.plan.set_rx_antennas(n_rx, self.n)

    def decoded(self, mode):
        """bool [n_blocks]: status 0 and the payload equal to the transmitted one"""
        self.plan.set_equaliser(m.EQ_MMSE if mode == "mmse" else m.EQ_ZF)
        st, bits = self.plan.run(self.d_sub)
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
            if cnt(name, "mmse", i - 1) == cnt(name, "mmse", i) == n_blocks and cnt(name, "zf", i) == cnt(name, "zf", i + 1) == 0:
                return {"kind": "window", "class": name, "snr_db": snrs[i], "mmse": [n_blocks, n_blocks], "zf": [0, 0]}
    best = None
    for name in table:
        for i in range(len(snrs)):
            d = cnt(name, "mmse", i) - cnt(name, "zf", i)
            if best is None or d > best[0]:
                best = (d, name, i)
    d, name, i = best
    return {"kind": "largest difference", "class": name, "snr_db": snrs[i], "mmse": cnt(name, "mmse", i), "zf": cnt(name, "zf", i)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=16)
    ap.add_argument("--snr-lo", type=int, default=0)
    ap.add_argument("--snr-hi", type=int, default=34)
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
    line = report(args, snrs, table, ctx.device_name)
    ctx.close()
    return 0 if line else 1


def report(args, snrs, table, device):
    """the table and the JSON line from the decoded shares: printed, and written to --out"""
    half = {name: {c: snr_at_half(snrs, table[name][c]) for c in MODES} for name in CLASSES}

    def gain(name):
        a, b = half[name]["zf"], half[name]["mmse"]
        return None if a is None or b is None else round(a - b, 2)

    sizes = {}
    for n, (mod, n_prb, rate) in TRAFFIC.items():
        size, G = tbs_for_rate(mod, n_prb, rate)
        sizes[n] = {"mod_type": mod, "N_prb": n_prb, "tbs": size, "G": G, "code_rate": round((size + 24) / G, 3)}
    worst_flat = max(abs(table[n]["mmse"][i] - table[n]["zf"][i]) * args.blocks for n in CLASSES if parts(n)[1] == "flat" for i in range(len(snrs)))
    value = value_point(snrs, table, args.blocks)
    out = {"workload": "pusch_mmse_sweep", "n_rb_ul": N_RB, "blocks_per_point": args.blocks, "max_delay": 3, "decoder": "BCJR x 8", "llr_noise_scale": 8.0,
           "traffic": sizes, "channels": {k: {"delay": v[0], "amp": v[1]} for k, v in CHANNELS.items()}, "snr_db": snrs, "decoded_share": table,
           "snr_db_at_half": half, "gain_db": {n: gain(n) for n in CLASSES}, "flat_largest_difference_blocks": int(round(worst_flat)), "value": value,
           "build_id": m.load_library().mi_lte_build_id().decode(), "device": device}
    lines = ["# tools/pusch_mmse_sweep.py --blocks %d --snr-lo %d --snr-hi %d on one MI355X (gfx950)" % (args.blocks, args.snr_lo, args.snr_hi),
             "# share of transport blocks decoded per SNR point (per antenna); zf / mmse: MI_LTE_EQ_ZF / MI_LTE_EQ_MMSE on the same captures, both",
             "# MI_LTE_DEMAP_MAXLOG with the noise-referenced gain (scale 8), BCJR x 8.  Channels: flat; a second path 4 samples late at 0.5 (a0.5) and",
             "# at 1.0 (a1.0) of the first one's amplitude; rx1 / rx2: one / two antennas.",
             "# gain_db: SNR at 50 %% block error of zf minus that of mmse.  Largest |mmse - zf| on a flat point: %d block(s).  value: %s"
             % (int(round(worst_flat)), json.dumps(value))]
    for name in CLASSES:
        s = sizes[parts(name)[0]]
        lines.append("# %s (mod_type %d, %d PRB, tbs %d, G %d, code rate %.3f): gain %s dB" % (name, s["mod_type"], s["N_prb"], s["tbs"], s["G"], s["code_rate"], gain(name)))
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
    return line


if __name__ == "__main__":
    sys.exit(main())
