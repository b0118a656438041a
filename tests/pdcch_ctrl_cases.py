"""The cases that test_pdcch_ctrl_model_cpu and test_pdcch_ctrl_model_gpu share: small batches of device subframes from the independent
modulator of pdcch_ctrl_model, built once per process and left unchanged.

Between them the cases cover N_rb 6 with N_symbs 2, 3, 4; N_rb 15 and 25 with cfi 1, 2, 3; N_rb 50 with cfi 2; a 4-port case at N_rb 100 with
N_g = 2 and cfi 3 (the most PHICH groups, and 69 CCEs: four 16-CCE chunks of the kernel and a short fifth); 1, 2 and 4 ports at every
bandwidth used; all four N_g; a unit with cfi 4 above 10 resource blocks; cells of every residue mod 3; cells whose PCFICH wraps round the
band's edge (cell mod 2 N_rb at 2 N_rb - 1 and just past N_rb / 2); cell 500 at 1.4 MHz, above N_reg, so that the cyclic shift wraps many times;
cells in which a PHICH group number passes a PCFICH group (nearly all); subframes 0 and 9."""
import functools

import numpy as np

import pdcch_ctrl_model as pm

FFT = {6: 128, 15: 256, 25: 512, 50: 1024, 75: 2048, 100: 2048}

# (n_rb, n_ant, N_g, [(cell, subframe, cfi)])
CASES = [
    (6, 1, "1/6", [(500, 0, 1), (11, 9, 2), (4, 3, 3), (0, 9, 1), (23, 0, 3)]),
    (6, 2, "1", [(500, 9, 3), (11, 0, 1), (4, 5, 2), (301, 0, 2)]),
    (6, 4, "2", [(500, 0, 2), (11, 9, 3), (4, 0, 1), (6, 7, 3)]),
    (15, 1, "1/2", [(29, 0, 1), (503, 9, 2), (7, 4, 3), (150, 9, 4)]),
    (15, 2, "2", [(29, 9, 3), (503, 0, 1), (8, 2, 2), (60, 9, 3)]),
    (15, 4, "1/6", [(29, 0, 2), (503, 9, 3), (9, 6, 1), (44, 0, 4)]),
    (25, 1, "1", [(49, 0, 1), (13, 9, 2), (44, 1, 3), (300, 9, 3)]),
    (25, 2, "1/6", [(49, 9, 3), (13, 0, 1), (44, 8, 2), (301, 0, 3)]),
    (25, 4, "1/2", [(49, 0, 2), (13, 9, 3), (44, 0, 1), (302, 5, 3), (27, 9, 4)]),
    (50, 1, "1", [(99, 0, 2), (26, 9, 2), (150, 3, 2), (401, 9, 2)]),
    (50, 2, "2", [(99, 9, 2), (27, 0, 2), (151, 9, 2), (402, 0, 2)]),
    (50, 4, "1/2", [(99, 0, 2), (26, 9, 2), (152, 4, 2), (403, 0, 2)]),
    (100, 1, "1/6", [(199, 0, 1), (51, 9, 2), (300, 0, 3), (17, 9, 2)]),
    (100, 2, "1", [(199, 9, 2), (52, 0, 1), (301, 9, 3), (18, 0, 2)]),
    (100, 4, "2", [(199, 0, 3), (51, 9, 3), (302, 0, 3), (19, 9, 3)]),
]
# Cases for MI_LTE_PDCCH_SEARCH_36211_REGS, sent and decoded with numbering = "36.211": cells in which a PHICH group is numbered past a PCFICH group
# that wrapped round the band's edge, so that the default tables differ (test_pdcch_ctrl_model_cpu asserts it), and four ports with a one-symbol
# region (15-4: 2 CCEs where the default tables have none; 100-4 unit 2).  batch() and reference() take their indices after CASES'.
CASES_36211 = [
    (6, 1, "1/6", [(6, 0, 3), (500, 9, 1), (21, 4, 2), (7, 9, 3)]),
    (6, 2, "1", [(9, 9, 2), (16, 0, 1), (499, 3, 3), (30, 9, 1)]),
    (15, 4, "1/6", [(9, 6, 1), (44, 0, 1), (38, 9, 2), (503, 0, 3)]),
    (25, 2, "1", [(63, 0, 3), (113, 9, 2), (471, 5, 3), (70, 9, 1)]),
    (50, 1, "2", [(125, 0, 2), (473, 9, 2), (130, 4, 2), (136, 9, 2)]),
    (100, 4, "2", [(450, 0, 3), (498, 9, 3), (461, 0, 1), (455, 9, 3)]),
]
ALL = CASES + CASES_36211
IDX_36211 = list(range(len(CASES), len(ALL)))
# Channel seeds of the "clean" batches: the first for which the model's own noiseless round trip returns every bit with magnitude 64 or more
# (a pair of elements in a deep fade of the smooth channel, where the first element's estimate no longer describes the second, can fall below)
CLEAN_SEED = [0, 1, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 2] + [0] * len(CASES_36211)
IDS = ["%d-%d-%s" % (c[0], c[1], c[2].replace("/", "_")) for c in CASES]
IDS_36211 = ["%d-%d-%s" % (c[0], c[1], c[2].replace("/", "_")) for c in CASES_36211]


def n_symbs(n_rb, cfi):
    return cfi + (1 if n_rb <= 10 else 0)


def n_cce_of(n_rb, n_ant, n_g, cell, cfi, numbering="library"):
    return pm.geometry(n_rb, n_ant, cell, pm.N_G[n_g], n_symbs(n_rb, cfi), numbering)[0]


@functools.lru_cache(maxsize=None)
def batch(i, kind, numbering="library"):
    """Case i as (grids float32 [n, 2 + 2 n_ant, 16, 1200], bits: per unit uint8 [N_cce, 72]).  kind: "clean" (no noise, true estimates),
    "noisy" (10 dB, noisy estimates), "low" (-3 dB, noisy estimates, the PCFICH's own elements without noise), "filler" (other data on the largest region every cell has: what a first
    run leaves in a plan's soft buffer).  Random bits on every CCE.  numbering: the positions of the library's default tables, or "36.211"."""
    n_rb, n_ant, n_g, units = ALL[i]
    rng = np.random.default_rng(1000 * i + {"clean": 1 + 10 * CLEAN_SEED[i], "noisy": 2, "low": 3, "filler": 4}[kind])
    snr = {"clean": None, "noisy": 10.0, "low": -3.0, "filler": 20.0}[kind]
    grids, bits = [], []
    for cell, sf, cfi in units:
        if kind == "filler":
            cfi = 4 if n_rb > 10 else 3
        b = rng.integers(0, 2, (n_cce_of(n_rb, n_ant, n_g, cell, cfi, numbering), 72)).astype(np.uint8)
        grids.append(pm.modulate(n_rb, n_ant, cell, sf, cfi, pm.N_G[n_g], b, rng, snr_db=snr, est_noise=kind != "clean", quiet_pcfich=kind == "low",
                                 numbering=numbering))
        bits.append(b)
    g = np.stack(grids)
    g.setflags(write=False)
    return g, bits


@functools.lru_cache(maxsize=None)
def reference(i, kind, variant=None, f32=False, numbering="library"):
    """pdcch_ctrl_model.decode of every unit of batch(i, kind, numbering), in float64 (or numpy float32)"""
    n_rb, n_ant, n_g, units = ALL[i]
    g, _ = batch(i, kind, numbering)
    return [pm.decode(n_rb, n_ant, cell, sf, pm.N_G[n_g], g[u], np.float32 if f32 else np.float64, variant, numbering) for u, (cell, sf, _) in enumerate(units)]


def all_subframes(kind):
    for i, (n_rb, n_ant, n_g, units) in enumerate(CASES):
        g, _ = batch(i, kind)
        for u, (cell, sf, _) in enumerate(units):
            yield n_rb, n_ant, cell, sf, pm.N_G[n_g], g[u]
