"""Parameter sets of tests/test_phich_gpu.py (kernel against tests/phich_model.py); tests/test_phich_cpu.py checks their margins and
that they cover what they claim.  The smallest shapes at which k_phich_decode can go wrong: one group on 8 free REGs (6 RB, N_g = 1/6), two
groups, group counts that are no multiple of anything (15 RB: 4, 25 RB: 4), and the table maximum of 25 groups = 75 REGs = 300 gather items,
more than the workgroup's 256 threads (100 RB, N_g = 2) -- each with 1, 2 and 4 ports.  Per case four units: cells of all three CRS shifts
(k mod 3), subframes 0 and 9, 20 dB SNR, frequency-selective smooth channels, noisy estimates."""
from fractions import Fraction

import numpy as np

import phich_model as pm

FFT = {6: 128, 15: 256, 25: 512, 50: 1024, 75: 2048, 100: 2048}
SHAPES = [(6, Fraction(1, 6)), (6, Fraction(2)), (15, Fraction(2)), (25, Fraction(1)), (100, Fraction(2))]
CELLS = [3, 100, 302, 503]   # k mod 3 = 0, 1, 2, 2
SUBFRAMES = [0, 9, 9, 0]
SNR_DB = 20.0

CASES = [dict(n_rb=n_rb, n_g=n_g, n_ant=n_ant, cells=CELLS, sfs=SUBFRAMES, seed=1000 * n_rb + 10 * n_ant + int(n_g * 6))
         for n_rb, n_g in SHAPES for n_ant in (1, 2, 4)]


def case_id(c):
    return "%drb-ng%s-%dport" % (c["n_rb"], str(c["n_g"]).replace("/", "_"), c["n_ant"])


_made = {}


def make(c):
    """(present, hi, subframes float32 [4, 2 + 2 n_ant, 16, 1200], model outputs per unit); made once per case and shared"""
    key = case_id(c)
    if key not in _made:
        rng = np.random.default_rng(c["seed"])
        n_grp = pm.n_group(c["n_rb"], c["n_g"])
        present, hi = pm.random_pattern(rng, len(c["cells"]), n_grp)
        sub = pm.modulate(c["n_rb"], c["n_ant"], c["cells"], c["sfs"], present, hi, rng, snr_db=SNR_DB)
        model = [pm.decode(c["n_rb"], c["n_ant"], n_grp, c["cells"][u], c["sfs"][u], sub[u]) for u in range(len(c["cells"]))]
        for a in (present, hi, sub):
            a.setflags(write=False)
        _made[key] = (present, hi, sub, model)
    return _made[key]
