"""Seeded random geometry for the max-log PDSCH demapper (k_pdsch_demod_llr<1 | 2 | 4>), the kernel the compiled reference cannot check: the
float64 model (tests/demap_llr_model.py) consumes estimate planes, not samples, so a case is three units of synthetic planes and twelve
allocations whose PRB sets, control regions and cells are drawn where the hand-picked shapes of tests/test_demap_llr_gpu.py and
tests/test_txdiv_gpu.py do not go: all six bandwidths, PRB lists that differ between the slots or do not ascend, every CRS shift, a control
region of 4 symbols, and small allocations in a plan whose largest one sits on either side of the 32 KiB that decides between LDS assembly and
direct stores.  Pure numpy; tests/test_demap_geometry_cpu.py holds the draw to what it promises, tests/test_demap_geometry_gpu.py runs it."""
import numpy as np

import demap_llr_model as dm
from fuzz_cases import BANDWIDTHS
from test_dlsch3gpp_cpu import tbs_table

N_RBS = [n_rb for _, _, n_rb in BANDWIDTHS]
FFT = {n_rb: fft for _, fft, n_rb in BANDWIDTHS}
KINDS = ("single", "run", "scattered", "slots_differ", "one_slot_in_window", "not_ascending")
BIG_PRB = {"lds_max": 56, "direct_min": 57}  # 16QAM, its own control region of 2 symbols: 12 * 56 * 48 = 32 256 soft-bit slots, 12 * 57 * 48 = 32 832
PARAMS = [(n_rb, n_ant, "small", 1000 * n_rb + n_ant) for n_rb in N_RBS for n_ant in (1, 2, 4)] + \
         [(n_rb, n_ant, v, 1000 * n_rb + 10 * (1 + k) + n_ant) for n_rb in (75, 100) for n_ant in (1, 2, 4) for k, v in enumerate(BIG_PRB)]


def param_id(p):
    return "%drb_%dport_%s" % p[:3]


def window_prbs(n_rb):
    """The first and last PRB that hold a sub-carrier of the PBCH / PSS / SSS window"""
    first, last = dm.sync_window(n_rb)
    return first // 12, last // 12


def near_window(n_rb):
    """Both band edges and every PRB within three of the window"""
    fp, lp = window_prbs(n_rb)
    return sorted({0, n_rb - 1} | set(range(max(0, fp - 3), min(n_rb, lp + 4))))


def plan_e_bytes(allocs, cfi):
    """What decides the plan's store path: the largest allocation's soft-bit slots (plan_layout's e_max: every sub-carrier outside the control
    region), in whole 32-bit scrambling words, rounded up to 64 bytes (pdsch_demod's e_bytes; assembled in LDS up to 32 768, stored directly past it)"""
    e_max = max((14 - (al.n_pdcch_symbs or cfi)) * al.N_prb * 12 * dm.QM[al.mod_type] for al in allocs)
    return ((e_max + 31) // 32 * 32 + 63) & ~63


def prb_lists(al):
    return [al.prb[0][i] for i in range(al.N_prb)], [al.prb[1][i] for i in range(al.N_prb)]


def kinds_of(al, n_rb):
    """The kinds of KINDS an allocation is, read off its PRB lists"""
    p0, p1 = prb_lists(al)
    fp, lp = window_prbs(n_rb)
    inside = lambda ps: any(fp <= p <= lp for p in ps)
    asc = all(b > a for a, b in zip(p0, p0[1:])) and all(b > a for a, b in zip(p1, p1[1:]))
    contiguous = all(b == a + 1 for a, b in zip(p0, p0[1:]))
    out = set()
    if p0 != p1:
        out.add("slots_differ")
        if inside(p0) != inside(p1):
            out.add("one_slot_in_window")
    elif not asc:
        out.add("not_ascending")
    elif len(p0) == 1:
        if p0[0] in (0, n_rb - 1, fp, lp):
            out.add("single")
    elif contiguous:
        if 2 <= len(p0) <= 8 and inside(p0) and (n_rb == 6 or not all(fp <= p <= lp for p in p0)):
            out.add("run")
    else:
        out.add("scattered")
    return out


def _run(rng, n_rb, edge):
    """2 .. 8 contiguous PRBs across one edge of the window: the PRB that holds its first (edge 0) or last (edge 1) sub-carrier and the PRB outside
    it.  At 6 RB the window is the band: anywhere."""
    fp, lp = window_prbs(n_rb)
    n = int(rng.integers(2, min(8, n_rb) + 1))
    if n_rb == 6:
        start = int(rng.integers(0, n_rb - n + 1))
    else:
        lo, hi = (fp - 1, fp) if edge == 0 else (lp, lp + 1)
        start = int(rng.integers(max(0, hi - n + 1), min(lo, n_rb - n) + 1))
    return list(range(start, start + n)), None


def _scattered(rng, n_rb):
    near = near_window(n_rb)
    while True:
        n = int(rng.integers(2, min(8, len(near) - 1) + 1))
        p = sorted(int(x) for x in rng.choice(near, n, replace=False))
        if p[-1] - p[0] + 1 > n:
            return p, None


def _draw_prbs(rng, n_rb, kind, edge):
    fp, lp = window_prbs(n_rb)
    near = near_window(n_rb)
    if kind == "single":
        return [int(rng.choice(sorted({0, n_rb - 1, fp, lp})))], None
    if kind == "run":
        return _run(rng, n_rb, edge)
    if kind == "scattered":
        return _scattered(rng, n_rb)
    if kind == "one_slot_in_window" and n_rb > 6:  # (at 6 RB every PRB is inside: the lists only differ)
        ins, outs = [p for p in near if fp <= p <= lp], [p for p in near if not fp <= p <= lp]
        n = int(rng.integers(1, 5))
        a, b = sorted(int(x) for x in rng.choice(ins, n, replace=False)), sorted(int(x) for x in rng.choice(outs, n, replace=False))
        return (a, b) if rng.random() < 0.5 else (b, a)
    if kind in ("slots_differ", "one_slot_in_window"):
        n = int(rng.integers(1, min(6, len(near) - 1) + 1))
        while True:
            a, b = (sorted(int(x) for x in rng.choice(near, n, replace=False)) for _ in range(2))
            if a != b:
                return a, b
    assert kind == "not_ascending"
    p = (_scattered(rng, n_rb) if rng.random() < 0.5 else _run(rng, n_rb, edge))[0]
    while True:
        q = [int(x) for x in rng.permutation(p)]
        if q != p:
            return q, None


def synthetic_planes(rng, n_ant, snr_db):
    """One unit, float32 [2 + 2 n_ant, 16, 1200]: test_demap_llr_cpu.synthetic_unit's two-tap estimate (gains 0.5 .. 1.5, up to 4 samples apart)
    under an independent complex gain of 0.5 .. 1.5 per port, unit-power symbols of the three modulations through the ports' mean, noise at snr_db.
    (No Alamouti pairs: the demapper is a function of the planes, and the model is held to the same planes.)"""
    k, sym = np.arange(dm.N_SC)[None, :], np.arange(16)[:, None]
    g0, g1 = rng.uniform(0.5, 1.5, 2) * np.exp(2j * np.pi * rng.random(2))
    common = g0 + g1 * np.exp(-2j * np.pi * (k - 600) * 4 / 2048) * np.exp(0.02j * sym)
    port = rng.uniform(0.5, 1.5, n_ant) * np.exp(2j * np.pi * rng.random(n_ant))
    h = port[:, None, None] * common[None]
    mod_of = rng.integers(1, 4, (16, dm.N_SC))
    s = np.zeros((16, dm.N_SC), complex)
    for mod in (1, 2, 3):
        pts, _ = dm.constellation(mod)
        s = np.where(mod_of == mod, pts[rng.integers(0, len(pts), s.shape)], s)
    hbar = h.mean(0)
    sigma = 10 ** (-snr_db / 20) * np.sqrt((np.abs(hbar) ** 2).mean() / 2)
    y = hbar * s + sigma * (rng.standard_normal(s.shape) + 1j * rng.standard_normal(s.shape))
    planes = np.zeros((2 + 2 * n_ant, 16, dm.N_SC), np.float32)
    planes[0], planes[1], planes[2:2 + n_ant], planes[2 + n_ant:] = y.real, y.imag, h.real, h.imag
    return planes


def draw(n_rb, n_ant, variant, seed):
    """(plan cfi, subframes [3], cells [3], allocations, planes float32 [3, 2 + 2 n_ant, 16, 1200]).  Units: subframes 0, 5 and one of the other
    eight; the cells' CRS shifts are three different residues mod 6 on one port (over the six bandwidths every residue) and all three residues
    mod 3 on two and four ports.  Four allocations per unit (tx_mode 2 on two and four ports): every kind of KINDS and every modulation at least
    once, a run across each edge of the window and the one-slot-in-window set in subframes 0 / 5; n_pdcch_symbs 0 (the plan's) .. 3, 4 as well at
    6 RB; tbs from the first rows of Table 7.1.7.2.1-1.  variant "lds_max" / "direct_min": one more 16QAM allocation of BIG_PRB[variant]
    contiguous PRBs with its own control region of 2 symbols."""
    import openlte_amd as m
    rng = np.random.default_rng(seed)
    table = tbs_table()
    cfi = int(rng.integers(1, 4))
    sfs = [0, 5, int(rng.choice([1, 2, 3, 4, 6, 7, 8, 9]))]
    if n_ant == 1:
        d = rng.choice(np.arange(1, 6), 2, replace=False)
        res = rng.permutation([N_RBS.index(n_rb), N_RBS.index(n_rb) + d[0], N_RBS.index(n_rb) + d[1]]) % 6
        cells = [int(r + 6 * rng.integers(0, 84)) for r in res]
    else:
        cells = [int(r + 3 * rng.integers(0, 168)) for r in rng.permutation(3)]
    planes = np.stack([synthetic_planes(rng, n_ant, float(rng.choice([20.0, 5.0]))) for _ in range(3)])
    # twelve (kind, edge) specs: the window-bound ones on slots of units 0 and 1, the rest anywhere
    bound = [("run", 0), ("run", 1), ("one_slot_in_window", 0)]
    free = [(k, int(rng.integers(0, 2))) for k in ("single", "scattered", "slots_differ", "not_ascending")] + \
           [(KINDS[int(rng.integers(0, len(KINDS)))], int(rng.integers(0, 2))) for _ in range(5)]
    spec = [None] * 12
    for pos, s in zip(rng.choice(8, 3, replace=False), bound):
        spec[int(pos)] = s
    for pos, s in zip([i for i in range(12) if spec[i] is None], rng.permutation(len(free))):
        spec[pos] = free[int(s)]
    mods = [int(x) for x in rng.permutation([1, 2, 3] + [int(v) for v in rng.integers(1, 4, 9)])]
    syms = [int(x) for x in rng.integers(0, 5 if n_rb == 6 else 4, 12)]
    if n_rb == 6 and 4 not in syms:
        syms[int(rng.integers(0, 12))] = 4
    rntis = [int(x) for x in rng.choice(np.arange(1, 0xFFF0), 13, replace=False)]
    allocs = []
    for i, (kind, edge) in enumerate(spec):
        p0, p1 = _draw_prbs(rng, n_rb, kind, edge)
        allocs.append(m.make_alloc(i // 4, mods[i], int(table[int(rng.integers(0, 4))][len(p0) - 1]), p0, rntis[i], tx_mode=1 if n_ant == 1 else 2,
                                   prbs_slot1=p1, n_pdcch_symbs=syms[i]))
    if variant != "small":
        n = BIG_PRB[variant]
        start = int(rng.integers(0, n_rb - n + 1))
        big = m.make_alloc(int(rng.integers(0, 3)), 2, int(table[10][n - 1]), list(range(start, start + n)), rntis[12], tx_mode=1 if n_ant == 1 else 2,
                           n_pdcch_symbs=2)
        allocs.insert(int(rng.integers(0, 13)), big)
    return cfi, sfs, cells, allocs, planes


def model_of(drawn, n_rb, n_ant, gain, T):
    """dm.demap of every allocation of a draw, in the plan's order"""
    cfi, sfs, cells, allocs, planes = drawn
    return [dm.demap(planes[al.unit], [al], sfs[al.unit], cells[al.unit], n_rb, cfi, n_ant, gain=gain, T=T)[0] for al in allocs]
