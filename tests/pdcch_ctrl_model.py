"""Float64 model of the first stage of the blind PDCCH search (include/mi_lte.h, "PDCCH, 3GPP mode", step 1 of mi_lte_pdcch_search_run: "The
de-mapper's arithmetic"): the control region's geometry written from 36.211 6.2.4 (resource-element groups), 6.7.4 (PCFICH), 6.9.3 (PHICH,
normal duration) and 6.8.5 (the PDCCH walk, the quadruplet interleaver of 36.212 5.1.4.2.1 and the cyclic shift); an independent modulator
for 1, 2 and 4 CRS ports from 36.211 6.7, 6.8, 6.3.3.3 and 6.3.4.3 with a DCI encoder on top (36.212 5.3.3: CRC16 XOR RNTI, tail-biting
convolutional code, rate matching); and the decoder of the header restated in float64 -- PCFICH decision, combiner, QPSK soft value,
descrambling.  Nothing here calls the library: the tests compare the two.

Shapes.  A device subframe is float32 [2 + 2 n_ant, 16, 1200]: y real, y imaginary, n_ant real estimate planes, n_ant imaginary estimate
planes; a grid index is l * 1200 + k.  `bits` is uint8 [N_cce, 72] with NIL (= 2, nothing sent) on every bit of an unused CCE.

PHICH positions.  6.9.3 numbers the resource-element groups the PCFICH left in ascending frequency.  The library (and its transmitter, and
the PHICH decoder of the same header) steps over the four PCFICH groups in the order 6.7.4 lists them, which is not ascending once
k_bar + floor(i N_rb / 2) N_sc / 2 wraps (header, "PHICH, 3GPP mode", Positions).  With four ports the library also takes N_rb groups off
N_reg for the second symbol's CRS when the region has one symbol only.  The header's step 1 names both.  numbering = "library" is that
documented numbering (phich_model.group_regs, the formula's N_reg) and what the comparison with the library uses; numbering = "36.211" is
6.9.3 and 6.8.1 read literally.  The two give the same tables wherever the PHICH groups come out the same and not (4 ports, 1 symbol).

Close calls.  The device evaluates the same formulas in float32, so an integer soft value can differ from this model's where
v = 127 (1 - dist) lies next to an integer, or a component of x next to an axis.  decode() flags, per soft bit,
  close_v:   |v - round(v)| < DELTA_V (and dist below the cap);
  close_sym: a component of the bit's symbol x lies within DELTA_X |x| of an axis (the quadrant, and with it dist, may be the neighbour's);
  close_bit: the bit's own component does (its sign may be the neighbour's).
DELTA_V and DELTA_X were not chosen in advance.  The header's formula was evaluated in numpy float32 and in float64 over the 10 dB and the
-3 dB inputs of pdcch_ctrl_cases (every case, PCFICH included; measure_f32_gap below, re-measured by test_pdcch_ctrl_model_cpu), and 8 times
the largest difference taken -- the factor covers FMA contraction and the hardware's divide and root, which numpy does not imitate:
  largest |v32 - v64| over unsaturated elements           : MEASURED_V = 4.844e-5 (3.78e-5 at 10 dB)  ->  DELTA_V = 3.88e-4
  largest |x32 - x64| / |x64| over either component of x   : MEASURED_X = 9.439e-6 (7.00e-7 at 10 dB)  ->  DELTA_X = 7.55e-5
(the -3 dB figure of x comes from elements whose noisy estimates nearly vanish, where the combiner's sums cancel)
The tests' limits -- at most 1 % of a case's bits may be close calls, at least half must be unsaturated -- are conditions on the inputs, not
measurements."""
from fractions import Fraction
import functools
import math

import numpy as np

from phich_model import gold, group_regs, pcfich_reg_numbers, smooth_channel
from test_ulsch_cqi_cpu import P_CONV, conv_tb, rm_index

N_SC = 1200
NIL = 2
NO_RE = 0xFFFFFFFF
MEASURED_V, MEASURED_X = 4.844e-5, 9.439e-6
DELTA_V, DELTA_X = 8 * MEASURED_V, 8 * MEASURED_X
R2 = 1.0 / math.sqrt(2.0)
CAP = 1.0 - 1.0 / 120
N_G = {"1/6": Fraction(1, 6), "1/2": Fraction(1, 2), "1": Fraction(1), "2": Fraction(2)}
# 36.212 table 5.3.4-1: CFI 1 .. 4 (the fourth is reserved, all zero)
CFI_WORDS = np.array([([0, 1, 1] * 11)[:32], ([1, 0, 1] * 11)[:32], ([1, 1, 0] * 11)[:32], [0] * 32], np.uint8)
VARIANTS = ("freq_first", "no_shift", "no_colperm", "swap4", "own_est", "norm2", "scr_off1")


# ---- a. geometry

def n_group(n_rb, n_g):
    return math.ceil(Fraction(n_g) * n_rb / 8)


@functools.lru_cache(maxsize=4096)
def pcfich_regs(n_rb, cell):
    """the four REGs of symbol 0 (REG n starts at sub-carrier 6 n), in the order 6.7.4 lists them"""
    k_bar = 6 * (cell % (2 * n_rb))
    regs = [((k_bar + ((i * n_rb) // 2) * 6) % (12 * n_rb)) // 6 for i in range(4)]
    assert [r - 0.5 for r in regs] == pcfich_reg_numbers(n_rb, cell)
    return tuple(regs)


@functools.lru_cache(maxsize=4096)
def phich_regs(n_rb, cell, n_g, numbering="library"):
    """REGs of symbol 0 of all PHICH groups, normal duration (6.9.3: n_i = (cell + m' + floor(i n_0 / 3)) mod n_0 among the REGs the PCFICH left)"""
    out = []
    free = sorted(set(range(2 * n_rb)) - set(pcfich_regs(n_rb, cell)))
    for m in range(n_group(n_rb, n_g)):
        if numbering == "library":
            out += group_regs(n_rb, cell, m)
        else:
            out += [free[(cell + m + (i * len(free)) // 3) % len(free)] for i in range(3)]
    return tuple(out)


_ORDER = {}


def interleaver_order(n, colperm=True):
    """36.212 5.1.4.2.1 on n quadruplets, NULLs removed: output position j holds input order[j]"""
    if (n, colperm) not in _ORDER:
        R = -(-n // 32)
        y = np.concatenate([np.full(32 * R - n, -1), np.arange(n)]).reshape(R, 32)
        w = (y[:, P_CONV] if colperm else y).T.reshape(-1)
        _ORDER[(n, colperm)] = w[w >= 0]
    return _ORDER[(n, colperm)]


def pcfich_res(n_rb, cell):
    """the 16 grid indices of the PCFICH: per REG the four of its six sub-carriers that carry no CRS of ports 0 / 1"""
    return np.array([6 * n + j for n in pcfich_regs(n_rb, cell) for j in range(6) if j % 3 != cell % 3], np.int64)


def geometry(n_rb, n_ant, cell, n_g, n_symbs, numbering="library", walk="time_first", shift=True, colperm=True):
    """(N_cce, cce_re int64 [N_cce, 36], pcfich_re int64 [16]): the inputs of the library's cce_res, the result as grid indices"""
    taken = np.zeros(2 * n_rb, bool)
    taken[list(pcfich_regs(n_rb, cell))] = True
    taken[list(phich_regs(n_rb, cell, n_g, numbering))] = True
    k0, sym = [], []
    for l in range(n_symbs):  # 6.2.4: symbol 0 always two REGs per PRB (CRS of ports 0 / 1 counted), symbol 1 two with four ports, else three
        k0.append(6 * np.flatnonzero(~taken) if l == 0 else 6 * np.arange(2 * n_rb) if (l == 1 and n_ant == 4) else 4 * np.arange(3 * n_rb))
        sym.append(np.full(len(k0[-1]), l))
    k0, sym = np.concatenate(k0), np.concatenate(sym)
    # N_REG: the groups not assigned to PCFICH or PHICH (6.8.1).  The library forms it as N_symbs 3 N_rb - N_rb - 4 - 3 N_group, less N_rb
    # with four ports, and leaves whatever the walk finds past that unused; that is the count itself except in the two cases the module
    # docstring names.
    n_reg = len(k0)
    if numbering == "library":
        n_reg = n_symbs * 3 * n_rb - n_rb - 4 - 3 * n_group(n_rb, n_g) - (n_rb if n_ant == 4 else 0)
    if n_reg <= 0:
        return 0, np.zeros((0, 36), np.int64), pcfich_res(n_rb, cell)
    idx = (np.lexsort((sym, k0)) if walk == "time_first" else np.lexsort((k0, sym)))[:n_reg]  # 6.8.5: k' outer, l' inner
    k0, sym = k0[idx], sym[idx]
    six = (sym == 0) | ((sym == 1) & (n_ant == 4))
    off6 = np.array([j for j in range(6) if j % 3 != cell % 3])
    re = sym[:, None] * N_SC + k0[:, None] + np.where(six[:, None], off6[None, :], np.arange(4)[None, :])
    order = interleaver_order(n_reg, colperm)
    quad = np.empty((n_reg, 4), np.int64)
    quad[order[(np.arange(n_reg) + (cell if shift else 0)) % n_reg]] = re  # w_bar(i) = w((i + cell) mod N_reg) goes to the i-th group walked
    n_cce = n_reg // 9
    return n_cce, quad[:9 * n_cce].reshape(n_cce, 36), pcfich_res(n_rb, cell)


def candidate_table(n_cce, cce_re):
    """the six common-space candidates as mi_lte_pdcch_re_tables lays them out: uint32 [6, 288], NO_RE for a CCE past the last"""
    out = np.full((6, 288), NO_RE, np.uint32)
    for c in range(6):
        L = 4 if c < 4 else 8
        first = (c if c < 4 else c - 4) * L
        for j in range(L):
            if first + j < n_cce:
                out[c, 36 * j:36 * (j + 1)] = cce_re[first + j]
    return out


# ---- b. modulator

def qpsk(b):
    """36.211 table 7.1.2-1 on bit pairs; NIL pairs send nothing"""
    b = np.asarray(b).reshape(-1, 2)
    d = ((1.0 - 2.0 * (b[:, 0] & 1)) + 1j * (1.0 - 2.0 * (b[:, 1] & 1))) * R2
    return np.where(b[:, 0] == NIL, 0.0, d)


def precode(d, n_ant):
    """36.211 6.3.3.3 / 6.3.4.3: complex128 [n_ant, len(d)]"""
    y = np.zeros((n_ant, len(d)), np.complex128)
    if n_ant == 1:
        y[0] = d
        return y
    for p0, p1, a in ([(0, 1, 0)] if n_ant == 2 else [(0, 2, 0), (1, 3, 2)]):
        x0, x1 = d[a::n_ant], d[a + 1::n_ant]
        y[p0, a::n_ant], y[p0, a + 1::n_ant] = x0 * R2, x1 * R2
        y[p1, a::n_ant], y[p1, a + 1::n_ant] = -np.conj(x1) * R2, np.conj(x0) * R2
    return y


def scramble(bits, c):
    bits = np.asarray(bits, np.uint8).reshape(-1)
    return np.where(bits == NIL, NIL, (bits ^ c) & 1).astype(np.uint8)


def modulate(n_rb, n_ant, cell, sf, cfi, n_g, bits, rng, snr_db=None, est_noise=True, dtype=np.float32, quiet_pcfich=False, dead_port=None, numbering="library"):
    """One device subframe: the PCFICH (cfi 1 .. 4) and the PDCCH bits through a smooth channel per port plus AWGN at snr_db relative to a
    QPSK symbol of unit power (None: none), with the true estimates (est_noise False or no noise) or noisy ones (noise power a quarter of the
    data's) on symbols 0 .. 3.  quiet_pcfich: no noise on the PCFICH's 16 elements and their estimates, so that the region's size survives an
    SNR at which the PCFICH itself would not decode.  dead_port: a port in total fade -- nothing of it arrives and its estimate plane is zero."""
    n_symbs = cfi + (1 if n_rb <= 10 else 0)
    n_cce, cce_re, pc_re = geometry(n_rb, n_ant, cell, n_g, n_symbs, numbering)
    assert np.shape(bits) == (n_cce, 72)
    tx = np.zeros((n_ant, 4 * N_SC), np.complex128)
    tx[:, pc_re] = precode(qpsk(scramble(CFI_WORDS[cfi - 1], gold((((sf + 1) * (2 * cell + 1)) << 9) + cell, 32))), n_ant)
    tx[:, cce_re.reshape(-1)] = precode(qpsk(scramble(bits, gold((sf << 9) + cell, 72 * n_cce))), n_ant)
    h = smooth_channel(rng, n_ant)
    if dead_port is not None:
        h[dead_port] = 0.0
    used = 12 * n_rb
    sigma = 0.0 if snr_db is None else 10.0 ** (-snr_db / 20.0)
    quiet = np.ones((4, N_SC))
    if quiet_pcfich:
        quiet[0, pc_re] = 0.0
    y = (np.tile(h, (1, 4)) * tx).sum(0).reshape(4, N_SC)
    y[:, :used] += sigma * quiet[:, :used] * (rng.normal(size=(4, used)) + 1j * rng.normal(size=(4, used))) * R2
    est = np.repeat(h[:, None, :], 4, axis=1)
    if est_noise and sigma:
        est[:, :, :used] += 0.5 * sigma * quiet[None, :, :used] * (rng.normal(size=(n_ant, 4, used)) + 1j * rng.normal(size=(n_ant, 4, used))) * R2
    if dead_port is not None:
        est[dead_port] = 0.0
    out = np.zeros((2 + 2 * n_ant, 16, N_SC), dtype)
    out[0, :4], out[1, :4] = y.real, y.imag
    out[2:2 + n_ant, :4], out[2 + n_ant:, :4] = est.real, est.imag
    return out


def crc16(bits):
    rem = 0
    for b in list(bits) + [0] * 16:
        rem = (rem << 1) | int(b)
        if rem & 0x10000:
            rem ^= 0x11021
    return rem


def dci_encode(payload, n_bits, rnti, L):
    """36.212 5.3.3 for one DCI: uint8 [72 L], the payload's first bit in bit n_bits - 1"""
    a = [(payload >> (n_bits - 1 - i)) & 1 for i in range(n_bits)]
    par = crc16(a) ^ rnti
    c = np.array(a + [(par >> (15 - i)) & 1 for i in range(16)], np.int64)
    return conv_tb(c)[rm_index(len(c), 72 * L)].astype(np.uint8)


def place_dcis(n_cce, recs):
    """bits [N_cce, 72] with records (rnti, L, first CCE, n_bits, payload) encoded in place, NIL elsewhere"""
    bits = np.full((n_cce, 72), NIL, np.uint8)
    for rnti, L, cce, n_bits, payload in recs:
        assert cce % L == 0 and cce + L <= n_cce and (bits[cce:cce + L] == NIL).all()
        bits[cce:cce + L] = dci_encode(payload, n_bits, rnti, L).reshape(L, 72)
    return bits


# ---- c. decoder (header, step 1: "The de-mapper's arithmetic")

def demap(sub, n_ant, re, c, dt=np.float64, own_est=False, swap4=False, norm2=False, delta_v=DELTA_V, delta_x=DELTA_X):
    """Elements re (grid indices, a multiple of n_ant of them) -> dict of per-bit arrays [2 len(re)]: soft (int), close_v, close_sym, close_bit, sat,
    and per element x_re, x_im, v; c: the scrambling bits of these soft bits; dt: the arithmetic's type"""
    re = np.asarray(re, np.int64)
    n_planes = (sub.shape[0] - 2) // 2
    f = lambda plane: sub[plane].reshape(-1)[re].astype(dt)
    yr, yi = f(0), f(1)
    hr, hi = [f(2 + p) for p in range(n_ant)], [f(2 + n_planes + p) for p in range(n_ant)]
    xr, xi = np.zeros(len(re), dt), np.zeros(len(re), dt)
    with np.errstate(all="ignore"):
        if n_ant == 1:
            hn = hr[0] * hr[0] + hi[0] * hi[0]
            xr, xi = (yr * hr[0] + yi * hi[0]) / hn, (yi * hr[0] - yr * hi[0]) / hn
        else:
            pairs = [(0, 1, 0)] if n_ant == 2 else ([(1, 3, 0), (0, 2, 2)] if swap4 else [(0, 2, 0), (1, 3, 2)])
            for A, B, a in pairs:  # elements a, a + 1 of every group of n_ant carry ports A, B
                ia, ib = np.arange(a, len(re), n_ant), np.arange(a + 1, len(re), n_ant)
                for tgt, first in ((ia, True), (ib, False)):
                    e = tgt if own_est else ia  # the pair's first element's estimates serve both
                    Ar, Ai, Br, Bi = hr[A][e], hi[A][e], hr[B][e], hi[B][e]
                    pa, pb = Ar * Ar + Ai * Ai, Br * Br + Bi * Bi
                    hn = (pa + pb) if norm2 else np.sqrt(pa * pa + pb * pb)
                    if first:  # x_a = (conj(h_A) y_a + h_B conj(y_b)) / hn
                        xr[tgt] = (Ar * yr[ia] + Ai * yi[ia] + Br * yr[ib] + Bi * yi[ib]) / hn
                        xi[tgt] = (Ar * yi[ia] - Ai * yr[ia] - Br * yi[ib] + Bi * yr[ib]) / hn
                    else:      # x_b = (conj(h_A) y_b - h_B conj(y_a)) / hn
                        xr[tgt] = (-Br * yr[ia] - Bi * yi[ia] + Ar * yr[ib] + Ai * yi[ib]) / hn
                        xi[tgt] = (Br * yi[ia] - Bi * yr[ia] + Ar * yi[ib] - Ai * yr[ib]) / hn
        r2, cap = dt(R2), dt(1) - dt(1) / dt(120)
        er, ei = np.where(xr > 0, r2, -r2), np.where(xi > 0, r2, -r2)
        dr, di = xr - er, xi - ei
        dist = np.sqrt(dr * dr + di * di)
        v = dt(127) * (dt(1) - np.minimum(dist, cap))
        m = np.where(np.isnan(v), 0, np.trunc(v)).astype(np.int64)  # a non-finite x (zero estimates): 0
        mag = np.sqrt(xr.astype(np.float64) ** 2 + xi.astype(np.float64) ** 2)
        near_r, near_i = np.abs(xr) < delta_x * mag, np.abs(xi) < delta_x * mag
        close_v = (np.abs(v - np.rint(v)) < delta_v) & (dist < cap)
    s = 1 - 2 * np.asarray(c, np.int64)
    two = lambda a, b: np.stack([a, b], axis=1).reshape(-1)
    return {"soft": two(np.where(er > 0, m, -m), np.where(ei > 0, m, -m)) * s, "close_v": two(close_v, close_v), "close_sym": two(near_r | near_i, near_r | near_i),
            "close_bit": two(near_r, near_i), "sat": two(dist >= cap, dist >= cap), "x_re": xr, "x_im": xi, "v": v, "dist": dist}


def decode(n_rb, n_ant, cell, sf, n_g, sub, dt=np.float64, variant=None, numbering="library"):
    """The header's step 1 on one device subframe: dict with cfi, n_cce and, over the 72 N_cce soft bits, the arrays of demap();
    pcfich: demap() of the PCFICH's 32 bits.  variant: one of VARIANTS, a decoder that is wrong in that one respect.  numbering: "library"
    (the default tables) or "36.211" (MI_LTE_PDCCH_SEARCH_36211_REGS)."""
    assert variant is None or variant in VARIANTS
    kw = {"own_est": variant == "own_est", "swap4": variant == "swap4", "norm2": variant == "norm2"}
    pc = demap(sub, n_ant, pcfich_res(n_rb, cell), gold((((sf + 1) * (2 * cell + 1)) << 9) + cell, 32), dt, **kw)
    ber = ((pc["soft"] < 0)[None, :] != (CFI_WORDS == 1)).sum(1)
    cfi = int(np.argmin(ber)) + 1 if ber.min() < 4 else 0  # the first minimum wins; accepted below 4 errors
    n_symbs = cfi + (1 if n_rb <= 10 else 0)
    if cfi == 0 or n_symbs > 4:
        return {"cfi": 0, "n_cce": 0, "pcfich": pc, "soft": np.zeros(0, np.int64)}
    n_cce, cce_re, _ = geometry(n_rb, n_ant, cell, n_g, n_symbs, numbering, walk="freq_first" if variant == "freq_first" else "time_first",
                                shift=variant != "no_shift", colperm=variant != "no_colperm")
    off = 1 if variant == "scr_off1" else 0
    out = demap(sub, n_ant, cce_re.reshape(-1), gold((sf << 9) + cell, 72 * n_cce + off)[off:], dt, **kw)
    out.update(cfi=cfi, n_cce=n_cce, pcfich=pc)
    return out


def compare(got, want):
    """got: integer soft bits; want: decode()'s dict.  (number of close calls, indices that differ by more than a close call allows): equal
    everywhere; on a close call the magnitude may differ by 1; on an axis close call the bit on the axis may take the other sign."""
    got, soft = np.asarray(got, np.int64), want["soft"]
    close = want["close_v"] | want["close_sym"]
    sign_ok = ((got < 0) == (soft < 0)) | want["close_bit"]
    ok = (got == soft) | (close & (np.abs(np.abs(got) - np.abs(soft)) <= 1) & sign_ok & (soft != 0))
    return int(close.sum()), np.flatnonzero(~ok)


def measure_f32_gap(subs):
    """subs: iterable of (n_rb, n_ant, cell, sf, n_g, sub).  (largest |v32 - v64| over unsaturated elements, largest component difference of
    x relative to |x64|) between the header's formula in numpy float32 and in float64, PCFICH elements included."""
    gv = gx = 0.0
    for n_rb, n_ant, cell, sf, n_g, sub in subs:
        a, b = decode(n_rb, n_ant, cell, sf, n_g, sub, np.float32), decode(n_rb, n_ant, cell, sf, n_g, sub, np.float64)
        for p, q in [(a["pcfich"], b["pcfich"])] + ([(a, b)] if a["n_cce"] == b["n_cce"] and b["n_cce"] else []):
            live = (q["dist"] < CAP) & (p["dist"] < CAP)
            mag = np.hypot(q["x_re"], q["x_im"])
            if live.any():
                gv = max(gv, float(np.abs(p["v"].astype(np.float64) - q["v"])[live].max()))
            fin = np.isfinite(mag) & (mag > 0)
            gx = max(gx, float((np.maximum(np.abs(p["x_re"] - q["x_re"]), np.abs(p["x_im"] - q["x_im"]))[fin] / mag[fin]).max()))
    return gv, gx
