"""Float64 model of the PHICH: the decoder of include/mi_lte.h ("PHICH, 3GPP mode") restated step by step, and an independent modulator for
1, 2 and 4 CRS ports written from 36.211 6.9.1 (modulation, orthogonal sequences, scrambling), 6.9.2 (layer mapping and precoding, with
6.3.3.3 / 6.3.4.3) and 6.9.3 (the quadruplets onto the group's three resource-element groups).  Nothing here calls the library: the
tests compare the two.

Shapes.  `present` and `hi` are uint8 [n_units, N_group, 8] (the shape of mi_lte_phich's present / b per unit).  A device subframe is
float32 [2 + 2 n_ant, 16, 1200]: y real, y imaginary, n_ant real estimate planes, n_ant imaginary estimate planes."""
from fractions import Fraction
import math

import numpy as np

WALSH = np.array([[1, 1, 1, 1], [1, -1, 1, -1], [1, 1, -1, -1], [1, -1, -1, 1]], np.float64)
Z0 = (1 + 1j) / math.sqrt(2.0)
N_SC = 1200


def seq_w(n):
    """w_n(j), 36.211 table 6.9.1-2 (normal cyclic prefix): four real rows, then the same four times j"""
    return WALSH[n % 4] * (1.0 if n < 4 else 1j)


def gold(c_init, n):
    """c(0) .. c(n-1) of 36.211 7.2"""
    x1 = [1] + [0] * 30
    x2 = [(c_init >> i) & 1 for i in range(31)]
    for i in range(1600 + n - 31):
        x1.append((x1[i + 3] + x1[i]) & 1)
        x2.append((x2[i + 3] + x2[i + 2] + x2[i + 1] + x2[i]) & 1)
    return np.array([(x1[i + 1600] + x2[i + 1600]) & 1 for i in range(n)], np.uint8)


def scramble_signs(subfr_num, cell):
    """s(e) = 1 - 2 c(e), e < 12"""
    return 1.0 - 2.0 * gold((((subfr_num + 1) * (2 * cell + 1)) << 9) + cell, 12).astype(np.float64)


def n_group(n_rb_dl, n_g):
    """ceil(N_g N_rb_dl / 8) in exact rationals; n_g a Fraction"""
    return math.ceil(Fraction(n_g) * n_rb_dl / 8)


def pcfich_reg_numbers(n_rb_dl, cell):
    """REG numbers (minus one half) of the four PCFICH REGs of symbol 0"""
    k_hat = 6 * (cell % (2 * n_rb_dl))
    return [((k_hat + ((i * n_rb_dl) // 2) * 6) % (12 * n_rb_dl)) // 6 - 0.5 for i in range(4)]


def group_regs(n_rb_dl, cell, m, raw=False):
    """REG numbers of group m's three REGs: counted among the REGs the PCFICH left (raw), then in the numbering of all REGs of symbol 0"""
    n_l = 2 * n_rb_dl - 4
    n_hat = [(cell + m + (i * n_l) // 3) % n_l for i in range(3)]
    if raw:
        return n_hat
    for pn in pcfich_reg_numbers(n_rb_dl, cell):
        n_hat = [n + 1 if n > pn else n for n in n_hat]
    return n_hat


def group_res(n_rb_dl, cell, m):
    """sub-carriers of RE(4 i + j): the four of each REG's six with k mod 3 != cell mod 3, in increasing k"""
    return [6 * n + j for n in group_regs(n_rb_dl, cell, m) for j in range(6) if j % 3 != cell % 3]


def port_pair(n_ant, i, m):
    """the two ports that carry quadruplet i of group m (36.211 6.9.2)"""
    if n_ant == 2:
        return 0, 1
    return (0, 2) if (i + m) % 2 == 0 else (1, 3)


def smooth_channel(rng, n_ant, flat=False):
    """complex128 [n_ant, 1200]: per port a few paths of random gain and delay (a smooth function of k), mean power about 1"""
    k = np.arange(N_SC)
    h = np.zeros((n_ant, N_SC), np.complex128)
    for p in range(n_ant):
        if flat:
            h[p] = rng.uniform(0.5, 1.5) * np.exp(2j * np.pi * rng.random())
            continue
        a = rng.normal(size=4) + 1j * rng.normal(size=4)
        a *= np.array([1.0, 0.5, 0.35, 0.25]) / math.sqrt(2.0)
        tau = np.concatenate([[0.0], rng.uniform(1.0, 40.0, 3)])
        h[p] = (a[:, None] * np.exp(-2j * np.pi * tau[:, None] * k[None, :] / 2048.0)).sum(0)
        h[p] /= math.sqrt(np.mean(np.abs(h[p]) ** 2))
    return h


def modulate_group(n_ant, m, present, hi, s):
    """complex128 [n_ant, 12]: what each port sends on RE(0) .. RE(11) of group m"""
    d = np.zeros(12, np.complex128)
    for n in range(8):
        if present[n]:
            z = -Z0 if hi[n] else Z0  # BPSK, 36.211 table 7.1.1-1
            d += np.tile(seq_w(n), 3) * s * z  # d(e) = w(e mod 4) (1 - 2 c(e)) z(floor(e / 4)), the three z equal (36.212 5.3.5)
    y = np.zeros((n_ant, 12), np.complex128)
    if n_ant == 1:
        y[0] = d
        return y
    for i in range(3):
        pa, pb = port_pair(n_ant, i, m)
        for e in (4 * i, 4 * i + 2):  # 36.211 6.3.4.3 on the pair (x0, x1) = (d(e), d(e + 1))
            x0, x1 = d[e], d[e + 1]
            y[pa, e], y[pa, e + 1] = x0 / math.sqrt(2.0), x1 / math.sqrt(2.0)
            y[pb, e], y[pb, e + 1] = -np.conj(x1) / math.sqrt(2.0), np.conj(x0) / math.sqrt(2.0)
    return y


def modulate(n_rb_dl, n_ant, cells, subfr_nums, present, hi, rng, snr_db=None, flat=False, est_noise=True, dtype=np.float32):
    """[n_units, 2 + 2 n_ant, 16, 1200] device subframes (float32 as the device holds them; float64 for the model's own round trip) with
    symbol 0 filled: the PHICH groups of every unit through a smooth random channel per port (flat: one gain per port) plus AWGN at snr_db
    (None: none) relative to one indicator of unit power, and the true (est_noise False or no noise) or noisy estimates (noise power a
    quarter of the data's)."""
    n_units, n_grp = present.shape[0], present.shape[1]
    out = np.zeros((n_units, 2 + 2 * n_ant, 16, N_SC), dtype)
    sigma = 0.0 if snr_db is None else 10.0 ** (-snr_db / 20.0)
    for u in range(n_units):
        h = smooth_channel(rng, n_ant, flat)
        s = scramble_signs(subfr_nums[u], cells[u])
        y = np.zeros(N_SC, np.complex128)
        for m in range(n_grp):
            k = group_res(n_rb_dl, cells[u], m)
            tx = modulate_group(n_ant, m, present[u, m], hi[u, m], s)
            y[k] += (h[:, k] * tx).sum(0)
        used = 12 * n_rb_dl
        y[:used] += sigma * (rng.normal(size=used) + 1j * rng.normal(size=used)) / math.sqrt(2.0)
        est = h.copy()
        if est_noise and sigma:
            est[:, :used] += 0.5 * sigma * (rng.normal(size=(n_ant, used)) + 1j * rng.normal(size=(n_ant, used))) / math.sqrt(2.0)
        out[u, 0, 0], out[u, 1, 0] = y.real, y.imag
        out[u, 2:2 + n_ant, 0], out[u, 2 + n_ant:, 0] = est.real, est.imag
    return out


def decode(n_rb_dl, n_ant, n_grp, cell, subfr_num, sub, pair=port_pair):
    """The decoder of mi_lte.h in float64 on one device subframe (float32 [2 + 2 n_ant, 16, 1200]).  Returns metric [N_group, 8],
    power [N_group], rep [N_group, 8, 3], hi [N_group, 8]; pair(n_ant, i, m): the port pair of a quadruplet (a test passes a wrong one)."""
    sub = sub.astype(np.float64)
    y = sub[0, 0] + 1j * sub[1, 0]
    h = sub[2:2 + n_ant, 0] + 1j * sub[2 + n_ant:2 + 2 * n_ant, 0]
    s = scramble_signs(subfr_num, cell)
    metric, power, rep = np.zeros((n_grp, 8)), np.zeros(n_grp), np.zeros((n_grp, 8, 3))
    for m in range(n_grp):
        k = group_res(n_rb_dl, cell, m)
        r, P = np.zeros(12, np.complex128), np.zeros(12)
        for e in range(12):
            if n_ant == 1:
                r[e], P[e] = y[k[e]] * np.conj(h[0, k[e]]), abs(h[0, k[e]]) ** 2
                continue
            pa, pb = pair(n_ant, e // 4, m)
            a, b = (e, e + 1) if e % 2 == 0 else (e - 1, e)
            if e == a:
                r[e] = math.sqrt(2.0) * (np.conj(h[pa, k[a]]) * y[k[a]] + h[pb, k[b]] * np.conj(y[k[b]]))
                P[e] = abs(h[pa, k[a]]) ** 2 + abs(h[pb, k[b]]) ** 2
            else:
                r[e] = math.sqrt(2.0) * (np.conj(h[pa, k[b]]) * y[k[b]] - h[pb, k[a]] * np.conj(y[k[a]]))
                P[e] = abs(h[pa, k[b]]) ** 2 + abs(h[pb, k[a]]) ** 2
        p_tot = P.sum()
        power[m] = p_tot
        if not (p_tot > 0 and math.isfinite(p_tot)):
            power[m] = 0.0
            continue
        for n in range(8):
            w = seq_w(n)
            for i in range(3):
                q = sum(np.conj(w[j]) * s[4 * i + j] * r[4 * i + j] for j in range(4))
                rep[m, n, i] = (q * np.conj(Z0)).real / p_tot
            metric[m, n] = rep[m, n, 0] + rep[m, n, 1] + rep[m, n, 2]
    return metric, power, rep, (metric < 0).astype(np.uint32)


def random_pattern(rng, n_units, n_grp, fill=0.5, full_group=True):
    """(present, hi) uint8 [n_units, N_group, 8]; with full_group the first group of unit 0 carries all eight sequences"""
    present = (rng.random((n_units, n_grp, 8)) < fill).astype(np.uint8)
    hi = rng.integers(0, 2, (n_units, n_grp, 8)).astype(np.uint8)
    if full_group:
        present[0, 0, :] = 1
    return present, hi
