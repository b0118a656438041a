"""float64 numpy restatement of the downlink CRS noise estimate and the 3GPP PDSCH plans' noise-referenced gain (include/mi_lte.h, "DL: CRS
noise estimate" and "PDSCH, 3GPP mode: noise-referenced gain"), next to demap_llr_model: one unit's planes (only the two y planes are read),
the cell's bandwidth and port count, the unit's subframe and cell; demap_llr_model.demap gives the bytes once the gain is known.

  rows()      the (port, CRS symbol) rows: ports 0 .. min(n_ant, 2) - 1 on symbols 0, 4, 7, 11
  pilots()    k_j = 6 j + (voff(p, i) + cell mod 6) mod 6 of one row
  crs()       the n_pil CRS values of one symbol (36.211 6.10.1.1), the same for every port
  t_ls()      t_j = y(symbol, k_j) conj(crs_j), complex128 [n_rows, n_pil]
  sigma2_t()  S / (6 n_rows (n_pil - 2)), S the sum over rows and j = 1 .. n_pil - 2 of |t[j-1] - 2 t[j] + t[j+1]|^2
  gain()      (float)(scale / (float)sigma2), 0 where sigma2 is 0 or not finite or the quotient leaves the float range
"""
from functools import lru_cache

import numpy as np

import demap_llr_model as dm

SYMBOLS = (0, 4, 7, 11)


def rows(n_ant):
    return [(p, i) for p in range(min(n_ant, 2)) for i in range(4)]


def voff(p, i):
    return 3 if (i + p) & 1 else 0


def pilots(n_rb, cell, p, i):
    return 6 * np.arange(2 * n_rb) + (voff(p, i) + cell % 6) % 6


@lru_cache(maxsize=None)
def crs(n_rb, cell, sf, sym):
    ns, l = 2 * sf + (1 if sym >= 7 else 0), sym % 7
    c = dm.gold((((7 * (ns + 1) + l + 1) * (2 * cell + 1)) << 10) + 2 * cell + 1, 440).astype(np.float64)
    m = np.arange(2 * n_rb) + 110 - n_rb
    return ((1 - 2 * c[2 * m]) + 1j * (1 - 2 * c[2 * m + 1])) / np.sqrt(2.0)


def t_ls(planes, n_rb, n_ant, sf, cell):
    out = []
    for port, i in rows(n_ant):  # (only the pilots are read: rows 14 and 15 of a front end's planes may hold anything)
        k = pilots(n_rb, cell, port, i)
        y = np.asarray(planes[0][SYMBOLS[i]][k], np.float64) + 1j * np.asarray(planes[1][SYMBOLS[i]][k], np.float64)
        out.append(y * np.conj(crs(n_rb, cell, sf, SYMBOLS[i])))
    return np.stack(out)


def second_differences(t):
    t = np.asarray(t, np.complex128)
    return t[:, :-2] - 2.0 * t[:, 1:-1] + t[:, 2:]


def sigma2_t(t):
    d = second_differences(t)
    return float((d.real * d.real + d.imag * d.imag).sum() / (6.0 * d.shape[0] * d.shape[1]))


def sigma2(planes, n_rb, n_ant, sf, cell):
    return sigma2_t(t_ls(planes, n_rb, n_ant, sf, cell))


def gain(scale, s2):
    """s2: the float32 estimate (the tap).  Returns the float value as a Python float."""
    s2 = np.float32(s2)
    with np.errstate(all="ignore"):
        g = np.float64(np.float32(scale)) / np.float64(s2)
        ok = np.isfinite(s2) and s2 > 0 and np.isfinite(np.float32(g))
        return float(np.float32(g)) if ok else 0.0
