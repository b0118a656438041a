"""float64 numpy restatement of the 3GPP PUSCH plans' DMRS noise estimate and noise-referenced gain (include/mi_lte.h, "PUSCH, 3GPP mode:
DMRS noise estimate and the noise-referenced gain"), next to pusch_llr_model: the same inputs as its h_polar (one unit's planes, the
allocation, the mi_lte_ul_dmrs_pusch sequence), and its demap() for the bytes once the gain is known.

  t_ls()      t_b[i] = y_b conj(r_b) on DMRS symbol b (rows 3 and 10) of the allocation's sub-carriers, complex128 [2, M]
  sigma2_t()  S / (120 N_prb), S the sum over both slots and the ten interior sub-carriers of every resource block of
              |t[i-1] - 2 t[i] + t[i+1]|^2
  gain()      (float)(scale / (float)sigma2), 0 where sigma2 is 0 or not finite or the quotient leaves the float range
"""
import numpy as np

import pusch_llr_model as pm


def t_ls(planes, al, dmrs):
    p = np.asarray(planes, np.float64)
    t = []
    for b, L in ((0, 3), (1, 10)):
        sc = pm.subcarriers(al, b)
        y = p[0, L, sc] + 1j * p[1, L, sc]
        r = np.asarray(dmrs[2 * b], np.float64) + 1j * np.asarray(dmrs[2 * b + 1], np.float64)
        t.append(y * np.conj(r))
    return np.stack(t)


def second_differences(t):
    """complex128 [2, N_prb, 10]: d_b[i] for i = 12 j + 1 .. 12 j + 10 -- never across a resource-block boundary"""
    t = np.asarray(t, np.complex128)
    blk = t.reshape(t.shape[0], -1, 12)
    return blk[:, :, :-2] - 2.0 * blk[:, :, 1:-1] + blk[:, :, 2:]


def sigma2_t(t):
    d = second_differences(t)
    n_prb = d.shape[1]
    return float((d.real * d.real + d.imag * d.imag).sum() / (120.0 * n_prb))


def sigma2(planes, al, dmrs):
    return sigma2_t(t_ls(planes, al, dmrs))


def gain(scale, s2):
    """s2: the float32 estimate (the tap).  Returns the float value as a Python float."""
    s2 = np.float32(s2)
    with np.errstate(all="ignore"):
        g = np.float64(np.float32(scale)) / np.float64(s2)
        ok = np.isfinite(s2) and s2 > 0 and np.isfinite(np.float32(g))
        return float(np.float32(g)) if ok else 0.0
