"""float64 numpy model of the 3GPP PUSCH plans' MI_LTE_DEMAP_MAXLOG (include/mi_lte.h, "PUSCH, 3GPP mode: max-log soft-decision demapping"),
built on demap_llr_model's llr_axis / soft_byte / in_guard / gold.  Two layers:

  exact      demap(): from the tapped symbols x_s[k], the tapped rho_s and the gain to the descrambled bytes at (k 12 + s) Q_m + q -- the
             kernel runs the same double operations in the same order, so the bytes agree outside the 2^-16 guard band.
  tolerance  rho(): from the subframe planes and mi_lte_ul_dmrs_pusch, the demodulator's polar interpolation between the two DMRS estimates
             (uplink.hip, "DMRS estimates and their interpolation slopes") restated in float64, and rho_s = M / sum_k 1 / |h_k(s)|^2;
             equalise_predecode(): from the same planes, the tapped symbols themselves -- the one-tap equaliser on that estimate and the
             transform pre-decoder as numpy's float64 inverse FFT (test_pusch_predecode_gpu.py).
"""
import numpy as np

import demap_llr_model as dm

N_SC = 1200
QM = dm.QM


def data_rows():
    """subframe row (OFDM symbol 0 .. 13) of data symbol s = 0 .. 11: the DMRS symbols 3 and 10 skipped"""
    return [L for L in range(14) if L not in (3, 10)]


def steps():
    """n of data symbol s: its distance from its slot's DMRS symbol, -3 .. -1, +1 .. +3"""
    return np.array([-3, -2, -1, 1, 2, 3] * 2, np.float64)


def subcarriers(al, b):
    """the allocation's M sub-carrier indices in slot b"""
    return np.concatenate([al.prb[b][i] * 12 + np.arange(12) for i in range(al.N_prb)])


def h_polar(planes, al, dmrs):
    """complex128 [12, M]: the interpolated estimate of every data symbol.  planes: one unit's float32 [2, 16, 1200]; dmrs: float32 [4, M]
    (ul_dmrs_pusch).  Per sub-carrier t_b = y_b conj(r_b) on DMRS symbol b (rows 3 and 10), f_mag = (|t_1| - |t_0|) / 7,
    f_ang = (arg t_1 - arg t_0, wrapped into (-pi, pi)) / 7, h(s) = (|t_b| + n f_mag) exp(i (arg t_b + n f_ang)), b the symbol's slot."""
    p = np.asarray(planes, np.float64)
    M = 12 * al.N_prb
    t = []
    for b, L in ((0, 3), (1, 10)):
        sc = subcarriers(al, b)
        y = p[0, L, sc] + 1j * p[1, L, sc]
        r = dmrs[2 * b].astype(np.float64) + 1j * dmrs[2 * b + 1].astype(np.float64)
        t.append(y * np.conj(r))
    mag, ang = [np.abs(v) for v in t], [np.angle(v) for v in t]
    f_mag = (mag[1] - mag[0]) / 7
    f_ang = ang[1] - ang[0]
    f_ang = np.where(f_ang >= np.pi, f_ang - 2 * np.pi, np.where(f_ang <= -np.pi, f_ang + 2 * np.pi, f_ang)) / 7
    h = np.zeros((12, M), np.complex128)
    for s, n in enumerate(steps()):
        b = s // 6
        h[s] = (mag[b] + n * f_mag) * np.exp(1j * (ang[b] + n * f_ang))
    return h


def equalised(planes, al, dmrs):
    """complex128 [12, M]: the one-tap equaliser's output z_s[k] = y_s[k] conj(h_s[k]) / |h_s[k]|^2 on the allocation's sub-carriers, y_s the
    subframe row data_rows()[s] of the symbol's slot and h = h_polar"""
    p = np.asarray(planes, np.float64)
    h = h_polar(planes, al, dmrs)
    z = np.zeros_like(h)
    for s, L in enumerate(data_rows()):
        sc = subcarriers(al, s // 6)
        y = p[0, L, sc] + 1j * p[1, L, sc]
        z[s] = y * np.conj(h[s]) / (h[s].real * h[s].real + h[s].imag * h[s].imag)
    return z


def equalise_predecode(planes, al, dmrs):
    """complex128 [12, M]: what k_pusch_demod<.., SPEC = true> taps (mi_lte_pusch_plan_set_llr_tap) -- the equalised symbols through the
    transform pre-decoder of 36.211 5.3.3, the unnormalised backward DFT times 1 / sqrt(M).  numpy's ifft divides by M, hence times sqrt(M)."""
    z = equalised(planes, al, dmrs)
    return np.fft.ifft(z, axis=1) * np.sqrt(z.shape[1])


def rho_of(h):
    """(rho [12], smallest |h|^2 per symbol [12], mean |h|^2 of the allocation): rho_s = M / sum_k 1 / |h_k(s)|^2, 0 where that is not finite"""
    w = h.real * h.real + h.imag * h.imag
    with np.errstate(all="ignore"):
        tot = (1.0 / w).sum(1)
        r = h.shape[1] / tot
        r = np.where(np.isfinite(tot) & np.isfinite(r) & np.isfinite(r.astype(np.float32)), r, 0.0)
    return r, w.min(1), w.mean()


def auto_gain(rho, mod, T):
    """(float)(T / (4 A^2 rhobar)), rhobar the mean in double of the twelve floats summed in order; 0 for a rhobar that is 0 or not finite or a
    gain past float.  Returns the float value as a Python float."""
    rbar = 0.0
    for v in np.asarray(rho, np.float32):
        rbar += float(v)
    rbar /= 12.0
    with np.errstate(all="ignore"):
        g = np.float64(T) / (dm.FOUR_A2[mod] * np.float64(rbar))
        ok = np.isfinite(rbar) and rbar > 0 and np.isfinite(np.float32(g))
    return float(np.float32(g)) if ok else 0.0


class Demapped:
    """bytes (int8 [12 M Q_m], descrambled, in the plan's order), x (the unrounded g L behind every byte), gain"""

    def __init__(self, bytes_, x, gain):
        self.bytes, self.x, self.gain = bytes_, x, gain


def demap(xs, rho, mod, c_init, gain=0.0, T=16):
    """xs: complex64 [12, M] tapped symbols; rho: float32 [12]; gain 0: automatic from rho.  The exact layer."""
    xs = np.asarray(xs)
    M, q = xs.shape[1], QM[mod]
    g = auto_gain(rho, mod, T) if gain == 0 else float(np.float32(gain))
    w = np.asarray(rho, np.float32).astype(np.float64)[:, None] * np.ones((1, M))
    xr, xi = xs.real.astype(np.float32).astype(np.float64), xs.imag.astype(np.float32).astype(np.float64)
    L = np.zeros((12, M, q))
    with np.errstate(all="ignore"):
        L[:, :, 0::2] = np.stack(dm.llr_axis(w * xr, w, mod), 2)
        L[:, :, 1::2] = np.stack(dm.llr_axis(w * xi, w, mod), 2)
        x = g * L
    c = dm.gold(c_init & 0x7FFFFFFF, 12 * M * q).reshape(12, M, q)  # scrambled in transmission order (s, k, q)
    x = np.where(c == 1, -x, x)
    x = np.ascontiguousarray(x.transpose(1, 0, 2)).reshape(-1)      # the channel de-interleaver: byte (k 12 + s) Q_m + q
    return Demapped(dm.soft_byte(x), x, g)
