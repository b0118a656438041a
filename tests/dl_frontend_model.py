"""A float64 model of mi_lte_dl_frontend_batch / mi_lte_ul_frontend_batch: OFDM demodulation and the CRS channel estimate of one subframe
unit, written from oracle/lte_oracle.c (lo_samples_to_symbols_dl, lo_get_dl_subframe_and_ce) and 36.211 6.10.1 / 7.2, with numpy's FFT as
the transform.  Nothing here restates a kernel: no Stockham passes, no wave-parallel unwrap, no row or column splits -- the unwrap is the
reference's serial rule, taken link by link as a cumulative sum, and every wrap decision reports how far it stood from +-pi.

What a float64 model cannot share with a float32 implementation is a wrap decision taken within rounding of +-pi; `forced` names such links
so that a test can hold an implementation to either outcome (tests/test_dl_frontend_model_gpu.py, the tie family)."""
import functools

import numpy as np

N_SC_MAX = 1200
SYM01, SYM23 = (0, 4, 7, 11, 14), (1, 8, 15)
VOFF = ((0, 3, 0, 3, 0), (3, 0, 3, 0, 3), (0, 3, 0), (3, 6, 3))  # 36.211 6.10.1.2: v of port p at its CRS symbols, before v_shift
TWO_PI = 2.0 * np.pi


def geom(fft):
    """(cp0, cpe, n_slot, samples per subframe) of an FFT size"""
    sc = 2048 // fft
    return 160 // sc, 144 // sc, 15360 // sc, 30720 // sc


def crs_symbols(p):
    return SYM01 if p < 2 else SYM23


def pilot_offset(p, i, cell):
    return (VOFF[p][i] + cell % 6) % 6


def window_start(fft, sym):
    """offset of symbol sym's (0 .. 15) FFT window from the unit's start: one sample inside the end of its cyclic prefix"""
    cp0, cpe, n_slot, _ = geom(fft)
    so = sym % 7
    return (sym // 7) * n_slot + so * (fft + cpe) + (cp0 - cpe if so else 0) + (cp0 if so == 0 else cpe) - 1


def symbol_rows(x, fft, n_rb, n_sym=16):
    """complex128 [n_sym, 12 n_rb]: x is the unit's complex samples from its start.  Guard band dropped, DC skipped, spectrum un-shifted:
    columns 0 .. half - 1 are bins N - half .. N - 1, columns half .. are bins 1 .. half."""
    return rows_at(x, fft, n_rb, [window_start(fft, s) for s in range(n_sym)])


def rows_at(x, fft, n_rb, starts):
    """complex128 [len(starts), 12 n_rb]: the same rows of the FFT windows that open at the given sample indices of x"""
    half = 6 * n_rb
    out = np.zeros((len(starts), 2 * half), np.complex128)
    for s, w in enumerate(starts):
        X = np.fft.fft(np.asarray(x[w:w + fft], np.complex128))
        out[s, :half], out[s, half:] = X[fft - half:], X[1:half + 1]
    return out


def ul_symbol_rows(x, fft, n_rb):
    """complex128 [14, 12 n_rb]: the uplink's half-sub-carrier-shifted grid -- the N-point FFT of x[n] exp(-i pi n / N), no DC skip"""
    half = 6 * n_rb
    rot = np.exp(-1j * np.pi * np.arange(fft) / fft)
    out = np.zeros((14, 2 * half), np.complex128)
    for s in range(14):
        w = window_start(fft, s)
        X = np.fft.fft(np.asarray(x[w:w + fft], np.complex128) * rot)
        out[s, :half], out[s, half:] = X[fft - half:], X[:half]
    return out


@functools.lru_cache(maxsize=None)
def gold(c_init, n):
    """c(0 .. n - 1) of 36.211 7.2 as uint8"""
    total = 1600 + n
    x1, x2 = np.zeros(total + 31, np.uint8), np.zeros(total + 31, np.uint8)
    x1[0] = 1
    x2[:31] = [(c_init >> b) & 1 for b in range(31)]
    for a in range(0, total, 28):  # x(n + 31) needs x up to n + 3: 28 steps at a time
        b = min(a + 28, total)
        x1[a + 31:b + 31] = x1[a + 3:b + 3] ^ x1[a:b]
        x2[a + 31:b + 31] = x2[a + 3:b + 3] ^ x2[a + 2:b + 2] ^ x2[a + 1:b + 1] ^ x2[a:b]
    return x1[1600:total] ^ x2[1600:total]


def crs(sf, sym, cell, n_rb):
    """complex128 [2 n_rb]: r_{l, ns}(m') at m' = m + 110 - n_rb of OFDM symbol sym (0 .. 15, 14 and 15 the next subframe's) -- 36.211
    6.10.1.1, normal cyclic prefix"""
    ns, l = (2 * sf + sym // 7) % 20, sym % 7
    c_init = 1024 * (7 * (ns + 1) + l + 1) * (2 * cell + 1) + 2 * cell + 1
    c = gold(c_init, 440).astype(np.float64)
    m = np.arange(2 * n_rb) + 110 - n_rb
    return ((1 - 2 * c[2 * m]) + 1j * (1 - 2 * c[2 * m + 1])) / np.sqrt(2.0)


def wrap(d):
    """d brought into (-pi, pi) by whole turns, as the reference's wrap_phase leaves p1 - p2"""
    return d - TWO_PI * np.round(d / TWO_PI)


class Result:
    """.symb complex128 [16, N_sc]; .mag / .ang: per port float64 [N_sym, N_sc], the rows after the frequency direction; .ce complex128
    [N_ant, 14, N_sc]; .margin_f: per port float64 [N_sym, n_pil - 1], pi - |step| of every frequency link; .margin_t: per port float64
    [segments, N_sc], the same for every time-direction wrap; .margin: the least of them all"""


def freq_rows(symb, sf, cell, n_rb, p, forced=()):
    """(mag, ang, margin) of port p: LS estimate at the pilots, the angle, the serial unwrap along frequency, linear interpolation between
    pilots and the reference's edge rule: below the first pilot the first slope is continued; above the last pilot the last slope is stepped
    with the same sign as below it (lo_get_dl_subframe_and_ce subtracts frac on both sides) -- a mirror image, not a continuation.
    forced: (p, i, j, turns) -- link j - 1 -> j of CRS symbol index i takes `turns` more whole turns than the rule gives."""
    n_pil, n_sc = 2 * n_rb, 12 * n_rb
    syms = crs_symbols(p)
    mag, ang, margin = np.zeros((len(syms), n_sc)), np.zeros((len(syms), n_sc)), np.zeros((len(syms), n_pil - 1))
    k_all = np.arange(n_sc)
    for i, sy in enumerate(syms):
        off = pilot_offset(p, i, cell)
        k = 6 * np.arange(n_pil) + off
        t = symb[sy, k] * np.conj(crs(sf, sy, cell, n_rb))
        m, r = np.abs(t), np.angle(t)
        step = wrap(np.diff(r))
        margin[i] = np.pi - np.abs(step)
        for fp, fi, fj, turns in forced:
            if fp == p and fi == i:
                step[fj - 1] += TWO_PI * turns
        u = r[0] + np.concatenate([[0.0], np.cumsum(step)])
        for src, dst in ((m, mag), (u, ang)):
            v = np.interp(k_all, k, src)
            lo, hi = k_all < k[0], k_all > k[-1]
            v[lo] = src[0] - (k[0] - k_all[lo]) * (src[1] - src[0]) / 6.0
            v[hi] = src[-1] - (k_all[hi] - k[-1]) * (src[-1] - src[-2]) / 6.0  # (the reference steps DOWN the last slope here too)
            dst[i] = v
    return mag, ang, margin


def time_interp(M, A, p):
    """(m [14, N_sc], a [14, N_sc], margin [segments, N_sc]) from the rows at the port's CRS symbols, in the reference's order: each later
    phase is wrapped against the already wrapped earlier one, the slope is the wrapped difference over the symbol distance, and ports 2 / 3
    reach symbol 0 by continuing the 1 -> 8 slope below symbol 1"""
    A = A.copy()
    m, a = np.zeros((14, M.shape[1])), np.zeros((14, M.shape[1]))
    syms = crs_symbols(p)
    margin = []
    for i in range(1, len(syms)):
        d = wrap(A[i] - A[i - 1])
        margin.append(np.pi - np.abs(d))
        A[i] = A[i - 1] + d
    for i in range(len(syms) - 1):
        lo, hi = syms[i], syms[i + 1]
        for z in range(lo, min(hi, 14)):
            f = (z - lo) / float(hi - lo)
            m[z], a[z] = M[i] + f * (M[i + 1] - M[i]), A[i] + f * (A[i + 1] - A[i])
    if p >= 2:
        m[0], a[0] = M[0] - (M[1] - M[0]) / 7.0, A[0] - (A[1] - A[0]) / 7.0
    return m, a, np.array(margin)


def dl_frontend(x, fft, n_rb, n_ant, sf, cell, forced=()):
    """The model of one unit.  x: complex samples from the unit's start (at least window_start(fft, 15) + fft of them)."""
    res = Result()
    res.symb = symbol_rows(x, fft, n_rb)
    res.mag, res.ang, res.margin_f, res.margin_t = [], [], [], []
    res.ce = np.zeros((n_ant, 14, 12 * n_rb), np.complex128)
    for p in range(n_ant):
        M, A, mf = freq_rows(res.symb, sf, cell, n_rb, p, forced)
        m, a, mt = time_interp(M, A, p)
        res.ce[p] = m * np.exp(1j * a)
        res.mag.append(M)
        res.ang.append(A)
        res.margin_f.append(mf)
        res.margin_t.append(mt)
    res.margin = min(min(float(v.min()) for v in res.margin_f), min(float(v.min()) for v in res.margin_t))
    return res
