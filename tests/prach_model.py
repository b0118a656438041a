"""A float64 model of the PRACH detector (openlte_amd/csrc/prach.hip: k_prach_fft, k_prach_bins, k_prach_corr and the host verdict), numpy
only: no library, no reference.  model() is the operation itself -- one FFT of the T_fft samples behind the cyclic prefix, the N_zc kept
bins, per root the inverse N_zc-point DFT of X_u conj(x_hat) and its power -- in complex128; verdict() restates the scalar verdict in the
float32 arithmetic and order of prach_verdicts; float32_floor() restates the kernels' own plan (decimation phases, power-of-two Stockham
FFTs, the P-term combination, Bluestein with 2048-point FFTs) in numpy float32, which is what a float32 transform of this structure costs
and so what the GPU tests' tight gates are made from.  No kernel result enters anything here."""
import numpy as np

M32 = 0xFFFFFFFF
BL = 2048  # the Bluestein FFT length

NCS_UNRESTRICTED = (0, 13, 15, 18, 22, 26, 32, 38, 46, 59, 76, 93, 119, 167, 279, 419)  # 36.211 table 5.7.2-2
NCS_RESTRICTED = (15, 18, 22, 26, 32, 38, 46, 55, 68, 82, 100, 128, 158, 202, 237)
NCS_FORMAT4 = (2, 4, 6, 8, 10, 12, 15)                                                   # 36.211 table 5.7.2-3


class Geom:
    """What prach_geom and prach_plan_common derive from (fft, N_rb, format, freq_offset): .N_zc, .T_fft, .T_cp (samples at the cell's rate),
    .start (first kept bin, before the T_fft / 2 shift), .P decimation phases of .N2 points each."""

    def __init__(self, fft, n_rb, fmt, freq_offset):
        sc = 2048 // fft  # 30.72 MHz / fs
        if fmt >= 4:
            self.N_zc, T_fft_30, T_cp_30, K, phi, self.P = 139, 4096, 448, 2, 2, 4
        else:
            self.N_zc, T_fft_30, T_cp_30, K, phi, self.P = 839, 24576, (3168, 21024, 6240, 21024)[fmt], 12, 7, 24
        self.T_fft, self.T_cp = T_fft_30 // sc, T_cp_30 // sc
        k_0 = (freq_offset * 12 - n_rb * 12 // 2 + fft // 2) & M32  # uint32 arithmetic, as the library's
        self.start = (phi + K * k_0 + K // 2) & M32
        self.N2 = self.T_fft // self.P
        assert self.P * self.N2 == self.T_fft and self.N2 & (self.N2 - 1) == 0
        self.occasion_samples = self.T_cp + self.T_fft

    def bin_index(self):
        """idx_b = (b + start + T_fft / 2) mod T_fft of the N_zc kept bins"""
        return (np.arange(self.N_zc, dtype=np.int64) + self.start + self.T_fft // 2) % self.T_fft


def sets(u, zczc, hs, fmt):
    """(N_cs, v_max) of the physical root u, prach_sets restated with its uint32 arithmetic (the verdict uses the first root's for every root)"""
    N = 139 if fmt >= 4 else 839
    N_cs = NCS_FORMAT4[zczc] if fmt >= 4 else NCS_RESTRICTED[zczc] if hs else NCS_UNRESTRICTED[zczc]
    if not hs:
        return N_cs, (0 if N_cs == 0 else N // N_cs - 1)
    p = next(p for p in range(1, N + 1) if (p * u) % N == 1)
    d_u = p if p < N // 2 else N - p

    def as_int32(v):
        v &= M32
        return v - (1 << 32) if v >= 1 << 31 else v

    if N_cs <= d_u < N // 3:
        shift = d_u // N_cs
        d_start = 2 * d_u + shift * N_cs
        group = N // d_start
        neg = max(0, as_int32(((N - 2 * d_u - group * d_start) & M32) // N_cs))
    else:
        shift = ((N - 2 * d_u) & M32) // N_cs
        d_start = (N - 2 * d_u + shift * N_cs) & M32
        group = d_u // d_start
        neg = min(max(0, as_int32(((d_u - group * d_start) & M32) // N_cs)), as_int32(shift))
    return N_cs, (shift * group + neg - 1) & M32


def root_spectra(u_list, N_zc):
    """(re, im) float32 [n_roots, 839], the form mi_lte_prach_plan_create_roots takes (the first N_zc of a row used): the Zadoff-Chu sequence
    x_u(n) = exp(-i pi u n (n + 1) / N_zc) rounded to float32 as the library rounds it, its N_zc-point DFT in float64, rounded to float32"""
    re, im = np.zeros((len(u_list), 839), np.float32), np.zeros((len(u_list), 839), np.float32)
    i = np.arange(N_zc, dtype=np.float64)
    for r, u in enumerate(u_list):
        ph = (((-np.pi * float(u)) * i) * (i + 1.0)) / float(N_zc)  # the library's order of operations
        x = np.cos(ph).astype(np.float32).astype(np.float64) + 1j * np.sin(ph).astype(np.float32).astype(np.float64)
        X = np.fft.fft(x)
        re[r, :N_zc], im[r, :N_zc] = X.real.astype(np.float32), X.imag.astype(np.float32)
    return re, im


def spectra_complex(roots, N_zc):
    """complex128 [n_roots, N_zc] of the (re, im) rows"""
    return roots[0][:, :N_zc].astype(np.float64) + 1j * roots[1][:, :N_zc].astype(np.float64)


def occasions(re, im, occ_start, g):
    """complex128 [n_occ, T_cp + T_fft]: the occasions at occ_start of one sample buffer"""
    ix = np.asarray(occ_start, np.int64)[:, None] + np.arange(g.occasion_samples)[None, :]
    return np.asarray(re, np.float64)[ix] + 1j * np.asarray(im, np.float64)[ix]


def stats_of(power):
    """(sum, max, first arg-max) over the last axis"""
    return power.sum(-1), power.max(-1), power.argmax(-1).astype(np.uint32)


def model(x, g, xu):
    """x complex128 [n_occ, >= T_cp + T_fft], xu complex128 [n_roots, N_zc] -> x_hat complex128 [n_occ, N_zc], power float64
    [n_occ, n_roots, N_zc], (sum, max, first arg-max) each [n_occ, n_roots]"""
    X = np.fft.fft(x[:, g.T_cp:g.T_cp + g.T_fft], axis=1)
    x_hat = X[:, g.bin_index()]
    out = g.N_zc * np.fft.ifft(xu[None, :, :] * np.conj(x_hat)[:, None, :], axis=2)
    power = out.real ** 2 + out.imag ** 2
    return x_hat, power, stats_of(power)


def threshold_ratio(stats, N_zc):
    """max / (50 ave) per occasion in float64, ave as the verdict forms it: the running value plus the root's sum, divided by N_zc after
    every root"""
    s, mx, _ = stats
    ave = np.zeros(s.shape[0])
    for r in range(s.shape[1]):
        ave = (ave + s[:, r]) / N_zc
    top = mx.max(1)
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(ave > 0, top / (50.0 * ave), 0.0)


def verdict(stats, N_cs, v_max, N_zc):
    """uint32 [n_occ, 3] (N_det_pre, det_pre, det_ta): prach_verdicts restated, float32 where it is float, in its order -- the first largest
    root wins, the average is divided after every root, >= 50 * ave, max_val != 0, and the timing advance's (uint32)(int64)(... - 1), which
    wraps to 0xFFFFFFFF at zero delay"""
    f = np.float32
    s, mx, off = (np.asarray(a) for a in stats)
    out = np.zeros((s.shape[0], 3), np.uint32)
    for o in range(s.shape[0]):
        ave, top, top_root, top_off = f(0), f(0), 0, 0
        for r in range(s.shape[1]):
            if f(mx[o, r]) > top:
                top, top_root, top_off = f(mx[o, r]), r, int(off[o, r])
            ave = f(ave + f(s[o, r]))
            ave = f(ave / f(N_zc))
        if top >= f(f(50) * ave) and top != 0:
            if N_cs == 0:
                pre = (top_root * ((v_max + 1) & M32)) & M32
                ta = int(((top_off % N_zc) * 29.155 / 16) - 1) & M32
            else:
                pre = (top_root * ((v_max + 1) & M32) + ((top_off + N_cs) % N_zc) // N_cs) & M32
                ta = int(((((N_cs - ((top_off + N_cs) % N_zc)) & M32) % N_cs) * 29.155 / 16) - 1) & M32
            out[o] = (1, pre, ta)
    return out


# ---- the float32 restatement of the kernels' plan

def _f32(x):
    return np.asarray(x, np.float32)


def _cmul(a, b):
    """cmulf: (a b) with four products and two sums, each rounded to float32; a, b = (re, im)"""
    return _f32(_f32(a[0] * b[0]) - _f32(a[1] * b[1])), _f32(_f32(a[0] * b[1]) + _f32(a[1] * b[0]))


def _tw_table():
    k = np.arange(BL // 2)
    return _f32(np.cos(-2 * np.pi * k / BL)), _f32(np.sin(-2 * np.pi * k / BL))


def fft_pow2_f32(re, im, tw=None):
    """lds_fft_pow2 in numpy float32 over the last axis (N = 2^n <= 2048 points, unnormalised, forward): radix-4 Stockham passes with the
    twiddles w, w^2 read from tw[k] = exp(-2 pi i k / 2048) and w^3 formed as their float32 product, one radix-2 pass when n is odd"""
    tw = tw or _tw_table()
    xr, xi = _f32(re), _f32(im)
    N = xr.shape[-1]
    Ns = 1
    while N // Ns >= 4:
        nb, st = N >> 2, 2048 // (Ns << 2)
        j = np.arange(nb)
        k = j & (Ns - 1)
        a, b, c, d = [(xr[..., j + q * nb], xi[..., j + q * nb]) for q in range(4)]
        if Ns > 1:
            w1, w2 = (tw[0][k * st], tw[1][k * st]), (tw[0][2 * k * st], tw[1][2 * k * st])
            b, c, d = _cmul(b, w1), _cmul(c, w2), _cmul(d, _cmul(w1, w2))
        s02, d02 = (_f32(a[0] + c[0]), _f32(a[1] + c[1])), (_f32(a[0] - c[0]), _f32(a[1] - c[1]))
        s13, d13 = (_f32(b[0] + d[0]), _f32(b[1] + d[1])), (_f32(b[1] - d[1]), _f32(d[0] - b[0]))
        j0 = ((j - k) << 2) + k
        yr, yi = np.empty_like(xr), np.empty_like(xi)
        yr[..., j0], yi[..., j0] = _f32(s02[0] + s13[0]), _f32(s02[1] + s13[1])
        yr[..., j0 + Ns], yi[..., j0 + Ns] = _f32(d02[0] + d13[0]), _f32(d02[1] + d13[1])
        yr[..., j0 + 2 * Ns], yi[..., j0 + 2 * Ns] = _f32(s02[0] - s13[0]), _f32(s02[1] - s13[1])
        yr[..., j0 + 3 * Ns], yi[..., j0 + 3 * Ns] = _f32(d02[0] - d13[0]), _f32(d02[1] - d13[1])
        xr, xi = yr, yi
        Ns <<= 2
    if Ns < N:
        st = 2048 // (Ns << 1)
        j = np.arange(N // 2)
        k = j & (Ns - 1)
        u = (xr[..., j], xi[..., j])
        v = _cmul((xr[..., j + N // 2], xi[..., j + N // 2]), (tw[0][k * st], tw[1][k * st]))
        j0 = ((j - k) << 1) + k
        yr, yi = np.empty_like(xr), np.empty_like(xi)
        yr[..., j0], yi[..., j0] = _f32(u[0] + v[0]), _f32(u[1] + v[1])
        yr[..., j0 + Ns], yi[..., j0 + Ns] = _f32(u[0] - v[0]), _f32(u[1] - v[1])
        xr, xi = yr, yi
    return xr, xi


def bluestein_tables(N_zc):
    """(chirp, bspec) as prach_bluestein_tables builds them: c[n] = exp(+i pi n^2 / N_zc) with n^2 reduced mod 2 N_zc in integers, float32; the
    2048-point spectrum of conj(c) wrapped to both ends (float64 FFT, rounded to float32)"""
    n = np.arange(N_zc, dtype=np.int64)
    ang = np.pi * ((n * n) % (2 * N_zc)).astype(np.float64) / N_zc
    b = np.zeros(BL, np.complex128)
    b[:N_zc] = np.cos(ang) - 1j * np.sin(ang)
    b[BL - n[1:]] = b[n[1:]]
    B = np.fft.fft(b)
    return (_f32(np.cos(ang)), _f32(np.sin(ang))), (_f32(B.real), _f32(B.imag))


def xhat_f32(x, g):
    """k_prach_fft + k_prach_bins in float32: x complex [n_occ, >= T_cp + T_fft] (values exact in float32) -> (re, im) float32 [n_occ, N_zc]"""
    seg = x[:, g.T_cp:g.T_cp + g.T_fft].reshape(x.shape[0], g.N2, g.P).transpose(0, 2, 1)  # [occ, r, i] = x[P i + r]
    Fr, Fi = fft_pow2_f32(seg.real, seg.imag)
    idx = g.bin_index()
    km = idx & (g.N2 - 1)
    ar, ai = np.zeros((x.shape[0], g.N_zc), np.float32), np.zeros((x.shape[0], g.N_zc), np.float32)
    for r in range(g.P):
        t = (r * idx) % g.T_fft
        arg = _f32(_f32(-2.0 * t) / np.float32(g.T_fft)).astype(np.float64)  # sincospif's float argument
        ws, wc = _f32(np.sin(np.pi * arg)), _f32(np.cos(np.pi * arg))
        vx, vy = Fr[:, r, km], Fi[:, r, km]
        ar = _f32(ar + _f32(_f32(vx * wc) - _f32(vy * ws)))
        ai = _f32(ai + _f32(_f32(vx * ws) + _f32(vy * wc)))
    return ar, ai


def power_f32(xh, roots, N_zc):
    """k_prach_corr in float32: xh = (re, im) float32 [n_occ, N_zc], roots = (re, im) float32 rows -> power float32 [n_occ, n_roots, N_zc]"""
    chirp, bspec = bluestein_tables(N_zc)
    ux, uy = _f32(roots[0][:, :N_zc])[None, :, :], _f32(roots[1][:, :N_zc])[None, :, :]
    hx, hy = xh[0][:, None, :], xh[1][:, None, :]
    inn = (_f32(_f32(ux * hx) + _f32(uy * hy)), _f32(_f32(uy * hx) - _f32(ux * hy)))
    v = _cmul(inn, chirp)
    A = (np.zeros(v[0].shape[:2] + (BL,), np.float32), np.zeros(v[0].shape[:2] + (BL,), np.float32))
    A[0][..., :N_zc], A[1][..., :N_zc] = v
    X = fft_pow2_f32(*A)
    Y = (_f32(_f32(X[0] * bspec[0]) - _f32(X[1] * bspec[1])), _f32(-_f32(_f32(X[0] * bspec[1]) + _f32(X[1] * bspec[0]))))
    Z = fft_pow2_f32(*Y)
    z = (_f32(Z[0][..., :N_zc] * np.float32(1.0 / BL)), _f32(-Z[1][..., :N_zc] * np.float32(1.0 / BL)))
    a = _cmul(z, chirp)
    return _f32(_f32(a[0] * a[0]) + _f32(a[1] * a[1]))


def float32_floor(x, g, roots):
    """The detector's own plan in numpy float32 -> x_hat complex128 [n_occ, N_zc] (float32 values), power float32 [n_occ, n_roots, N_zc], (sum,
    max, first arg-max) with the sum taken in float32"""
    xh = xhat_f32(x, g)
    p = power_f32(xh, roots, g.N_zc)
    return xh[0].astype(np.float64) + 1j * xh[1].astype(np.float64), p, (p.sum(-1, dtype=np.float32), p.max(-1), p.argmax(-1).astype(np.uint32))


# ---- error figures

def xhat_errors(got, want):
    """(rel-L2, largest elementwise error over the occasion's RMS), per occasion; an all-zero occasion must be reproduced exactly"""
    d = np.abs(np.asarray(got, np.complex128) - want)
    e = (np.abs(want) ** 2).sum(1)
    zero = e == 0
    safe = np.where(zero, 1.0, e)
    l2, el = np.sqrt((d ** 2).sum(1) / safe), d.max(1) / np.sqrt(safe / want.shape[1])
    bad = zero & (d.max(1) > 0)
    return np.where(bad, np.inf, l2), np.where(bad, np.inf, el)


def power_errors(got, want):
    """(rel-L2, largest elementwise error over the profile's maximum), per (occasion, root); an all-zero profile must be reproduced exactly"""
    d = np.abs(np.asarray(got, np.float64) - want)
    e, top = (want ** 2).sum(-1), want.max(-1)
    zero = top == 0
    l2, el = np.sqrt((d ** 2).sum(-1) / np.where(zero, 1.0, e)), d.max(-1) / np.where(zero, 1.0, top)
    bad = zero & (d.max(-1) > 0)
    return np.where(bad, np.inf, l2), np.where(bad, np.inf, el)


def scalar_errors(got, want):
    """relative error of got against want, 0 where both are exactly 0"""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(want == 0, np.where(got == 0, 0.0, np.inf), np.abs(got - want) / np.where(want == 0, 1.0, np.abs(want)))
