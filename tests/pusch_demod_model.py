"""float64 numpy model of the 3GPP PUSCH plans' demodulator k_pusch_demod as include/mi_lte.h states it ("PUSCH, 3GPP mode: max-log
soft-decision demapping", "DMRS noise estimate and the noise-referenced gain", "receive-antenna combining", "MMSE equalisation"), built
on demap_llr_model's llr_axis / soft_byte / in_guard / gold and arranged as the kernel's argument blocks are: the receiver is written once,
for a list of n_rx units' planes (float32 [2, 16, 1200] each, antenna 0 first), and one antenna is a list of one -- a bare unit's planes
stands for that list wherever `planes` is taken.  Layers, and which of them the tests hold the kernel to exactly:

  tolerance  h_polar(): from the subframe planes and mi_lte_ul_dmrs_pusch, the demodulator's polar interpolation between the two DMRS
             estimates (uplink.hip, "DMRS estimates and their interpolation slopes") restated in float64; power(), numerator(): P_s[i] =
             sum_r |h_r|^2 and sum_r y_r conj(h_r); sigma2(): (sum_r S_r) / (120 N_prb n_rx), S_r the sum over both slots and the ten
             interior sub-carriers of every resource block of |t[i-1] - 2 t[i] + t[i+1]|^2, t_b[i] = y_b conj(r_b) (t_ls);
             zf(): z = num / P, rho_s = M / sum_i 1 / P_s[i]; mmse(): z = num q, nu_s = s2 mean_i q, w_s = (1 - nu_s) / nu_s and the rho
             tap s2 w_s, q = 1 / (P + s2); predecode(): the transform pre-decoder as numpy's float64 inverse FFT; taps(): all of it on one
             case.  combined / equalised / equalise_predecode / rho / rho_of name what the zero-forcing tests read of it.
  exact      demap(), demap_mmse(): from the tapped symbols, the tapped rho_s or nu_s and the gain to the descrambled bytes at
             (k 12 + s) Q_m + q -- the kernel runs the same double operations in the same order, so the bytes agree outside the 2^-16
             guard band; nothing after the taps knows about antennas.  gain(), auto_gain(): the float the kernel forms, exactly.
  float32    combined_f32(): the kernel's own float operations on the estimate and the equaliser (uplink.hip: the DMRS phase, slot_h, the
             equaliser item), one rounding per operation; stockham_f32() / predecode_f32(): the transform on the kernel's radix plan; with
             predecode_planes_f32 over both, what a float32 receiver of this structure costs against the float64 model -- the figure the
             GPU tests' tight gate is a multiple of (pusch_demod_cases.float32_floor).
  launch     launch(): pusch_launch_plan (openlte_amd/csrc/pusch_launch.h) restated for its five families, from s_par / rx_s_par,
             threads and lds_bytes, by which the GPU tests choose their sizes; test_pusch_launch_cpu holds it against the C++ rule.

No kernel result enters anything here."""
import numpy as np

import demap_llr_model as dm

N_SC = 1200
QM = dm.QM


# ---- geometry

def data_rows():
    """subframe row (OFDM symbol 0 .. 13) of data symbol s = 0 .. 11: the DMRS symbols 3 and 10 skipped"""
    return [L for L in range(14) if L not in (3, 10)]


def steps():
    """n of data symbol s: its distance from its slot's DMRS symbol, -3 .. -1, +1 .. +3"""
    return np.array([-3, -2, -1, 1, 2, 3] * 2, np.float64)


def subcarriers(al, b):
    """the allocation's M sub-carrier indices in slot b"""
    return np.concatenate([al.prb[b][i] * 12 + np.arange(12) for i in range(al.N_prb)])


def antennas(planes):
    """the list of antennas' planes: `planes` itself, or the list of one that a bare unit's float32 [2, 16, 1200] stands for"""
    return [planes] if np.ndim(planes) == 3 else list(planes)


# ---- the estimate (tolerance)

def t_ls(planes, al, dmrs):
    """complex128 [2, M]: t_b[i] = y_b conj(r_b) on DMRS symbol b (rows 3 and 10) of the allocation's sub-carriers.  planes: one unit's;
    dmrs: float32 [4, M] (ul_dmrs_pusch)"""
    p = np.asarray(planes, np.float64)
    t = []
    for b, L in ((0, 3), (1, 10)):
        sc = subcarriers(al, b)
        y = p[0, L, sc] + 1j * p[1, L, sc]
        r = np.asarray(dmrs[2 * b], np.float64) + 1j * np.asarray(dmrs[2 * b + 1], np.float64)
        t.append(y * np.conj(r))
    return np.stack(t)


def h_polar(planes, al, dmrs):
    """complex128 [n_rx, 12, M] ([12, M] for a bare unit's planes): the interpolated estimate of every data symbol on every antenna.  Per
    sub-carrier t_b = t_ls on DMRS symbol b, f_mag = (|t_1| - |t_0|) / 7, f_ang = (arg t_1 - arg t_0, wrapped into (-pi, pi)) / 7,
    h(s) = (|t_b| + n f_mag) exp(i (arg t_b + n f_ang)), b the symbol's slot."""
    out = []
    for p in antennas(planes):
        t = t_ls(p, al, dmrs)
        mag, ang = [np.abs(v) for v in t], [np.angle(v) for v in t]
        f_mag = (mag[1] - mag[0]) / 7
        f_ang = ang[1] - ang[0]
        f_ang = np.where(f_ang >= np.pi, f_ang - 2 * np.pi, np.where(f_ang <= -np.pi, f_ang + 2 * np.pi, f_ang)) / 7
        h = np.zeros((12, 12 * al.N_prb), np.complex128)
        for s, n in enumerate(steps()):
            b = s // 6
            h[s] = (mag[b] + n * f_mag) * np.exp(1j * (ang[b] + n * f_ang))
        out.append(h)
    return out[0] if np.ndim(planes) == 3 else np.stack(out)


def power(h):
    """float64 [12, M]: P_s[i] = sum_r (Re h_r^2 + Im h_r^2), r ascending"""
    P = h[0].real * h[0].real + h[0].imag * h[0].imag
    for hr in h[1:]:
        P = P + (hr.real * hr.real + hr.imag * hr.imag)
    return P


def numerator(planes, al, dmrs, h=None):
    """complex128 [12, M]: sum_r y_r(s)[i] conj(h_r(s)[i]), r ascending, y_r(s) the subframe row data_rows()[s] of antenna r on the
    allocation's sub-carriers of the symbol's slot"""
    planes = antennas(planes)
    h = h_polar(planes, al, dmrs) if h is None else h
    num = np.zeros(h.shape[1:], np.complex128)
    for r, p in enumerate(planes):
        p = np.asarray(p, np.float64)
        for s, L in enumerate(data_rows()):
            sc = subcarriers(al, s // 6)
            num[s] = num[s] + (p[0, L, sc] + 1j * p[1, L, sc]) * np.conj(h[r, s])
    return num


def second_differences(t):
    """complex128 [2, N_prb, 10]: d_b[i] for i = 12 j + 1 .. 12 j + 10 -- never across a resource-block boundary"""
    t = np.asarray(t, np.complex128)
    blk = t.reshape(t.shape[0], -1, 12)
    return blk[:, :, :-2] - 2.0 * blk[:, :, 1:-1] + blk[:, :, 2:]


def sigma2_t(ts):
    """(sum_r S_r) / (120 N_prb n_rx) from the antennas' least-squares products ts[r] (complex [2, M]; a bare [2, M] is the list of one),
    S_r the sum of |second_differences|^2 on antenna r"""
    ts = [ts] if np.ndim(ts) == 2 else ts
    S, n_prb = 0.0, np.asarray(ts[0]).shape[1] // 12
    for t in ts:
        d = second_differences(t)
        S = S + (d.real * d.real + d.imag * d.imag).sum()
    return float(S / (120.0 * n_prb * len(ts)))


def sigma2(planes, al, dmrs):
    return sigma2_t([t_ls(p, al, dmrs) for p in antennas(planes)])


def gain(scale, s2):
    """(float)(scale / (float)sigma2), 0 where sigma2 is 0 or not finite or the quotient leaves the float range.  s2: the float32 estimate
    (the tap).  Returns the float value as a Python float."""
    s2 = np.float32(s2)
    with np.errstate(all="ignore"):
        g = np.float64(np.float32(scale)) / np.float64(s2)
        ok = np.isfinite(s2) and s2 > 0 and np.isfinite(np.float32(g))
        return float(np.float32(g)) if ok else 0.0


# ---- the equalisers (tolerance)

def zf(num, P):
    """(z [12, M], rho [12]) of the zero-forcing receiver from the numerator and P: z = num / P (the header's (1 / P) factor as a division:
    in float64 the two differ by an ulp), rho_s = M / sum_i 1 / P_s[i]"""
    with np.errstate(all="ignore"):
        return num / P, P.shape[1] / (1.0 / P).sum(1)


def mmse(num, P, s2):
    """(z [12, M], nu [12], w [12], rho tap [12]) from the numerator sum_r y_r conj(h_r) [12, M], P [12, M] and s2.  w = 0 where nu is not
    finite or outside (0, 1)."""
    with np.errstate(all="ignore"):
        q = 1.0 / (P + s2)
        z = num * q
        nu = q.sum(1) * s2 / P.shape[1]
        nf = np.asarray(nu, np.float64).astype(np.float32)  # the contract's nu_s is a float: one that rounds to 0 or 1 carries no information
        ok = np.isfinite(nf) & (nf > 0) & (nf < 1)
        w = np.where(ok, (1.0 - nu) / np.where(ok, nu, 1.0), 0.0)
        return z, nu, w, np.where(ok, s2 * w, 0.0)


def predecode(z):
    """the transform pre-decoder of 36.211 5.3.3: the unnormalised backward DFT times 1 / sqrt(M).  numpy's ifft divides by M, hence times
    sqrt(M)."""
    return np.fft.ifft(z, axis=1) * np.sqrt(z.shape[1])


def tw(x, nu, w):
    """(t, w) of every symbol as the MMSE de-mapper takes them: t = x / nu_s (complex: both axes), 0 where w_s = 0"""
    ok = w > 0
    with np.errstate(all="ignore"):
        return np.where(ok[:, None], x / np.where(ok, nu, 1.0)[:, None], 0.0), w


def taps(planes, al, dmrs):
    """{x [12, M], nu, w, rho (the tap s2 w), s2, rho_zf, x_zf, P}: what an MMSE run reports, and the zero-forcing run's on the same planes"""
    h = h_polar(antennas(planes), al, dmrs)
    num, P, s2 = numerator(planes, al, dmrs, h), power(h), sigma2(planes, al, dmrs)
    z, nu, w, rho_tap = mmse(num, P, s2)
    z0, rho0 = zf(num, P)
    return {"x": predecode(z), "nu": nu, "w": w, "rho": rho_tap, "s2": s2, "rho_zf": rho0, "x_zf": predecode(z0), "P": P}


def combined(planes, al, dmrs):
    """complex128 [12, M]: the maximum-ratio combined symbol z_s[i] = (sum_r y_r(s)[i] conj(h_r(s)[i])) / P_s[i]"""
    return zf(numerator(planes, al, dmrs), power(h_polar(antennas(planes), al, dmrs)))[0]


def equalised(planes, al, dmrs):
    """complex128 [12, M]: the one-tap equaliser's output z_s[k] = y_s[k] conj(h_s[k]) / |h_s[k]|^2 of one unit's planes -- combined() of
    one antenna"""
    return combined([planes], al, dmrs)


def equalise_predecode(planes, al, dmrs):
    """complex128 [12, M]: what k_pusch_demod<.., SPEC = true> taps on a zero-forcing run (mi_lte_pusch_plan_set_llr_tap) -- the combined
    symbols through the transform pre-decoder"""
    return predecode(combined(planes, al, dmrs))


def rho_of(h):
    """(rho [12], smallest P per symbol [12], mean P of the allocation) of the estimate h [n_rx, 12, M] or [12, M]: rho_s = M / sum_i 1 /
    P_s[i], 0 where that is not finite"""
    P = power(h if h.ndim == 3 else h[None])
    with np.errstate(all="ignore"):
        tot = (1.0 / P).sum(1)
        r = P.shape[1] / tot
        r = np.where(np.isfinite(tot) & np.isfinite(r) & np.isfinite(r.astype(np.float32)), r, 0.0)
    return r, P.min(1), P.mean()


def rho(planes, al, dmrs):
    return rho_of(h_polar(planes, al, dmrs))


# ---- the de-mappers (exact)

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


def _axes(xs):
    """the tapped symbols' two axes, float32 values as float64 [12, M] each"""
    xs = np.asarray(xs)
    return xs.real.astype(np.float32).astype(np.float64), xs.imag.astype(np.float32).astype(np.float64)


def _demapped(tr, ti, w, g, mod, c_init):
    """Both de-mappers' tail: llr_axis(t, w) on either axis (tr, ti, w: [12, M]), times the gain, descrambled, de-interleaved, rounded"""
    M, q = w.shape[1], QM[mod]
    L = np.zeros((12, M, q))
    with np.errstate(all="ignore"):
        L[:, :, 0::2] = np.stack(dm.llr_axis(tr, w, mod), 2)
        L[:, :, 1::2] = np.stack(dm.llr_axis(ti, w, mod), 2)
        x = g * L
    c = dm.gold(c_init & 0x7FFFFFFF, 12 * M * q).reshape(12, M, q)  # scrambled in transmission order (s, k, q)
    x = np.where(c == 1, -x, x)
    x = np.ascontiguousarray(x.transpose(1, 0, 2)).reshape(-1)      # the channel de-interleaver: byte (k 12 + s) Q_m + q
    return Demapped(dm.soft_byte(x), x, g)


def demap(xs, rho, mod, c_init, gain=0.0, T=16):
    """The zero-forcing de-mapper: axis(w x, w) with w = rho_s.  xs: complex64 [12, M] tapped symbols; rho: float32 [12]; gain 0: automatic
    from rho."""
    xr, xi = _axes(xs)
    g = auto_gain(rho, mod, T) if gain == 0 else float(np.float32(gain))
    w = np.asarray(rho, np.float32).astype(np.float64)[:, None] * np.ones((1, xr.shape[1]))
    with np.errstate(all="ignore"):
        return _demapped(w * xr, w * xi, w, g, mod, c_init)


def demap_mmse(xs, nu, mod, c_init, scale):
    """The MMSE de-mapper: t = x / nu_s, w = (1 - nu_s) / nu_s, both 0 where nu_s is not finite or outside (0, 1); g = (float)scale.
    xs: complex64 [12, M] tapped symbols; nu: float32 [12] tapped; scale: the noise setter's."""
    xr, xi = _axes(xs)
    nu = np.asarray(nu, np.float32).astype(np.float64)
    ok = np.isfinite(nu) & (nu > 0) & (nu < 1)
    nus = np.where(ok, nu, 1.0)
    w = (np.where(ok, (1.0 - nus) / nus, 0.0))[:, None] * np.ones((1, xr.shape[1]))
    with np.errstate(all="ignore"):
        tr, ti = np.where(ok[:, None], xr / nus[:, None], 0.0), np.where(ok[:, None], xi / nus[:, None], 0.0)
    return _demapped(tr, ti, w, float(np.float32(scale)), mod, c_init)


# ---- the float32 restatement: the transform

def _f32(x):
    return np.asarray(x, np.float32)


def _cmul32(ar, ai, br, bi):
    """(a b) with each of the four products and the two sums rounded to float32"""
    return _f32(_f32(ar * br) - _f32(ai * bi)), _f32(_f32(ar * bi) + _f32(ai * br))


def radix_plan(n_prb):
    """[(R, Ns)]: pusch_shapes' passes for M = 12 N_prb in the order they run -- 9, 3, 5, 8, 4, 2 while they divide what is left, then the
    primes from 7 up -- each with Ns, the product of the radices before it"""
    rem, Ns, plan = 12 * n_prb, 1, []
    while rem > 1:
        for R in (9, 3, 5, 8, 4, 2):
            if rem % R == 0:
                break
        else:
            R = 7
            while rem % R:
                R += 2
        plan.append((R, Ns))
        Ns *= R
        rem //= R
    return plan


FIXED_RADICES = (9, 3, 5, 8, 4, 2)  # dft_pass_r<R>; any other radix runs the generic pass (dft_pass)


def stockham_f32(z, n_prb):
    """The backward DFT of every row of z (complex [S, M]) as a float32 Stockham transform on the kernel's radix plan: twiddles and roots of
    unity exp(2 pi i t / M) rounded to complex64, every product and every sum rounded to float32.  A fixed-radix pass multiplies input r by
    the twiddle w^(r k) and sums the R products with the roots exp(2 pi i r q / R) in order (the kernel's butterflies do the same sums in
    fewer operations); the generic pass sums the R products with the one table entry r (k + q Ns) M / (Ns R) mod M, as dft_pass does.
    Returns (re, im) float32 [S, M], unscaled."""
    z = np.asarray(z)
    S, M = z.shape
    t = np.arange(M)
    tw_re, tw_im = _f32(np.cos(2 * np.pi * t / M)), _f32(np.sin(2 * np.pi * t / M))
    xr, xi = _f32(z.real), _f32(z.imag)
    for R, Ns in radix_plan(n_prb):
        nb, tstride = M // R, M // (Ns * R)
        j = np.arange(nb)
        k = j % Ns
        yr, yi = np.zeros((S, M), np.float32), np.zeros((S, M), np.float32)
        vr, vi = [], []
        for r in range(R):
            ar, ai = xr[:, j + r * nb], xi[:, j + r * nb]
            if R in FIXED_RADICES and Ns > 1 and r > 0:
                ar, ai = _cmul32(ar, ai, tw_re[r * k * tstride], tw_im[r * k * tstride])
            vr.append(ar)
            vi.append(ai)
        for q in range(R):
            if R in FIXED_RADICES:
                root = np.exp(2j * np.pi * ((np.arange(R) * q) % R) / R)
                wr, wi = [_f32(v.real) for v in root], [_f32(v.imag) for v in root]
            else:
                idx = (np.arange(R)[:, None] * ((k + q * Ns) * tstride)[None, :]) % M
                wr, wi = tw_re[idx], tw_im[idx]
            sr, si = np.zeros((S, nb), np.float32), np.zeros((S, nb), np.float32)
            for r in range(R):
                if R in FIXED_RADICES and (r == 0 or q == 0):
                    pr, pi = vr[r], vi[r]  # a root of exactly 1: the butterflies add these terms as they are
                else:
                    pr, pi = _cmul32(vr[r], vi[r], wr[r], wi[r])
                sr, si = _f32(sr + pr), _f32(si + pi)
            yr[:, (j - k) * R + k + q * Ns], yi[:, (j - k) * R + k + q * Ns] = sr, si
        xr, xi = yr, yi
    return xr, xi


def predecode_f32(z, n_prb):
    """complex128 [12, M]: stockham_f32 of the equalised values rounded to float32, times (float)(1 / sqrt(M)) in float32"""
    re, im = stockham_f32(z, n_prb)
    scale = np.float32(1.0 / np.sqrt(float(12 * n_prb)))
    return _f32(re * scale).astype(np.float64) + 1j * _f32(im * scale).astype(np.float64)


# ---- the float32 restatement: the estimate and the equaliser

def _slot_h32(mag, f_mag, u, f, n):
    """slot_h: cm = mag + n f_mag, ph = u f^n (f^-n = conj f^n), h = cm ph; every product and sum rounded to float32"""
    fr, fi = f[abs(n) - 1]
    if n < 0:
        fi = -fi
    cm = _f32(mag + _f32(np.float32(n) * f_mag))
    pr, pi = _cmul32(u[0], u[1], fr, fi)
    return _f32(cm * pr), _f32(cm * pi)


def combined_f32(planes, al, dmrs, s2=None):
    """(re, im) float32 [12, M]: the equalised symbols by the kernel's float operations in the kernel's order -- zero forcing's num (1 / P),
    or with s2 (the float of the noise estimate, which the kernel sums in double) MMSE's num q, q = 1.0f / (P + s2).  numpy's float32 sqrt
    and division are correctly rounded as the device's are; arctan2, cos and sin are numpy's in float64 rounded to float32 where the
    device's float functions are a few ulp off that."""
    M = 12 * al.N_prb
    steps = [-3, -2, -1, 1, 2, 3]
    c_re, c_im, P = np.zeros((12, M), np.float32), np.zeros((12, M), np.float32), np.zeros((12, M), np.float32)
    for p in antennas(planes):
        p = _f32(p)
        mag, u, ang = [], [], []
        for b, L in ((0, 3), (1, 10)):
            sc = subcarriers(al, b)
            cr, ci, dr, di = p[0, L, sc], p[1, L, sc], _f32(dmrs[2 * b]), _f32(dmrs[2 * b + 1])
            t_re, t_im = _f32(_f32(cr * dr) + _f32(ci * di)), _f32(_f32(ci * dr) - _f32(cr * di))
            m_ = _f32(np.sqrt(_f32(_f32(t_re * t_re) + _f32(t_im * t_im))))
            with np.errstate(all="ignore"):
                u.append((np.where(m_ > 0, _f32(t_re / m_), np.float32(1)), np.where(m_ > 0, _f32(t_im / m_), np.float32(0))))
            mag.append(m_)
            ang.append(_f32(np.arctan2(t_im.astype(np.float64), t_re.astype(np.float64))))
        f_mag = _f32(_f32(mag[1] - mag[0]) / np.float32(7))
        f_ang = _f32(ang[1] - ang[0]).astype(np.float64)
        f_ang = _f32(np.where(f_ang >= np.pi, f_ang - 2 * np.pi, np.where(f_ang <= -np.pi, f_ang + 2 * np.pi, f_ang)))
        f_ang = _f32(f_ang / np.float32(7)).astype(np.float64)
        f1 = (_f32(np.cos(f_ang)), _f32(np.sin(f_ang)))
        f2 = _cmul32(f1[0], f1[1], f1[0], f1[1])
        f3 = _cmul32(f2[0], f2[1], f1[0], f1[1])
        for s, L in enumerate(data_rows()):
            b = s // 6
            sc = subcarriers(al, b)
            h_re, h_im = _slot_h32(mag[b], f_mag, u[b], (f1, f2, f3), steps[s % 6])
            zr, zi = p[0, L, sc], p[1, L, sc]
            c_re[s] = _f32(c_re[s] + _f32(_f32(zr * h_re) + _f32(zi * h_im)))
            c_im[s] = _f32(c_im[s] + _f32(_f32(zi * h_re) - _f32(zr * h_im)))
            P[s] = _f32(P[s] + _f32(_f32(h_re * h_re) + _f32(h_im * h_im)))
    with np.errstate(all="ignore"):
        if s2 is None:
            hn = _f32(np.float32(1) / P)
            return _f32(c_re * hn), _f32(c_im * hn)
        q = _f32(np.float32(1) / _f32(P + np.float32(s2)))
        return _f32(c_re * q), _f32(c_im * q)


def predecode_planes_f32(planes, al, dmrs, s2=None):
    """complex128 [12, M]: combined_f32 through the float32 Stockham transform and the (float)(1 / sqrt(M)) scale (predecode_f32)"""
    re, im = combined_f32(planes, al, dmrs, s2)
    return predecode_f32(re.astype(np.float64) + 1j * im.astype(np.float64), al.N_prb)


# ---- the launch

LLR_BLOCK_BYTES = 464    # wsum[4][12] (double) | rho[12] (float) | nsum[4] (double) behind the scrambling words
LDS_LIMIT = 160 * 1024   # the MI355X's per-workgroup LDS (the library queries the device)


def words(n_prb, q_m):
    """scrambling words the launch keeps for an allocation: ceil(12 M Q_m / 32) + 2"""
    return (144 * n_prb * q_m + 31) // 32 + 2


def threads(M_max):
    """the workgroup width the run function picks without MI_LTE_PUSCH_THREADS; a combining launch's whatever that says"""
    return 192 if M_max <= 96 else 256


def s_par(M_max):
    """data symbols a workgroup transforms side by side: as many of 12, 6, 3, 2, 1 as keep the two ping-pong buffers (S_par M_max float2 each)
    within 40 KiB"""
    S = 12
    while S > 1 and S * M_max * 2 * 8 > 40 * 1024:
        S = 6 if S == 12 else 3 if S == 6 else S - 1
    return S


def lds_front(n_rx, M_max, W, S):
    """dynamic LDS in front of the LLR block: n_rx sets of nine estimate rows, the twiddles, two ping-pong buffers of S symbols, W
    scrambling words -- all of a plain launch's"""
    return 36 * n_rx * M_max + 8 * M_max * (1 + 2 * S) + 4 * W


def lds_bytes(n_rx, M_max, W, S):
    """dynamic LDS of a noise-referenced or combining launch: lds_front rounded up to 8, and the LLR block"""
    return (lds_front(n_rx, M_max, W, S) + 7) // 8 * 8 + LLR_BLOCK_BYTES


def rx_s_par(n_rx, M_max, W, limit=LDS_LIMIT):
    """data symbols a combining workgroup transforms side by side: s_par's value, stepped further down 12, 6, 3, 2, 1 until the whole
    launch fits the device's per-workgroup LDS; 0: it does not fit, and the setter refuses"""
    S = s_par(M_max)
    while lds_bytes(n_rx, M_max, W, S) > limit:
        if S == 1:
            return 0
        S = 6 if S == 12 else 3 if S == 6 else S - 1
    return S


def launch(n_rx, M_max, W, maxlog, noise, mmse, limit=LDS_LIMIT, override=0):
    """(fits, family, threads, S_par, lds_off, lds_bytes, label): pusch_launch_plan for a plan whose widest allocation has M_max
    sub-carriers and whose longest keeps W scrambling words.  plain: no LLR block.  One antenna (llr, llr_noise): s_par, a validated
    MI_LTE_PUSCH_THREADS or threads, the LLR block 32 bytes shorter without the noise sums.  Two and four (llr_rx): rx_s_par stepped to
    the limit and refused at 0, its own width, the noise launch's block either way.  mmse, read with maxlog and the noise gain on only:
    the noise-on launch of the same n_rx under the family llr_mmse and its label."""
    if not maxlog:
        S = s_par(M_max)
        return 1, "plain", override or threads(M_max), S, 0, lds_front(1, M_max, W, S), "k_pusch_demod"
    if n_rx <= 1:
        S = s_par(M_max)
        total = lds_bytes(1, M_max, W, S)
        out = (1, "llr_noise" if noise else "llr", override or threads(M_max), S, total - LLR_BLOCK_BYTES, total - (0 if noise else 32), "k_pusch_demod_llr")
    else:
        S = rx_s_par(n_rx, M_max, W, limit)
        total = lds_bytes(n_rx, M_max, W, S or 1)
        out = (1 if S else 0, "llr_rx", threads(M_max), S, total - LLR_BLOCK_BYTES, total, "k_pusch_demod_llr_rx")
    return (out[0], "llr_mmse") + out[2:6] + ("k_pusch_demod_llr_mmse",) if mmse and noise else out
