"""float64 numpy restatement of the 3GPP PUSCH plans' MMSE equalisation (include/mi_lte.h, "PUSCH, 3GPP mode: MMSE equalisation"), built on
pusch_rxdiv_model: every function takes a list of n_rx units' planes (antenna 0 first; a list of one is the single-antenna receiver).

  core       mmse(): from the combiner's numerator, P and s2 to z = num q, nu_s = s2 mean_i q, w_s = (1 - nu_s) / nu_s and the rho tap s2 w_s,
             q = 1 / (P + s2); zf(): the zero-forcing counterpart (z = num / P, rho_s = M / sum 1 / P) the consequences are stated against.
  tolerance  numerator(), taps(): the core on pusch_rxdiv_model's h_polar, power and sigma2, and numpy's FFT as the transform pre-decoder.
  exact      demap(): the de-mapper on tapped symbols and tapped nu_s -- t = u / nu_s, w = (1 - nu_s) / nu_s, both 0 where nu_s is not
             finite or outside (0, 1), demap_llr_model's llr_axis and soft_byte, g = (float)scale.
  float32    combined_f32(), predecode_f32(): pusch_rxdiv_model's float32 restatement of the estimate and the combiner with the kernel's
             q = 1.0f / (P + s2) in place of 1 / P, and pusch_predecode_cases' float32 transform behind it (float32_floor, gates).
  launch     launch(): the MMSE launch -- the noise-on launch of the same n_rx under its own family and label.
  cases      case(): pusch_rxdiv_model.case's planes with every antenna's channel multiplied by 1 + a exp(i phi_r) exp(-2 pi i k d / N);
             flat_case(): planes whose |h| is one constant on every sub-carrier, slot and antenna (the phases stay random, so sigma2 does
             not vanish): P is the same everywhere and MMSE has to give zero forcing's bytes.  GPU_SIZES: the case table.

No kernel result enters anything here."""
import functools

import numpy as np

import demap_llr_model as dm
import pusch_llr_model as pm
import pusch_predecode_cases as pc
import pusch_rxdiv_model as rxm

N_FFT = 2048
# the GPU tests' sizes per n_rx (test_pusch_mmse_gpu): a partial wavefront, the 192 / 256 width step, every S_par step, the radix-47 pass,
# the largest; for four antennas the same widths and early steps and the LDS-forced S_par steps.  A plan takes N_prb divisible by 2, 3 or
# 5 only, so the steps 17 | 18 and 71 | 72 (four antennas: 70 | 71) are held from the planned sizes next to them, 16 | 18 and 70 | 72.
GPU_SIZES = {1: (1, 8, 9, 16, 18, 35, 36, 70, 72, 94, 99), 2: (1, 8, 9, 16, 18, 35, 36, 70, 72, 94, 99),
             4: (1, 8, 9, 16, 18, 35, 36, 65, 66, 70, 72, 76)}
MODS = (1, 2, 3)  # QPSK / 16QAM / 64QAM: size number i of a row runs with MODS[i % 3]; four antennas from 65 PRB on with 64QAM


def gpu_keys(n_rx):
    """((n_prb, n_rx, seed, mod), ..) of the GPU tests' two-path cases (the LDS-forced S_par steps 65 | 66 and 70 | 71 and the last size
    admitted, 76, are those of a 64QAM allocation's scrambling words)"""
    return tuple((n, n_rx, 5, 3 if n_rx == 4 and n >= 65 else MODS[i % 3]) for i, n in enumerate(GPU_SIZES[n_rx]))


# ---- the core

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


def zf(num, P):
    """(z, rho [12]) of the zero-forcing receiver on the same numerator and P"""
    with np.errstate(all="ignore"):
        return num / P, P.shape[1] / (1.0 / P).sum(1)


def predecode(z):
    """the transform pre-decoder of 36.211 5.3.3: the unnormalised backward DFT times 1 / sqrt(M)"""
    return np.fft.ifft(z, axis=1) * np.sqrt(z.shape[1])


def tw(x, nu, w):
    """(t, w) of every symbol as the de-mapper takes them: t = x / nu_s (complex: both axes), 0 where w_s = 0"""
    ok = w > 0
    with np.errstate(all="ignore"):
        return np.where(ok[:, None], x / np.where(ok, nu, 1.0)[:, None], 0.0), w


# ---- the tolerance layer

def numerator(planes, al, dmrs, h=None):
    """complex128 [12, M]: sum_r y_r(s)[i] conj(h_r(s)[i]), r ascending"""
    h = rxm.h_polar(planes, al, dmrs) if h is None else h
    num = np.zeros(h.shape[1:], np.complex128)
    for r, p in enumerate(planes):
        p = np.asarray(p, np.float64)
        for s, L in enumerate(pm.data_rows()):
            sc = pm.subcarriers(al, s // 6)
            num[s] = num[s] + (p[0, L, sc] + 1j * p[1, L, sc]) * np.conj(h[r, s])
    return num


def taps(planes, al, dmrs):
    """{x [12, M], nu, w, rho (the tap s2 w), s2, rho_zf, x_zf}: what an MMSE run reports, and the zero-forcing run's on the same planes"""
    h = rxm.h_polar(planes, al, dmrs)
    num, P, s2 = numerator(planes, al, dmrs, h), rxm.power(h), rxm.sigma2(planes, al, dmrs)
    z, nu, w, rho = mmse(num, P, s2)
    z0, rho0 = zf(num, P)
    return {"x": predecode(z), "nu": nu, "w": w, "rho": rho, "s2": s2, "rho_zf": rho0, "x_zf": predecode(z0), "P": P}


# ---- the exact layer

def demap(xs, nu, mod, c_init, scale):
    """xs: complex64 [12, M] tapped symbols; nu: float32 [12] tapped; scale: the noise setter's.  pusch_llr_model.Demapped."""
    xs = np.asarray(xs)
    M, q = xs.shape[1], pm.QM[mod]
    nu = np.asarray(nu, np.float32).astype(np.float64)
    ok = np.isfinite(nu) & (nu > 0) & (nu < 1)
    nus = np.where(ok, nu, 1.0)
    w = (np.where(ok, (1.0 - nus) / nus, 0.0))[:, None] * np.ones((1, M))
    xr, xi = xs.real.astype(np.float32).astype(np.float64), xs.imag.astype(np.float32).astype(np.float64)
    g = float(np.float32(scale))
    L = np.zeros((12, M, q))
    with np.errstate(all="ignore"):
        tr, ti = np.where(ok[:, None], xr / nus[:, None], 0.0), np.where(ok[:, None], xi / nus[:, None], 0.0)
        L[:, :, 0::2] = np.stack(dm.llr_axis(tr, w, mod), 2)
        L[:, :, 1::2] = np.stack(dm.llr_axis(ti, w, mod), 2)
        x = g * L
    c = dm.gold(c_init & 0x7FFFFFFF, 12 * M * q).reshape(12, M, q)
    x = np.where(c == 1, -x, x)
    x = np.ascontiguousarray(x.transpose(1, 0, 2)).reshape(-1)
    return pm.Demapped(dm.soft_byte(x), x, g)


# ---- the float32 restatement of the estimate and the equaliser

_f32 = pc._f32


def combined_f32(planes, al, dmrs):
    """(re, im) float32 [12, M]: z by the kernel's float operations in the kernel's order -- pusch_rxdiv_model.combined_f32 with
    q = 1.0f / (P + s2), s2 the float of the float64 noise estimate (the kernel sums it in double)"""
    M = 12 * al.N_prb
    steps = [-3, -2, -1, 1, 2, 3]
    s2 = np.float32(rxm.sigma2(planes, al, dmrs))
    c_re, c_im, P = np.zeros((12, M), np.float32), np.zeros((12, M), np.float32), np.zeros((12, M), np.float32)
    for p in planes:
        p = _f32(p)
        mag, u, ang = [], [], []
        for b, L in ((0, 3), (1, 10)):
            sc = pm.subcarriers(al, b)
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
        f2 = pc._cmul32(f1[0], f1[1], f1[0], f1[1])
        f3 = pc._cmul32(f2[0], f2[1], f1[0], f1[1])
        for s, L in enumerate(pm.data_rows()):
            b = s // 6
            sc = pm.subcarriers(al, b)
            h_re, h_im = rxm._slot_h32(mag[b], f_mag, u[b], (f1, f2, f3), steps[s % 6])
            zr, zi = p[0, L, sc], p[1, L, sc]
            c_re[s] = _f32(c_re[s] + _f32(_f32(zr * h_re) + _f32(zi * h_im)))
            c_im[s] = _f32(c_im[s] + _f32(_f32(zi * h_re) - _f32(zr * h_im)))
            P[s] = _f32(P[s] + _f32(_f32(h_re * h_re) + _f32(h_im * h_im)))
    with np.errstate(all="ignore"):
        q = _f32(np.float32(1) / _f32(P + s2))
        return _f32(c_re * q), _f32(c_im * q)


def predecode_f32(planes, al, dmrs):
    re, im = combined_f32(planes, al, dmrs)
    return pc.predecode_f32(re.astype(np.float64) + 1j * im.astype(np.float64), al.N_prb)


# ---- the launch

def launch(n_rx, M_max, W, limit=rxm.LDS_LIMIT, override=0):
    """(fits, family, threads, S_par, lds_off, lds_bytes, label) of an MMSE run: the noise-on launch of the same n_rx -- k_pusch_demod_llr's
    for one antenna (pusch_predecode_cases.s_par and threads, a validated MI_LTE_PUSCH_THREADS), k_pusch_demod_llr_rx's for two and four
    (pusch_rxdiv_model.s_par stepped to the limit, its own width) -- under the family llr_mmse"""
    if n_rx <= 1:
        S, T = pc.s_par(M_max), override or pc.threads(M_max)
    else:
        S, T = rxm.s_par(n_rx, M_max, W, limit), rxm.threads(M_max)
    total = rxm.lds_bytes(max(n_rx, 1), M_max, W, S or 1)
    return (1 if S else 0, "llr_mmse", T, S, total - rxm.LLR_BLOCK_BYTES, total, "k_pusch_demod_llr_mmse")


# ---- cases

def two_path(planes, al, a, d, phis):
    """planes [n_rx] with every row of antenna r multiplied, on grid sub-carrier k, by 1 + a exp(i phi_r) exp(-2 pi i k d / N)"""
    k = np.arange(pm.N_SC)
    out = []
    for p, phi in zip(planes, phis):
        f = 1.0 + a * np.exp(1j * phi) * np.exp(-2j * np.pi * k * d / N_FFT)
        g = (np.asarray(p[0], np.float64) + 1j * np.asarray(p[1], np.float64)) * f[None, :]
        q = np.zeros_like(p)
        q[0], q[1] = g.real, g.imag
        out.append(q)
    return out


class Case:
    """as pusch_rxdiv_model.Case, and .a, .d, .phis of the second path"""


@functools.lru_cache(maxsize=None)
def case(n_prb, n_rx, seed=0, mod=1, a=0.5, d=37):
    """(cached and shared: read-only) pusch_rxdiv_model.case(n_prb, n_rx, seed, mod) through a second path of relative amplitude a, d samples
    late (of 2048: a ripple period of 2048 / d sub-carriers, several periods inside a wide allocation) and a phase per antenna"""
    b = rxm.case(n_prb, n_rx, seed, mod)
    c = Case()
    c.__dict__.update(b.__dict__)
    c.a, c.d = a, d
    c.phis = np.random.default_rng([77, seed, n_prb, n_rx]).uniform(-np.pi, np.pi, n_rx)
    c.planes = two_path(b.planes, b.al, a, d, c.phis)
    return c


@functools.lru_cache(maxsize=None)
def flat_case(n_prb, n_rx, seed=0, mod=1, mag=1.0):
    """(cached and shared: read-only) the allocation, DMRS and noise rows of pusch_rxdiv_model.case with DMRS rows whose channel has the
    one magnitude `mag` on every sub-carrier, slot and antenna and pusch_predecode_cases.build_planes' random phases: P_s[i] = n_rx mag^2
    up to the float roundings, while the second differences of the phases keep sigma2 near mag^2"""
    b = rxm.case(n_prb, n_rx, seed, mod)
    c = Case()
    c.__dict__.update(b.__dict__)
    c.planes = []
    for r in range(n_rx):
        rng = np.random.default_rng([78, seed, n_prb, r])
        p = np.array(b.planes[r])
        ang0 = rng.uniform(-np.pi, np.pi, c.M)
        ang = [ang0, ang0 + rng.uniform(-2.5, 2.5, c.M)]
        for s, L in ((0, 3), (1, 10)):
            g = mag * np.exp(1j * ang[s]) * (b.dmrs[2 * s].astype(np.float64) + 1j * b.dmrs[2 * s + 1].astype(np.float64))
            sc = pm.subcarriers(b.al, s)
            p[0, L, sc], p[1, L, sc] = g.real, g.imag
        c.planes.append(p)
    return c


@functools.lru_cache(maxsize=None)
def expected(key, flat=False):
    """taps() of case(*key) or flat_case(*key) (cached and shared: read-only)"""
    c = flat_case(*key) if flat else case(*key)
    t = taps(c.planes, c.al, c.dmrs)
    for v in t.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return t


@functools.lru_cache(maxsize=None)
def float32_floor(keys):
    """(worst rel-L2, worst elementwise error / RMS) of predecode_f32 against the float64 model over the two-path cases `keys`"""
    l2w = elw = 0.0
    for k in keys:
        c = case(*k)
        l2, el = pc.errors(predecode_f32(c.planes, c.al, c.dmrs), expected(k)["x"])
        l2w, elw = max(l2w, float(l2.max())), max(elw, float(el.max()))
    return l2w, elw


def gates(keys):
    """(rel-L2 gate, elementwise gate): pusch_predecode_cases.GATE_FACTOR x float32_floor(keys), capped at the hard gates"""
    l2, el = float32_floor(tuple(keys))
    return min(pc.GATE_FACTOR * l2, pc.TOL_SYMB), min(pc.GATE_FACTOR * el, 10 * pc.TOL_SYMB)
