"""float64 numpy restatement of the 3GPP PUSCH plans' receive-antenna combining (include/mi_lte.h, "PUSCH, 3GPP mode: receive-antenna
combining"), built on pusch_llr_model and pusch_noise_model: every function takes a list of n_rx units' planes (float32 [2, 16, 1200] each,
antenna 0 first) where its single-antenna counterpart takes one, and equals that counterpart for a list of one.  Layers:

  tolerance  h_polar(), combined(), equalise_predecode(), rho(), sigma2(): the per-antenna polar estimates, the maximum-ratio combined
             symbol z = (sum_r y_r conj(h_r)) / sum_r |h_r|^2, the transform pre-decoder as numpy's FFT, rho_s = M / sum_i 1 / P_s[i] and
             sigma2 = (sum_r S_r) / (120 N_prb n_rx).
  exact      pusch_llr_model.demap as it stands: nothing after the tapped symbols, the tapped rho and the gain knows about antennas.
  float32    combined_f32(): the kernel's own float operations on the estimate and the combiner (uplink.hip: the DMRS phase, slot_h, the
             equaliser item), one rounding per operation; with pusch_predecode_cases.predecode_f32 behind it, what a float32 receiver of
             this structure costs against the float64 model -- the figure the GPU tests' tight gate is a multiple of (float32_floor).
  launch     s_par(), lds_bytes(), threads(): Python restatements of the host code that shapes the combining launch.
  cases      case(): well-conditioned planes per antenna from pusch_predecode_cases.build_planes with independent generators.

No kernel result enters anything here."""
import functools

import numpy as np

import pusch_llr_model as pm
import pusch_noise_model as nm
import pusch_predecode_cases as pc

LLR_BLOCK_BYTES = 464    # wsum[4][12] (double) | rho[12] (float) | nsum[4] (double) behind the scrambling words
LDS_LIMIT = 160 * 1024   # the MI355X's per-workgroup LDS (the library queries the device)


# ---- the float64 model

def h_polar(planes, al, dmrs):
    """complex128 [n_rx, 12, M]: pusch_llr_model.h_polar of every antenna"""
    return np.stack([pm.h_polar(p, al, dmrs) for p in planes])


def power(h):
    """float64 [12, M]: P_s[i] = sum_r (Re h_r^2 + Im h_r^2), r ascending"""
    P = h[0].real * h[0].real + h[0].imag * h[0].imag
    for hr in h[1:]:
        P = P + (hr.real * hr.real + hr.imag * hr.imag)
    return P


def combined(planes, al, dmrs):
    """complex128 [12, M]: z_s[i] = (sum_r y_r(s)[i] conj(h_r(s)[i])) / P_s[i] on the allocation's sub-carriers (the header's (1 / P) factor
    as a division: in float64 the two differ by an ulp, and a list of one antenna then is pusch_llr_model.equalised to the last bit)"""
    h = h_polar(planes, al, dmrs)
    num = np.zeros(h.shape[1:], np.complex128)
    for r, p in enumerate(planes):
        p = np.asarray(p, np.float64)
        for s, L in enumerate(pm.data_rows()):
            sc = pm.subcarriers(al, s // 6)
            num[s] = num[s] + (p[0, L, sc] + 1j * p[1, L, sc]) * np.conj(h[r, s])
    with np.errstate(all="ignore"):
        return num / power(h)


def equalise_predecode(planes, al, dmrs):
    """complex128 [12, M]: what k_pusch_demod_llr_rx taps -- the combined symbols through the unnormalised backward DFT times 1 / sqrt(M)"""
    z = combined(planes, al, dmrs)
    return np.fft.ifft(z, axis=1) * np.sqrt(z.shape[1])


def rho(planes, al, dmrs):
    """(rho [12], smallest P per symbol [12], mean P of the allocation): pusch_llr_model.rho_of with P in place of |h|^2"""
    P = power(h_polar(planes, al, dmrs))
    with np.errstate(all="ignore"):
        tot = (1.0 / P).sum(1)
        r = P.shape[1] / tot
        r = np.where(np.isfinite(tot) & np.isfinite(r) & np.isfinite(r.astype(np.float32)), r, 0.0)
    return r, P.min(1), P.mean()


def sigma2_t(ts):
    """(sum_r S_r) / (120 N_prb n_rx) from the antennas' least-squares products ts[r] (complex [2, M]), S_r the second-difference sum of
    pusch_noise_model on antenna r"""
    S, n_prb = 0.0, np.asarray(ts[0]).shape[1] // 12
    for t in ts:
        d = nm.second_differences(t)
        S = S + (d.real * d.real + d.imag * d.imag).sum()
    return float(S / (120.0 * n_prb * len(ts)))


def sigma2(planes, al, dmrs):
    return sigma2_t([nm.t_ls(p, al, dmrs) for p in planes])


# ---- the float32 restatement of the estimate and the combiner

_f32 = pc._f32


def _slot_h32(mag, f_mag, u, f, n):
    """slot_h: cm = mag + n f_mag, ph = u f^n (f^-n = conj f^n), h = cm ph; every product and sum rounded to float32"""
    fr, fi = f[abs(n) - 1]
    if n < 0:
        fi = -fi
    cm = _f32(mag + _f32(np.float32(n) * f_mag))
    pr, pi = pc._cmul32(u[0], u[1], fr, fi)
    return _f32(cm * pr), _f32(cm * pi)


def combined_f32(planes, al, dmrs):
    """(re, im) float32 [12, M]: the combined symbols by the kernel's float operations in the kernel's order.  numpy's float32 sqrt and
    division are correctly rounded as the device's are; arctan2, cos and sin are numpy's in float64 rounded to float32 where the device's
    float functions are a few ulp off that."""
    M = 12 * al.N_prb
    steps = [-3, -2, -1, 1, 2, 3]
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
            h_re, h_im = _slot_h32(mag[b], f_mag, u[b], (f1, f2, f3), steps[s % 6])
            zr, zi = p[0, L, sc], p[1, L, sc]
            c_re[s] = _f32(c_re[s] + _f32(_f32(zr * h_re) + _f32(zi * h_im)))
            c_im[s] = _f32(c_im[s] + _f32(_f32(zi * h_re) - _f32(zr * h_im)))
            P[s] = _f32(P[s] + _f32(_f32(h_re * h_re) + _f32(h_im * h_im)))
    with np.errstate(all="ignore"):
        hn = _f32(np.float32(1) / P)
        return _f32(c_re * hn), _f32(c_im * hn)


def predecode_f32(planes, al, dmrs):
    """complex128 [12, M]: combined_f32 through pusch_predecode_cases' float32 Stockham transform and the (float)(1 / sqrt(M)) scale"""
    re, im = combined_f32(planes, al, dmrs)
    return pc.predecode_f32(re.astype(np.float64) + 1j * im.astype(np.float64), al.N_prb)


# ---- the launch

def words(n_prb, q_m):
    """scrambling words the launch keeps for an allocation: ceil(12 M Q_m / 32) + 2"""
    return (144 * n_prb * q_m + 31) // 32 + 2


def lds_bytes(n_rx, M_max, W, S):
    """dynamic LDS of the launch: n_rx sets of nine estimate rows, the twiddles, two ping-pong buffers of S symbols, W scrambling words,
    rounded up to 8, and the LLR block.  At n_rx = 1 the noise-referenced single-antenna launch's."""
    return (36 * n_rx * M_max + 8 * M_max * (1 + 2 * S) + 4 * W + 7) // 8 * 8 + LLR_BLOCK_BYTES


def s_par(n_rx, M_max, W, limit=LDS_LIMIT):
    """data symbols a combining workgroup transforms side by side: pusch_predecode_cases.s_par's value, stepped further down 12, 6, 3, 2, 1
    until the whole launch fits the device's per-workgroup LDS; 0: it does not fit, and the setter refuses"""
    S = pc.s_par(M_max)
    while lds_bytes(n_rx, M_max, W, S) > limit:
        if S == 1:
            return 0
        S = 6 if S == 12 else 3 if S == 6 else S - 1
    return S


def threads(M_max):
    """the combining launch's width: the run function's own choice, whatever MI_LTE_PUSCH_THREADS says"""
    return pc.threads(M_max)


# ---- cases

class Case:
    """One allocation on a unit of its own with n_rx antennas: .n_prb, .M, .sf, .al, .dmrs float32 [4, M], .planes [n_rx] of float32
    [2, 16, 1200], .c_init"""


def gapped_runs(n_prb):
    """PRB lists with a gap, other in slot 1 than in slot 0: the first half of the allocation from PRB p, the rest from p + half + gap"""
    half = (n_prb + 1) // 2
    room = pc.N_RB - n_prb
    out = []
    for start, gap in ((1 + n_prb % 3, 2 + n_prb % 4), (n_prb % 2, 1 + n_prb % 3)):
        gap = min(gap, room)
        start = min(start, room - gap)
        out.append(list(range(start, start + half)) + list(range(start + half + gap, start + gap + n_prb)))
    return out


@functools.lru_cache(maxsize=None)
def case(n_prb, n_rx, seed=0, mod=1):
    """(cached and shared: read-only) n_prb PRB of modulation mod at I_TBS 0 on gapped PRB lists (contiguous where the carrier has no room),
    antenna r's planes from pusch_predecode_cases.build_planes with a generator of its own"""
    import openlte_amd as m
    from test_dlsch3gpp_cpu import tbs_table
    c = Case()
    c.n_prb, c.M, c.sf, c.seed, c.n_rx = n_prb, 12 * n_prb, (n_prb + seed) % 10, seed, n_rx
    p0, p1 = gapped_runs(n_prb)
    c.al = m.make_alloc(0, mod, int(tbs_table()[0][n_prb - 1]), p0, 0x200 + n_prb, prbs_slot1=p1)
    c.dmrs = m.ul_dmrs_pusch(m.UlCfg(*pc.ULC), pc.CELL, c.sf, n_prb)
    c.planes = [pc.build_planes(np.random.default_rng([seed, n_prb, r]), c.al, c.dmrs) for r in range(n_rx)]
    c.c_init = (c.al.rnti << 14) | (c.sf << 9) | pc.CELL
    return c


@functools.lru_cache(maxsize=None)
def expected(n_prb, n_rx, seed=0, mod=1):
    c = case(n_prb, n_rx, seed, mod)
    x = equalise_predecode(c.planes, c.al, c.dmrs)
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def float32_floor(keys):
    """(worst rel-L2, worst elementwise error / RMS) of predecode_f32 against the float64 model over the cases keys = ((n_prb, n_rx, seed,
    mod), ..)"""
    l2w = elw = 0.0
    for k in keys:
        c = case(*k)
        l2, el = pc.errors(predecode_f32(c.planes, c.al, c.dmrs), expected(*k))
        l2w, elw = max(l2w, float(l2.max())), max(elw, float(el.max()))
    return l2w, elw


def gates(keys):
    """(rel-L2 gate, elementwise gate): pusch_predecode_cases.GATE_FACTOR x float32_floor(keys), capped at the hard gates TOL_SYMB and
    10 TOL_SYMB"""
    l2, el = float32_floor(tuple(keys))
    return min(pc.GATE_FACTOR * l2, pc.TOL_SYMB), min(pc.GATE_FACTOR * el, 10 * pc.TOL_SYMB)
