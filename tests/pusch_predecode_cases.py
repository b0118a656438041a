"""Cases for the PUSCH equaliser / transform pre-decoder tests (test_pusch_predecode_cpu.py, test_pusch_predecode_gpu.py): the transform
sizes the 3GPP mode plans, Python restatements of the host code that shapes the launch (pusch_shapes' radix plan, the run function's S_par
and workgroup width), a builder of well-conditioned subframe planes that needs no front end, and a float32 restatement of the transform
whose error against numpy's float64 FFT sets the GPU tests' tight gate.  No kernel result enters anything here."""
import functools

import numpy as np

import pusch_llr_model as pm

N_RB = 100               # the cell of every case: DlCfg(2048, 100, 1, 0)
ULC = (3, 0, 0, 2, 1)    # UlCfg, test_ulsch3gpp_gpu's
CELL = 301
SEEDS = (0, 1)           # the builder's seeds: 0 where a size runs in a plan of its own, 1 where it shares a plan
TOL_SYMB = 1e-5          # the project's FFT-stage figure (test_uplink_gpu / test_frontend_gpu): rel-L2 per symbol; elementwise 10 x
GATE_FACTOR = 8.0        # tight gate = GATE_FACTOR x the float32 restatement's worst error, capped at the hard gate (see float32_floor)


def planned_sizes():
    """the 74 N_prb a 3GPP plan of a 100-RB cell accepts: 1, and every N_prb <= 99 divisible by 2, 3 or 5"""
    return [n for n in range(1, N_RB) if n == 1 or n % 2 == 0 or n % 3 == 0 or n % 5 == 0]


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


def s_par(M_max):
    """data symbols a workgroup transforms side by side: as many of 12, 6, 3, 2, 1 as keep the two ping-pong buffers (S_par M_max float2 each)
    within 40 KiB"""
    S = 12
    while S > 1 and S * M_max * 2 * 8 > 40 * 1024:
        S = 6 if S == 12 else 3 if S == 6 else S - 1
    return S


def threads(M_max):
    """the workgroup width the run function picks without MI_LTE_PUSCH_THREADS"""
    return 192 if M_max <= 96 else 256


class Case:
    """One allocation on a unit of its own: .n_prb, .M, .sf, .al (unit to be set by the plan's builder), .dmrs float32 [4, M], .planes float32
    [2, 16, 1200]"""


def prb_runs(n_prb):
    """the first PRB of the allocation's run in slot 0 and in slot 1: never 0, and different wherever the carrier has room"""
    hi = N_RB - n_prb
    return min(hi, 1 + n_prb % 7), max(1, hi - n_prb % 5)


def build_planes(rng, al, dmrs):
    """One unit's float32 [2, 16, 1200].  Rows 3 and 10 on the allocation's sub-carriers: h_b[k] r_b[k], |h_b[k]| uniform in [0.8, 1.25] per
    sub-carrier and slot, arg h_0[k] uniform in (-pi, pi), arg h_1[k] = arg h_0[k] + delta[k] with |delta| <= 2.5 rad -- so the extrapolated
    magnitude stays >= 0.8 - 3 * 0.45 / 7 and the slot-to-slot phase step stays 0.6 rad inside the +-pi wrap.  Everything else on rows
    0 .. 13: complex normal of unit variance, independent per row and sub-carrier."""
    M = 12 * al.N_prb
    g = (rng.standard_normal((14, pm.N_SC)) + 1j * rng.standard_normal((14, pm.N_SC))) / np.sqrt(2.0)
    ang0 = rng.uniform(-np.pi, np.pi, M)
    ang = [ang0, ang0 + rng.uniform(-2.5, 2.5, M)]
    for b, L in ((0, 3), (1, 10)):
        h = rng.uniform(0.8, 1.25, M) * np.exp(1j * ang[b])
        r = dmrs[2 * b].astype(np.float64) + 1j * dmrs[2 * b + 1].astype(np.float64)
        g[L, pm.subcarriers(al, b)] = h * r
    planes = np.zeros((2, 16, pm.N_SC), np.float32)
    planes[0, :14], planes[1, :14] = g.real, g.imag
    return planes


@functools.lru_cache(maxsize=None)
def case(n_prb, seed=0):
    """the case of one size and builder seed (cached and shared: treat it as read-only): a QPSK grant at I_TBS 0 on PRB runs that start at a
    non-zero PRB, other in slot 1 than in slot 0"""
    import openlte_amd as m
    from test_dlsch3gpp_cpu import tbs_table
    c = Case()
    c.n_prb, c.M, c.sf, c.seed = n_prb, 12 * n_prb, n_prb % 10, seed
    p0, p1 = prb_runs(n_prb)
    c.al = m.make_alloc(0, 1, int(tbs_table()[0][n_prb - 1]), list(range(p0, p0 + n_prb)), 0x100 + n_prb, prbs_slot1=list(range(p1, p1 + n_prb)))
    c.dmrs = m.ul_dmrs_pusch(m.UlCfg(*ULC), CELL, c.sf, n_prb)
    c.planes = build_planes(np.random.default_rng(1000 * seed + n_prb), c.al, c.dmrs)
    return c


@functools.lru_cache(maxsize=None)
def expected(n_prb, seed=0):
    """complex128 [12, M]: the model's equalised, pre-decoded symbols of case(n_prb, seed) (cached and shared: read-only)"""
    c = case(n_prb, seed)
    x = pm.equalise_predecode(c.planes, c.al, c.dmrs)
    x.setflags(write=False)
    return x


def errors(got, want):
    """(rel-L2 per data symbol [12], largest elementwise error over the symbol's RMS [12]) of got against want, both [12, M]"""
    d = np.abs(np.asarray(got, np.complex128) - want)
    rms = np.sqrt((np.abs(want) ** 2).mean(1))
    return np.sqrt((d ** 2).sum(1) / (np.abs(want) ** 2).sum(1)), d.max(1) / rms


# ---- the float32 restatement of the transform

def _f32(x):
    return np.asarray(x, np.float32)


def _cmul32(ar, ai, br, bi):
    """(a b) with each of the four products and the two sums rounded to float32"""
    return _f32(_f32(ar * br) - _f32(ai * bi)), _f32(_f32(ar * bi) + _f32(ai * br))


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


@functools.lru_cache(maxsize=None)
def float32_floor():
    """{(n_prb, seed): (worst rel-L2, worst elementwise error / RMS)} of predecode_f32 against numpy's float64 FFT, both on the model's
    equalised values rounded to float32, for every planned size and builder seed: what a float32 transform of this structure costs on the
    tests' own inputs, with no kernel in the loop."""
    out = {}
    for seed in SEEDS:
        for n in planned_sizes():
            c = case(n, seed)
            z = pm.equalised(c.planes, c.al, c.dmrs)
            z32 = _f32(z.real).astype(np.float64) + 1j * _f32(z.imag).astype(np.float64)
            l2, el = errors(predecode_f32(z32, n), np.fft.ifft(z32, axis=1) * np.sqrt(c.M))
            out[(n, seed)] = (float(l2.max()), float(el.max()))
    return out


def gates():
    """(rel-L2 gate, elementwise gate) of the GPU tests: GATE_FACTOR x the float32 restatement's worst figures over all sizes and seeds, capped
    at the hard gate TOL_SYMB (10 TOL_SYMB elementwise).  Why 8: the kernel's butterflies order their operations differently (radix 9 as
    3 x 3, radix 8 as 2 x 4), its twiddles come from sincospif and its estimate from atan2f / sincosf, a few ulp from correctly rounded, and
    the equaliser adds some ten float roundings per element in front of the transform; each moves a float32 transform's error by a small
    factor, none by an order of magnitude."""
    fl = float32_floor()
    return (min(GATE_FACTOR * max(v[0] for v in fl.values()), TOL_SYMB),
            min(GATE_FACTOR * max(v[1] for v in fl.values()), 10 * TOL_SYMB))
