"""Cases for the tests that hold k_pusch_demod to pusch_demod_model (test_pusch_predecode_*, test_pusch_rxdiv_*, test_pusch_mmse_*): the
transform sizes the 3GPP mode plans, builders of well-conditioned subframe planes that need no front end, the cached expectations of
the float64 model on them, and the GPU tests' gates.  Which layer asserts what:

  cases      case(): one allocation of every planned size on contiguous PRB runs, one antenna (the equaliser / pre-decoder tests);
             rx_case(): n_rx antennas on gapped PRB lists, antenna r's planes from build_planes with a generator of its own;
             two_path_case(): rx_case's planes with every antenna's channel multiplied by 1 + a exp(i phi_r) exp(-2 pi i k d / N);
             flat_case(): planes whose |h| is one constant on every sub-carrier, slot and antenna (the phases stay random, so sigma2 does
             not vanish): P is the same everywhere and MMSE has to give zero forcing's bytes.  GPU_SIZES: the MMSE tests' case table.
  expected   expected(), rx_expected(), mmse_expected(): pusch_demod_model's equalise_predecode / taps on those cases, float64.
  gates      float32_floor(): what pusch_demod_model's float32 restatement costs against the float64 expectation on the tests' own inputs;
             gates(): GATE_FACTOR times its worst figures, capped at the project's hard gates TOL_SYMB and 10 TOL_SYMB.
  views      rx_view, mmse_view: the names the combining and the MMSE test files read under one alias each.

No kernel result enters anything here."""
import copy
import functools
import types

import numpy as np

import pusch_demod_model as pm
from pusch_demod_model import FIXED_RADICES, radix_plan, s_par, stockham_f32, threads  # read by the pre-decoder tests with the cases

N_RB = 100               # the cell of every case: DlCfg(2048, 100, 1, 0)
N_FFT = 2048
ULC = (3, 0, 0, 2, 1)    # UlCfg, test_ulsch3gpp_gpu's
CELL = 301
SEEDS = (0, 1)           # the builder's seeds: 0 where a size runs in a plan of its own, 1 where it shares a plan
TOL_SYMB = 1e-5          # the project's FFT-stage figure (test_uplink_gpu / test_frontend_gpu): rel-L2 per symbol; elementwise 10 x
GATE_FACTOR = 8.0        # tight gate = GATE_FACTOR x the float32 restatement's worst error, capped at the hard gate (see float32_floor)
# the MMSE GPU tests' sizes per n_rx (test_pusch_mmse_gpu): a partial wavefront, the 192 / 256 width step, every S_par step, the radix-47
# pass, the largest; for four antennas the same widths and early steps and the LDS-forced S_par steps.  A plan takes N_prb divisible by 2, 3
# or 5 only, so the steps 17 | 18 and 71 | 72 (four antennas: 70 | 71) are held from the planned sizes next to them, 16 | 18 and 70 | 72.
GPU_SIZES = {1: (1, 8, 9, 16, 18, 35, 36, 70, 72, 94, 99), 2: (1, 8, 9, 16, 18, 35, 36, 70, 72, 94, 99),
             4: (1, 8, 9, 16, 18, 35, 36, 65, 66, 70, 72, 76)}
MODS = (1, 2, 3)  # QPSK / 16QAM / 64QAM: size number i of a row runs with MODS[i % 3]; four antennas from 65 PRB on with 64QAM


# ---- sizes and layouts

def planned_sizes():
    """the 74 N_prb a 3GPP plan of a 100-RB cell accepts: 1, and every N_prb <= 99 divisible by 2, 3 or 5"""
    return [n for n in range(1, N_RB) if n == 1 or n % 2 == 0 or n % 3 == 0 or n % 5 == 0]


def gpu_keys(n_rx):
    """((n_prb, n_rx, seed, mod), ..) of the GPU tests' two-path cases (the LDS-forced S_par steps 65 | 66 and 70 | 71 and the last size
    admitted, 76, are those of a 64QAM allocation's scrambling words)"""
    return tuple((n, n_rx, 5, 3 if n_rx == 4 and n >= 65 else MODS[i % 3]) for i, n in enumerate(GPU_SIZES[n_rx]))


def prb_runs(n_prb):
    """the first PRB of the allocation's run in slot 0 and in slot 1: never 0, and different wherever the carrier has room"""
    hi = N_RB - n_prb
    return min(hi, 1 + n_prb % 7), max(1, hi - n_prb % 5)


def gapped_runs(n_prb):
    """PRB lists with a gap, other in slot 1 than in slot 0: the first half of the allocation from PRB p, the rest from p + half + gap"""
    half = (n_prb + 1) // 2
    room = N_RB - n_prb
    out = []
    for start, gap in ((1 + n_prb % 3, 2 + n_prb % 4), (n_prb % 2, 1 + n_prb % 3)):
        gap = min(gap, room)
        start = min(start, room - gap)
        out.append(list(range(start, start + half)) + list(range(start + half + gap, start + gap + n_prb)))
    return out


# ---- builders of planes

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


def flat_planes(rng, planes, al, dmrs, mag):
    """a copy of one unit's planes whose DMRS rows carry a channel of the one magnitude `mag` on every sub-carrier and slot, with
    build_planes' random phases"""
    M = 12 * al.N_prb
    p = np.array(planes)
    ang0 = rng.uniform(-np.pi, np.pi, M)
    ang = [ang0, ang0 + rng.uniform(-2.5, 2.5, M)]
    for s, L in ((0, 3), (1, 10)):
        g = mag * np.exp(1j * ang[s]) * (dmrs[2 * s].astype(np.float64) + 1j * dmrs[2 * s + 1].astype(np.float64))
        sc = pm.subcarriers(al, s)
        p[0, L, sc], p[1, L, sc] = g.real, g.imag
    return p


# ---- cases

class Case:
    """One allocation on a unit of its own: .n_prb, .M, .sf, .seed, .al (unit to be set by the plan's builder), .dmrs float32 [4, M],
    .planes (case(): float32 [2, 16, 1200]; every other builder: [n_rx] of them, with .n_rx), .c_init; a two-path case's .a, .d, .phis"""

    def __init__(self, n_prb, sf, seed, mod, prbs, rnti, **more):
        import openlte_amd as m
        from test_dlsch3gpp_cpu import tbs_table
        self.n_prb, self.M, self.sf, self.seed = n_prb, 12 * n_prb, sf, seed
        self.al = m.make_alloc(0, mod, int(tbs_table()[0][n_prb - 1]), prbs[0], rnti, prbs_slot1=prbs[1])
        self.dmrs = m.ul_dmrs_pusch(m.UlCfg(*ULC), CELL, sf, n_prb)
        self.c_init = (rnti << 14) | (sf << 9) | CELL
        self.__dict__.update(more)

    def with_planes(self, planes, **more):
        """this case on other planes"""
        c = copy.copy(self)
        c.__dict__.update(more, planes=planes)
        return c


@functools.lru_cache(maxsize=None)
def case(n_prb, seed=0):
    """the case of one size and builder seed (cached and shared: treat it as read-only): a QPSK grant at I_TBS 0 on PRB runs that start at a
    non-zero PRB, other in slot 1 than in slot 0"""
    c = Case(n_prb, n_prb % 10, seed, 1, [list(range(p, p + n_prb)) for p in prb_runs(n_prb)], 0x100 + n_prb)
    c.planes = build_planes(np.random.default_rng(1000 * seed + n_prb), c.al, c.dmrs)
    return c


@functools.lru_cache(maxsize=None)
def rx_case(n_prb, n_rx, seed=0, mod=1):
    """(cached and shared: read-only) n_prb PRB of modulation mod at I_TBS 0 on gapped PRB lists (contiguous where the carrier has no room),
    antenna r's planes from build_planes with a generator of its own"""
    c = Case(n_prb, (n_prb + seed) % 10, seed, mod, gapped_runs(n_prb), 0x200 + n_prb, n_rx=n_rx)
    c.planes = [build_planes(np.random.default_rng([seed, n_prb, r]), c.al, c.dmrs) for r in range(n_rx)]
    return c


@functools.lru_cache(maxsize=None)
def two_path_case(n_prb, n_rx, seed=0, mod=1, a=0.5, d=37):
    """(cached and shared: read-only) rx_case(n_prb, n_rx, seed, mod) through a second path of relative amplitude a, d samples late (of
    2048: a ripple period of 2048 / d sub-carriers, several periods inside a wide allocation) and a phase per antenna"""
    b = rx_case(n_prb, n_rx, seed, mod)
    phis = np.random.default_rng([77, seed, n_prb, n_rx]).uniform(-np.pi, np.pi, n_rx)
    return b.with_planes(two_path(b.planes, b.al, a, d, phis), a=a, d=d, phis=phis)


@functools.lru_cache(maxsize=None)
def flat_case(n_prb, n_rx, seed=0, mod=1, mag=1.0):
    """(cached and shared: read-only) the allocation, DMRS and noise rows of rx_case with DMRS rows whose channel has the one magnitude
    `mag` on every sub-carrier, slot and antenna and build_planes' random phases: P_s[i] = n_rx mag^2 up to the float roundings, while the
    second differences of the phases keep sigma2 near mag^2"""
    b = rx_case(n_prb, n_rx, seed, mod)
    return b.with_planes([flat_planes(np.random.default_rng([78, seed, n_prb, r]), b.planes[r], b.al, b.dmrs, mag) for r in range(n_rx)])


# ---- expectations

def _read_only(x):
    for v in x.values() if isinstance(x, dict) else [x]:
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def expected(n_prb, seed=0):
    """complex128 [12, M]: the model's equalised, pre-decoded symbols of case(n_prb, seed) (cached and shared: read-only)"""
    c = case(n_prb, seed)
    return _read_only(pm.equalise_predecode(c.planes, c.al, c.dmrs))


@functools.lru_cache(maxsize=None)
def rx_expected(n_prb, n_rx, seed=0, mod=1):
    """the same of rx_case(n_prb, n_rx, seed, mod)"""
    c = rx_case(n_prb, n_rx, seed, mod)
    return _read_only(pm.equalise_predecode(c.planes, c.al, c.dmrs))


@functools.lru_cache(maxsize=None)
def mmse_expected(key, flat=False):
    """pusch_demod_model.taps of two_path_case(*key) or flat_case(*key) (cached and shared: read-only)"""
    c = flat_case(*key) if flat else two_path_case(*key)
    return _read_only(pm.taps(c.planes, c.al, c.dmrs))


def errors(got, want):
    """(rel-L2 per data symbol [12], largest elementwise error over the symbol's RMS [12]) of got against want, both [12, M]"""
    d = np.abs(np.asarray(got, np.complex128) - want)
    rms = np.sqrt((np.abs(want) ** 2).mean(1))
    return np.sqrt((d ** 2).sum(1) / (np.abs(want) ** 2).sum(1)), d.max(1) / rms


# ---- the float32 floor and the gates: (restatement, expectation) pairs, both called with a case's key

@functools.lru_cache(maxsize=None)
def _z32(n_prb, seed):
    c = case(n_prb, seed)
    z = pm.equalised(c.planes, c.al, c.dmrs)
    return pm._f32(z.real).astype(np.float64) + 1j * pm._f32(z.imag).astype(np.float64)


def _transform_f32(n_prb, seed):
    return pm.predecode_f32(_z32(n_prb, seed), n_prb)


def _transform_f64(n_prb, seed):
    return pm.predecode(_z32(n_prb, seed))


def _rx_f32(*key):
    c = rx_case(*key)
    return pm.predecode_planes_f32(c.planes, c.al, c.dmrs)


def _mmse_f32(*key):
    c = two_path_case(*key)
    return pm.predecode_planes_f32(c.planes, c.al, c.dmrs, np.float32(pm.sigma2(c.planes, c.al, c.dmrs)))


def _mmse_f64(*key):
    return mmse_expected(key)["x"]


# the transform alone, both sides on the model's equalised values rounded to float32, at every planned size and builder seed: what a float32
# transform of this structure costs on the tests' own inputs; the combining and the MMSE receiver whole, from the planes
TRANSFORM = (_transform_f32, _transform_f64)
RX = (_rx_f32, rx_expected)
MMSE = (_mmse_f32, _mmse_f64)
TRANSFORM_KEYS = tuple((n, seed) for seed in SEEDS for n in planned_sizes())


@functools.lru_cache(maxsize=None)
def _floor(pair, keys):
    out = {}
    for k in keys:
        l2, el = errors(pair[0](*k), pair[1](*k))
        out[k] = (float(l2.max()), float(el.max()))
    return out


def float32_floor(pair=TRANSFORM, keys=TRANSFORM_KEYS):
    """{key: (worst rel-L2, worst elementwise error / RMS)} of the pair's float32 restatement against its float64 expectation over the
    cases `keys`, with no kernel in the loop (cached and shared: read-only)"""
    return _floor(pair, tuple(keys))


def worst(floor):
    return max(v[0] for v in floor.values()), max(v[1] for v in floor.values())


def gates(pair=TRANSFORM, keys=TRANSFORM_KEYS):
    """(rel-L2 gate, elementwise gate) of the GPU tests: GATE_FACTOR x the float32 restatement's worst figures over `keys`, capped at the
    hard gate TOL_SYMB (10 TOL_SYMB elementwise).  Why 8: the kernel's butterflies order their operations differently (radix 9 as 3 x 3,
    radix 8 as 2 x 4), its twiddles come from sincospif and its estimate from atan2f / sincosf, a few ulp from correctly rounded, and the
    equaliser adds some ten float roundings per element in front of the transform; each moves a float32 transform's error by a small
    factor, none by an order of magnitude."""
    l2, el = worst(float32_floor(pair, keys))
    return min(GATE_FACTOR * l2, TOL_SYMB), min(GATE_FACTOR * el, 10 * TOL_SYMB)


# ---- views: pusch_demod_model's names and this module's under one alias, and on top the names a receiver's tests read its own
# case / expectation / gate / launch functions by

def _view(**own):
    return types.SimpleNamespace(**{**vars(pm), **globals(), **own})


rx_view = _view(case=rx_case, expected=rx_expected, s_par=pm.rx_s_par,
           float32_floor=lambda keys: worst(float32_floor(RX, keys)), gates=lambda keys: gates(RX, keys))
mmse_view = _view(case=two_path_case, expected=mmse_expected, demap=pm.demap_mmse,
                  launch=lambda n_rx, M_max, W, limit=pm.LDS_LIMIT, override=0: pm.launch(n_rx, M_max, W, 1, 1, 1, limit, override),
                  float32_floor=lambda keys: worst(float32_floor(MMSE, keys)), gates=lambda keys: gates(MMSE, keys))
