"""GPU: receive-antenna combining on the 3GPP PUSCH plans (mi_lte_pusch_plan_set_rx_antennas, k_pusch_demod_llr_rx) against the float64
model of include/mi_lte.h's text (tests/pusch_demod_model.py): the tapped symbols, rho_s, sigma2 and the gain on synthetic planes of two and
four antennas at the sizes where the launch changes shape; the bytes by pusch_demod_model.demap on the run's own taps; the same grid on
every antenna and an all-zero antenna against the single-antenna run; a plan that never saw the setter, or went to 2 and back to 1, is the
plan it was; transport blocks, control information and HARQ through the transmit chain; every refusal of the contract; and what a second
antenna buys at a point profiles/pusch_rxdiv_sweep.txt names.

Gates of the tapped symbols, per data symbol.  Hard: rel-L2 < 1e-5 and elementwise < 1e-4 of the symbol's RMS (pusch_demod_cases).
Tight: 8 x the error of the float32 restatement of the estimate, the combiner and the transform on each test's own inputs
(pusch_demod_cases.float32_floor; 1.8e-7 .. 2.0e-7 rel-L2 on these cases), capped at the hard gate.

Measured on an MI355X (worst rel-L2 / worst elementwise error over RMS per plan set of test_taps_against_the_model; tight gates
1.4e-6 .. 1.6e-6 / 3.1e-6 .. 6.9e-6):
  narrow_2      1, 6, 8 PRB x 2, 192 threads, NaN spare units   2.08e-7 / 5.83e-7
  narrow_4      1 | 6, 8 PRB x 4, 192 threads                   1.92e-7 / 4.97e-7
  mixed_4       1, 9, 25 PRB x 4, 256 threads, S_par 6          2.27e-7 / 6.08e-7
  s_par_2       16 | 18 | 35 | 36 | 70 | 72 PRB x 2             2.23e-7 / 6.99e-7
  s_par_4_low   16 | 18 | 35 | 36 PRB x 4                       2.23e-7 / 8.27e-7
  s_par_4_high  66 | 68 | 72 | 74 | 78 PRB x 4, S_par 3 2 2 1 1 2.18e-7 / 7.92e-7
  wide_2        94, 96, 99 PRB x 2 (radix 47; 144 KB of LDS)    2.30e-7 / 9.13e-7 -- the worst of all
rho within 1.3e-7 and sigma2 within 5.3e-8 of the model (bounds 1e-4); the kernel sits at 1.2 x the float32 restatement, a seventh of the
tight gate.  Bytes: 0 of 12 384 per plan and gain differ from the exact layer, 4 .. 14 in the guard band.  The same grid on every antenna
and a single live antenna give the single-antenna run's taps bit for bit (2 t is exact, and so is 0 + t), rho ratios of exactly n_rx and 1,
sigma2 ratios of exactly 1 and 1 / n_rx.
"""
import ctypes as C
import os
import sys

import numpy as np
import pytest

import demap_llr_model as dm
import pusch_demod_cases as pc
import pusch_demod_model as nm
import pusch_demod_model as pm
from pusch_demod_cases import rx_view as rxm
from test_pusch_harq_gpu import decode
from test_ulsch3gpp_gpu import FFT, QM, ULC, grant
from test_ulsch_cqi_cpu import CRC_OK, NO_CRC, pack_bits
from test_ulsch_uci_cpu import uci
from test_ulsch_uci_gpu import Grant, tbs_at_most

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))

pytestmark = pytest.mark.gpu

ERR_INVALID, ERR_UNSUPPORTED = -1, -4
# profiles/pusch_rxdiv_sweep.txt (16 transport blocks per point, the sweep's seeds): the class and the SNR of test_value
# No class of the sweep has the window of DESIGN section 8 (two antennas 16 / 16 at p - 1 and p, each antenna alone 0 / 16 at p and p + 1): 3 dB
# between the curves and 1 dB steps leave it one step short (64qam_r0.5_flat: two antennas 16 / 16 from 8 dB, one antenna 0 / 16 up to 9 dB
# and 15 or 16 / 16 at 10 dB).  So the fallback: the first point of the largest difference, 16 / 16 against 0 / 16 and 0 / 16.
VALUE_CLASS, VALUE_SNR_DB = "16qam_r0.5_flat", 6


@pytest.fixture(autouse=True)
def own_choice_of_width(monkeypatch):
    monkeypatch.delenv("MI_LTE_PUSCH_THREADS", raising=False)


class Run:
    """One 3GPP plan over the cases (pusch_demod_cases.rx_case), one unit and one allocation each, on n_rx antennas with the symbol tap on.
    d_subframes is antenna-major with ant_stride = units + spare; the spare units of every antenna are NaN, so a read of one poisons the
    result.  planes: [unit][antenna], by default the cases' own."""

    def __init__(self, ctx, cases, n_rx, spare=0, planes=None):
        import openlte_amd as m
        self.ctx, self.cases, self.n_rx, self.n = ctx, cases, n_rx, len(cases)
        self.stride = self.n + spare
        cfg, ul = m.DlCfg(2048, pc.N_RB, 1, 0), m.UlCfg(*pc.ULC)
        self.allocs = []
        for u, c in enumerate(cases):
            al = m.PdschAlloc.from_buffer_copy(c.al)
            al.unit = u
            self.allocs.append(al)
        planes = [c.planes for c in cases] if planes is None else planes
        grid = np.full((n_rx * self.stride, 2, 16, pm.N_SC), np.nan, np.float32)
        for u in range(self.n):
            for r in range(n_rx):
                grid[r * self.stride + u] = planes[u][r]
        self.d_sub = ctx.to_device(grid)
        self.plan = ctx.pusch_plan_3gpp(cfg, ul, [c.sf for c in cases], [pc.CELL] * self.n, self.allocs)
        self.plan.set_llr_tap(True)
        if n_rx > 1:
            self.plan.set_rx_antennas(n_rx, self.stride)
            assert self.plan.rx_antennas() == (n_rx, self.stride)

    def run(self, gain=1.0, noise=0.0):
        """one MAXLOG run: {x: taps per allocation, rho, s2, g, e: soft bits per allocation, st}"""
        import openlte_amd as m
        self.plan.set_demapper(m.DEMAP_MAXLOG, gain)
        self.plan.set_llr_noise(noise)
        st, _ = self.plan.run(self.d_sub)
        want = "k_pusch_demod_llr_rx:1," if self.n_rx > 1 else "k_pusch_demod_llr:1,"
        assert self.ctx.last_kernels().startswith(want), self.ctx.last_kernels()
        return {"x": [self.plan.llr_symbols(a) for a in range(self.n)], "rho": self.plan.llr_rho(), "s2": self.plan.llr_noise(),
                "g": self.plan.llr_gain(), "e": [self.plan.soft_bits(a) for a in range(self.n)], "st": st}

    def close(self):
        self.plan.close()
        self.d_sub.free()


def keys_of(sizes, n_rx, seed=0, mods=None):
    return tuple((n, n_rx, seed, 1 if mods is None else mods[i]) for i, n in enumerate(sizes))


def check_taps(what, out, keys, worst):
    """taps, rho and sigma2 of one noise-referenced run against the model; prints, then asserts; folds the figures into worst"""
    gates = rxm.gates(keys)
    assert gates[0] <= pc.TOL_SYMB and gates[1] <= 10 * pc.TOL_SYMB
    bad = []
    for a, k in enumerate(keys):
        c = rxm.case(*k)
        got = out["x"][a]
        assert got.shape == (12, c.M) and got.dtype == np.complex64 and np.isfinite(got).all(), (what, k)
        l2, el = pc.errors(got, rxm.expected(*k))
        want_rho = rxm.rho(c.planes, c.al, c.dmrs)[0]
        want_s2 = rxm.sigma2(c.planes, c.al, c.dmrs)
        d_rho = float((np.abs(out["rho"][a].astype(np.float64) - want_rho) / want_rho).max())
        d_s2 = abs(float(out["s2"][a]) - want_s2) / want_s2
        print("%s, %d PRB x %d antennas: rel-L2 %.3g, elementwise / RMS %.3g (gates %.3g / %.3g); rho off by %.3g, sigma2 by %.3g"
              % (what, c.n_prb, c.n_rx, l2.max(), el.max(), gates[0], gates[1], d_rho, d_s2))
        worst["l2"], worst["el"] = max(worst["l2"], float(l2.max())), max(worst["el"], float(el.max()))
        worst["rho"], worst["s2"] = max(worst["rho"], d_rho), max(worst["s2"], d_s2)
        if not ((l2 < gates[0]).all() and (el < gates[1]).all() and d_rho <= 1e-4 and d_s2 <= 1e-4):
            bad.append((k, float(l2.max()), float(el.max()), d_rho, d_s2))
    assert not bad, (what, bad)


def check_gains(out, keys, noise):
    """the gain is (float)(scale / tap) exactly, or the automatic formula on the tapped rho (to 2^-18, test_pusch_llr_gpu's rule)"""
    import openlte_amd as m
    for a, k in enumerate(keys):
        if noise:
            assert out["g"][a] == np.float32(nm.gain(noise, out["s2"][a])) and out["g"][a] > 0, (k, out["g"][a], out["s2"][a])
        else:
            want = pm.auto_gain(out["rho"][a], k[3], m.DEMAP_AUTO_T)
            assert want > 0 and abs(float(out["g"][a]) - want) <= 2.0 ** -18 * want, (k, out["g"][a], want)


# (name, n_rx, plans, spare units): every plan a tuple of sizes in one plan.  s_par: the two planned sizes on either side of every step of
# the combining launch's S_par rule, each alone so that M_max is its own M (QPSK grants: for four antennas 12 | 6 at 16 | 18, 6 | 3 at
# 35 | 36, 3 | 2 at 66 | 68, 2 | 1 at 72 | 74, and 78, the last size admitted)
TAP_PLANS = [
    ("narrow_2", 2, [(1, 6, 8)], 2),          # 192 threads, M = 12 under a wavefront, M_max > M, NaN in the units that are not the plan's
    ("narrow_4", 4, [(1,), (6, 8)], 1),
    ("mixed_4", 4, [(1, 9, 25)], 0),          # 256 threads from 9 PRB on; 25 PRB on four antennas
    ("s_par_2", 2, [(16,), (18,), (35,), (36,), (70,), (72,)], 0),
    ("s_par_4_low", 4, [(16,), (18,), (35,), (36,)], 0),
    ("s_par_4_high", 4, [(66,), (68,), (72,), (74,), (78,)], 0),
    ("wide_2", 2, [(94, 96, 99)], 1),         # a generic radix-47 pass; 96 and 99 PRB on two antennas: 144 KB of LDS
]


@pytest.mark.parametrize("name,n_rx,plans,spare", TAP_PLANS, ids=[p[0] for p in TAP_PLANS])
def test_taps_against_the_model(ctx, name, n_rx, plans, spare):
    """Gate 1.  Every plan runs with the noise-referenced gain (sigma2 tap, the NOISE instantiation) and with the automatic gain (the
    other one): the taps and rho of the two runs are the same bits, and both runs' gains follow their rule."""
    worst = {"l2": 0.0, "el": 0.0, "rho": 0.0, "s2": 0.0}
    for sizes in plans:
        keys = keys_of(sizes, n_rx)
        M_max, W = 12 * max(sizes), max(rxm.words(n, 2) for n in sizes)
        assert rxm.s_par(n_rx, M_max, W) > 0
        r = Run(ctx, [rxm.case(*k) for k in keys], n_rx, spare=spare)
        noisy = r.run(gain=0.0, noise=8.0)
        auto = r.run(gain=0.0, noise=0.0)
        r.close()
        check_taps("%s %s (S_par %d, %d threads)" % (name, list(sizes), rxm.s_par(n_rx, M_max, W), rxm.threads(M_max)), noisy, keys, worst)
        check_gains(noisy, keys, 8.0)
        check_gains(auto, keys, 0.0)
        assert all(x.tobytes() == y.tobytes() for x, y in zip(noisy["x"], auto["x"])) and noisy["rho"].tobytes() == auto["rho"].tobytes()
    print("%s: worst rel-L2 %.3g, elementwise / RMS %.3g, rho %.3g, sigma2 %.3g" % (name, worst["l2"], worst["el"], worst["rho"], worst["s2"]))


def test_s_par_steps_are_the_ones_tested():
    """the sizes of TAP_PLANS' s_par rows sit on either side of every step of the rule (QPSK grants)"""
    for n_rx, pairs in ((2, ((16, 18, 12, 6), (35, 36, 6, 3), (70, 72, 3, 2))), (4, ((16, 18, 12, 6), (35, 36, 6, 3), (66, 68, 3, 2), (72, 74, 2, 1)))):
        steps = []
        sizes = [n for n in pc.planned_sizes() if rxm.s_par(n_rx, 12 * n, rxm.words(n, 2))]
        for lo, hi in zip(sizes, sizes[1:]):
            a, b = (rxm.s_par(n_rx, 12 * n, rxm.words(n, 2)) for n in (lo, hi))
            if a != b:
                steps.append((lo, hi, a, b))
        assert tuple(steps) == pairs, (n_rx, steps)
        assert sizes[-1] == (99 if n_rx == 2 else 78)


@pytest.mark.parametrize("n_rx", [2, 4])
def test_bytes_against_the_exact_layer(ctx, n_rx):
    """Gate 2.  QPSK on 1 PRB, 16QAM on 6, 64QAM on 10 in one plan, under the automatic gain, a fixed one and the noise-referenced one:
    no byte differs from pusch_demod_model.demap(taps, rho tap, gain tap) outside the guard band, at most one step inside it, the band
    under 1 % of the soft bits (test_pusch_llr_gpu's cap); the bytes are graded; a second run gives the same bytes."""
    import openlte_amd as m
    sizes, mods = (1, 6, 10), (1, 2, 3)
    keys = keys_of(sizes, n_rx, seed=2, mods=mods)
    r = Run(ctx, [rxm.case(*k) for k in keys], n_rx, spare=1)
    auto = r.run(gain=0.0)
    fixed = float(np.float32(1.5 * np.median(auto["g"])))
    for what, out, gains in (("automatic", auto, auto["g"]), ("fixed", r.run(gain=fixed), [fixed] * 3), ("noise-referenced", None, None)):
        if out is None:
            out = r.run(gain=0.0, noise=8.0)
            gains = out["g"]
            check_gains(out, keys, 8.0)
        n_guard = n_all = 0
        every = []
        for a, k in enumerate(keys):
            c = rxm.case(*k)
            assert (out["rho"][a] > 0).all() and float(out["g"][a]) == float(np.float32(gains[a]))
            want = pm.demap(out["x"][a], out["rho"][a], k[3], c.c_init, gain=float(gains[a]), T=m.DEMAP_AUTO_T)
            e = out["e"][a]
            assert len(e) == len(want.bytes) == 144 * c.n_prb * QM[k[3]]
            d = np.abs(e.astype(np.int32) - want.bytes)
            guard = dm.in_guard(want.x)
            print("%d antennas, %s gain, %d PRB Q_m %d: %d soft bits, %d in the guard band, %d differ (%d outside it), gain %.9g"
                  % (n_rx, what, c.n_prb, QM[k[3]], len(e), guard.sum(), (d != 0).sum(), (d[~guard] != 0).sum(), gains[a]))
            assert not d[~guard].any() and d.max() <= 1, (what, k)
            n_guard, n_all = n_guard + int(guard.sum()), n_all + len(e)
            every.append(e)
        every = np.concatenate(every).astype(int)
        assert n_guard < 0.01 * n_all and len(np.unique(every)) > 64  # (graded bytes: the planes' data rows are noise, few reach the clamp)
        again = r.run(gain=0.0 if what != "fixed" else fixed, noise=8.0 if what == "noise-referenced" else 0.0)
        assert all(x.tobytes() == y.tobytes() for x, y in zip(out["e"], again["e"]))
    r.close()


def against_single(what, out, single, keys, n_rx, rho_factor, s2_factor):
    """taps within gate 1's tolerances of the single-antenna run's, rho rho_factor times and sigma2 s2_factor times its values to 1e-6"""
    gates = rxm.gates(keys)
    for a, k in enumerate(keys):
        l2, el = pc.errors(out["x"][a], single["x"][a].astype(np.complex128))
        d_rho = float(np.abs(out["rho"][a].astype(np.float64) / (rho_factor * single["rho"][a].astype(np.float64)) - 1).max())
        d_s2 = abs(float(out["s2"][a]) / (s2_factor * float(single["s2"][a])) - 1)
        print("%s, %d PRB x %d: taps against the single-antenna run rel-L2 %.3g, elementwise %.3g; rho ratio off by %.3g, sigma2 ratio by %.3g"
              % (what, k[0], n_rx, l2.max(), el.max(), d_rho, d_s2))
        assert (l2 < gates[0]).all() and (el < gates[1]).all(), (what, k)
        assert d_rho <= 1e-6 and d_s2 <= 1e-6, (what, k, d_rho, d_s2)


@pytest.fixture(scope="module")
def single_run(ctx):
    """the single-antenna run of antenna 0 of the cases the duplicated- and dead-antenna tests share (computed once, read-only)"""
    keys = keys_of((1, 6, 25), 2, seed=3)
    r = Run(ctx, [rxm.case(*k) for k in keys], 1, planes=[[rxm.case(*k).planes[0]] for k in keys])
    out = r.run(gain=0.0, noise=8.0)
    r.close()
    assert (out["s2"] > 0).all() and (out["rho"] > 0).all()
    return keys, out


@pytest.mark.parametrize("n_rx", [2, 4])
def test_the_same_grid_on_every_antenna(ctx, single_run, n_rx):
    """Gate 3: the single-antenna symbols, n_rx times rho, the same sigma2"""
    keys, single = single_run
    r = Run(ctx, [rxm.case(*k) for k in keys], n_rx, spare=1, planes=[[rxm.case(*k).planes[0]] * n_rx for k in keys])
    out = r.run(gain=0.0, noise=8.0)
    r.close()
    against_single("the same grid on every antenna", out, single, keys, n_rx, float(n_rx), 1.0)


@pytest.mark.parametrize("n_rx,live", [(2, 0), (2, 1), (4, 2)])
def test_dead_antennas(ctx, single_run, n_rx, live):
    """Gate 4: every antenna but `live` all zero -- taps and rho are the live antenna's single-antenna run, sigma2 is 1 / n_rx of its
    estimate.  All antennas zero: rho = 0, gain 0, every soft bit 0, and the plan decodes again afterwards."""
    keys, single = single_run
    zero = np.zeros((2, 16, pm.N_SC), np.float32)
    planes = [[rxm.case(*k).planes[0] if r == live else zero for r in range(n_rx)] for k in keys]
    r = Run(ctx, [rxm.case(*k) for k in keys], n_rx, planes=planes)
    out = r.run(gain=0.0, noise=8.0)
    against_single("one live antenna (%d)" % live, out, single, keys, n_rx, 1.0, 1.0 / n_rx)
    dark = r.ctx.alloc(r.d_sub.nbytes)
    dark.zero()
    lit, r.d_sub = r.d_sub, dark
    for noise in (8.0, 0.0):
        nothing = r.run(gain=0.0, noise=noise)
        assert not nothing["rho"].any() and not nothing["g"].any() and not any(e.any() for e in nothing["e"]), noise
        assert (nothing["st"] == 2).all()
    r.d_sub = lit
    dark.free()
    back = r.run(gain=0.0, noise=8.0)
    assert all(x.tobytes() == y.tobytes() for x, y in zip(back["e"], out["e"]))
    r.close()


def test_setter_is_inert_at_one_antenna(ctx):
    """Gate 5.  A plan that never saw the setter and one set to 2 antennas, run, and set back to 1: bytes, taps, rho, sigma2 and gain
    byte for byte, under k_pusch_demod_llr; the run in between is k_pusch_demod_llr_rx's and differs; two combining runs agree."""
    keys = keys_of((1, 6, 25), 2, seed=3)
    cases = [rxm.case(*k) for k in keys]
    plain = Run(ctx, cases, 1, planes=[[c.planes[0]] for c in cases])
    assert plain.plan.rx_antennas() == (1, 0)
    other = Run(ctx, cases, 2)
    for noise in (0.0, 8.0):
        want = plain.run(gain=0.0, noise=noise)
        other.n_rx = 2
        other.plan.set_rx_antennas(2, other.stride)
        first, second = other.run(gain=0.0, noise=noise), other.run(gain=0.0, noise=noise)
        for key in ("x", "e"):
            assert all(x.tobytes() == y.tobytes() for x, y in zip(first[key], second[key]))
            assert any(x.tobytes() != y.tobytes() for x, y in zip(first[key], want[key]))
        other.n_rx = 1
        other.plan.set_rx_antennas(1, 12345)  # ant_stride is ignored
        assert other.plan.rx_antennas() == (1, 0)
        got = other.run(gain=0.0, noise=noise)  # (antenna 0 of unit u is subframe u in both layouts)
        for key in ("x", "e"):
            assert all(x.tobytes() == y.tobytes() for x, y in zip(got[key], want[key])), (noise, key)
        assert all(got[key].tobytes() == want[key].tobytes() for key in ("rho", "s2", "g", "st"))
    plain.close()
    other.close()


# ---- through the transmit chain

class RxUnits:
    """Uplink units of one 100- or 25-RB cell from the 3GPP transmitter on n_rx antennas (synth.ul_units_3gpp_rx: one payload, a gain,
    phase, delay and noise of its own per antenna), through one front-end call over the antenna-major units"""

    def __init__(self, ctx, n_rb, sfs, cell, allocs, n_rx, snr_db, seed, payload=None, ucis=None, ctrl=None, spare=0):
        import openlte_amd as m
        from openlte_amd import synth
        self.ctx, self.cfg, self.ul = ctx, m.DlCfg(FFT[n_rb], n_rb, 1, 0), m.UlCfg(*ULC)
        self.sfs, self.cells, self.allocs, self.ucis, self.n_rx = list(sfs), [cell] * len(sfs), allocs, ucis, n_rx
        self.stride = len(sfs) + spare
        kw = {} if ucis is None else dict(uci=ucis, **ctrl)
        iq, self.tx = synth.ul_units_3gpp_rx(self.cfg, self.ul, self.sfs, self.cells, allocs, 1, n_rx, ant_stride=self.stride, seed=seed,
                                             payload=payload, max_delay=3, snr_db=snr_db, peak=100.0, **kw)
        _, self.d_sub = ctx.ul_frontend(self.cfg, iq.reshape(-1, 2), np.arange(iq.shape[0]) * iq.shape[1], keep=True)

    def plan(self, n_rx=None):
        import openlte_amd as m
        p = self.ctx.pusch_plan_3gpp(self.cfg, self.ul, self.sfs, self.cells, self.allocs, uci=self.ucis)
        p.set_demapper(m.DEMAP_MAXLOG, 0.0)
        p.set_rx_antennas(self.n_rx if n_rx is None else n_rx, self.stride)
        return p

    def free(self):
        self.d_sub.free()


def test_transport_blocks_through_the_transmit_chain(ctx):
    """Gate 6.  Two antennas at 30 dB, 100-RB cell: 64QAM on 96 PRB in thirteen code blocks, 16QAM on 10 PRB and QPSK on 1 PRB, one per
    unit, under the automatic and the noise-referenced gain: status 0 and the sent bits."""
    import openlte_amd as m
    from test_dlsch3gpp_gpu import tbs
    allocs = [m.make_alloc(0, 3, tbs(26, 99), list(range(2, 98)), 0x301), grant(1, 2, 15, 10, 40, 0x302), grant(2, 1, 5, 1, 77, 0x303)]
    assert m.ulsch_layout(allocs[0].tbs, 0, 2)["C"] == 13 and allocs[0].N_prb == 96
    un = RxUnits(ctx, 100, [3, 8, 0], 17, allocs, 2, 30.0, seed=200, spare=1)
    plan = un.plan()
    for noise in (0.0, 8.0):
        plan.set_llr_noise(noise)
        st, bits = plan.run(un.d_sub)
        assert ctx.last_kernels().startswith("k_pusch_demod_llr_rx:1,k_dl3_desc:1,"), ctx.last_kernels()
        print("noise scale %g: status %s, rho of the 96-PRB grant %.3g .. %.3g" % (noise, list(st), plan.llr_rho()[0].min(), plan.llr_rho()[0].max()))
        assert (st == 0).all()
        assert all((bits[a] == un.tx[a, 0, :al.tbs]).all() for a, al in enumerate(allocs))
    plan.close()
    un.free()


def test_control_information_through_the_transmit_chain(ctx):
    """Gate 6.  A plan with control information on two antennas at 30 dB: the sent HARQ-ACK and RI bits, the sent 5-bit CQI report from
    the device's decoder, and the transport blocks."""
    import openlte_amd as m
    o = np.array([1, 0, 1, 1, 0], np.uint8)
    gs = [Grant(2, tbs_at_most(6, 1000), 6, 0, 0x211, uci(1, 8, 1, 4, 40), [1], [1], seed=21),
          Grant(3, tbs_at_most(10, 3000), 10, 8, 0x212, uci(2, 12, 2, 6, 0), [1, 0], [0, 1], seed=22),
          Grant(1, tbs_at_most(2, 150), 2, 20, 0x213)]
    gs[0].cqi = m.cqi_encode(5, o, 40)
    allocs = [m.make_alloc(k, g.mod, g.tbs, list(range(g.prb0, g.prb0 + g.n_prb)), g.rnti, rv_idx=g.rv) for k, g in enumerate(gs)]
    un = RxUnits(ctx, 25, [1, 4, 7], 33, allocs, 2, 30.0, seed=210, ucis=[g.u for g in gs],
                 ctrl=dict(ack=[g.ack for g in gs], ri=[g.ri for g in gs], cqi=[g.cqi for g in gs]))
    plan = un.plan()
    plan.set_cqi_decode([5, 0, 0])
    st, bits = plan.run(un.d_sub)
    assert ctx.last_kernels().startswith("k_pusch_demod_llr_rx:1,k_ulsch_uci_gather:1,k_ulsch_uci_decide:1,k_ulsch_cqi_decode:1,k_dl3_desc:1,")
    rec, cqi = plan.uci_results(), plan.cqi_results()
    for k, g in enumerate(gs):
        print("alloc %d: status %d, ack %s ri %s" % (k, st[k], rec[k]["ack"], rec[k]["ri"]))
        assert st[k] == 0 and (bits[k] == un.tx[k, 0, :g.tbs]).all(), k
        assert list(rec[k]["ack"])[:g.u.O_ack] == g.ack and list(rec[k]["ri"])[:g.u.O_ri] == g.ri, (k, rec[k])
    assert cqi[0]["O"] == 5 and cqi[0]["bits"] == pack_bits(o) and cqi[0]["crc"] in (NO_CRC, CRC_OK), cqi[0]
    plan.close()
    un.free()


def test_harq_through_the_transmit_chain(ctx):
    """Gate 6.  A first transmission through mi_lte_pusch_decode_run_harq equals the plain run byte for byte; two transmissions of a code
    rate above 1 (16QAM on 10 PRB, rv 0 then rv 2, two antennas each, the noise-referenced gain) fail alone and decode combined."""
    import openlte_amd as m
    from test_dlsch3gpp_cpu import tbs_table
    G = 144 * 10 * 4
    size = min((int(s) for s in tbs_table()[:, 9] if s + 24 <= 6144), key=lambda s: abs(G / (s + 24) - 0.95))
    assert 0.9 <= G / (size + 24) < 1.0
    pool = ctx.harq_pool(4)
    payload = None
    for k, rv in enumerate((0, 2)):
        allocs = [m.make_alloc(0, 2, size, list(range(5, 15)), 0x401, rv_idx=rv), m.make_alloc(1, 2, size, list(range(30, 40)), 0x402, rv_idx=rv)]
        un = RxUnits(ctx, 100, [2, 6], 222, allocs, 2, 30.0, seed=220 + k, payload=payload)
        payload = un.tx
        plan = un.plan()
        plan.set_llr_noise(8.0)
        plain = decode(un, plan)
        assert plain["kernels"].startswith("k_pusch_demod_llr_rx:1,") and (plain["st"] != 0).all(), plain["st"]
        alone = decode(un, plan, pool, [2, 3], True)
        assert alone["kernels"].startswith("k_pusch_demod_llr_rx:1,")
        assert alone["st"].tobytes() == plain["st"].tobytes() and alone["rows"].tobytes() == plain["rows"].tobytes()
        assert alone["cb_ok"].tobytes() == plain["cb_ok"].tobytes() and all(x.tobytes() == y.tobytes() for x, y in zip(alone["cb_soft"], plain["cb_soft"]))
        h = decode(un, plan, pool, [0, 1], k == 0)
        if k == 1:
            assert (h["st"] == 0).all(), h["st"]
            assert all((h["rows"][a, :size] == un.tx[a, 0, :size]).all() for a in range(2))
            assert all(pool.state(a)["n_tx"] == 2 for a in range(2))
        plan.close()
        un.free()
    pool.close()


def test_refusals_leave_the_plan_runnable(ctx):
    """Gate 7.  INVALID_ARG: a NULL plan, n_rx of 0, 3, 5 or 8, n_rx > 1 with ant_stride under the plan's units, NULL outputs of the getter.
    UNSUPPORTED: a reference-mode plan (any n_rx, INVALID_ARG winning for a bad n_rx), four antennas on 80 PRB (no S_par fits the device's
    LDS) while two are accepted, and a run with n_rx > 1 under the default demapper -- which names its reason, launches nothing and lets
    the plan run again once either setting changes.  After each the plan gives the bytes it gave before."""
    import openlte_amd as m
    L = ctx.L
    keys = keys_of((6, 25), 2, seed=3)
    r = Run(ctx, [rxm.case(*k) for k in keys], 2, spare=1)
    want = r.run(gain=0.0)

    def same():
        got = r.run(gain=0.0)
        assert all(x.tobytes() == y.tobytes() for x, y in zip(got["e"], want["e"])) and r.plan.rx_antennas() == (2, 3)

    for n_rx in (0, 3, 5, 8):
        assert L.mi_lte_pusch_plan_set_rx_antennas(r.plan.h, n_rx, 3) == ERR_INVALID, n_rx
    assert L.mi_lte_pusch_plan_set_rx_antennas(None, 2, 3) == ERR_INVALID
    for n_rx in (2, 4):
        assert L.mi_lte_pusch_plan_set_rx_antennas(r.plan.h, n_rx, 1) == ERR_INVALID and L.mi_lte_pusch_plan_set_rx_antennas(r.plan.h, n_rx, 0) == ERR_INVALID
    a, b = C.c_uint32(), C.c_uint32()
    assert L.mi_lte_pusch_plan_rx_antennas(None, C.byref(a), C.byref(b)) == ERR_INVALID
    assert L.mi_lte_pusch_plan_rx_antennas(r.plan.h, None, C.byref(b)) == ERR_INVALID and L.mi_lte_pusch_plan_rx_antennas(r.plan.h, C.byref(a), None) == ERR_INVALID
    same()
    # the default demapper has no combiner: the run refuses, the plan stays runnable
    r.plan.set_demapper(m.DEMAP_REF)
    d_out, d_st = ctx.alloc(r.plan.n_alloc * r.plan.out_stride), ctx.alloc(4 * r.plan.n_alloc)
    before = ctx.last_kernels()
    assert L.mi_lte_pusch_decode_run(ctx.h, r.plan.h, r.d_sub.ptr, d_out.ptr, d_st.ptr) == ERR_UNSUPPORTED
    assert b"max-log" in L.mi_lte_last_error(ctx.h) and ctx.last_kernels() == before
    r.plan.set_rx_antennas(1)
    assert L.mi_lte_pusch_decode_run(ctx.h, r.plan.h, r.d_sub.ptr, d_out.ptr, d_st.ptr) == 0 and ctx.last_kernels().startswith("k_pusch_demod:1,")
    ctx.sync()
    r.plan.set_rx_antennas(2, 3)
    assert L.mi_lte_pusch_decode_run(ctx.h, r.plan.h, r.d_sub.ptr, d_out.ptr, d_st.ptr) == ERR_UNSUPPORTED
    d_out.free()
    d_st.free()
    same()  # (Run.run sets MAXLOG again)
    # a reference-mode plan
    cfg, ul = m.DlCfg(2048, pc.N_RB, 1, 0), m.UlCfg(*pc.ULC)
    ref_plan = ctx.pusch_plan(cfg, ul, [rxm.case(*keys[0]).sf], [pc.CELL], [r.allocs[0]])
    ref_plan.run(r.d_sub)
    e0 = ref_plan.soft_bits(0)
    for n_rx in (1, 2, 4):
        assert L.mi_lte_pusch_plan_set_rx_antennas(ref_plan.h, n_rx, 3) == ERR_UNSUPPORTED, n_rx
    assert L.mi_lte_pusch_plan_set_rx_antennas(ref_plan.h, 3, 3) == ERR_INVALID
    assert ref_plan.rx_antennas() == (1, 0)
    ref_plan.run(r.d_sub)
    assert ctx.last_kernels().startswith("k_pusch_demod:1,") and (ref_plan.soft_bits(0) == e0).all()
    ref_plan.close()
    same()
    r.close()
    # four antennas past the LDS: 80 PRB of QPSK is the first planned size the rule refuses; two antennas take it
    assert rxm.s_par(4, 960, rxm.words(80, 2)) == 0 and rxm.s_par(4, 936, rxm.words(78, 2)) == 1 and rxm.s_par(2, 960, rxm.words(80, 2)) == 2
    wide = Run(ctx, [rxm.case(80, 2, 3)], 2)
    first = wide.run(gain=0.0)
    assert L.mi_lte_pusch_plan_set_rx_antennas(wide.plan.h, 4, 1) == ERR_UNSUPPORTED
    assert wide.plan.rx_antennas() == (2, 1)
    again = wide.run(gain=0.0)
    assert again["e"][0].tobytes() == first["e"][0].tobytes()
    wide.close()


def test_value(ctx):
    """Gate 8.  The class VALUE_CLASS of profiles/pusch_rxdiv_sweep.txt at VALUE_SNR_DB (16 transport blocks, the sweep's seeds), the first
    point of the sweep's largest difference: two antennas decode strictly more blocks -- status 0, the payload equal to the transmitted
    bits -- than either antenna alone, on the same captures.  Measured: 16 of 16 against 0 and 0."""
    import pusch_rxdiv_sweep as sw
    p = sw.Point(ctx, VALUE_CLASS, float(VALUE_SNR_DB), 16)
    n = {mode: int(p.decoded(mode).sum()) for mode in ("ant0", "ant1", "rx2")}
    p.close()
    print("%s at %d dB: %s of 16 transport blocks decoded" % (VALUE_CLASS, VALUE_SNR_DB, n))
    assert n["rx2"] > max(n["ant0"], n["ant1"]), n
