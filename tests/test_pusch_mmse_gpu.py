"""GPU: MMSE equalisation on the 3GPP PUSCH plans (mi_lte_pusch_plan_set_equaliser, k_pusch_demod_llr_mmse) against the float64 model of
include/mi_lte.h's text (tests/pusch_demod_model.py): the tapped symbols, nu_s, the rho tap, sigma2 and the gain on two-path planes of one,
two and four antennas at the sizes where the launch changes shape; the bytes by the model's de-mapper on the run's own taps; flat planes
against the zero-forcing noise-referenced run; a plan that never saw the setter, or went to MMSE and back, is the plan it was; the
degenerate grids and every refusal of the contract; transport blocks, control information and HARQ through the multipath generator; and
what the equaliser buys at the point profiles/pusch_mmse_sweep.txt names.

Gates of the tapped symbols, per data symbol (test_pusch_rxdiv_gpu's rule).  Hard: rel-L2 < 1e-5 and elementwise < 1e-4 of the symbol's
RMS.  Tight: 8 x the error of the float32 restatement of the estimate, the equaliser and the transform on each row's own cases
(pusch_demod_cases.float32_floor: 2.1e-7 .. 2.3e-7 rel-L2), capped at the hard gate.  Scalars (nu_s, the rho tap, sigma2): 1e-4.

Sizes.  A plan takes N_prb divisible by 2, 3 or 5 only (and 1), so no 17 or 71 PRB: the S_par steps there are held from the planned sizes on
either side, 16 | 18 and 70 | 72 (test_sizes_sit_on_the_steps).

Measured on an MI355X (1 / 2 / 4 antennas): worst rel-L2 2.10e-7 / 2.13e-7 / 2.24e-7, elementwise over RMS 9.9e-7 / 8.0e-7 / 7.7e-7 (tight
gates 1.6e-6 .. 1.8e-6 / 6.6e-6 .. 9.9e-6); nu_s within 1.0e-7, the rho tap within 1.8e-7, sigma2 within 5.3e-8.  Bytes: 0 of 254 880 /
254 880 / 369 792 differ from the model's de-mapper, 37 / 52 / 85 in the guard band.  Flat planes: 0 of 12 384 bytes differ from the
zero-forcing run, on one, two and four antennas.  test_value: 16 of 16 against 0 of 16."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

import demap_llr_model as dm
import pusch_demod_cases as pc
import pusch_demod_model as pm
from pusch_demod_cases import mmse_view as mm, rx_view as rxm
from test_pusch_harq_gpu import decode
from test_pusch_mmse_cpu import FLAT_KEYS
from test_pusch_rxdiv_gpu import Run, RxUnits
from test_ulsch3gpp_gpu import QM, grant
from test_ulsch_cqi_cpu import CRC_OK, NO_CRC, pack_bits
from test_ulsch_uci_cpu import uci
from test_ulsch_uci_gpu import Grant, tbs_at_most

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))

pytestmark = pytest.mark.gpu

ERR_INVALID, ERR_UNSUPPORTED = -1, -4
SCALE = 8.0
PATHS = ([0, 4], [1.0, 1.0])  # two equal-power paths 4 samples apart
# profiles/pusch_mmse_sweep.txt (16 transport blocks per point, the sweep's seeds): the curve and the SNR of test_value, by DESIGN section 8's
# window rule -- the first point p of the first curve where MMSE decodes 16 / 16 at p - 1 and p and zero forcing 0 / 16 at p and p + 1
# (one antenna, two equal-power paths: MMSE 16 / 16 from 14 dB on, zero forcing 0 / 16 up to 16 dB and 16 / 16 from 32 dB on)
VALUE_CLASS, VALUE_SNR_DB = "16qam_r0.5_a1.0_rx1", 15


@pytest.fixture(autouse=True)
def own_choice_of_width(monkeypatch):
    monkeypatch.delenv("MI_LTE_PUSCH_THREADS", raising=False)


class MmseRun(Run):
    """test_pusch_rxdiv_gpu.Run with the equaliser as a setting of the run: {.., nu} and the launched kernel's name checked"""

    def run(self, gain=0.0, noise=SCALE, eq=None):
        import openlte_amd as m
        eq = m.EQ_MMSE if eq is None else eq
        self.plan.set_demapper(m.DEMAP_MAXLOG, gain)
        self.plan.set_llr_noise(noise)
        self.plan.set_equaliser(eq)
        assert self.plan.equaliser() == eq
        st, _ = self.plan.run(self.d_sub)
        self.kernels = self.ctx.last_kernels()
        want = "k_pusch_demod_llr_mmse:1," if eq == m.EQ_MMSE else "k_pusch_demod_llr_rx:1," if self.n_rx > 1 else "k_pusch_demod_llr:1,"
        assert self.kernels.startswith(want), self.kernels
        out = {"x": [self.plan.llr_symbols(a) for a in range(self.n)], "rho": self.plan.llr_rho(), "s2": self.plan.llr_noise(),
               "g": self.plan.llr_gain(), "e": [self.plan.soft_bits(a) for a in range(self.n)], "st": st}
        if eq == m.EQ_MMSE:
            out["nu"] = self.plan.llr_nu()
        return out


def plans_of(n_rx):
    """the row's sizes as plans: 1 and 8 PRB share one (192 threads, M = 12 under a wavefront, M_max > M, NaN in a spare unit), every other
    size has a plan of its own so that M_max, and with it the width, S_par and the LDS, is its own"""
    keys = mm.gpu_keys(n_rx)
    return [keys[:2]] + [(k,) for k in keys[2:]]


def test_sizes_sit_on_the_steps():
    """the table's sizes are sizes a plan takes and cover what they are there for: the width step 8 | 9, the S_par steps 16 | 18 and
    35 | 36 (and 70 | 72 on one and two antennas), a generic radix (94 = 2 x 47), the largest size; on four antennas the LDS-forced steps
    65 | 66 and 70 | 72 and the last 64QAM size admitted, 76"""
    assert pc.threads(96) == 192 and pc.threads(108) == 256
    assert all(n == 1 or n in pc.planned_sizes() for sizes in mm.GPU_SIZES.values() for n in sizes)
    assert 17 not in pc.planned_sizes() and 71 not in pc.planned_sizes()
    for n_rx in (1, 2):
        S = [mm.launch(n_rx, 12 * n, rxm.words(n, QM[k[3]]))[3] for n, k in zip(mm.GPU_SIZES[n_rx], mm.gpu_keys(n_rx))]
        assert S == [12, 12, 12, 12, 6, 6, 3, 3, 2, 2, 2], (n_rx, S)
    keys = mm.gpu_keys(4)
    S = [mm.launch(4, 12 * n, rxm.words(n, QM[k[3]]))[3] for n, k in zip(mm.GPU_SIZES[4], keys)]
    assert S == [12, 12, 12, 12, 6, 6, 3, 3, 2, 2, 1, 1], S
    assert all(k[3] == 3 for k in keys if k[0] in (65, 66, 70, 71, 76)) and mm.launch(4, 12 * 78, rxm.words(78, 6))[0] == 0
    assert 47 in [R for R, _ in pc.radix_plan(94)] and 99 == max(pc.planned_sizes())


@pytest.mark.parametrize("n_rx", [1, 2, 4])
def test_taps_and_bytes_against_the_model(ctx, n_rx):
    """Taps: x against the model by the tight gate, nu_s, the rho tap (float)(s2 w_s) and sigma2 to 1e-4, the gain exactly (float)scale.
    Bytes: every byte against pusch_demod_model.demap_mmse on the run's own (x, nu_s) -- none differs outside the guard band, at most one step
    inside it, the band under 1 % of the soft bits (test_pusch_llr_gpu's comparison).  A second run gives the same bytes and taps."""
    all_keys = mm.gpu_keys(n_rx)
    gates = mm.gates(all_keys)
    assert gates[0] <= pc.TOL_SYMB and gates[1] <= 10 * pc.TOL_SYMB
    worst = {"l2": 0.0, "el": 0.0, "nu": 0.0, "rho": 0.0, "s2": 0.0}
    n_guard = n_all = n_diff = 0
    bad = []
    for keys in plans_of(n_rx):
        r = MmseRun(ctx, [mm.case(*k) for k in keys], n_rx, spare=1 if len(keys) > 1 else 0)
        out, again = r.run(), r.run()
        r.close()
        assert all(x.tobytes() == y.tobytes() for key in ("x", "e") for x, y in zip(out[key], again[key]))
        assert all(out[key].tobytes() == again[key].tobytes() for key in ("nu", "rho", "s2", "g", "st"))
        for a, k in enumerate(keys):
            c, want = mm.case(*k), mm.expected(k)
            got = out["x"][a]
            assert got.shape == (12, c.M) and got.dtype == np.complex64 and np.isfinite(got).all(), k
            l2, el = pc.errors(got, want["x"])
            d_nu = float((np.abs(out["nu"][a].astype(np.float64) - want["nu"]) / want["nu"]).max())
            d_rho = float((np.abs(out["rho"][a].astype(np.float64) - want["rho"]) / want["rho"]).max())
            d_s2 = abs(float(out["s2"][a]) - want["s2"]) / want["s2"]
            print("%d PRB x %d antennas, Q_m %d: rel-L2 %.3g, elementwise / RMS %.3g (gates %.3g / %.3g); nu off by %.3g, the rho tap by %.3g, sigma2 by %.3g; nu %.3g .. %.3g"
                  % (c.n_prb, n_rx, QM[k[3]], l2.max(), el.max(), gates[0], gates[1], d_nu, d_rho, d_s2, out["nu"][a].min(), out["nu"][a].max()))
            for key, v in (("l2", l2.max()), ("el", el.max()), ("nu", d_nu), ("rho", d_rho), ("s2", d_s2)):
                worst[key] = max(worst[key], float(v))
            if not ((l2 < gates[0]).all() and (el < gates[1]).all() and d_nu <= 1e-4 and d_rho <= 1e-4 and d_s2 <= 1e-4):
                bad.append((k, float(l2.max()), float(el.max()), d_nu, d_rho, d_s2))
            assert out["g"][a] == np.float32(SCALE), (k, out["g"][a])
            assert (out["rho"][a] >= np.float32(want["rho_zf"] * (1 - 1e-4))).all(), k
            model = mm.demap(got, out["nu"][a], k[3], c.c_init, SCALE)
            e = out["e"][a]
            assert len(e) == len(model.bytes) == 144 * c.n_prb * QM[k[3]]
            d = np.abs(e.astype(np.int32) - model.bytes)
            guard = dm.in_guard(model.x)
            print("    %d soft bits, %d in the guard band, %d differ (%d outside it), %d distinct values"
                  % (len(e), guard.sum(), (d != 0).sum(), (d[~guard] != 0).sum(), len(np.unique(e))))
            assert not d[~guard].any() and d.max() <= 1, k
            assert len(np.unique(e)) > 32 or c.n_prb == 1, k  # graded bytes
            n_guard, n_all, n_diff = n_guard + int(guard.sum()), n_all + len(e), n_diff + int((d != 0).sum())
    print("%d antennas: worst rel-L2 %.3g, elementwise / RMS %.3g, nu %.3g, rho tap %.3g, sigma2 %.3g; %d of %d bytes differ from the exact layer, %d in the guard band"
          % (n_rx, worst["l2"], worst["el"], worst["nu"], worst["rho"], worst["s2"], n_diff, n_all, n_guard))
    assert not bad, bad
    assert n_guard < 0.01 * n_all


@pytest.mark.parametrize("n_rx", [1, 2, 4])
def test_flat_planes_give_zero_forcings_bytes(ctx, n_rx):
    """P the same on every sub-carrier (pusch_demod_cases.flat_case; QPSK on 1 PRB, 16QAM on 6, 64QAM on 10): the MMSE bytes against the
    zero-forcing noise-referenced run of the same plan -- no byte differs by more than 1, at most 0.5 % differ.  The cap is a condition:
    test_pusch_mmse_cpu shows that the two float64 models differ in no byte on these planes."""
    import openlte_amd as m
    keys = FLAT_KEYS[n_rx]
    r = MmseRun(ctx, [mm.flat_case(*k) for k in keys], n_rx, spare=1)
    zf, mmse = r.run(eq=m.EQ_ZF), r.run(eq=m.EQ_MMSE)
    r.close()
    n_diff = n_all = 0
    for a, k in enumerate(keys):
        d = np.abs(zf["e"][a].astype(np.int32) - mmse["e"][a].astype(np.int32))
        print("flat, %d PRB x %d antennas, Q_m %d: %d of %d bytes differ, largest step %d; nu %.4g, rho tap / rho %.8g, %d distinct values"
              % (k[0], n_rx, QM[k[3]], (d != 0).sum(), len(d), d.max(), mmse["nu"][a][0], (mmse["rho"][a] / zf["rho"][a]).max(), len(np.unique(mmse["e"][a]))))
        assert d.max() <= 1 and len(np.unique(mmse["e"][a])) > 32, k
        assert np.abs(mmse["rho"][a] / zf["rho"][a] - 1).max() <= 1e-5 and mmse["s2"][a] == zf["s2"][a], k
        n_diff, n_all = n_diff + int((d != 0).sum()), n_all + len(d)
    print("flat planes, %d antennas: %d of %d bytes differ (%.4f %%)" % (n_rx, n_diff, n_all, 100.0 * n_diff / n_all))
    assert n_diff <= 0.005 * n_all


@pytest.mark.parametrize("n_rx,gain,noise", [(1, 0.0, 0.0), (1, 1.5, 0.0), (1, 0.0, SCALE), (2, 0.0, 0.0), (2, 0.0, SCALE)],
                         ids=["llr_auto", "llr_fixed", "llr_noise", "rx2_auto", "rx2_noise"])
def test_setter_is_inert_at_zero_forcing(ctx, n_rx, gain, noise):
    """A plan that never saw the setter, and a plan run, set to MMSE (and run so where the run is admitted) and set back: the bytes, the
    taps and the launched kernels' names of the plan's run before."""
    import openlte_amd as m
    keys = tuple((n, n_rx, 7, mod) for n, mod in ((1, 1), (6, 2), (25, 3)))
    cases = [mm.case(*k) for k in keys]

    def run_of(r):
        r.plan.set_demapper(m.DEMAP_MAXLOG, gain)
        r.plan.set_llr_noise(noise)
        st, _ = r.plan.run(r.d_sub)
        return {"k": ctx.last_kernels(), "x": [r.plan.llr_symbols(a).tobytes() for a in range(r.n)], "e": [r.plan.soft_bits(a).tobytes() for a in range(r.n)],
                "t": [r.plan.llr_rho().tobytes(), r.plan.llr_noise().tobytes(), r.plan.llr_gain().tobytes(), st.tobytes()]}

    never, other = Run(ctx, cases, n_rx), Run(ctx, cases, n_rx)
    want, before = run_of(never), run_of(other)
    assert want == before and want["k"].startswith("k_pusch_demod_llr_rx:1," if n_rx > 1 else "k_pusch_demod_llr:1,")
    assert ctx.L.mi_lte_pusch_plan_llr_nu(other.plan.h, C.byref(C.c_void_p())) == ERR_INVALID  # (no tap before MMSE is first set)
    other.plan.set_equaliser(m.EQ_MMSE)
    assert other.plan.equaliser() == m.EQ_MMSE and not other.plan.llr_nu().any()
    if noise:
        st, _ = other.plan.run(other.d_sub)
        assert ctx.last_kernels().startswith("k_pusch_demod_llr_mmse:1,") and other.plan.llr_nu().all()
        assert [other.plan.soft_bits(a).tobytes() for a in range(other.n)] != want["e"]
    other.plan.set_equaliser(m.EQ_ZF)
    assert other.plan.equaliser() == m.EQ_ZF and run_of(other) == want and run_of(never) == want
    never.close()
    other.close()


def test_degenerate_grids(ctx):
    """Zero grids: every byte 0, the gain 0, status 2, and the plan decodes again.  One live antenna among zero grids: the taps of the
    live antenna's single-antenna MMSE run at half (a quarter of) its sigma2, i.e. not its bytes but the model's on those taps.  A
    constant channel so small that the second differences' squares leave the float range: sigma2 = 0 with P > 0 -- all-zero bytes, status 2."""
    keys = tuple((n, 2, 8, mod) for n, mod in ((1, 1), (6, 2), (25, 3)))
    cases = [mm.case(*k) for k in keys]
    zero = np.zeros((2, 16, pm.N_SC), np.float32)
    r = MmseRun(ctx, cases, 2)
    lit = r.run()
    dark = ctx.alloc(r.d_sub.nbytes)
    dark.zero()
    keep, r.d_sub = r.d_sub, dark
    nothing = r.run()
    assert not nothing["g"].any() and not any(e.any() for e in nothing["e"]) and (nothing["st"] == 2).all() and not nothing["s2"].any()
    r.d_sub = keep
    dark.free()
    back = r.run()
    assert all(x.tobytes() == y.tobytes() for x, y in zip(back["e"], lit["e"]))
    r.close()
    for n_rx, live in ((2, 1), (4, 2)):
        planes = [[c.planes[0] if a == live else zero for a in range(n_rx)] for c in cases]
        r = MmseRun(ctx, cases, n_rx, planes=planes)
        out = r.run()
        r.close()
        for a, (k, c) in enumerate(zip(keys, cases)):
            want = mm.taps(planes[a], c.al, c.dmrs)
            alone = mm.taps([c.planes[0]], c.al, c.dmrs)
            assert np.isclose(want["s2"], alone["s2"] / n_rx, rtol=1e-12)
            l2, el = pc.errors(out["x"][a], want["x"])
            d_nu = float((np.abs(out["nu"][a] - want["nu"]) / want["nu"]).max())
            print("antenna %d of %d alive, %d PRB: rel-L2 %.3g, elementwise %.3g, nu off by %.3g, sigma2 by %.3g"
                  % (live, n_rx, k[0], l2.max(), el.max(), d_nu, abs(out["s2"][a] / want["s2"] - 1)))
            assert (l2 < pc.TOL_SYMB).all() and (el < 10 * pc.TOL_SYMB).all() and d_nu <= 1e-4 and abs(out["s2"][a] / want["s2"] - 1) <= 1e-4
            model = mm.demap(out["x"][a], out["nu"][a], k[3], c.c_init, SCALE)
            d = np.abs(out["e"][a].astype(np.int32) - model.bytes)
            assert not d[~dm.in_guard(model.x)].any() and d.max() <= 1
    tiny = []
    for c in cases:
        p = np.array(c.planes[0]) * np.float32(2.0 ** -56)
        for b, L in ((0, 3), (1, 10)):
            sc = pm.subcarriers(c.al, b)
            p[0, L, sc], p[1, L, sc] = c.dmrs[2 * b] * np.float32(2.0 ** -56), c.dmrs[2 * b + 1] * np.float32(2.0 ** -56)
        tiny.append([p])
    r = MmseRun(ctx, cases, 1, planes=tiny)
    out = r.run()
    r.close()
    print("constant channel 2^-56: sigma2 %s, rho tap %s, nu %s" % (out["s2"], out["rho"][0][:3], out["nu"][0][:3]))
    assert not out["s2"].any() and not out["g"].any() and not any(e.any() for e in out["e"]) and (out["st"] == 2).all()


def test_refusals_leave_the_plan_runnable(ctx):
    """INVALID_ARG: a NULL plan, an unknown mode, NULL outputs of the getters, the nu tap before MMSE was ever set.  UNSUPPORTED: a
    reference-mode plan, for any mode (INVALID_ARG winning for an unknown one), whose nu tap stays refused.  A run or HARQ run with MMSE set
    under the default demapper or without the noise gain names its reason and launches nothing; the plan runs again once either changes."""
    import openlte_amd as m
    L = ctx.L
    keys = tuple((n, 1, 9, mod) for n, mod in ((6, 1), (25, 2)))
    r = MmseRun(ctx, [mm.case(*k) for k in keys], 1)
    want = r.run()

    def same():
        got = r.run()
        assert all(x.tobytes() == y.tobytes() for x, y in zip(got["e"], want["e"])) and got["nu"].tobytes() == want["nu"].tobytes()

    mode, p = C.c_uint32(), C.c_void_p()
    assert L.mi_lte_pusch_plan_set_equaliser(None, 1) == ERR_INVALID
    for bad in (2, 3, 0xFFFFFFFF):
        assert L.mi_lte_pusch_plan_set_equaliser(r.plan.h, bad) == ERR_INVALID and r.plan.equaliser() == m.EQ_MMSE
    assert L.mi_lte_pusch_plan_equaliser(None, C.byref(mode)) == ERR_INVALID and L.mi_lte_pusch_plan_equaliser(r.plan.h, None) == ERR_INVALID
    assert L.mi_lte_pusch_plan_llr_nu(None, C.byref(p)) == ERR_INVALID and L.mi_lte_pusch_plan_llr_nu(r.plan.h, None) == ERR_INVALID
    same()
    d_out, d_st = ctx.alloc(r.plan.n_alloc * r.plan.out_stride), ctx.alloc(4 * r.plan.n_alloc)
    pool = ctx.harq_pool(2)
    bind = C.cast(m.harq_binds(r.plan.n_alloc, [0, 1], True), C.c_void_p)
    for what, undo in ((lambda: r.plan.set_demapper(m.DEMAP_REF), lambda: r.plan.set_demapper(m.DEMAP_MAXLOG, 0.0)),
                       (lambda: r.plan.set_llr_noise(0.0), lambda: r.plan.set_llr_noise(SCALE))):
        what()
        before = ctx.last_kernels()
        assert L.mi_lte_pusch_decode_run(ctx.h, r.plan.h, r.d_sub.ptr, d_out.ptr, d_st.ptr) == ERR_UNSUPPORTED
        assert b"MMSE" in L.mi_lte_last_error(ctx.h) and ctx.last_kernels() == before
        assert L.mi_lte_pusch_decode_run_harq(ctx.h, r.plan.h, pool.h, bind, r.d_sub.ptr, d_out.ptr, d_st.ptr) == ERR_UNSUPPORTED
        assert b"MMSE" in L.mi_lte_last_error(ctx.h) and ctx.last_kernels() == before
        r.plan.set_equaliser(m.EQ_ZF)  # either setting makes it runnable: the equaliser ..
        assert L.mi_lte_pusch_decode_run(ctx.h, r.plan.h, r.d_sub.ptr, d_out.ptr, d_st.ptr) == 0 and ctx.last_kernels().startswith("k_pusch_demod")
        ctx.sync()
        r.plan.set_equaliser(m.EQ_MMSE)
        assert L.mi_lte_pusch_decode_run(ctx.h, r.plan.h, r.d_sub.ptr, d_out.ptr, d_st.ptr) == ERR_UNSUPPORTED
        undo()                          # .. or the demapper / the noise gain
        assert L.mi_lte_pusch_decode_run(ctx.h, r.plan.h, r.d_sub.ptr, d_out.ptr, d_st.ptr) == 0 and ctx.last_kernels().startswith("k_pusch_demod_llr_mmse:1,")
        ctx.sync()
        same()
    pool.close()
    d_out.free()
    d_st.free()
    cfg, ul = m.DlCfg(2048, pc.N_RB, 1, 0), m.UlCfg(*pc.ULC)
    ref_plan = ctx.pusch_plan(cfg, ul, [mm.case(*keys[0]).sf], [pc.CELL], [r.allocs[0]])
    ref_plan.run(r.d_sub)
    e0 = ref_plan.soft_bits(0)
    for md in (0, 1):
        assert L.mi_lte_pusch_plan_set_equaliser(ref_plan.h, md) == ERR_UNSUPPORTED
    assert L.mi_lte_pusch_plan_set_equaliser(ref_plan.h, 2) == ERR_INVALID and ref_plan.equaliser() == m.EQ_ZF
    assert L.mi_lte_pusch_plan_llr_nu(ref_plan.h, C.byref(p)) == ERR_INVALID
    ref_plan.run(r.d_sub)
    assert ctx.last_kernels().startswith("k_pusch_demod:1,") and (ref_plan.soft_bits(0) == e0).all()
    ref_plan.close()
    same()
    r.close()


# ---- through the multipath generator

class PathUnits(RxUnits):
    """test_pusch_rxdiv_gpu.RxUnits through the multipath generator (PATHS; every antenna its own phases through its own seed)"""

    def __init__(self, ctx, n_rb, sfs, cell, allocs, n_rx, snr_db, seed, payload=None, ucis=None, ctrl=None, spare=0):
        kw = dict(ctrl or {})
        kw["paths"] = PATHS
        if ucis is None:  # (RxUnits passes ctrl on only with descriptors: the paths ride in their place)
            import openlte_amd as m
            from openlte_amd import synth
            from test_ulsch3gpp_gpu import FFT, ULC
            self.ctx, self.cfg, self.ul = ctx, m.DlCfg(FFT[n_rb], n_rb, 1, 0), m.UlCfg(*ULC)
            self.sfs, self.cells, self.allocs, self.ucis, self.n_rx = list(sfs), [cell] * len(sfs), allocs, None, n_rx
            self.stride = len(sfs) + spare
            iq, self.tx = synth.ul_units_3gpp_rx(self.cfg, self.ul, self.sfs, self.cells, allocs, 1, n_rx, ant_stride=self.stride, seed=seed,
                                                 payload=payload, max_delay=3, snr_db=snr_db, peak=100.0, paths=PATHS)
            _, self.d_sub = ctx.ul_frontend(self.cfg, iq.reshape(-1, 2), np.arange(iq.shape[0]) * iq.shape[1], keep=True)
        else:
            RxUnits.__init__(self, ctx, n_rb, sfs, cell, allocs, n_rx, snr_db, seed, payload=payload, ucis=ucis, ctrl=kw, spare=spare)


def mmse_plan(un):
    import openlte_amd as m
    p = un.plan()
    p.set_llr_noise(SCALE)
    p.set_equaliser(m.EQ_MMSE)
    return p


def test_transport_blocks_through_two_paths(ctx):
    """Two equal-power paths at 30 dB, 100-RB cell: 64QAM on 96 PRB in thirteen code blocks on two antennas, and a single-antenna 16QAM
    grant on 10 PRB: status 0 and the sent bits."""
    import openlte_amd as m
    from test_dlsch3gpp_gpu import tbs
    wide = [m.make_alloc(0, 3, tbs(26, 99), list(range(2, 98)), 0x301)]
    assert m.ulsch_layout(wide[0].tbs, 0, 2)["C"] == 13 and wide[0].N_prb == 96
    for allocs, n_rx, sfs in ((wide, 2, [3]), ([grant(0, 2, 15, 10, 40, 0x302)], 1, [8])):
        un = PathUnits(ctx, 100, sfs, 17, allocs, n_rx, 30.0, seed=300 + n_rx, spare=1)
        plan = mmse_plan(un)
        st, bits = plan.run(un.d_sub)
        assert ctx.last_kernels().startswith("k_pusch_demod_llr_mmse:1,k_dl3_desc:1,"), ctx.last_kernels()
        print("%d antennas, %d PRB: status %s, nu %.3g .. %.3g" % (n_rx, allocs[0].N_prb, list(st), plan.llr_nu().min(), plan.llr_nu().max()))
        assert (st == 0).all() and all((bits[a] == un.tx[a, 0, :al.tbs]).all() for a, al in enumerate(allocs))
        plan.close()
        un.free()


def test_control_information_through_two_paths(ctx):
    """A plan with control information on two antennas at 30 dB through two paths, MMSE: the sent HARQ-ACK and RI bits, the sent 5-bit CQI
    report from the device's decoder, and the transport blocks."""
    import openlte_amd as m
    o = np.array([1, 0, 1, 1, 0], np.uint8)
    gs = [Grant(2, tbs_at_most(6, 1000), 6, 0, 0x211, uci(1, 8, 1, 4, 40), [1], [1], seed=21),
          Grant(3, tbs_at_most(10, 3000), 10, 8, 0x212, uci(2, 12, 2, 6, 0), [1, 0], [0, 1], seed=22),
          Grant(1, tbs_at_most(2, 150), 2, 20, 0x213)]
    gs[0].cqi = m.cqi_encode(5, o, 40)
    allocs = [m.make_alloc(k, g.mod, g.tbs, list(range(g.prb0, g.prb0 + g.n_prb)), g.rnti, rv_idx=g.rv) for k, g in enumerate(gs)]
    un = PathUnits(ctx, 25, [1, 4, 7], 33, allocs, 2, 30.0, seed=310, ucis=[g.u for g in gs],
                   ctrl=dict(ack=[g.ack for g in gs], ri=[g.ri for g in gs], cqi=[g.cqi for g in gs]))
    plan = mmse_plan(un)
    plan.set_cqi_decode([5, 0, 0])
    st, bits = plan.run(un.d_sub)
    assert ctx.last_kernels().startswith("k_pusch_demod_llr_mmse:1,k_ulsch_uci_gather:1,k_ulsch_uci_decide:1,k_ulsch_cqi_decode:1,k_dl3_desc:1,")
    rec, cqi = plan.uci_results(), plan.cqi_results()
    for k, g in enumerate(gs):
        print("alloc %d: status %d, ack %s ri %s" % (k, st[k], rec[k]["ack"], rec[k]["ri"]))
        assert st[k] == 0 and (bits[k] == un.tx[k, 0, :g.tbs]).all(), k
        assert list(rec[k]["ack"])[:g.u.O_ack] == g.ack and list(rec[k]["ri"])[:g.u.O_ri] == g.ri, (k, rec[k])
    assert cqi[0]["O"] == 5 and cqi[0]["bits"] == pack_bits(o) and cqi[0]["crc"] in (NO_CRC, CRC_OK), cqi[0]
    plan.close()
    un.free()


def test_harq_pair_equalised_either_way(ctx):
    """Two transmissions of a code rate above 1 through two paths at 30 dB (16QAM on 10 PRB, rv 0 then rv 2, two antennas): the first
    equalised zero-forcing under the noise-referenced gain, the second MMSE -- one scale: neither returns the sent bits alone, combined
    they do."""
    import openlte_amd as m
    from test_dlsch3gpp_cpu import tbs_table
    G = 144 * 10 * 4
    size = min((int(s) for s in tbs_table()[:, 9] if s + 24 <= 6144), key=lambda s: abs(G / (s + 24) - 0.95))
    assert 0.9 <= G / (size + 24) < 1.0
    pool = ctx.harq_pool(2)
    payload = None
    for k, rv in enumerate((0, 2)):
        allocs = [m.make_alloc(0, 2, size, list(range(5, 15)), 0x401, rv_idx=rv), m.make_alloc(1, 2, size, list(range(30, 40)), 0x402, rv_idx=rv)]
        un = PathUnits(ctx, 100, [2, 6], 222, allocs, 2, 30.0, seed=320 + k, payload=payload)
        payload = un.tx
        plan = un.plan()
        plan.set_llr_noise(SCALE)
        plan.set_equaliser(m.EQ_MMSE if k else m.EQ_ZF)
        plain = decode(un, plan)
        assert plain["kernels"].startswith("k_pusch_demod_llr_mmse:1," if k else "k_pusch_demod_llr_rx:1,")
        print("transmission %d alone: status %s" % (k, list(plain["st"])))  # (fewer soft bits than payload bits: it cannot return them)
        assert not any((plain["rows"][a, :size] == un.tx[a, 0, :size]).all() for a in range(2))
        h = decode(un, plan, pool, [0, 1], k == 0)
        assert h["kernels"].startswith("k_pusch_demod_llr_mmse:1," if k else "k_pusch_demod_llr_rx:1,")
        if k == 1:
            assert (h["st"] == 0).all(), h["st"]
            assert all((h["rows"][a, :size] == un.tx[a, 0, :size]).all() for a in range(2))
            assert all(pool.state(a)["n_tx"] == 2 for a in range(2))
        plan.close()
        un.free()
    pool.close()


def test_value(ctx):
    """The curve VALUE_CLASS of profiles/pusch_mmse_sweep.txt at VALUE_SNR_DB (16 transport blocks, the sweep's seeds): MMSE decodes at
    least as many blocks -- status 0, the payload equal to the transmitted bits -- as zero forcing under the noise-referenced gain on the
    same captures, and strictly more.  Measured in the sweep: 16 of 16 against 0."""
    import pusch_mmse_sweep as sw
    p = sw.Point(ctx, VALUE_CLASS, float(VALUE_SNR_DB), 16)
    n = {mode: int(p.decoded(mode).sum()) for mode in ("zf", "mmse")}
    p.close()
    print("%s at %d dB: %s of 16 transport blocks decoded" % (VALUE_CLASS, VALUE_SNR_DB, n))
    assert n["mmse"] > n["zf"], n
