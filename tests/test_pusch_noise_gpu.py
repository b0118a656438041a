"""GPU: the DMRS noise estimate of k_pusch_demod_llr and the noise-referenced gain built on it (mi_lte_pusch_plan_set_llr_noise,
mi_lte_pusch_plan_llr_noise).  sigma2_a against the float64 restatement of include/mi_lte.h's text (tests/pusch_demod_model.py) on the
front end's planes; the gain exactly (float)(scale / tap); the bytes by test_pusch_llr_gpu's rules with the tapped gain in pusch_demod_model's
demap(); a plan that turns the setter on and off again is the plan it was; the estimate moves by 10 dB when the noise does; control
information and the CQI decoder take the bytes as they take any other; the edges and refusals of the header."""
import ctypes as C

import numpy as np
import pytest

import demap_llr_model as dm
import pusch_demod_model as nm
import pusch_demod_model as pm
from test_pusch_llr_gpu import CASES, SNRS, c_init, outputs, same_outputs, units_of
from test_ulsch3gpp_gpu import FFT, QM, ULC, grant
from test_ulsch_cqi_cpu import ZERO, model as cqi_model
from test_ulsch_uci_gpu import UciUnits, check_gather_and_sums, exact_grants

pytestmark = pytest.mark.gpu

ERR_INVALID, ERR_UNSUPPORTED = -1, -4


def scale_of(snr_db):
    """`scale` times the LLR in natural units meets the int8 clamp at an LLR of 127 / scale.  The header's starting point 8 clamps at 16: at
    20 dB most 64QAM amplitude bits stay under that (a whole decision interval is (2 A)^2 / sigma^2 ~ 10) and every sign bit of an outer
    point is far over it.  At 5 dB an LLR of 16 is a three-sigma event of an outermost point, too rare to demand of a 24-PRB plan, so the
    5 dB plans run at 32 (clamp at an LLR of 4)."""
    return 8.0 if snr_db >= 10 else 32.0


def planes_of(un):
    return un.d_sub.download(np.float32).reshape(len(un.sfs), 2, 16, pm.N_SC)


def model_sigma2(un, planes):
    import openlte_amd as m
    return np.array([nm.sigma2(planes[al.unit], al, m.ul_dmrs_pusch(un.ul, un.cells[al.unit], un.sfs[al.unit], al.N_prb)) for al in un.allocs])


def noise_plan(un, scale):
    import openlte_amd as m
    plan = un.plan()
    plan.set_demapper(m.DEMAP_MAXLOG, 0.0)
    plan.set_llr_noise(scale)
    return plan


def test_sigma2_tap_against_the_model(ctx):
    """Plans A-E at 20 and 5 dB: the tap against the float64 restatement, relative difference <= 1e-4 -- the bound of
    test_rho_against_the_float64_restatement, for its reason: the kernel's float error per term is a few ulp of |t| (6e-8 each, forming
    t, its magnitude, its unit vector and their product), the differences and the sum are in double, and a second difference of noise at
    5 .. 20 dB is 0.1 .. 1 times |t|, so the float error stays under 1e-5 of it.  No allocation is left out."""
    worst = 0.0
    for name in CASES:
        for snr_db in SNRS:
            un = units_of(ctx, name, snr_db)
            want = model_sigma2(un, planes_of(un))
            plan = noise_plan(un, 8.0)
            plan.run(un.d_sub)
            got = plan.llr_noise()
            rel = np.abs(got.astype(np.float64) - want) / want
            for a, al in enumerate(un.allocs):
                print("%s %2.0f dB allocation %d (%3d PRB): sigma2 %.6g, model %.6g, relative difference %.3g" % (name, snr_db, a, al.N_prb, got[a], want[a], rel[a]))
            assert (want > 0).all() and (rel <= 1e-4).all(), (name, snr_db, rel)
            worst = max(worst, float(rel.max()))
            plan.close()
            un.free()
    print("sigma2: largest relative difference %.3g" % worst)


def check_bytes(plan, un, gains):
    """test_pusch_llr_gpu.check_against_model's rules with one gain per allocation: identical to the model outside the guard band, at most one
    step inside it, the band under 1 % of the soft bits.  Returns every byte of the plan."""
    import openlte_amd as m
    rho = plan.llr_rho()
    n_guard = n_all = 0
    every = []
    for a, al in enumerate(un.allocs):
        e, xs = plan.soft_bits(a), plan.llr_symbols(a)
        assert xs.shape == (12, 12 * al.N_prb) and np.isfinite(xs).all() and (rho[a] > 0).all(), a
        r = pm.demap(xs, rho[a], al.mod_type, c_init(un, a), gain=float(gains[a]), T=m.DEMAP_AUTO_T)
        assert len(e) == len(r.bytes) == 144 * al.N_prb * QM[al.mod_type], (a, len(e))
        assert r.gain == float(gains[a])
        d = np.abs(e.astype(np.int32) - r.bytes)
        guard = dm.in_guard(r.x)
        print("allocation %d (%d PRB, Q_m %d): %d soft bits, %d in the guard band, %d differ (%d of them outside it), largest difference %d; gain %.9g"
              % (a, al.N_prb, QM[al.mod_type], len(e), guard.sum(), (d != 0).sum(), (d[~guard] != 0).sum(), d.max(), gains[a]))
        assert not d[~guard].any(), (a, int((d[~guard] != 0).sum()))
        assert d.max() <= 1, a
        n_guard += int(guard.sum())
        n_all += len(e)
        every.append(e)
    assert n_guard < 0.01 * n_all, (n_guard, n_all)
    return np.concatenate(every)


@pytest.mark.parametrize("snr_db", SNRS)
@pytest.mark.parametrize("name", CASES)
def test_gain_and_bytes(ctx, name, snr_db):
    """llr_gain is (float)(scale / tap) exactly, whatever gain set_demapper was given (automatic, then a fixed 3.0); the bytes obey the
    model's rules with the tapped gain; clamped and graded bytes are both present; two runs give identical bytes and taps."""
    import openlte_amd as m
    un = units_of(ctx, name, snr_db)
    scale = scale_of(snr_db)
    plan = noise_plan(un, scale)
    plan.set_llr_tap(True)
    n = len(un.allocs)
    first = None
    for fixed in (0.0, 3.0):
        plan.set_demapper(m.DEMAP_MAXLOG, fixed)
        plan.run(un.d_sub)
        assert ctx.last_kernels().startswith("k_pusch_demod_llr:1,k_dl3_desc:1,k_dl3_rm_i8:1,")
        s2, g = plan.llr_noise(), plan.llr_gain()
        want_g = np.array([nm.gain(scale, v) for v in s2], np.float32)
        assert (s2 > 0).all() and (g > 0).all() and g.tobytes() == want_g.tobytes(), (s2, g, want_g)
        e = [plan.soft_bits(a) for a in range(n)]
        if first is None:
            every = check_bytes(plan, un, g)
            n_clamped, n_graded = int((np.abs(every.astype(int)) == 127).sum()), int((np.abs(every.astype(int)) < 127).sum())
            print("%s %2.0f dB scale %g: %d clamped and %d graded bytes" % (name, snr_db, scale, n_clamped, n_graded))
            assert n_clamped > 0 and n_graded > 0
            first = (e, s2, g, plan.llr_rho())
        else:  # the gain handed to set_demapper is out of play
            assert all(x.tobytes() == y.tobytes() for x, y in zip(e, first[0]))
        plan.run(un.d_sub)
        assert all(plan.soft_bits(a).tobytes() == first[0][a].tobytes() for a in range(n))
        assert plan.llr_noise().tobytes() == first[1].tobytes() and plan.llr_gain().tobytes() == first[2].tobytes()
        assert plan.llr_rho().tobytes() == first[3].tobytes()
    plan.close()
    un.free()


class FlatUnits:
    """One 100-RB unit, 50 PRB of QPSK, through a channel of unit gain (a random phase and a delay of up to 3 samples stay)"""

    def __init__(self, ctx, snr_db, seed):
        import openlte_amd as m
        from openlte_amd import synth
        self.ctx, self.cfg, self.ul = ctx, m.DlCfg(FFT[100], 100, 1, 0), m.UlCfg(*ULC)
        self.sfs, self.cells, self.allocs = [4], [211], [grant(0, 1, 9, 50, 20, 0xC1)]
        iq, self.tx = synth.ul_units_3gpp(self.cfg, self.ul, self.sfs, self.cells, self.allocs, 1, gain=(1.0, 1.0), max_delay=3, snr_db=snr_db,
                                          peak=100.0, seed=seed)
        _, self.d_sub = ctx.ul_frontend(self.cfg, iq.reshape(-1, 2), [0], keep=True)

    def plan(self):
        return self.ctx.pusch_plan_3gpp(self.cfg, self.ul, self.sfs, self.cells, self.allocs)

    def free(self):
        self.d_sub.free()


def test_physical_sanity_ten_db(ctx):
    """The same seed at 5 and at 15 dB: with P = mean |t|^2 - sigma2 from the model's own t, (sigma2 / P) at 5 dB over (sigma2 / P) at
    15 dB lies within 10 [0.75, 1.25] (the ratio's standard deviation from the CPU spread at 50 PRB is 6 %), for the kernel's tap."""
    import openlte_amd as m
    inv_snr = []
    for snr_db in (5.0, 15.0):
        un = FlatUnits(ctx, snr_db, seed=77)
        al = un.allocs[0]
        t = nm.t_ls(planes_of(un)[0], al, m.ul_dmrs_pusch(un.ul, un.cells[0], un.sfs[0], al.N_prb))
        plan = noise_plan(un, 8.0)
        plan.run(un.d_sub)
        s2 = float(plan.llr_noise()[0])
        assert abs(s2 - nm.sigma2_t(t)) <= 1e-4 * nm.sigma2_t(t)
        P = float((np.abs(t) ** 2).mean()) - s2
        print("%2.0f dB: sigma2 %.6g, P %.6g, sigma2 / P = %.2f dB" % (snr_db, s2, P, 10 * np.log10(s2 / P)))
        assert P > 0
        inv_snr.append(s2 / P)
        plan.close()
        un.free()
    ratio = inv_snr[0] / inv_snr[1]
    print("ratio %.3f" % ratio)
    assert 7.5 <= ratio <= 12.5, ratio


def test_setter_on_then_off_is_inert(ctx):
    """A plan that never calls the setter and one that turns it on, runs and turns it off again: the MAXLOG bytes, rows, status, cb_ok, cb_soft
    and the gain and rho taps agree byte for byte; the run in between differs."""
    import openlte_amd as m
    un = units_of(ctx, "A", 9.0)
    plain, other = un.plan(), un.plan()
    for p in (plain, other):
        p.set_demapper(m.DEMAP_MAXLOG, 0.0)
    want = outputs(plain, un)
    g0, r0 = plain.llr_gain(), plain.llr_rho()
    assert not plain.llr_noise().any()
    other.set_llr_noise(8.0)
    mid = outputs(other, un)
    assert any((x != y).any() for x, y in zip(mid["e"], want["e"])) and (other.llr_noise() > 0).all()
    other.set_llr_noise(0.0)
    got = outputs(other, un)
    assert ctx.last_kernels().startswith("k_pusch_demod_llr:1,")
    assert same_outputs(got, want)
    assert other.llr_gain().tobytes() == g0.tobytes() and other.llr_rho().tobytes() == r0.tobytes()
    assert same_outputs(outputs(plain, un), want)
    for p in (plain, other):
        p.close()
    un.free()


def test_setter_waits_for_maxlog(ctx):
    """On a plan with the default demapper the setter changes nothing -- the same bytes, k_pusch_demod, a sigma2 tap of zeros -- until MAXLOG
    is chosen; then the run uses scale / sigma2."""
    import openlte_amd as m
    un = units_of(ctx, "B", 20.0)
    plain, plan = un.plan(), un.plan()
    want = outputs(plain, un)
    plan.set_llr_noise(8.0)
    got = outputs(plan, un)
    assert ctx.last_kernels().startswith("k_pusch_demod:1,")
    assert same_outputs(got, want) and not plan.llr_noise().any() and not plan.llr_gain().any()
    plan.set_demapper(m.DEMAP_MAXLOG, 0.0)
    plan.run(un.d_sub)
    assert ctx.last_kernels().startswith("k_pusch_demod_llr:1,")
    s2, g = plan.llr_noise(), plan.llr_gain()
    assert (s2 > 0).all() and g.tobytes() == np.array([nm.gain(8.0, v) for v in s2], np.float32).tobytes()
    for p in (plain, plan):
        p.close()
    un.free()


def test_control_information_and_cqi_decoder(ctx):
    """test_ulsch_uci_gpu's exact_grants under the noise-referenced gain with CQI decoding on: data_soft / cqi_soft, the sums and decided
    bits equal the numpy rules on the tapped soft bits; the CQI record equals mi_lte_cqi_decode_batch and the CPU model on the plan's own
    cqi_soft tap."""
    import openlte_amd as m
    grants = exact_grants()
    un = UciUnits(ctx, 25, 33, grants, 15.0, seed=41)
    plan = un.plan()
    plan.set_demapper(m.DEMAP_MAXLOG, 0.0)
    plan.set_llr_noise(8.0)
    plan.set_cqi_decode([0, 5, 0, 0, 0, 0])
    plan.run(un.d_sub)
    assert ctx.last_kernels().startswith("k_pusch_demod_llr:1,k_ulsch_uci_gather:1,k_ulsch_uci_decide:1,k_ulsch_cqi_decode:1,k_dl3_desc:1,"), ctx.last_kernels()
    s2, g = plan.llr_noise(), plan.llr_gain()
    assert (s2 > 0).all() and g.tobytes() == np.array([nm.gain(8.0, v) for v in s2], np.float32).tobytes()
    rec = plan.uci_results()
    graded = 0
    for k in range(len(grants)):
        check_gather_and_sums(un, plan, rec, k)
        graded += len(np.unique(np.abs(plan.soft_bits(k))))
    assert graded > 100
    got = plan.cqi_results()
    soft = plan.cqi_soft(1)
    assert len(soft) == 40
    batch = ctx.cqi_decode_batch(soft, [(0, 40, 5)])
    want = cqi_model([(soft, 5)])
    print("CQI record under the noise-referenced gain: %s" % got[1])
    assert got[1] == batch[0] == want[0] and got[1]["O"] == 5
    assert [got[k] for k in (0, 2, 3, 4, 5)] == [ZERO] * 5
    plan.close()
    un.free()


def test_zero_grid(ctx):
    """An all-zero grid: sigma2 = 0, g = 0, all-zero bytes, status 2 and no cb_ok bit."""
    un = units_of(ctx, "A", 20.0)
    plan = noise_plan(un, 8.0)
    n = len(un.allocs)
    zero = ctx.alloc(un.d_sub.nbytes)
    zero.zero()
    st, bits = plan.run(zero)
    zero.free()
    s2, g = plan.llr_noise(), plan.llr_gain()
    print("all-zero grid: status %s, sigma2 %s, gains %s" % (list(st), list(s2), list(g)))
    assert (s2 == 0).all() and (g == 0).all() and not any(plan.soft_bits(b).any() for b in range(n))
    assert (st == 2).all() and not plan.cb_ok().any()
    plan.run(un.d_sub)
    assert (plan.llr_noise() > 0).all() and (plan.llr_gain() > 0).all()
    plan.close()
    un.free()


def test_refusals_leave_the_plan_as_it_was(ctx):
    """A NULL plan, a negative, infinite or NaN scale: INVALID_ARG; a reference-mode plan: UNSUPPORTED, and INVALID_ARG for its tap.  After
    each the plan runs as before."""
    import openlte_amd as m
    L = ctx.L
    un = units_of(ctx, "B", 20.0)
    plan = noise_plan(un, 8.0)
    want = outputs(plan, un)
    s2 = plan.llr_noise()
    p = C.c_void_p()

    def same():
        got = outputs(plan, un)
        assert ctx.last_kernels().startswith("k_pusch_demod_llr:1,")
        assert same_outputs(got, want) and plan.llr_noise().tobytes() == s2.tobytes()

    for scale in (-1.0, float("inf"), float("-inf"), float("nan")):
        assert L.mi_lte_pusch_plan_set_llr_noise(plan.h, scale) == ERR_INVALID, scale
        same()
    assert L.mi_lte_pusch_plan_set_llr_noise(None, 8.0) == ERR_INVALID
    assert L.mi_lte_pusch_plan_llr_noise(None, C.byref(p)) == ERR_INVALID and L.mi_lte_pusch_plan_llr_noise(plan.h, None) == ERR_INVALID
    same()
    one = [grant(0, 1, 9, 6, 3, 0x71)]
    ref_plan = ctx.pusch_plan(un.cfg, un.ul, un.sfs[:1], un.cells[:1], one)
    ref_plan.run(un.d_sub)
    e0 = ref_plan.soft_bits(0)
    assert L.mi_lte_pusch_plan_set_llr_noise(ref_plan.h, 8.0) == ERR_UNSUPPORTED
    assert L.mi_lte_pusch_plan_set_llr_noise(ref_plan.h, 0.0) == ERR_UNSUPPORTED
    assert L.mi_lte_pusch_plan_set_llr_noise(ref_plan.h, -1.0) == ERR_INVALID
    assert L.mi_lte_pusch_plan_llr_noise(ref_plan.h, C.byref(p)) == ERR_INVALID
    ref_plan.run(un.d_sub)
    assert ctx.last_kernels().startswith("k_pusch_demod:1,") and (ref_plan.soft_bits(0) == e0).all()
    ref_plan.close()
    same()
    plan.close()
    un.free()
