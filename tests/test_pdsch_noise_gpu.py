"""GPU: the downlink CRS noise estimate (k_dl_crs_noise, mi_lte_dl_crs_noise_run) and the noise-referenced gain the 3GPP PDSCH plans build on it
(mi_lte_pdsch_plan_set_llr_noise, mi_lte_pdsch_plan_llr_noise).  sigma2 against the float64 restatement of include/mi_lte.h's text
(tests/pdsch_noise_model.py) on synthetic planes and on the front end's; the gain exactly (float)(scale / tap); the bytes by
test_demap_llr_gpu.check_against_model's rules with the tapped gain handed to demap_llr_model.demap; a plan that turns the setter on and off
again is the plan it was; the HARQ sat16 chain over the tapped bytes; the degenerate input and the refusals of the header; and what the
common scale buys two combined transmissions at the point profiles/pdsch_harq_sweep.txt names."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

import demap_llr_model as dm
import pdsch_noise_model as nm
import test_txdiv_gpu as txd
from demap_geometry_cases import FFT as FFT_OF, synthetic_planes
from test_demap_llr_gpu import N_SOFT, case, check_against_model, mixed_units, mk, planes_of
from test_dlsch3gpp_gpu import tbs
from test_harq_gpu import Tx, decode, gather_sums, sat16

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))

pytestmark = pytest.mark.gpu

ERR_INVALID, ERR_UNSUPPORTED = -1, -4
# profiles/pdsch_harq_sweep.txt (16 transport blocks per point, the sweep's seeds, rv 0 then rv 2 combined, BCJR x 8): see test_value
# No class has a window at 1 dB steps (N8 16 / 16 at p and p - 1, A 0 / 16 at p and p + 1): the automatic gain's waterfall is one to three
# steps wide and starts where N8's ends.  All three classes reach the largest difference, 16 blocks against none; the point is the first
# such SNR of the class that holds it longest (3 and 4 dB), 64QAM followed by QPSK.
VALUE_RULE, VALUE_CLASS, VALUE_SNR_DB = "largest_difference", "64qam_then_qpsk", 3


def scale_of(snr_db):
    """`scale` times the LLR in natural units meets the int8 clamp at an LLR of 127 / scale (test_pusch_noise_gpu.scale_of's choice, for its
    reason).  The header's convention 8 clamps at 16: at 20 dB most 64QAM amplitude bits stay under that (a whole decision interval is
    (2 A)^2 / sigma^2 ~ 10) and every sign bit of an outer point is far over it.  At 5 dB an LLR of 16 is a three-sigma event of an outermost
    point, too rare to demand of a one-PRB allocation, so the 5 dB plans run at 32 (clamp at an LLR of 4)."""
    return 8.0 if snr_db >= 10 else 32.0


def model_sigma2(planes, n_rb, n_ant, sfs, cells):
    return np.array([nm.sigma2(planes[u], n_rb, n_ant, sfs[u], cells[u]) for u in range(len(sfs))])


def with_crs(rng, planes, n_rb, n_ant, sf, cell, snr_db):
    """The CRS of ports 0 and 1 written into one unit's y planes through the unit's own estimate planes, with white noise snr_db under port 0's
    mean power"""
    h = planes[2:2 + n_ant].astype(np.float64) + 1j * planes[2 + n_ant:].astype(np.float64)
    sigma = np.sqrt((np.abs(h[0]) ** 2).mean() * 10 ** (-snr_db / 10) / 2)
    for p, i in nm.rows(n_ant):
        sym, k = nm.SYMBOLS[i], nm.pilots(n_rb, cell, p, i)
        v = h[p, sym, k] * nm.crs(n_rb, cell, sf, sym) + sigma * (rng.standard_normal(len(k)) + 1j * rng.standard_normal(len(k)))
        planes[0, sym, k], planes[1, sym, k] = v.real, v.imag
    return planes


@pytest.mark.parametrize("n_ant", [1, 2, 4])
@pytest.mark.parametrize("n_rb", [6, 15, 100])
def test_standalone_kernel_against_the_model(ctx, n_rb, n_ant):
    """Three units of seeded synthetic planes per call (demap_geometry_cases.synthetic_planes, the CRS written into the y planes at 20, 5 and
    20 dB), cells whose CRS shift makes voff + v_shift wrap past 6 (residues 4 and 5) and not wrap (residue 1), subframes 0, 5, 9: the relative
    difference to the float64 model is <= 1e-4 for every unit -- the PUSCH test's bound, for its reason: a float least-squares product carries
    a few ulp of |t|, the differences and sums are in double, and a second difference of noise at 5 .. 20 dB is 0.1 .. 1 times |t|, so the
    float error stays under 1e-5 of it.  Two runs give identical bytes."""
    import openlte_amd as m
    rng = np.random.default_rng(100 * n_rb + n_ant)
    sfs, cells, snrs = [0, 5, 9], [4 + 6 * 7, 1 + 6 * 50, 503], [20.0, 5.0, 20.0]
    assert [c % 6 for c in cells] == [4, 1, 5]
    planes = np.stack([with_crs(rng, synthetic_planes(rng, n_ant, snrs[u]), n_rb, n_ant, sfs[u], cells[u], snrs[u]) for u in range(3)])
    want = model_sigma2(planes, n_rb, n_ant, sfs, cells)
    cfg = m.DlCfg(FFT_OF[n_rb], n_rb, n_ant, 0)
    d_sub = ctx.to_device(planes)
    got = ctx.dl_crs_noise(cfg, d_sub, sfs, cells)
    assert ctx.last_kernels() == "k_dl_crs_noise:1"
    again = ctx.dl_crs_noise(cfg, d_sub, sfs, cells)
    d_sub.free()
    rel = np.abs(got.astype(np.float64) - want) / want
    for u in range(3):
        print("%3d RB, %d port(s), unit %d (subframe %d, cell %3d, %2.0f dB): sigma2 %.6g, model %.6g, relative difference %.3g"
              % (n_rb, n_ant, u, sfs[u], cells[u], snrs[u], got[u], want[u], rel[u]))
    assert got.shape == (3,) and (want > 0).all() and (rel <= 1e-4).all(), rel
    assert again.tobytes() == got.tobytes()


def test_compact_planes_give_the_same_floats(ctx):
    """One capture through the front end twice, into full and into MI_LTE_CE_COMPACT planes: the estimate reads only the y planes, so the two
    calls give the same floats, and they are the model's on the downloaded planes."""
    import openlte_amd as m
    from openlte_amd import synth
    n_rb, cfi, sfs, cells, per_unit, _ = case("25rb_window")
    allocs = [a for row in per_unit for a in row]
    full = m.DlCfg(FFT_OF[n_rb], n_rb, 1, m.IQ_I8)
    iq, _ = synth.dl_units_3gpp(full, sfs, cells, allocs, len(per_unit[0]), N_SOFT, n_pdcch_symbs=cfi, snr_db=12.0, max_delay=4, seed=77)
    n = len(sfs)
    d_iq, d_start = ctx.to_device(iq.reshape(-1, 2)), ctx.to_device((np.arange(n) * iq.shape[1]).astype(np.uint64))
    d_sf, d_cell = ctx.to_device(np.asarray(sfs, np.uint32)), ctx.to_device(np.asarray(cells, np.uint32))
    got = {}
    for fmt in (m.IQ_I8, m.IQ_I8 | m.CE_COMPACT):
        cfg = m.DlCfg(FFT_OF[n_rb], n_rb, 1, fmt)
        d_sub = ctx.alloc(n * ctx.subframe_floats(1) * 4)
        d_sub.zero()
        ctx.dl_frontend_dev(cfg, d_iq, None, d_start, d_sf, d_cell, n, d_sub)
        got[fmt] = ctx.dl_crs_noise(cfg, d_sub, sfs, cells)
        if fmt == m.IQ_I8:
            want = model_sigma2(d_sub.download(np.float32).reshape(n, 4, 16, dm.N_SC), n_rb, 1, sfs, cells)
        d_sub.free()
    for b in (d_iq, d_start, d_sf, d_cell):
        b.free()
    print("full %s, compact %s, model %s" % (got[m.IQ_I8], got[m.IQ_I8 | m.CE_COMPACT], want))
    assert got[m.IQ_I8].tobytes() == got[m.IQ_I8 | m.CE_COMPACT].tobytes()
    assert (want > 0).all() and (np.abs(got[m.IQ_I8] - want) <= 1e-4 * want).all()


def noise_model(t, planes, n_rb, cfi, n_ant, unit_gain):
    """demap_llr_model.demap of every allocation with its unit's gain as a fixed gain, in the plan's order"""
    import openlte_amd as m
    out = []
    for u in range(len(t.sfs)):
        out += dm.demap(planes[u], [al for al in t.allocs if al.unit == u], t.sfs[u], t.cells[u], n_rb, cfi, n_ant, gain=float(unit_gain[u]), T=m.DEMAP_AUTO_T)
    return out


def check_noise_run(ctx, t, plan, planes, n_rb, cfi, n_ant, scale, label):
    """After a MAXLOG run of `plan` with the noise gain at `scale`: the tap against the model on `planes` (<= 1e-4, every unit), the gains exactly
    (float)(scale / tap[unit]), the bytes by check_against_model's rules with those gains, clamped and graded bytes both present, and the
    kernels the run names.  Returns the tap."""
    assert ctx.last_kernels().startswith("k_dl_crs_noise:1,%s:1,k_dl3_desc:1," % label), ctx.last_kernels()
    tap, gains = plan.llr_noise(), plan.llr_gain()
    want = model_sigma2(planes, n_rb, n_ant, t.sfs, t.cells)
    rel = np.abs(tap.astype(np.float64) - want) / want
    print("sigma2 %s, model %s, largest relative difference %.3g" % (tap, want, rel.max()))
    assert tap.shape == (len(t.sfs),) and (want > 0).all() and (rel <= 1e-4).all(), rel
    unit_gain = np.array([np.float32(np.float64(scale) / np.float64(v)) for v in tap], np.float32)
    assert all(gains[a] == unit_gain[al.unit] == np.float32(nm.gain(scale, tap[al.unit])) for a, al in enumerate(t.allocs)), (gains, unit_gain)
    # (check_against_model with gain 0 holds the tap to the model's gain within 2^-18; it is exact, by the line above)
    e = check_against_model(plan, t, noise_model(t, planes, n_rb, cfi, n_ant, unit_gain), 0.0)
    n_clamped, n_graded = int((np.abs(e.astype(int)) == 127).sum()), int((np.abs(e.astype(int)) < 127).sum())
    print("scale %g: %d clamped and %d graded bytes" % (scale, n_clamped, n_graded))
    assert n_clamped > 0 and n_graded > 0
    return tap


@pytest.mark.parametrize("name", ["6rb_1prb", "25rb_window", "100rb"])
def test_plan_tap_gain_and_bytes(ctx, name):
    """test_demap_llr_gpu's shapes (the LDS path and direct stores) at 20 and 5 dB on the front end's planes: check_noise_run's checks,
    whatever gain set_demapper was given; two runs give identical bytes and taps.  The scale per SNR is scale_of's."""
    import openlte_amd as m
    n_rb, cfi, sfs, cells, per_unit, _ = case(name)
    mean = []
    for snr_db in (20.0, 5.0):
        t = Tx(ctx, n_rb, sfs, cells, per_unit, N_SOFT, cfi, snr_db, seed=int(snr_db) + len(name))
        planes = planes_of(t)
        plan = t.plan(N_SOFT)
        plan.set_demapper(m.DEMAP_MAXLOG, 3.0)
        plan.set_llr_noise(scale_of(snr_db))
        decode(t, plan)
        tap = check_noise_run(ctx, t, plan, planes, n_rb, cfi, 1, scale_of(snr_db), "k_pdsch_demod_llr")
        e, g = [plan.soft_bits(a) for a in range(plan.n_alloc)], plan.llr_gain()
        plan.set_demapper(m.DEMAP_MAXLOG, 0.0)  # the gain handed to set_demapper is out of play
        decode(t, plan)
        assert all(plan.soft_bits(a).tobytes() == e[a].tobytes() for a in range(plan.n_alloc))
        assert plan.llr_noise().tobytes() == tap.tobytes() and plan.llr_gain().tobytes() == g.tobytes()
        mean.append(float(tap.mean()))
        plan.close()
        t.free()
    print("%s: mean sigma2 %.6g at 20 dB, %.6g at 5 dB, ratio %.2f dB" % (name, mean[0], mean[1], 10 * np.log10(mean[1] / mean[0])))


@pytest.mark.parametrize("name", ["A", "B"])
def test_transmit_diversity(ctx, name):
    """The smallest shapes of test_txdiv_gpu (A: 6 RB on two ports, B: 25 RB on four, astride the sync window) at 20 and 5 dB: the same checks
    under the transmit-diversity label; the estimate uses ports 0 and 1 on four ports too."""
    import openlte_amd as m
    for snr_db in (20.0, 5.0):
        t, _ = txd.make(ctx, name, snr_db, seed=int(snr_db) + ord(name))
        plan = t.plan(N_SOFT)
        plan.set_demapper(m.DEMAP_MAXLOG, 0.0)
        plan.set_llr_noise(scale_of(snr_db))
        decode(t, plan)
        check_noise_run(ctx, t, plan, t.planes(), t.n_rb, t.cfi, t.n_ant, scale_of(snr_db), "k_pdsch_demod_llr_txd")
        plan.close()
        t.free()


def everything(t, plan):
    h = decode(t, plan)
    h["kernels"], h["e"], h["gain"] = t.ctx.last_kernels(), [plan.soft_bits(a) for a in range(plan.n_alloc)], plan.llr_gain()
    return h


def same(x, y):
    return x["kernels"] == y["kernels"] and x["gain"].tobytes() == y["gain"].tobytes() and (x["st"] == y["st"]).all() and (x["rows"] == y["rows"]).all() \
        and (x["cb_ok"] == y["cb_ok"]).all() and all(a.tobytes() == b.tobytes() for a, b in zip(x["e"], y["e"])) \
        and all((a == b).all() for a, b in zip(x["cb_soft"], y["cb_soft"]))


def test_on_and_off(ctx):
    """A MAXLOG plan run with the setter off, on, and off again: the third run gives the first run's bytes, gains, status, output rows and
    last_kernels exactly, and the run in between differs.  On a plan with the default demapper the setter changes nothing -- k_pdsch_demod, the
    same bytes, a tap of zeros -- until MAXLOG is chosen."""
    import openlte_amd as m
    n_rb, cfi, sfs, cells, per_unit, _ = case("25rb_window")
    t = Tx(ctx, n_rb, sfs, cells, per_unit, N_SOFT, cfi, 9.0, seed=3)
    plan = t.plan(N_SOFT)
    ref_run = everything(t, plan)
    assert ref_run["kernels"].startswith("k_pdsch_demod:1,") and not plan.llr_noise().any() and plan.llr_noise().shape == (len(sfs),)
    plan.set_llr_noise(8.0)
    assert same(everything(t, plan), ref_run) and not plan.llr_noise().any() and not plan.llr_gain().any()
    plan.set_llr_noise(0.0)
    plan.set_demapper(m.DEMAP_MAXLOG, 0.0)
    first = everything(t, plan)
    assert first["kernels"].startswith("k_pdsch_demod_llr:1,k_dl3_desc:1,") and not plan.llr_noise().any()
    plan.set_llr_noise(8.0)
    mid = everything(t, plan)
    assert mid["kernels"] == "k_dl_crs_noise:1," + first["kernels"]
    assert (plan.llr_noise() > 0).all() and any((a != b).any() for a, b in zip(mid["e"], first["e"]))
    tap = plan.llr_noise()
    plan.set_llr_noise(0.0)
    assert same(everything(t, plan), first)
    assert plan.llr_noise().tobytes() == tap.tobytes()  # (the tap keeps the last noise-on run's estimates)
    plan.close()
    t.free()


def test_harq_sat16_chain(ctx, ref, ref_phy):
    """rv 0 and then rv 2 under the noise gain through mi_lte_pdsch_decode_run_harq: after each, the int16 buffer is the sat16 chain over the
    runs' tapped soft bits (test_harq_gpu.gather_sums), exactly, and the decoder's input its clamp."""
    import openlte_amd as m
    n_soft = 125184
    pool = ctx.harq_pool(8)
    model, payload = {}, None
    for k, rv in enumerate((0, 2)):
        sfs, cells, per_unit = mixed_units(rv=rv)
        t = Tx(ctx, 25, sfs, cells, per_unit, n_soft, 2, 6.0 + 4 * k, seed=20 + k, payload=payload)
        payload = t.tx
        plan = t.plan(n_soft)
        plan.set_demapper(m.DEMAP_MAXLOG, 0.0)
        plan.set_llr_noise(8.0)
        n = plan.n_alloc
        h = decode(t, plan, pool, list(range(n)), k == 0)
        assert ctx.last_kernels().startswith("k_dl_crs_noise:1,k_pdsch_demod_llr:1,k_dl3_desc:1,k_harq_bind:1,k_harq_rm:1,"), ctx.last_kernels()
        tap = plan.llr_noise()
        assert (tap > 0).all() and all(plan.llr_gain()[a] == np.float32(nm.gain(8.0, tap[al.unit])) for a, al in enumerate(t.allocs))
        for a, al in enumerate(t.allocs):
            v, lay = gather_sums(ref, ref_phy, plan, a, al, n_soft)
            model[a] = sat16(sat16(v) if k == 0 else model[a] + sat16(v))
            got = pool.soft(a)
            assert got.shape == model[a].shape and (got == model[a]).all(), (k, a)
            assert (h["cb_soft"][a] == np.clip(model[a], -127, 127)).all(), (k, a)
            assert pool.state(a)["n_tx"] == k + 1
        plan.close()
        t.free()
    assert max(int(np.abs(v).max()) for v in model.values()) > 127
    pool.close()


def test_zero_y_planes(ctx):
    """All-zero y planes under the front end's (non-zero) estimate planes: sigma2 = 0 and g_a = 0, every soft bit 0, status 2 and no cb_ok bit;
    after it a run on the good planes decodes as it did."""
    import openlte_amd as m
    n_rb, cfi, sfs, cells, per_unit, _ = case("25rb_window")
    t = Tx(ctx, n_rb, sfs, cells, per_unit, N_SOFT, cfi, 20.0, seed=8)
    plan = t.plan(N_SOFT)
    plan.set_demapper(m.DEMAP_MAXLOG, 0.0)
    plan.set_llr_noise(8.0)
    want = everything(t, plan)
    good_tap = plan.llr_noise()
    planes = planes_of(t).copy()
    planes[:, :2] = 0
    assert planes[:, 2:].any()
    keep, t.d_sub = t.d_sub, ctx.to_device(planes)
    h = decode(t, plan)
    s2, g = plan.llr_noise(), plan.llr_gain()
    print("all-zero y planes: status %s, sigma2 %s, gains %s" % (list(h["st"]), list(s2), list(g)))
    assert (s2 == 0).all() and (g == 0).all() and not any(plan.soft_bits(a).any() for a in range(plan.n_alloc))
    assert (h["st"] == 2).all() and not h["cb_ok"].any()
    t.d_sub.free()
    t.d_sub = keep
    assert same(everything(t, plan), want) and plan.llr_noise().tobytes() == good_tap.tobytes() and (good_tap > 0).all()
    plan.close()
    t.free()


def test_refusals_leave_everything_usable(ctx):
    """A negative, infinite or NaN scale and a NULL plan: INVALID_ARG; a reference-mode plan: UNSUPPORTED, and INVALID_ARG for its tap; the
    standalone call: INVALID_ARG for every NULL pointer, n_units = 0, a bandwidth that is none of the six and a port count of 3.  After each
    the plan and the standalone call run as before."""
    import openlte_amd as m
    L = ctx.L
    n_rb, cfi, sfs, cells, per_unit, _ = case("25rb_window")
    t = Tx(ctx, n_rb, sfs, cells, per_unit, N_SOFT, cfi, 20.0, seed=9)
    plan = t.plan(N_SOFT)
    plan.set_demapper(m.DEMAP_MAXLOG, 0.0)
    plan.set_llr_noise(8.0)
    want = everything(t, plan)
    tap = plan.llr_noise()
    alone = ctx.dl_crs_noise(t.cfg, t.d_sub, sfs, cells)
    assert alone.tobytes() == tap.tobytes()
    p, n = C.c_void_p(), C.c_uint32()

    def unchanged():
        assert same(everything(t, plan), want) and plan.llr_noise().tobytes() == tap.tobytes()
        assert ctx.dl_crs_noise(t.cfg, t.d_sub, sfs, cells).tobytes() == alone.tobytes()

    for scale in (-1.0, float("inf"), float("-inf"), float("nan")):
        assert L.mi_lte_pdsch_plan_set_llr_noise(plan.h, scale) == ERR_INVALID, scale
        unchanged()
    assert L.mi_lte_pdsch_plan_set_llr_noise(None, 8.0) == ERR_INVALID
    assert L.mi_lte_pdsch_plan_llr_noise(None, C.byref(p), C.byref(n)) == ERR_INVALID
    assert L.mi_lte_pdsch_plan_llr_noise(plan.h, None, C.byref(n)) == ERR_INVALID and L.mi_lte_pdsch_plan_llr_noise(plan.h, C.byref(p), None) == ERR_INVALID
    unchanged()
    # a reference-mode plan
    ref_plan = ctx.pdsch_plan(t.cfg, cfi, [mk(0, 1, tbs(5, 3), [8, 9, 10], 0x41)])
    ref_plan.run(t.d_sub, sfs, cells)
    e0 = ref_plan.soft_bits(0)
    assert L.mi_lte_pdsch_plan_set_llr_noise(ref_plan.h, 8.0) == ERR_UNSUPPORTED
    assert L.mi_lte_pdsch_plan_set_llr_noise(ref_plan.h, 0.0) == ERR_UNSUPPORTED
    assert L.mi_lte_pdsch_plan_set_llr_noise(ref_plan.h, -1.0) == ERR_INVALID
    assert L.mi_lte_pdsch_plan_llr_noise(ref_plan.h, C.byref(p), C.byref(n)) == ERR_INVALID
    ref_plan.run(t.d_sub, sfs, cells)
    assert ctx.last_kernels().startswith("k_pdsch_demod:1,") and (ref_plan.soft_bits(0) == e0).all()
    ref_plan.close()
    unchanged()
    # the standalone call
    d_s2 = ctx.alloc(4 * len(sfs))
    args = [ctx.h, C.byref(t.cfg), t.d_sub.ptr, t.d_sf.ptr, t.d_cell.ptr, len(sfs), d_s2.ptr]
    for i in (0, 1, 2, 3, 4, 6):
        bad = list(args)
        bad[i] = None
        assert L.mi_lte_dl_crs_noise_run(*bad) == ERR_INVALID, i
    bad = list(args)
    bad[5] = 0
    assert L.mi_lte_dl_crs_noise_run(*bad) == ERR_INVALID
    for cfg in (m.DlCfg(t.cfg.fft_size, 10, 1, 0), m.DlCfg(t.cfg.fft_size, 0, 1, 0), m.DlCfg(t.cfg.fft_size, 110, 1, 0), m.DlCfg(t.cfg.fft_size, n_rb, 3, 0),
                m.DlCfg(t.cfg.fft_size, n_rb, 0, 0)):
        bad = list(args)
        bad[1] = C.byref(cfg)
        assert L.mi_lte_dl_crs_noise_run(*bad) == ERR_INVALID, (cfg.N_rb_dl, cfg.N_ant)
    assert L.mi_lte_dl_crs_noise_run(*args) == 0
    assert d_s2.download(np.float32).tobytes() == alone.tobytes()
    d_s2.free()
    unchanged()
    plan.close()
    t.free()


def test_value(ctx):
    """The point of profiles/pdsch_harq_sweep.txt with the sweep's seeds (tools/pdsch_harq_sweep.py): two combined transmissions, rv 0 then rv 2,
    16 transport blocks, BCJR x 8.  Rule "window": N8 decodes 16 / 16 at VALUE_SNR_DB and 1 dB under it and A 0 / 16 at VALUE_SNR_DB and 1 dB
    over it.  Rule "largest_difference" (no class has such a window at 1 dB steps): VALUE_SNR_DB is the first SNR of VALUE_CLASS with the
    largest N8 - A.  Either way, at VALUE_SNR_DB the noise-referenced gain at scale 8 decodes at least as many blocks as the automatic gain
    and strictly more than the default demapper.  Measured there (64qam_then_qpsk, 3 dB): N8 16, A 0, R 0 of 16."""
    import pdsch_harq_sweep as sw
    p = sw.Point(ctx, VALUE_CLASS, float(VALUE_SNR_DB), 16)
    n_ok = {mode: int(p.decoded(mode).sum()) for mode in ("R", "A", "N8")}
    p.close()
    print("%s at %d dB (%s): %s of 16 transport blocks decoded" % (VALUE_CLASS, VALUE_SNR_DB, VALUE_RULE, n_ok))
    assert n_ok["N8"] >= n_ok["A"] and n_ok["N8"] > n_ok["R"], n_ok
