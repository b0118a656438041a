"""GPU: the 3GPP PUSCH plans' max-log soft-decision demapper (mi_lte_pusch_plan_set_demapper, k_pusch_demod_llr).  Its bytes against the
float64 model of include/mi_lte.h's text on the tapped symbols and reliabilities (tests/pusch_demod_model.py, the exact layer), the
reliabilities rho_s against the model's restatement of the polar interpolation (the tolerance layer); a plan that never opts in, or opts out
again, is the plan it was; everything after the soft-bit buffer -- rate un-matching, the BCJR model, the control-information gather, sums
and decisions, the CQI decoder -- does with the graded bytes what it does with the default demapper's; and what the soft decisions buy: at an
SNR profiles/pusch_llr_sweep.txt names, every transport block of one of its classes decodes with them and none without."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

import demap_llr_model as dm
import pusch_demod_model as pm
from test_ulsch3gpp_gpu import QM, Units, check_blocks_exact, grant
from test_ulsch_cqi_cpu import ZERO, model as cqi_model
from test_ulsch_uci_gpu import UciUnits, check_gather_and_sums, exact_grants

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))

pytestmark = pytest.mark.gpu

ERR_INVALID, ERR_UNSUPPORTED = -1, -4
# profiles/pusch_llr_sweep.txt (16 transport blocks per point, the sweep's seeds).  With 1 dB steps the window below takes some 4 dB between
# the two curves and steep ones; the uplink's gap at unit gain is 2.0 .. 3.1 dB with one code block, so the issue's classes and the
# single-block ones the sweep was widened by (64QAM at code rates 0.15 .. 0.75) are all a step or two short, as are the two-block classes.
# The window opens on 96 PRB of a 100-RB cell, where a transport block of six code blocks at code rate 0.38 makes both curves steep:
# MAXLOG 16 / 16 from 11 dB on, the default demapper 0 / 16 up to 13 dB.
VALUE_CLASS, VALUE_SNR_DB = "64qam_r0.4_flat_100rb", 12


def case(name):
    """(n_rb, subframes, cell, allocations per unit): the shapes the kernel can go wrong at.
    A  1 PRB QPSK (M = 12, narrower than a wavefront), 6 PRB 16QAM, 10 PRB 64QAM (a radix-5 pass) in one unit, two units: 256 threads, S_par = 12
    B  6 PRB only, the three modulations over three units: the 192-thread instantiation, M_max = 72
    C  24 PRB 64QAM + 1 PRB 16QAM: S_par = 6, a tiny allocation in a wide plan
    D  100-RB cell, 40 PRB 16QAM: S_par = 3 (with 2 PRB of 64QAM next to it: under the automatic gain a 16QAM soft bit ends at 4 T = 64 on a
       noiseless outermost point, so at 20 dB a plan of 16QAM alone has no byte at the clamp, which every plan here has to show)
    E  100-RB cell, 96 PRB 64QAM: S_par = 2, 82 944 soft bits"""
    if name == "A":
        return 25, [2, 7], 40, [[grant(u, 1, 5, 1, 0, 0x61 + 8 * u), grant(u, 2, 15, 6, 1, 0x62 + 8 * u, rv=1), grant(u, 3, 22, 10, 7, 0x63 + 8 * u)]
                                for u in range(2)]
    if name == "B":
        return 25, [1, 4, 8], 77, [[grant(0, 1, 9, 6, 3, 0x71)], [grant(1, 2, 15, 6, 10, 0x72, rv=2)], [grant(2, 3, 22, 6, 19, 0x73)]]
    if name == "C":
        return 25, [3], 5, [[grant(0, 3, 22, 24, 0, 0x81), grant(0, 2, 15, 1, 24, 0x82)]]
    if name == "D":
        return 100, [6], 301, [[grant(0, 2, 15, 40, 13, 0x91), grant(0, 3, 22, 2, 60, 0x92)]]
    assert name == "E"
    return 100, [9], 123, [[grant(0, 3, 22, 96, 2, 0xA1)]]


CASES = ["A", "B", "C", "D", "E"]
SNRS = [20.0, 5.0]


# Seeds.  test_rho_against_the_float64_restatement leaves out symbols whose smallest modelled |h|^2 is under 1e-3 of the allocation's mean and
# wants them under 1 % of all symbols: at 5 dB an estimate of 288 or 1152 noisy sub-carriers has such a sub-carrier on one symbol in a few, so
# the seeds of C and E at 5 dB are ones for which the float64 model (pm.h_polar on the front end's planes, no kernel result) shows none.
SEEDS = {("C", 5.0): 4, ("E", 5.0): 3}


def units_of(ctx, name, snr_db):
    n_rb, sfs, cell, per_unit = case(name)
    seed = SEEDS.get((name, snr_db)) or int(snr_db) + 7 * CASES.index(name)
    return Units(ctx, n_rb, sfs, cell, per_unit, snr_db, seed=seed)


def c_init(un, k):
    al = un.allocs[k]
    return (al.rnti << 14) | (un.sfs[al.unit] << 9) | un.cells[al.unit]


def slots(plan, n_alloc):
    """Every allocation's whole slot of the soft-bit buffer (its share rounded up to 64 bytes), int8"""
    ctx, out = plan.ctx, []
    for a in range(n_alloc):
        pe, pn = C.c_void_p(), C.c_uint32()
        ctx._check(ctx.L.mi_lte_pusch_plan_soft_bits(plan.h, a, C.byref(pe), C.byref(pn)))
        buf = np.empty((pn.value + 63) & ~63, np.int8)
        ctx._check(ctx.L.mi_lte_memcpy_d2h(ctx.h, buf.ctypes.data, pe.value, buf.nbytes))
        out.append(buf)
    return out


def check_against_model(plan, un, gain):
    """The rules of the bytes, on the run's own taps: identical to the model outside the guard band, at most one step inside it, the band under
    1 % of the soft bits; the gain within 2^-18 of the model's (automatic) or the argument itself (fixed).  Returns every byte of the plan."""
    import openlte_amd as m
    gains, rho = plan.llr_gain(), plan.llr_rho()
    n_guard = n_all = 0
    every = []
    for a, al in enumerate(un.allocs):
        e, xs = plan.soft_bits(a), plan.llr_symbols(a)
        assert xs.shape == (12, 12 * al.N_prb) and np.isfinite(xs).all() and (rho[a] > 0).all(), a
        r = pm.demap(xs, rho[a], al.mod_type, c_init(un, a), gain=gain, T=m.DEMAP_AUTO_T)
        assert len(e) == len(r.bytes) == 144 * al.N_prb * QM[al.mod_type], (a, len(e))
        d = np.abs(e.astype(np.int32) - r.bytes)
        guard = dm.in_guard(r.x)
        print("allocation %d (%d PRB, Q_m %d): %d soft bits, %d in the guard band, %d differ (%d of them outside it), largest difference %d; gain %.9g, model %.9g"
              % (a, al.N_prb, QM[al.mod_type], len(e), guard.sum(), (d != 0).sum(), (d[~guard] != 0).sum(), d.max(), gains[a], r.gain))
        assert not d[~guard].any(), (a, int((d[~guard] != 0).sum()))
        assert d.max() <= 1, a
        if gain == 0:
            assert r.gain > 0 and abs(float(gains[a]) - r.gain) <= 2.0 ** -18 * r.gain, (a, gains[a], r.gain)
        else:
            assert gains[a] == np.float32(gain), (a, gains[a])
        n_guard += int(guard.sum())
        n_all += len(e)
        every.append(e)
    assert n_guard < 0.01 * n_all, (n_guard, n_all)
    return np.concatenate(every)


@pytest.mark.parametrize("snr_db", SNRS)
@pytest.mark.parametrize("name", CASES)
def test_bytes_and_gains_against_the_model(ctx, name, snr_db):
    """max_delay = 3 and noise at 20 and 5 dB.  Automatic gain, then a fixed one 1.5 x the median automatic one on the same plan: bytes and
    gains by the model's rules, clamped and graded bytes both present, e_len and every byte outside the allocations' ranges as the default
    demapper's run left them, two consecutive runs byte-identical."""
    import openlte_amd as m
    un = units_of(ctx, name, snr_db)
    plan = un.plan()
    plan.run(un.d_sub)
    assert ctx.last_kernels().startswith("k_pusch_demod:1,")
    n = len(un.allocs)
    ref_len, ref_slots = [len(plan.soft_bits(a)) for a in range(n)], slots(plan, n)
    plan.set_llr_tap(True)
    fixed = None
    for k in range(2):
        gain = 0.0 if k == 0 else fixed
        plan.set_demapper(m.DEMAP_MAXLOG, gain)
        plan.run(un.d_sub)
        assert ctx.last_kernels().startswith("k_pusch_demod_llr:1,k_dl3_desc:1,k_dl3_rm_i8:1,")
        e = check_against_model(plan, un, gain)
        assert (np.abs(e) == 127).any() and (np.abs(e) < 127).any()
        got, g1, r1 = slots(plan, n), plan.llr_gain(), plan.llr_rho()
        for a in range(n):
            assert len(plan.soft_bits(a)) == ref_len[a], a
            assert (got[a][ref_len[a]:] == ref_slots[a][ref_len[a]:]).all(), a
        plan.run(un.d_sub)
        again = slots(plan, n)
        assert all(x.tobytes() == y.tobytes() for x, y in zip(got, again))
        assert g1.tobytes() == plan.llr_gain().tobytes() and r1.tobytes() == plan.llr_rho().tobytes()
        if k == 0:
            fixed = float(np.float32(1.5 * np.median(g1)))
    plan.close()
    un.free()


def test_rho_against_the_float64_restatement(ctx):
    """rho_s of every allocation of plans A-E at 20 and 5 dB against M / sum_k 1 / |h_k(s)|^2 on the model's float64 polar interpolation:
    relative difference <= 1e-4 (the kernel's float error per term is a few ulp, 6e-8 each, and the sum is in double; what is left is the
    float rounding of mag + n f_mag, which is only bounded relative to the magnitudes it is formed from).  Symbols whose smallest modelled
    |h|^2 is under 1e-3 of the allocation's mean are left out -- the cancellation in mag + n f_mag is unbounded there -- and must be under
    1 % of all symbols."""
    import openlte_amd as m
    n_all = n_out = 0
    worst = 0.0
    for name in CASES:
        for snr_db in SNRS:
            un = units_of(ctx, name, snr_db)
            planes = un.d_sub.download(np.float32).reshape(len(un.sfs), 2, 16, pm.N_SC)
            plan = un.plan()
            plan.set_demapper(m.DEMAP_MAXLOG, 0.0)
            plan.run(un.d_sub)
            rho = plan.llr_rho()
            for a, al in enumerate(un.allocs):
                dmrs = m.ul_dmrs_pusch(un.ul, un.cells[al.unit], un.sfs[al.unit], al.N_prb)
                want, w_min, w_mean = pm.rho_of(pm.h_polar(planes[al.unit], al, dmrs))
                keep = w_min >= 1e-3 * w_mean
                rel = np.abs(rho[a].astype(np.float64) - want) / want
                print("%s %2.0f dB allocation %d (%3d PRB): rho %.4g .. %.4g, relative difference up to %.3g, %d symbols left out"
                      % (name, snr_db, a, al.N_prb, rho[a].min(), rho[a].max(), rel[keep].max() if keep.any() else 0.0, (~keep).sum()))
                assert (rel[keep] <= 1e-4).all(), (name, snr_db, a, rel)
                worst = max(worst, float(rel[keep].max()) if keep.any() else 0.0)
                n_all += 12
                n_out += int((~keep).sum())
            plan.close()
            un.free()
    print("rho: %d symbols, %d left out, largest relative difference %.3g" % (n_all, n_out, worst))
    assert n_out < 0.01 * n_all, (n_out, n_all)


def outputs(plan, un):
    st, bits = plan.run(un.d_sub)
    n = len(un.allocs)
    return {"st": st, "bits": bits, "cb_ok": plan.cb_ok(), "e": [plan.soft_bits(a) for a in range(n)], "cb_soft": [plan.cb_soft(a) for a in range(n)]}


def same_outputs(a, b):
    return (a["st"].tobytes() == b["st"].tobytes() and a["cb_ok"].tobytes() == b["cb_ok"].tobytes()
            and all(x.tobytes() == y.tobytes() for k in ("bits", "e", "cb_soft") for x, y in zip(a[k], b[k])))


def test_opt_in_is_inert(ctx):
    """The same input through a plan that never calls the setter and through one set to MAXLOG, run, and set back to REF: soft bits, output rows,
    status, cb_ok and cb_soft byte for byte, and last_kernels starts with k_pusch_demod:1; the MAXLOG run in between differs."""
    import openlte_amd as m
    un = units_of(ctx, "A", 9.0)
    plain, other = un.plan(), un.plan()
    want = outputs(plain, un)
    assert ctx.last_kernels().startswith("k_pusch_demod:1,")
    other.set_demapper(m.DEMAP_MAXLOG, 0.0)
    mid = outputs(other, un)
    assert ctx.last_kernels().startswith("k_pusch_demod_llr:1,")
    assert not same_outputs(mid, want) and any((x != y).any() for x, y in zip(mid["e"], want["e"]))
    other.set_demapper(m.DEMAP_REF, 123.0)
    got = outputs(other, un)
    assert ctx.last_kernels().startswith("k_pusch_demod:1,")
    assert same_outputs(got, want)
    assert same_outputs(outputs(plain, un), want)
    for p in (plain, other):
        p.close()
    un.free()


def test_downstream_unchanged(ctx, port, ref, ref_phy):
    """A MAXLOG plan with one, two and three code blocks per transport block: cb_soft is the reference's ULSCH rate un-matching of the tapped
    soft bits, the rows, verdicts and cb_ok are the plain-C BCJR models' on those blocks (test_ulsch3gpp_gpu.check_blocks_exact)."""
    import openlte_amd as m
    per_unit = [[grant(0, 2, 15, 20, 0, 0xB1)], [grant(1, 3, 26, 24, 1, 0xB2, rv=1)], [grant(2, 1, 9, 10, 7, 0xB3, rv=2)], [grant(3, 3, 22, 6, 18, 0xB4, rv=3)]]
    un = Units(ctx, 25, [0, 5, 3, 8], 17, per_unit, 9.0, seed=31)
    plan = un.plan()
    plan.set_demapper(m.DEMAP_MAXLOG, 0.0)
    res = []
    for mode, n_iter in ((m.TURBO_BCJR, 8), (m.TURBO_BCJR_BLOCK, 6)):
        plan.set_decoder(mode, n_iter, 1)
        st, bits = plan.run(un.d_sub)
        assert ctx.last_kernels().startswith("k_pusch_demod_llr:1,")
        res.append((st, bits, plan.cb_ok()))
    seen, n_pass, n_fail = check_blocks_exact(port, ref, ref_phy, plan, un.allocs, res)
    print("MAXLOG uplink blocks: C %s, status %s / %s" % (sorted(seen), list(res[0][0]), list(res[1][0])))
    assert seen >= {1, 2, 3}
    e = np.concatenate([plan.soft_bits(a) for a in range(len(un.allocs))])
    assert len(np.unique(np.abs(e))) > 64  # (graded bytes went through)
    plan.close()
    un.free()


def test_control_information_on_graded_bytes(ctx):
    """test_ulsch_uci_gpu's exact_grants under MAXLOG, CQI decoding on for the second of them: data_soft / cqi_soft, S_ack / S_ri and the
    decided bits equal gather_py / sums_py / decide_py on the tapped soft bits; the CQI record equals the CPU model on cqi_soft; last_kernels
    lists the control-information kernels behind k_pusch_demod_llr:1."""
    import openlte_amd as m
    grants = exact_grants()
    un = UciUnits(ctx, 25, 33, grants, 15.0, seed=41)
    Os = [0, 5, 0, 0, 0, 0]
    assert grants[1].u.Q_cqi == 40
    for with_cqi in (False, True):
        plan = un.plan()
        plan.set_demapper(m.DEMAP_MAXLOG, 0.0)
        if with_cqi:
            plan.set_cqi_decode(Os)
        plan.run(un.d_sub)
        tail = ",k_ulsch_uci_gather:1,k_ulsch_uci_decide:1" + (",k_ulsch_cqi_decode:1" if with_cqi else "") + ",k_dl3_desc:1,"
        assert ctx.last_kernels().startswith("k_pusch_demod_llr:1" + tail), ctx.last_kernels()
        rec = plan.uci_results()
        graded = 0
        for k in range(len(grants)):
            check_gather_and_sums(un, plan, rec, k)
            graded += len(np.unique(np.abs(plan.soft_bits(k))))
        assert graded > 100
        if with_cqi:
            got = plan.cqi_results()
            want = cqi_model([(plan.cqi_soft(1), 5)])
            print("CQI record under MAXLOG: %s" % got[1])
            assert got[1] == want[0] and got[1]["O"] == 5
            assert [got[k] for k in (0, 2, 3, 4, 5)] == [ZERO] * 5
        plan.close()
    un.free()


def test_noiseless_every_soft_bit_has_the_coded_bits_sign(ctx):
    """The units of test_ulsch3gpp_gpu.test_demodulator_every_soft_bit_noiseless (static flat channel, int8 samples at peak 100: 16QAM and
    64QAM at 24 PRB, QPSK at 10 PRB, 64QAM at 99 PRB): every MAXLOG soft bit has the sign of the transmitted coded bit and none is 0."""
    import openlte_amd as m
    un25 = Units(ctx, 25, [1, 6, 9], 77, [[grant(0, 2, 15, 24, 0, 0x71)], [grant(1, 3, 26, 24, 1, 0x72, rv=1)], [grant(2, 1, 9, 10, 5, 0x73, rv=3)]],
                 0, seed=4, clean=True)
    un100 = Units(ctx, 100, [4], 78, [[grant(0, 3, 26, 99, 0, 0x74)]], 0, seed=5, clean=True)
    for un in (un25, un100):
        plan = un.plan()
        plan.set_demapper(m.DEMAP_MAXLOG, 0.0)
        plan.run(un.d_sub)
        assert ctx.last_kernels().startswith("k_pusch_demod_llr:1,")
        for k, al in enumerate(un.allocs):
            soft, e = plan.soft_bits(k), un.coded(k)
            assert soft.shape == e.shape
            bad = int(((soft < 0) != (e == 1)).sum() + (soft == 0).sum())
            print("noiseless MAXLOG: N_prb %d Q_m %d: %d of %d soft bits off, min |soft| %d" % (al.N_prb, QM[al.mod_type], bad, len(e), int(np.abs(soft.astype(int)).min())))
            assert bad == 0, (al.N_prb, al.mod_type, bad)
        plan.close()
        un.free()


def test_value_every_block_with_soft_decisions_none_without(ctx):
    """The class VALUE_CLASS of profiles/pusch_llr_sweep.txt (16 transport blocks per point, the sweep's seeds): at VALUE_SNR_DB and 1 dB
    under it MAXLOG decodes every block -- status 0, the payload equal to the transmitted bits -- and at VALUE_SNR_DB and 1 dB over it the
    default demapper decodes none, on the same subframes."""
    import openlte_amd as m
    import pusch_llr_sweep as sw
    for snr, modes in ((VALUE_SNR_DB - 1, (m.DEMAP_MAXLOG,)), (VALUE_SNR_DB, (m.DEMAP_MAXLOG, m.DEMAP_REF)), (VALUE_SNR_DB + 1, (m.DEMAP_REF,))):
        p = sw.Point(ctx, VALUE_CLASS, float(snr), 16)
        for mode in modes:
            ok = p.decoded(mode)
            print("%s at %d dB, demapper %d: %d of %d transport blocks decoded" % (VALUE_CLASS, snr, mode, ok.sum(), len(ok)))
            assert ok.all() if mode == m.DEMAP_MAXLOG else not ok.any(), (snr, mode, ok)
        p.close()


def test_edges_zeroed_dmrs_sub_carriers(ctx):
    """Fixed gain, plan A.  (1) One sub-carrier of the 16QAM allocation zeroed on DMRS symbol 0 alone: the polar interpolation runs its
    magnitude from 0 to the other slot's estimate, so no data symbol has a zero estimate -- the symbols it poisons are the model's (none;
    asserted), every rho_s of the allocation stays positive and matches the restatement, and the other allocations' bytes do not move.
    (2) The same sub-carrier zeroed on both DMRS symbols: the estimate is 0 on all twelve data symbols, every rho_s of that allocation is
    0 and every byte of it is 0; the other allocations' bytes and rho do not move."""
    import openlte_amd as m
    un = units_of(ctx, "A", 20.0)
    plan = un.plan()
    n = len(un.allocs)
    plan.set_demapper(m.DEMAP_MAXLOG, 0.0)
    plan.run(un.d_sub)
    fixed = float(np.median(plan.llr_gain()))
    plan.set_demapper(m.DEMAP_MAXLOG, fixed)
    plan.run(un.d_sub)
    before, rho0 = [plan.soft_bits(a) for a in range(n)], plan.llr_rho()
    planes = un.d_sub.download(np.float32).reshape(len(un.sfs), 2, 16, pm.N_SC)
    a = 4  # unit 1's 6-PRB 16QAM allocation
    al = un.allocs[a]
    assert (al.unit, al.N_prb, al.mod_type) == (1, 6, 2)
    dmrs = m.ul_dmrs_pusch(un.ul, un.cells[1], un.sfs[1], al.N_prb)
    for rows in ((3,), (3, 10)):
        holed = planes.copy()
        for L in rows:
            holed[1, :, L, pm.subcarriers(al, L // 7)[17]] = 0
        want, w_min, w_mean = pm.rho_of(pm.h_polar(holed[1], al, dmrs))
        poisoned = want == 0
        assert (w_min[~poisoned] >= 1e-3 * w_mean).all()  # (the tolerance's own condition, test_rho_against_the_float64_restatement)
        assert poisoned.sum() == (0 if len(rows) == 1 else 12)
        d = ctx.to_device(holed)
        plan.run(d)
        d.free()
        rho = plan.llr_rho()
        print("DMRS rows %s zeroed on one sub-carrier: rho %s" % (rows, rho[a]))
        assert (rho[a][poisoned] == 0).all() and (rho[a][~poisoned] > 0).all()
        assert (np.abs(rho[a][~poisoned] - want[~poisoned]) <= 1e-4 * want[~poisoned]).all()
        e = plan.soft_bits(a).reshape(-1, 12, QM[al.mod_type])
        assert not e[:, poisoned].any()
        assert (plan.llr_gain() == np.float32(fixed)).all()
        for b in range(n):
            if b != a:
                assert (plan.soft_bits(b) == before[b]).all() and (rho[b] == rho0[b]).all(), b
    plan.close()
    un.free()


def test_edges_zero_grid_and_rails(ctx):
    """An all-zero grid under the automatic gain: all-zero bytes with the default plan's e_len, finite zero gains and rho, status 2 and no
    cb_ok bit (the erasure rule of the mode's verdict).  A gain of 1e9 x the automatic one: every byte is +-127."""
    import openlte_amd as m
    un = units_of(ctx, "A", 20.0)
    plan = un.plan()
    n = len(un.allocs)
    plan.run(un.d_sub)
    e_len = [len(plan.soft_bits(b)) for b in range(n)]
    plan.set_demapper(m.DEMAP_MAXLOG, 0.0)
    plan.run(un.d_sub)
    auto = plan.llr_gain()
    assert (auto > 0).all()
    zero = ctx.alloc(un.d_sub.nbytes)
    zero.zero()
    st, bits = plan.run(zero)
    zero.free()
    g, rho = plan.llr_gain(), plan.llr_rho()
    print("all-zero grid: status %s, gains %s" % (list(st), list(g)))
    assert all(len(plan.soft_bits(b)) == e_len[b] and not plan.soft_bits(b).any() for b in range(n))
    assert np.isfinite(g).all() and (g == 0).all() and np.isfinite(rho).all() and (rho == 0).all()
    assert (st == 2).all() and not plan.cb_ok().any()
    big = float(np.float32(1e9 * auto.max()))
    plan.set_demapper(m.DEMAP_MAXLOG, big)
    plan.run(un.d_sub)
    for b in range(n):
        assert (np.abs(plan.soft_bits(b).astype(int)) == 127).all(), b
    assert (plan.llr_gain() == np.float32(big)).all()
    plan.close()
    un.free()


def test_refusals_leave_the_plan_as_it_was(ctx):
    """An unknown mode, a negative, infinite or NaN gain, a NULL plan: INVALID_ARG; MAXLOG on a reference-mode plan: UNSUPPORTED, REF accepted
    there.  After each the plan runs as before.  The taps on a reference-mode plan: INVALID_ARG; before any run: zeros; the symbol tap
    before set_llr_tap: INVALID_ARG.  (Plans with control information accept MAXLOG: test_control_information_on_graded_bytes.)"""
    import openlte_amd as m
    L = ctx.L
    un = units_of(ctx, "B", 20.0)
    plan = un.plan()
    p, cnt = C.c_void_p(), C.c_uint32()
    # before any run
    assert (plan.llr_gain() == 0).all() and (plan.llr_rho() == 0).all()
    assert L.mi_lte_pusch_plan_llr_symbols(plan.h, 0, C.byref(p), C.byref(cnt)) == ERR_INVALID
    plan.set_llr_tap(True)
    assert plan.llr_symbols(0).shape == (12, 72) and not plan.llr_symbols(0).any()
    plan.set_llr_tap(False)
    assert L.mi_lte_pusch_plan_llr_symbols(plan.h, 0, C.byref(p), C.byref(cnt)) == ERR_INVALID
    plan.set_demapper(m.DEMAP_MAXLOG, 0.0)
    want = outputs(plan, un)

    def same():
        got = outputs(plan, un)
        assert ctx.last_kernels().startswith("k_pusch_demod_llr:1,")
        assert same_outputs(got, want)

    for mode, gain in ((2, 0.0), (0xFFFFFFFF, 1.0), (m.DEMAP_MAXLOG, -1.0), (m.DEMAP_MAXLOG, float("inf")), (m.DEMAP_MAXLOG, float("nan"))):
        assert L.mi_lte_pusch_plan_set_demapper(plan.h, mode, gain) == ERR_INVALID, (mode, gain)
        same()
    assert L.mi_lte_pusch_plan_set_demapper(None, m.DEMAP_MAXLOG, 0.0) == ERR_INVALID
    assert L.mi_lte_pusch_plan_llr_gain(None, C.byref(p)) == ERR_INVALID and L.mi_lte_pusch_plan_llr_gain(plan.h, None) == ERR_INVALID
    assert L.mi_lte_pusch_plan_llr_rho(None, C.byref(p)) == ERR_INVALID and L.mi_lte_pusch_plan_llr_rho(plan.h, None) == ERR_INVALID
    assert L.mi_lte_pusch_plan_set_llr_tap(None, 1) == ERR_INVALID
    assert L.mi_lte_pusch_plan_llr_symbols(plan.h, len(un.allocs), C.byref(p), C.byref(cnt)) == ERR_INVALID
    # a reference-mode plan (QPSK, one code block): refused, still runs its own demapper; REF is accepted there
    one = [grant(0, 1, 9, 6, 3, 0x71)]
    ref_plan = ctx.pusch_plan(un.cfg, un.ul, un.sfs[:1], un.cells[:1], one)
    ref_plan.run(un.d_sub)
    e0 = ref_plan.soft_bits(0)
    assert L.mi_lte_pusch_plan_set_demapper(ref_plan.h, m.DEMAP_MAXLOG, 0.0) == ERR_UNSUPPORTED
    assert L.mi_lte_pusch_plan_set_demapper(ref_plan.h, m.DEMAP_REF, 0.0) == 0
    assert L.mi_lte_pusch_plan_llr_gain(ref_plan.h, C.byref(p)) == ERR_INVALID and L.mi_lte_pusch_plan_llr_rho(ref_plan.h, C.byref(p)) == ERR_INVALID
    assert L.mi_lte_pusch_plan_set_llr_tap(ref_plan.h, 1) == ERR_INVALID
    assert L.mi_lte_pusch_plan_llr_symbols(ref_plan.h, 0, C.byref(p), C.byref(cnt)) == ERR_INVALID
    ref_plan.run(un.d_sub)
    assert ctx.last_kernels().startswith("k_pusch_demod:1,") and (ref_plan.soft_bits(0) == e0).all()
    ref_plan.close()
    same()
    plan.close()
    un.free()
