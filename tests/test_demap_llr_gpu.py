"""GPU: the 3GPP PDSCH plans' max-log soft-decision demapper (mi_lte_pdsch_plan_set_demapper, k_pdsch_demod_llr<1>; tests/test_txdiv_gpu.py runs
the same kernel and the same model on two and four ports).  Its bytes and gains against the float64 model of include/mi_lte.h's text (tests/demap_llr_model.py); a plan that never opts in, or opts out again, is the plan it was;
everything after the soft-bit buffer does with the graded bytes what it does with the default demapper's (rate un-matching, the BCJR model,
the HARQ sat16 chain); and what the soft decisions buy: at an SNR profiles/demap_llr_sweep.txt names, every transport block of the sweep's
64QAM class decodes with them and none without."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

import demap_llr_model as dm
from test_dlsch3gpp_gpu import FFT, check_blocks_exact, tbs
from test_harq_gpu import Tx, decode, gather_sums, sat16

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))

pytestmark = pytest.mark.gpu

ERR_INVALID, ERR_UNSUPPORTED = -1, -4
N_SOFT = 1237248
# profiles/demap_llr_sweep.txt (16 transport blocks per point, the sweep's seeds).  Its two rate-0.5 classes draw every unit's channel gain from
# 0.5 .. 1.5, which spreads a point's blocks over 9.5 dB: no SNR of theirs has one demapper decode every block and the other none.  The value
# and HARQ points are therefore taken from the sweep's unit-gain classes: the same 64QAM transport block, every unit at gain 1.
VALUE_CLASS, VALUE_SNR_DB = "64qam_r0.33_flat", 6  # MAXLOG: 16 / 16 here and at 5 dB; the default demapper: 0 / 16 here and at 7 dB
HARQ_CLASS, HARQ_SNR_DB = "64qam_r0.5_flat", 5     # one transmission: 0 / 16 under either demapper (3 .. 6 dB)


def mk(unit, mod, size, prbs, rnti, rv=0, cfi=0):
    import openlte_amd as m
    return m.make_alloc(unit, mod, size, list(prbs), rnti, rv_idx=rv, n_pdcch_symbs=cfi)


def case(name):
    """(n_rb, plan cfi, subframes, cells, allocations per unit, direct stores).  The smallest shapes the kernel can go wrong at: 1 and 6 PRB in a
    6-RB cell in subframes 0 (PBCH + sync signals over the whole band), 5 and 3; allocations astride the 25-RB cell's PBCH / PSS / SSS window
    (sub-carriers 114..185: PRBs 9 and 15 split 6 + 6) in subframes 0 and 5; control regions of 1, 2 and 3 symbols, one of them the
    allocation's own; the three modulations in one plan; one 100-PRB 64QAM allocation (90 000 soft bits: past the LDS cap, so stored directly;
    a pair table of 1 400 entries)."""
    if name == "6rb_1prb":
        return 6, 3, [0, 5, 3], [11, 250, 77], [[mk(u, 1, tbs(0, 1), [0], 0x21), mk(u, 2, tbs(0, 1), [2], 0x22), mk(u, 3, tbs(0, 1), [5], 0x23, cfi=2)]
                                                for u in range(3)], False
    if name == "6rb_6prb":
        return 6, 2, [0, 5, 3], [12, 251, 78], [[mk(u, (3, 2, 1)[u], tbs(3, 6), range(6), 0x31 + u)] for u in range(3)], False
    if name == "25rb_window":
        return 25, 1, [0, 5], [301, 42], [[mk(u, 1, tbs(5, 3), [8, 9, 10], 0x41), mk(u, 2, tbs(5, 3), [11, 12, 13], 0x42, cfi=3),
                                           mk(u, 3, tbs(9, 4), [14, 15, 16, 17], 0x43, cfi=2)] for u in range(2)], False
    assert name == "100rb"
    return 100, 1, [4], [503], [[mk(0, 3, tbs(15, 100), range(100), 0x51)]], True


def planes_of(t):
    n = len(t.sfs)
    assert t.ctx.subframe_floats(1) == 4 * 16 * dm.N_SC
    return t.d_sub.download(np.float32).reshape(n, 4, 16, dm.N_SC)


def slot_bytes(plan, al, cfi):
    cfi = al.n_pdcch_symbs if al.n_pdcch_symbs else cfi
    return ((14 - cfi) * al.N_prb * 12 * dm.QM[al.mod_type] + 63) & ~63


def slots(plan, allocs, cfi):
    """Every allocation's whole slot of the soft-bit buffer (its share rounded up to 64 bytes), int8"""
    ctx, out = plan.ctx, []
    for a, al in enumerate(allocs):
        pe, pn = C.c_void_p(), C.c_void_p()
        ctx._check(ctx.L.mi_lte_pdsch_plan_soft_bits(plan.h, a, C.byref(pe), C.byref(pn)))
        buf = np.empty(slot_bytes(plan, al, cfi), np.int8)
        ctx._check(ctx.L.mi_lte_memcpy_d2h(ctx.h, buf.ctypes.data, pe.value, buf.nbytes))
        out.append(buf)
    return out


def model_of(t, planes, n_rb, cfi, gain):
    import openlte_amd as m
    out = []
    for u in range(len(t.sfs)):
        out += dm.demap(planes[u], [al for al in t.allocs if al.unit == u], t.sfs[u], t.cells[u], n_rb, cfi, gain=gain, T=m.DEMAP_AUTO_T)
    return out


def check_against_model(plan, t, model, gain):
    """The rules of the bytes: identical outside the guard band, at most one step inside it, the band under 1 % of the soft bits; the gains within
    2^-18 (automatic) or the argument itself (fixed).  Returns every byte of the plan."""
    gains = plan.llr_gain()
    n_guard = n_all = 0
    every = []
    for a, (al, r) in enumerate(zip(t.allocs, model)):
        e = plan.soft_bits(a)
        assert len(e) == len(r.bytes) > 0, (a, len(e), len(r.bytes))
        d = np.abs(e.astype(np.int32) - r.bytes)
        guard = dm.in_guard(r.x)
        print("allocation %d: %d soft bits, %d in the guard band, %d differ (%d of them outside it), largest difference %d; gain %.9g, model %.9g"
              % (a, len(e), guard.sum(), (d != 0).sum(), (d[~guard] != 0).sum(), d.max(), gains[a], r.gain))
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


@pytest.mark.parametrize("snr_db", [20.0, 5.0])
@pytest.mark.parametrize("name", ["6rb_1prb", "6rb_6prb", "25rb_window", "100rb"])
def test_bytes_and_gains_against_the_model(ctx, name, snr_db):
    """max_delay = 4 and noise at 20 and 5 dB: w varies over the allocation and the clamp is reached.  Automatic gain, then a fixed one on the
    same plan; e_len and every byte outside the allocations' ranges as the default demapper's run left them."""
    import openlte_amd as m
    n_rb, cfi, sfs, cells, per_unit, direct = case(name)
    t = Tx(ctx, n_rb, sfs, cells, per_unit, N_SOFT, cfi, snr_db, seed=int(snr_db) + len(name))
    planes = planes_of(t)
    plan = t.plan(N_SOFT)
    decode(t, plan)
    assert ctx.last_kernels().startswith("k_pdsch_demod:1,")
    ref_len, ref_slots = [len(plan.soft_bits(a)) for a in range(plan.n_alloc)], slots(plan, t.allocs, cfi)
    auto = model_of(t, planes, n_rb, cfi, 0.0)
    fixed = float(np.float32(1.5 * np.median([r.gain for r in auto])))  # (a fixed gain of the automatic one's order: graded bytes and clamped ones)
    for gain in (0.0, fixed):
        plan.set_demapper(m.DEMAP_MAXLOG, gain)
        decode(t, plan)
        assert ctx.last_kernels().startswith("k_pdsch_demod_llr:1,k_dl3_desc:1,k_dl3_rm_i8:1,")
        e = check_against_model(plan, t, auto if gain == 0 else model_of(t, planes, n_rb, cfi, gain), gain)
        assert (np.abs(e) == 127).any() and (np.abs(e) < 127).any()
        got = slots(plan, t.allocs, cfi)
        for a in range(plan.n_alloc):
            n = len(plan.soft_bits(a))
            assert n == ref_len[a], a
            keep = n if direct else (n + 15) & ~15  # (assembled in LDS, an allocation leaves in 16-byte stores)
            assert (got[a][keep:] == ref_slots[a][keep:]).all(), a
    plan.close()
    t.free()


def test_opt_in_is_inert(ctx):
    """The same input through a plan that never calls the setter and through one set to MAXLOG, run, and set back to REF: soft bits, output rows,
    verdicts and cb_soft byte for byte, and last_kernels names k_pdsch_demod."""
    import openlte_amd as m
    n_rb, cfi, sfs, cells, per_unit, _ = case("25rb_window")
    t = Tx(ctx, n_rb, sfs, cells, per_unit, N_SOFT, cfi, 9.0, seed=3)
    plain, other = t.plan(N_SOFT), t.plan(N_SOFT)
    want = decode(t, plain)
    assert ctx.last_kernels().startswith("k_pdsch_demod:1,")
    want_e = [plain.soft_bits(a) for a in range(plain.n_alloc)]
    other.set_demapper(m.DEMAP_MAXLOG, 0.0)
    mid = decode(t, other)
    assert ctx.last_kernels().startswith("k_pdsch_demod_llr:1,")
    assert any((other.soft_bits(a) != want_e[a]).any() for a in range(plain.n_alloc))
    other.set_demapper(m.DEMAP_REF, 123.0)
    got = decode(t, other)
    assert ctx.last_kernels().startswith("k_pdsch_demod:1,")
    assert (got["st"] == want["st"]).all() and (got["rows"] == want["rows"]).all() and (got["cb_ok"] == want["cb_ok"]).all()
    for a in range(plain.n_alloc):
        assert (other.soft_bits(a) == want_e[a]).all() and (got["cb_soft"][a] == want["cb_soft"][a]).all(), a
    assert mid["st"].shape == want["st"].shape
    for p in (plain, other):
        p.close()
    t.free()


def mixed_units(rv=0):
    """25 RB, two units: a two-block 64QAM grant next to a QPSK one, and a 16QAM grant in subframe 5"""
    return [3, 5], [17, 301], [[mk(0, 3, tbs(20, 18), range(0, 18), 0x61, rv=rv), mk(0, 1, tbs(9, 7), range(18, 25), 0x62, rv=rv)],
                               [mk(1, 2, tbs(14, 12), range(5, 17), 0x63, rv=rv), mk(1, 3, tbs(20, 8), range(17, 25), 0x64, rv=rv)]]


def test_downstream_unchanged(ctx, port, ref, ref_phy):
    """A MAXLOG plan: cb_soft is the reference's rate un-matching of the tapped soft bits, summed and saturated; the output rows, verdicts and
    cb_ok are the plain-C BCJR model's on those blocks (test_dlsch3gpp_gpu.check_blocks_exact)."""
    import openlte_amd as m
    n_soft = 125184
    sfs, cells, per_unit = mixed_units(rv=1)
    t = Tx(ctx, 25, sfs, cells, per_unit, n_soft, 2, 8.0, seed=11)
    plan = t.plan(n_soft)
    plan.set_demapper(m.DEMAP_MAXLOG, 0.0)
    st, bits = plan.run(t.d_sub, sfs, cells)
    seen, n_pass, n_fail = check_blocks_exact(port, ref, ref_phy, plan, t.allocs, [(st, bits, plan.cb_ok())], n_soft)
    assert {nc for nc, K, lim in seen} >= {1, 2}
    e = np.concatenate([plan.soft_bits(a) for a in range(plan.n_alloc)])
    assert len(np.unique(np.abs(e))) > 64  # (graded bytes went through)
    plan.close()
    t.free()


def test_harq_first_transmission_and_sat16_chain(ctx, ref, ref_phy):
    """MAXLOG through mi_lte_pdsch_decode_run_harq: a first transmission is the plain MAXLOG run byte for byte; after rv 0 and then rv 2 the int16
    buffer is the sat16 chain over the two runs' tapped soft bits, exactly."""
    import openlte_amd as m
    n_soft = 125184
    pool = ctx.harq_pool(8)
    model, payload = {}, None
    for k, rv in enumerate((0, 2)):
        sfs, cells, per_unit = mixed_units(rv=rv)
        t = Tx(ctx, 25, sfs, cells, per_unit, n_soft, 2, 6.0 + k, seed=20 + k, payload=payload)
        payload = t.tx
        plan = t.plan(n_soft)
        plan.set_demapper(m.DEMAP_MAXLOG, 0.0)
        n = plan.n_alloc
        if k == 0:
            plain = decode(t, plan)
            e_plain = [plan.soft_bits(a) for a in range(n)]
            first = decode(t, plan, pool, list(range(4, 4 + n)), True)
            assert ctx.last_kernels().startswith("k_pdsch_demod_llr:1,k_dl3_desc:1,k_harq_bind:1,k_harq_rm:1,")
            assert (first["st"] == plain["st"]).all() and (first["rows"] == plain["rows"]).all() and (first["cb_ok"] == plain["cb_ok"]).all()
            for a in range(n):
                assert (first["cb_soft"][a] == plain["cb_soft"][a]).all() and (plan.soft_bits(a) == e_plain[a]).all(), a
        h = decode(t, plan, pool, list(range(n)), k == 0)
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


class GainTx(Tx):
    """Tx with the synthesiser's range of channel gains as an argument"""

    def __init__(self, ctx, n_rb, sfs, cells, per_unit, n_soft, cfi, snr_db, seed, payload=None, gain=(0.5, 1.5)):
        import openlte_amd as m
        from openlte_amd import synth
        self.ctx, self.cfg, self.cfi, self.sfs, self.cells = ctx, m.DlCfg(FFT[n_rb], n_rb, 1, 0), cfi, list(sfs), list(cells)
        self.n_alloc = len(per_unit[0])
        self.allocs = [a for row in per_unit for a in row]
        iq, self.tx = synth.dl_units_3gpp(self.cfg, sfs, cells, self.allocs, self.n_alloc, n_soft, n_pdcch_symbs=cfi, gain=gain, snr_db=snr_db,
                                          max_delay=4, seed=seed, payload=payload)
        n, ul = len(sfs), iq.shape[1]
        d_iq, d_start = ctx.to_device(iq.reshape(-1, 2)), ctx.to_device((np.arange(n) * ul).astype(np.uint64))
        self.d_sf, self.d_cell = ctx.to_device(np.asarray(sfs, np.uint32)), ctx.to_device(np.asarray(cells, np.uint32))
        self.d_sub = ctx.alloc(n * ctx.subframe_floats(1) * 4)
        ctx.dl_frontend_dev(self.cfg, d_iq, None, d_start, self.d_sf, self.d_cell, n, self.d_sub)
        d_iq.free()
        d_start.free()


def sweep_point(ctx, name, snr_db, payload=None, rv=0, seed_shift=0):
    """One class of the sweep at one SNR, with its seeds (tools/demap_llr_sweep.py): the units on the device."""
    import demap_llr_sweep as sw
    sfs, cells, allocs = sw.class_units(name, 16)
    per_unit = [[mk(al.unit, al.mod_type, al.tbs, [al.prb[0][i] for i in range(al.N_prb)], al.rnti, rv=rv)] for al in allocs]
    return GainTx(ctx, sw.N_RB, sfs, cells, per_unit, sw.N_SOFT, sw.CFI, float(snr_db), seed=sw.point_seed(name, snr_db) + seed_shift, payload=payload,
                  gain=sw.CLASSES[name][3])


def decoded(t, plan, h):
    return np.array([h["st"][a] == 0 and (h["rows"][a, :al.tbs] == t.payload(a)).all() for a, al in enumerate(t.allocs)])


def test_value_every_block_with_soft_decisions_none_without(ctx):
    """The class VALUE_CLASS of profiles/demap_llr_sweep.txt (64QAM, one code block, 16 transport blocks per point, the sweep's seeds; the
    issue's 64QAM class at code rate 0.5 has no such SNR, with or without the spread of channel gains: at unit gain MAXLOG decodes every
    block from 8 dB and the default demapper none up to 9 dB, one step short; at code rate 0.33 the window is open): at VALUE_SNR_DB and
    1 dB under it MAXLOG decodes every block -- status 0, the payload equal to the transmitted bits -- and at VALUE_SNR_DB and 1 dB over it
    the default demapper decodes none, on the same subframes."""
    import openlte_amd as m
    for snr, modes in ((VALUE_SNR_DB - 1, (m.DEMAP_MAXLOG,)), (VALUE_SNR_DB, (m.DEMAP_MAXLOG, m.DEMAP_REF)), (VALUE_SNR_DB + 1, (m.DEMAP_REF,))):
        t = sweep_point(ctx, VALUE_CLASS, snr)
        plan = t.plan(N_SOFT)
        for mode in modes:
            plan.set_demapper(mode, 0.0)
            ok = decoded(t, plan, decode(t, plan))
            print("%d dB, demapper %d: %d of %d transport blocks decoded" % (snr, mode, ok.sum(), len(ok)))
            assert ok.all() if mode == m.DEMAP_MAXLOG else not ok.any(), (snr, mode, ok)
        plan.close()
        t.free()


def test_harq_pair_decodes_what_one_transmission_cannot(ctx):
    """HARQ_CLASS at HARQ_SNR_DB, where profiles/demap_llr_sweep.txt has one transmission fail under both demappers: rv 0 fails alone under
    both; rv 0 and rv 2 combined in the pool under MAXLOG decode every block."""
    import openlte_amd as m
    pool = ctx.harq_pool(32)
    payload = None
    for k, rv in enumerate((0, 2)):
        t = sweep_point(ctx, HARQ_CLASS, HARQ_SNR_DB, payload=payload, rv=rv, seed_shift=5000 * k)
        payload = t.tx
        plan = t.plan(N_SOFT)
        n = plan.n_alloc
        for mode in (m.DEMAP_REF, m.DEMAP_MAXLOG):
            plan.set_demapper(mode, 0.0)
            alone = decoded(t, plan, decode(t, plan))
            print("rv %d alone, demapper %d: %d of %d decoded" % (rv, mode, alone.sum(), n))
            if rv == 0:
                assert not alone.any(), (mode, alone)
        h = decode(t, plan, pool, list(range(n)), k == 0)
        ok = decoded(t, plan, h)
        print("after transmission %d: %d of %d decoded" % (k + 1, ok.sum(), n))
        if k == 1:
            assert ok.all(), ok
            assert all(pool.state(a)["n_tx"] == 2 for a in range(n))
        plan.close()
        t.free()
    pool.close()


def test_edges(ctx):
    """One zeroed estimate element: 0 for its Q_m bytes only (fixed gain: the others do not move).  A large fixed gain: every byte on the
    +-127 rails."""
    import openlte_amd as m
    n_rb, cfi, sfs, cells, per_unit, _ = case("25rb_window")
    t = Tx(ctx, n_rb, sfs, cells, per_unit, N_SOFT, cfi, 20.0, seed=8)
    plan = t.plan(N_SOFT)
    n = plan.n_alloc
    plan.set_demapper(m.DEMAP_MAXLOG, 0.0)
    decode(t, plan)
    fixed = float(plan.llr_gain().mean())  # (a fixed gain of the automatic one's order)
    plan.set_demapper(m.DEMAP_MAXLOG, fixed)
    decode(t, plan)
    before = [plan.soft_bits(a) for a in range(n)]
    planes = planes_of(t)
    # the 64QAM allocation of unit 1: its 100th resource element
    a = 5
    al = t.allocs[a]
    pos = dm.pdsch_res(al, t.sfs[1], t.cells[1], n_rb, cfi)[100]
    holed = planes.copy()
    holed.reshape(2, 4, -1)[1, 2:, pos] = 0
    keep = t.d_sub
    t.d_sub = ctx.to_device(holed)
    decode(t, plan)
    for b in range(n):
        e = plan.soft_bits(b)
        if b == a:
            assert not e[600:606].any() and before[a][600:606].any()
            e = e.copy()
            e[600:606] = before[a][600:606]
        assert (e == before[b]).all(), b
    # rails
    plan.set_demapper(m.DEMAP_MAXLOG, 1e9 * fixed)
    t.d_sub.free()
    t.d_sub = keep
    decode(t, plan)
    for b in range(n):
        assert (np.abs(plan.soft_bits(b)) == 127).all(), b
    assert (plan.llr_gain() == np.float32(1e9 * fixed)).all()
    plan.close()
    t.free()


def test_all_zero_grid_and_estimate(ctx):
    """An all-zero grid and an all-zero h: all-zero soft bits with the default plan's e_len, no NaN in the gain tap (0 under the automatic
    gain), status 2 and no CRC bit in cb_ok: all-zero channel values make every BCJR decision 0, and the all-zero block divides by both CRC
    generators, so the verdict kernels treat a block without a single non-zero channel value as an erasure."""
    import openlte_amd as m
    n_rb, cfi, sfs, cells, per_unit, _ = case("25rb_window")
    t = Tx(ctx, n_rb, sfs, cells, per_unit, N_SOFT, cfi, 20.0, seed=8)
    plan = t.plan(N_SOFT)
    decode(t, plan)
    e_len = [len(plan.soft_bits(b)) for b in range(plan.n_alloc)]
    t.d_sub.zero()
    plan.set_demapper(m.DEMAP_MAXLOG, 0.0)
    h = decode(t, plan)
    g = plan.llr_gain()
    print("all-zero input: status %s, gains %s" % (list(h["st"]), list(g)))
    assert all(len(plan.soft_bits(b)) == e_len[b] and not plan.soft_bits(b).any() for b in range(plan.n_alloc))
    assert np.isfinite(g).all() and (g == 0).all(), g
    assert (h["st"] == 2).all(), h["st"]
    assert not h["cb_ok"].any() and not any(b.any() for b in h["cb_soft"])
    plan.close()
    t.free()


def test_refusals_leave_the_plan_runnable(ctx):
    """MAXLOG on a reference-mode plan and on a compact-estimate 3GPP plan: UNSUPPORTED; an unknown mode, a negative, infinite or NaN gain, a
    NULL plan: INVALID_ARG.  After each the plan runs as before."""
    import openlte_amd as m
    L = ctx.L
    n_rb, cfi, sfs, cells, per_unit, _ = case("25rb_window")
    t = Tx(ctx, n_rb, sfs, cells, per_unit, N_SOFT, cfi, 20.0, seed=9)
    plan = t.plan(N_SOFT)
    plan.set_demapper(m.DEMAP_MAXLOG, 0.0)
    want = decode(t, plan)
    want_e = [plan.soft_bits(a) for a in range(plan.n_alloc)]

    def same():
        got = decode(t, plan)
        assert ctx.last_kernels().startswith("k_pdsch_demod_llr:1,")
        assert (got["st"] == want["st"]).all() and (got["rows"] == want["rows"]).all()
        assert all((plan.soft_bits(a) == want_e[a]).all() for a in range(plan.n_alloc))

    for mode, gain, rc in ((2, 0.0, ERR_INVALID), (0xFFFFFFFF, 1.0, ERR_INVALID), (m.DEMAP_MAXLOG, -1.0, ERR_INVALID),
                           (m.DEMAP_MAXLOG, float("inf"), ERR_INVALID), (m.DEMAP_MAXLOG, float("nan"), ERR_INVALID)):
        assert L.mi_lte_pdsch_plan_set_demapper(plan.h, mode, gain) == rc, (mode, gain)
        same()
    assert L.mi_lte_pdsch_plan_set_demapper(None, m.DEMAP_MAXLOG, 0.0) == ERR_INVALID
    p = C.c_void_p()
    assert L.mi_lte_pdsch_plan_llr_gain(None, C.byref(p)) == ERR_INVALID and L.mi_lte_pdsch_plan_llr_gain(plan.h, None) == ERR_INVALID
    # a reference-mode plan: refused, and it still runs its own demapper; REF is accepted there
    ref_plan = ctx.pdsch_plan(t.cfg, cfi, [mk(0, 1, tbs(5, 3), [8, 9, 10], 0x41)])
    assert L.mi_lte_pdsch_plan_set_demapper(ref_plan.h, m.DEMAP_MAXLOG, 0.0) == ERR_UNSUPPORTED
    assert L.mi_lte_pdsch_plan_set_demapper(ref_plan.h, m.DEMAP_REF, 0.0) == 0
    assert L.mi_lte_pdsch_plan_llr_gain(ref_plan.h, C.byref(p)) == ERR_INVALID
    ref_plan.run(t.d_sub, t.sfs, t.cells)
    assert ctx.last_kernels().startswith("k_pdsch_demod:1,")
    ref_plan.close()
    # a 3GPP plan over the compact estimate format
    compact = ctx.pdsch_plan_3gpp(m.DlCfg(t.cfg.fft_size, n_rb, 1, m.CE_COMPACT), cfi, t.allocs, N_SOFT)
    assert L.mi_lte_pdsch_plan_set_demapper(compact.h, m.DEMAP_MAXLOG, 0.0) == ERR_UNSUPPORTED
    compact.close()
    same()
    plan.close()
    t.free()
