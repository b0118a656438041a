"""GPU: the PUSCH plans' 3GPP transport-block mode (mi_lte_pusch_plan_create_3gpp): the demodulator with the transform pre-decoder scaled
as 36.211 5.3.3 has it, and UL-SCH transport blocks of 1..13 code blocks (36.212 5.2.2).  The reference cannot decode these (its
pre-decoder scales by sqrt(M) and its UL-SCH handles one block), so each stage is pinned to what specifies it: the soft bits' signs to the
reference-mode plan's and to the transmitted coded bits, rate un-matching to the reference's own liblte_phy_rate_unmatch_turbo run as
ULSCH with N_codeblocks = C, the decode to the plain-C model of the BCJR decoder the plan ran, the assembly to a numpy desegmentation with
both CRCs, and the whole chain to the transmitted bits (mi_lte_synth_ul_units_3gpp_i8)."""
import ctypes as C

import numpy as np
import pytest

from test_dlsch3gpp_gpu import expect_from_blocks, tbs
from test_ulsch3gpp_cpu import CHAN_ULSCH

pytestmark = pytest.mark.gpu

ERR_INVALID, ERR_UNSUPPORTED = -1, -4
FFT = {25: 512, 100: 2048}
ULC = (3, 0, 0, 2, 1)
QM = {1: 2, 2: 4, 3: 6}


def grant(unit, mod, itbs, n_prb, prb0, rnti, rv=0):
    import openlte_amd as m
    return m.make_alloc(unit, mod, tbs(itbs, n_prb), list(range(prb0, prb0 + n_prb)), rnti, rv_idx=rv)


class Units:
    """Uplink units of one cell from the 3GPP transmitter, through the front end: .allocs (unit-major), .tx, .d_sub (device subframes)."""

    def __init__(self, ctx, n_rb, sfs, cell, per_unit, snr_db, seed, clean=False):
        import openlte_amd as m
        from openlte_amd import synth
        self.ctx, self.cfg, self.ul = ctx, m.DlCfg(FFT[n_rb], n_rb, 1, 0), m.UlCfg(*ULC)
        self.sfs, self.cells, self.n_alloc = list(sfs), [cell] * len(sfs), len(per_unit[0])
        self.allocs = [a for u in per_unit for a in u]
        chan = dict(gain=(1.0, 1.0), max_delay=0, snr_db=200.0) if clean else dict(max_delay=3, snr_db=snr_db)  # clean: noiseless, static
        self.iq, self.tx = synth.ul_units_3gpp(self.cfg, self.ul, self.sfs, self.cells, self.allocs, self.n_alloc, peak=100.0, seed=seed, **chan)
        n = len(self.sfs)
        _, self.d_sub = ctx.ul_frontend(self.cfg, self.iq.reshape(-1, 2), np.arange(n) * self.iq.shape[1], keep=True)

    def plan(self, spec=True):
        make = self.ctx.pusch_plan_3gpp if spec else self.ctx.pusch_plan
        return make(self.cfg, self.ul, self.sfs, self.cells, self.allocs)

    def sent(self, k):
        return self.tx[k // self.n_alloc, k % self.n_alloc, :self.allocs[k].tbs]

    def coded(self, k):
        """the G coded bits of allocation k in the order of the plan's soft bits (before the channel interleaver)"""
        from openlte_amd import synth
        al = self.allocs[k]
        return synth.ulsch_encode_3gpp(self.sent(k), 12 * 12 * al.N_prb * QM[al.mod_type], QM[al.mod_type], al.rv_idx)

    def free(self):
        self.d_sub.free()


def run_decoders(units, decoders, packed=False):
    plan = units.plan()
    if packed:
        plan.set_packed(True)
    res = []
    for mode, n_iter in decoders:
        plan.set_decoder(mode, n_iter, 1)
        st, bits = plan.run(units.d_sub)
        res.append((st, bits, plan.cb_ok()))
    return plan, res


# ---- demodulator

def test_demodulator_signs_equal_the_reference_mode_plan(ctx):
    """15 dB, single-block QPSK / 16QAM / 64QAM grants on a 25-RB cell through both kinds of plan: a positive factor on the de-mapper's
    input moves no sign of a QPSK soft bit, and cannot move the half-plane bits (q = 0, 1) of a 16QAM / 64QAM symbol at all -- they agree
    byte for byte.  The amplitude bits (q >= 2) are decisions on |x| against fixed thresholds, so they are exactly what the factor changes:
    the reference-mode plan sees M times the point and puts every symbol in the outermost ring, which is the defect this mode removes."""
    per_unit = [[grant(0, 1, 9, 10, 0, 0x61), grant(0, 2, 15, 12, 10, 0x62, rv=1)],
                [grant(1, 3, 22, 6, 3, 0x63), grant(1, 1, 9, 6, 12, 0x64, rv=2)]]
    un = Units(ctx, 25, [2, 7], 40, per_unit, 15.0, seed=3)
    p_ref, p_3g = un.plan(spec=False), un.plan()
    p_ref.run(un.d_sub)
    p_3g.run(un.d_sub)
    assert "k_pusch_demod" in ctx.last_kernels() and "k_dl3_rm_i8" in ctx.last_kernels()
    for k, al in enumerate(un.allocs):
        a, b = p_ref.soft_bits(k), p_3g.soft_bits(k)
        assert a.shape == b.shape == (12 * 12 * al.N_prb * QM[al.mod_type],)
        assert (a != 0).all() and (b != 0).all()
        q = QM[al.mod_type]
        if al.mod_type == 1:
            assert ((a < 0) == (b < 0)).all(), k
            assert (np.abs(a.astype(int)) == 1).all() and np.abs(b.astype(int)).max() > 64  # saturated there, soft here
        else:
            assert (a.reshape(-1, q)[:, :2] == b.reshape(-1, q)[:, :2]).all(), k
            assert (a.reshape(-1, q)[:, 2:] != b.reshape(-1, q)[:, 2:]).any()
    p_ref.close()
    p_3g.close()
    un.free()


def test_demodulator_every_soft_bit_noiseless(ctx):
    """Noiseless units (static flat channel, int8 samples at peak 100): every soft bit of a 3GPP plan has the sign of the coded bit the
    transmitter produced -- int8 quantisation leaves a 64QAM decision more than ten standard deviations -- for 16QAM and 64QAM at 24 PRB,
    64QAM at 99 PRB and QPSK; QPSK magnitudes are above 64, where the reference-mode plan gives 1 for every one of them (the defect: its
    de-mapper sees M times the constellation point, and every distance saturates)."""
    un25 = Units(ctx, 25, [1, 6, 9], 77, [[grant(0, 2, 15, 24, 0, 0x71)], [grant(1, 3, 26, 24, 1, 0x72, rv=1)], [grant(2, 1, 9, 10, 5, 0x73, rv=3)]],
                 0, seed=4, clean=True)
    un100 = Units(ctx, 100, [4], 78, [[grant(0, 3, 26, 99, 0, 0x74)]], 0, seed=5, clean=True)
    for un in (un25, un100):
        plan = un.plan()
        plan.run(un.d_sub)
        for k, al in enumerate(un.allocs):
            soft, e = plan.soft_bits(k), un.coded(k)
            assert soft.shape == e.shape
            bad = int(((soft < 0) != (e == 1)).sum() + (soft == 0).sum())
            print("noiseless: N_prb %d Q_m %d: %d of %d soft bits off, min |soft| %d" % (al.N_prb, QM[al.mod_type], bad, len(e), int(np.abs(soft.astype(int)).min())))
            assert bad == 0, (al.N_prb, al.mod_type, bad)
            if al.mod_type == 1:
                assert (np.abs(soft.astype(int)) > 64).all()
        plan.close()
    qpsk = [k for k, al in enumerate(un25.allocs) if al.mod_type == 1]
    import openlte_amd as m
    one = [m.make_alloc(0, 1, un25.allocs[k].tbs, [un25.allocs[k].prb[0][i] for i in range(un25.allocs[k].N_prb)], un25.allocs[k].rnti,
                        rv_idx=un25.allocs[k].rv_idx) for k in qpsk]
    # the same subframe through a reference-mode plan (unit 0 of a buffer that starts at the QPSK unit)
    d_unit = ctx.ul_frontend(un25.cfg, un25.iq[qpsk[0]].reshape(-1, 2), [0], keep=True)[1]
    p_ref = ctx.pusch_plan(un25.cfg, un25.ul, [un25.sfs[qpsk[0]]], [un25.cells[0]], one)
    p_ref.run(d_unit)
    a = p_ref.soft_bits(0)
    assert ((a < 0) == (un25.coded(qpsk[0]) == 1)).all() and (np.abs(a.astype(int)) == 1).all()
    p_ref.close()
    d_unit.free()
    un25.free()
    un100.free()


# ---- code-block stages

def check_blocks_exact(port, ref, ref_phy, plan, allocs, res):
    """test_dlsch3gpp_gpu.check_blocks_exact for the uplink: cb_soft against the reference's rate un-matching (ULSCH: N_cb = K_w) of the
    tap's [off_r, off_r + E_r) slice, NULL -> 0 and sums clamped to +-127; output row, status and cb_ok against the plain-C BCJR models'
    decisions (BCJR x 8, BCJR_BLOCK x 6, the order of res) + the numpy desegmentation.  Returns ({C}, passes, failures)."""
    import openlte_amd as m
    n_fail = n_pass = 0
    seen = set()
    for a, al in enumerate(allocs):
        e = plan.soft_bits(a)
        lay = m.ulsch_layout(al.tbs, len(e), QM[al.mod_type], al.rv_idx)
        nc, K = lay["C"], lay["K"]
        seen.add(nc)
        blocks = plan.cb_soft(a)
        assert blocks.shape == (nc, 3 * (K + 4))
        for r in range(nc):
            es = e[lay["off"][r]:lay["off"][r] + lay["E"][r]].astype(np.float32)
            d = np.zeros(3 * (K + 4), np.float32)
            ref.ref_rate_unmatch_turbo(ref_phy, es.copy(), lay["E"][r], K, nc, 1, 1, 1, CHAN_ULSCH, al.rv_idx, d)
            want = np.where(d == 10000.0, 0, np.clip(d, -127, 127)).astype(np.int8)
            assert (blocks[r] == want).all(), (a, r)
        for (st, bits, cb_ok), model, n_iter in zip(res, (port.lo_turbo_decode_bcjr, port.lo_turbo_decode_bcjr_block), (8, 6)):
            c_bits = np.zeros((nc, K), np.uint8)
            for r in range(nc):
                model(np.ascontiguousarray(blocks[r].astype(np.int16)), K, n_iter, 1, c_bits[r])
            want_bits, want_st, want_mask = expect_from_blocks(c_bits, al.tbs)
            assert (bits[a] == want_bits).all(), a
            assert (st[a], cb_ok[a]) == (want_st, want_mask), (a, st[a], cb_ok[a], want_st, want_mask)
            n_pass += st[a] == 0
            n_fail += st[a] != 0
    return seen, n_pass, n_fail


@pytest.mark.parametrize("packed", [False, True])
def test_rate_unmatch_decode_and_assembly_exact(ctx, port, ref, ref_phy, packed):
    """A 25-RB batch with C = 1, 2, 3 (6200, 7224, 17 568 and single-block grants), rv 0-3, QPSK / 16QAM / 64QAM, and the 13-block grant of
    a 100-RB cell (73 712), at an SNR where some transport blocks pass and some fail; under BCJR x 8 and BCJR_BLOCK x 6."""
    import openlte_amd as m
    dec = ((m.TURBO_BCJR, 8), (m.TURBO_BCJR_BLOCK, 6))
    per_unit = [[grant(0, 2, 15, 20, 0, 0x81, rv=0)], [grant(1, 2, 15, 24, 0, 0x82, rv=1)], [grant(2, 3, 26, 24, 1, 0x83, rv=0)],
                [grant(3, 1, 9, 10, 7, 0x84, rv=2)], [grant(4, 2, 15, 12, 3, 0x85, rv=3)], [grant(5, 3, 22, 6, 18, 0x86, rv=2)]]
    assert [a[0].tbs for a in per_unit[:3]] == [6200, 7224, 17568]
    un25 = Units(ctx, 25, [0, 5, 3, 8, 1, 6], 17, per_unit, 12.0, seed=5 + packed)
    un100 = Units(ctx, 100, [4], 301, [[grant(0, 3, 26, 99, 0, 0x87)]], 12.0, seed=7 + packed)
    assert un100.allocs[0].tbs == 73712
    seen, n_pass, n_fail = set(), 0, 0
    for un in (un25, un100):
        plan, res = run_decoders(un, dec, packed)
        s, p, f = check_blocks_exact(port, ref, ref_phy, plan, un.allocs, res)
        print("uplink 3GPP blocks: C %s, status %s / %s" % (sorted(s), list(res[0][0]), list(res[1][0])))
        seen |= s
        n_pass += p
        n_fail += f
        plan.close()
        un.free()
    assert seen >= {1, 2, 3, 13}
    assert {a.rv_idx for a in un25.allocs} == {0, 1, 2, 3} and {a.mod_type for a in un25.allocs} == {1, 2, 3}
    assert n_pass > 0 and n_fail > 0, (n_pass, n_fail)


# ---- end to end

def check_end_to_end(un, res):
    import openlte_amd as m
    for i, (st, bits, cb_ok) in enumerate(res):
        for k, al in enumerate(un.allocs):
            assert st[k] == 0, ("decoder #%d" % i, k, al.tbs, st[k], cb_ok[k], int((bits[k] != un.sent(k)).sum()))
            assert (bits[k] == un.sent(k)).all(), k
            assert cb_ok[k] == (1 << m.ulsch_layout(al.tbs, 0, 2)["C"]) - 1


def test_end_to_end_25rb(ctx):
    """30 dB: 16QAM with two blocks, 64QAM with two and three, QPSK, and a single-block 16QAM grant at rv 1; every transport block equals
    its transmitted bits with status 0 and a full cb_ok under BCJR x 8, BCJR_EARLY and BCJR_BLOCK."""
    import openlte_amd as m
    dec = ((m.TURBO_BCJR, 8), (m.TURBO_BCJR_EARLY, 8), (m.TURBO_BCJR_BLOCK, 8))
    per_unit = [[grant(0, 2, 15, 20, 2, 0x91)], [grant(1, 3, 26, 24, 0, 0x92)], [grant(2, 3, 22, 20, 4, 0x93)], [grant(3, 1, 9, 10, 12, 0x94, rv=3)],
                [grant(4, 2, 15, 12, 6, 0x95, rv=1)]]
    un = Units(ctx, 25, [0, 5, 2, 9, 7], 123, per_unit, 30.0, seed=25)
    plan, res = run_decoders(un, dec)
    check_end_to_end(un, res)
    assert sorted(m.ulsch_layout(a.tbs, 0, 2)["C"] for a in un.allocs) == [1, 1, 2, 2, 3]
    assert plan.out_stride >= 17568
    plan.close()
    un.free()


def test_end_to_end_13_blocks(ctx):
    """30 dB, 100-RB cell: the 99-PRB, I_TBS 26 grant (73 712 bits = 13 x 5 696, code rate 0.86 on hard 64QAM decisions) at rv 0."""
    import openlte_amd as m
    dec = ((m.TURBO_BCJR, 8), (m.TURBO_BCJR_EARLY, 8), (m.TURBO_BCJR_BLOCK, 8))
    un = Units(ctx, 100, [3], 7, [[grant(0, 3, 26, 99, 0, 0xA1)]], 30.0, seed=100)
    plan, res = run_decoders(un, dec)
    check_end_to_end(un, res)
    assert m.ulsch_layout(un.allocs[0].tbs, 0, 2)["C"] == 13 and plan.out_stride >= 73712
    plan.close()
    un.free()


# ---- refusals

def test_refusals(ctx):
    """Every documented refusal, each followed by a run of a good plan: the reference-mode create still refuses C > 1; the 3GPP create
    refuses BPSK, an N_prb without a transform plan, a tbs outside the table and a PRB outside the carrier; set_decoder on both kinds."""
    import openlte_amd as m
    L = ctx.L
    un = Units(ctx, 25, [4], 9, [[grant(0, 2, 15, 20, 0, 0xB1)]], 30.0, seed=8)
    good = un.plan()

    def still_runs():
        st, bits = good.run(un.d_sub)
        assert st[0] == 0 and (bits[0] == un.sent(0)).all()

    def create(fn, cfg, allocs):
        arr = (m.PdschAlloc * len(allocs))(*allocs)
        h = C.c_void_p()
        rc = fn(ctx.h, C.byref(cfg), C.byref(un.ul), np.array([4], np.uint32), np.array([9], np.uint32), 1, C.cast(arr, C.c_void_p), len(allocs), C.byref(h))
        if rc == 0:
            L.mi_lte_pusch_plan_destroy(ctx.h, h)
        still_runs()
        return rc

    cfg100 = m.DlCfg(2048, 100, 1, 0)
    ok = m.make_alloc(0, 2, 6200, list(range(20)), 0xB2)
    assert create(L.mi_lte_pusch_plan_create_3gpp, un.cfg, [ok]) == 0
    assert create(L.mi_lte_pusch_plan_create, un.cfg, [ok]) == ERR_UNSUPPORTED
    assert create(L.mi_lte_pusch_plan_create, cfg100, [m.make_alloc(0, 3, 73712, list(range(99)), 0xB3)]) == ERR_UNSUPPORTED
    assert create(L.mi_lte_pusch_plan_create_3gpp, cfg100, [m.make_alloc(0, 3, 73712, list(range(99)), 0xB3)]) == 0
    bad = [(m.make_alloc(0, 0, 6200, list(range(20)), 0xB4), ERR_UNSUPPORTED),          # BPSK
           (m.make_alloc(0, 2, 1800, list(range(7)), 0xB5), ERR_UNSUPPORTED),           # 7 PRB: no transform plan
           (m.make_alloc(0, 2, 6200, list(range(25)), 0xB6), ERR_UNSUPPORTED),          # N_prb = N_rb_ul
           (m.make_alloc(0, 2, 6128, list(range(20)), 0xB7), ERR_UNSUPPORTED),          # not a table size (filler bits)
           (m.make_alloc(0, 2, 75384, list(range(20)), 0xB8), ERR_UNSUPPORTED),         # past the table
           (m.make_alloc(0, 2, 6200, list(range(6, 26)), 0xB9), ERR_INVALID)]           # PRB 25 of a 25-RB carrier
    for al, want in bad:
        assert create(L.mi_lte_pusch_plan_create_3gpp, un.cfg, [ok, al]) == want, (al.tbs, al.N_prb, al.mod_type)
    # set_decoder
    assert L.mi_lte_pusch_plan_set_decoder(good.h, m.TURBO_REF, 8, 1) == ERR_UNSUPPORTED
    assert L.mi_lte_pusch_plan_set_decoder(good.h, m.TURBO_BCJR, 8, 0) == ERR_INVALID
    assert L.mi_lte_pusch_plan_set_decoder(good.h, m.TURBO_BCJR, 0, 1) == ERR_INVALID
    still_runs()
    for mode in (m.TURBO_BCJR_EARLY, m.TURBO_BCJR_BLOCK, m.TURBO_BCJR):
        assert L.mi_lte_pusch_plan_set_decoder(good.h, mode, 8, 1) == 0
        still_runs()
    one = m.make_alloc(0, 1, 1544, list(range(10)), 0xBA)
    p_ref = ctx.pusch_plan(un.cfg, un.ul, [4], [9], [one])
    for mode in (m.TURBO_REF, m.TURBO_BCJR, m.TURBO_BCJR_EARLY, m.TURBO_BCJR_BLOCK):
        for spec in (0, 1):
            assert L.mi_lte_pusch_plan_set_decoder(p_ref.h, mode, 8, spec) == ERR_UNSUPPORTED
    assert L.mi_lte_pusch_plan_set_output(p_ref.h, 1) == ERR_UNSUPPORTED
    p, nc, k = C.c_void_p(), C.c_uint32(), C.c_uint32()
    assert L.mi_lte_pusch_plan_cb_soft(p_ref.h, 0, C.byref(p), C.byref(nc), C.byref(k)) == ERR_INVALID
    assert L.mi_lte_pusch_plan_cb_ok(p_ref.h, C.byref(p)) == ERR_INVALID
    p_ref.run(un.d_sub)  # (and stays a plan that runs)
    still_runs()
    p_ref.close()
    good.close()
    un.free()
