"""GPU: the 3GPP PDSCH plans on cells of two and four CRS ports (mi_lte_pdsch_plan_create_3gpp_txdiv): transmit diversity, the N_L = 2 code-block
concatenation and the max-log demapper of the Alamouti pairs (k_pdsch_demod_llr<2 | 4>, labelled k_pdsch_demod_llr_txd).  Units come from the
library's transmit-diversity generator (mi_lte_synth_dl_units_3gpp_txdiv_i8) through the front end with the cell's port count.  The default demapper is the reference-mode
plan's byte for byte; MAXLOG's bytes and gains are the float64 model's of include/mi_lte.h's text (tests/demap_llr_model.py) under the rules of
tests/test_demap_llr_gpu.py; noiseless units decode with every soft bit's sign right; E_r and the offsets follow N_L = 2; HARQ combining,
inertness, the refusals, and what the soft decisions buy at the point profiles/txdiv_llr_sweep.txt names."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

import demap_llr_model as dm
from test_demap_llr_gpu import check_against_model, slots
from test_dlsch3gpp_gpu import FFT, tbs
from test_harq_gpu import NULL, Tx, decode, sat16

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))

pytestmark = pytest.mark.gpu

ERR_INVALID, ERR_UNSUPPORTED = -1, -4
N_SOFT = 1237248
# profiles/txdiv_llr_sweep.txt, value_point (16 transport blocks per point, the sweep's seeds).  No class of the sweep has an SNR where MAXLOG
# decodes 16 / 16 there and 1 dB below while the default demapper decodes 0 / 16 there and 1 dB above (64QAM: MAXLOG is complete from 8 dB, the
# default demapper decodes its first blocks at 10 dB; 16QAM: 5 dB and 6 dB), so the point is the first of the largest difference: 16 blocks
# against none.
VALUE_RULE, VALUE_CLASS, VALUE_SNR_DB = "largest_difference", "64qam_r0.5", 8


def mk(unit, mod, size, prbs, rnti, rv=0, cfi=0, txm=2):
    import openlte_amd as m
    return m.make_alloc(unit, mod, size, list(prbs), rnti, rv_idx=rv, tx_mode=txm, n_pdcch_symbs=cfi)


class TxD:
    """test_harq_gpu.Tx for a cell of n_ant ports: the transmit-diversity generator's units through the front end, on the device"""

    def __init__(self, ctx, n_rb, n_ant, sfs, cells, per_unit, n_soft, cfi, snr_db, seed, payload=None, gain=(0.5, 1.5)):
        import openlte_amd as m
        from openlte_amd import synth
        self.ctx, self.cfg, self.cfi, self.sfs, self.cells, self.n_ant = ctx, m.DlCfg(FFT[n_rb], n_rb, n_ant, 0), cfi, list(sfs), list(cells), n_ant
        self.n_rb, self.n_alloc = n_rb, len(per_unit[0])
        self.allocs = [a for row in per_unit for a in row]
        iq, self.tx = synth.dl_units_3gpp_txdiv(self.cfg, sfs, cells, self.allocs, self.n_alloc, n_soft, n_pdcch_symbs=cfi, gain=gain, snr_db=snr_db,
                                                max_delay=4, seed=seed, payload=payload)
        n, ul = len(sfs), iq.shape[1]
        d_iq, d_start = ctx.to_device(iq.reshape(-1, 2)), ctx.to_device((np.arange(n) * ul).astype(np.uint64))
        self.d_sf, self.d_cell = ctx.to_device(np.asarray(sfs, np.uint32)), ctx.to_device(np.asarray(cells, np.uint32))
        self.d_sub = ctx.alloc(n * ctx.subframe_floats(n_ant) * 4)
        ctx.dl_frontend_dev(self.cfg, d_iq, None, d_start, self.d_sf, self.d_cell, n, self.d_sub)
        d_iq.free()
        d_start.free()

    def payload(self, a):
        return self.tx[a // self.n_alloc, a % self.n_alloc, :self.allocs[a].tbs]

    def plan(self, n_soft):
        return self.ctx.pdsch_plan_3gpp_txdiv(self.cfg, self.cfi, self.allocs, n_soft)

    def planes(self):
        return self.d_sub.download(np.float32).reshape(len(self.sfs), 2 + 2 * self.n_ant, 16, dm.N_SC)

    def free(self):
        for b in (self.d_sf, self.d_cell, self.d_sub):
            b.free()


def case(name):
    """(n_rb, n_ant, plan cfi, subframes, cells, allocations per unit, direct stores): the smallest shapes this kernel can go wrong at.
    A: 1-PRB allocations of the three modulations in a 6-RB two-port cell, subframes 0 (PBCH + sync signals over the whole band), 5 and 3, one
    with its own control-region size; QPSK sits on the band's edge, 16QAM and 64QAM on PRBs 1 and 4: on the PRBs at the edge and next to the
    carrier the front end's estimate (extrapolated past the last pilot, interpolated across the unused centre sub-carrier) is off by more than
    their decision distance under a timing offset, with or without transmit diversity, and the noiseless test would measure that.
    B: a 25-RB four-port cell in subframes 0 and 5, PRBs [8, 9, 10] and [14 .. 17] astride the PBCH / PSS / SSS window (sub-carriers
    114 .. 185: the half PRBs 9 and 15; [8, 9, 10] has 30 elements in symbols 5 and 6, so a quad straddles two symbols and the four-port pair
    parity continues across table entries; no pair leaves its entry: tests/test_demap_geometry_cpu.py) and one allocation clear of it.
    C: B's allocations on two ports.  D: one 100-PRB 64QAM allocation on two
    ports: past the LDS cap, so stored directly, and the largest pair table."""
    if name == "A":
        return 6, 2, 3, [0, 5, 3], [11, 250, 77], [[mk(u, 1, tbs(0, 1), [0], 0x21), mk(u, 2, tbs(0, 1), [1], 0x22), mk(u, 3, tbs(0, 1), [4], 0x23, cfi=2)]
                                                   for u in range(3)], False
    if name in ("B", "C"):
        return 25, 4 if name == "B" else 2, 1, [0, 5], [301, 42], [[mk(u, 1, tbs(5, 3), [8, 9, 10], 0x41), mk(u, 2, tbs(5, 3), [20, 21, 22], 0x42, cfi=3),
                                                                    mk(u, 3, tbs(9, 4), [14, 15, 16, 17], 0x43, cfi=2)] for u in range(2)], False
    assert name == "D"
    return 100, 2, 1, [4], [503], [[mk(0, 3, tbs(15, 100), range(100), 0x51)]], True


def make(ctx, name, snr_db, seed, gain=(0.5, 1.5)):
    n_rb, n_ant, cfi, sfs, cells, per_unit, direct = case(name)
    return TxD(ctx, n_rb, n_ant, sfs, cells, per_unit, N_SOFT, cfi, snr_db, seed, gain=gain), direct


def model_of(t, planes, gain):
    import openlte_amd as m
    out = []
    for u in range(len(t.sfs)):
        out += dm.demap(planes[u], [al for al in t.allocs if al.unit == u], t.sfs[u], t.cells[u], t.n_rb, t.cfi, t.n_ant, gain=gain, T=m.DEMAP_AUTO_T)
    return out


@pytest.mark.parametrize("name", ["A", "B", "C"])
def test_default_demapper_is_the_reference_mode_plan(ctx, name):
    """MI_LTE_DEMAP_REF: the soft-bit tap and e_len of the transmit-diversity plan equal those of a mi_lte_pdsch_plan_create plan over the same
    subframes and allocations (all of one code block, which the reference mode accepts), and the run lists k_pdsch_demod."""
    t, _ = make(ctx, name, 12.0, seed=31)
    plan = t.plan(N_SOFT)
    decode(t, plan)
    assert ctx.last_kernels().startswith("k_pdsch_demod:1,k_dl3_desc:1,k_dl3_rm_i8:1,")
    assert all(al.tbs + 24 <= 6144 for al in t.allocs)
    ref_plan = ctx.pdsch_plan(t.cfg, t.cfi, t.allocs)
    ref_plan.run(t.d_sub, t.sfs, t.cells)
    assert ctx.last_kernels().startswith("k_pdsch_demod:1,")
    for a in range(plan.n_alloc):
        got, want = plan.soft_bits(a), ref_plan.soft_bits(a)
        assert len(got) == len(want) > 0 and len(got) % (t.n_ant * dm.QM[t.allocs[a].mod_type]) == 0, (a, len(got), len(want))
        assert (got == want).all(), a
    ref_plan.close()
    plan.close()
    t.free()


@pytest.mark.parametrize("snr_db", [20.0, 5.0])
@pytest.mark.parametrize("name", ["A", "B", "C", "D"])
def test_bytes_and_gains_against_the_model(ctx, name, snr_db):
    """MAXLOG under the automatic gain, then a fixed one on the same plan, by test_demap_llr_gpu.check_against_model's rules; e_len and every
    byte outside the allocations' ranges as the default demapper's run left them."""
    import openlte_amd as m
    t, direct = make(ctx, name, snr_db, seed=int(snr_db) + ord(name))
    planes = t.planes()
    plan = t.plan(N_SOFT)
    decode(t, plan)
    assert ctx.last_kernels().startswith("k_pdsch_demod:1,")
    ref_len, ref_slots = [len(plan.soft_bits(a)) for a in range(plan.n_alloc)], slots(plan, t.allocs, t.cfi)
    auto = model_of(t, planes, 0.0)
    fixed = float(np.float32(1.5 * np.median([r.gain for r in auto])))  # (of the automatic one's order: graded bytes and clamped ones)
    for gain in (0.0, fixed):
        plan.set_demapper(m.DEMAP_MAXLOG, gain)
        decode(t, plan)
        assert ctx.last_kernels().startswith("k_pdsch_demod_llr_txd:1,k_dl3_desc:1,k_dl3_rm_i8:1,")
        e = check_against_model(plan, t, auto if gain == 0 else model_of(t, planes, gain), gain)
        assert (np.abs(e) == 127).any() and (np.abs(e) < 127).any()
        got = slots(plan, t.allocs, t.cfi)
        for a in range(plan.n_alloc):
            n = len(plan.soft_bits(a))
            assert n == ref_len[a], a
            keep = n if direct else (n + 15) & ~15  # (assembled in LDS, an allocation leaves in 16-byte stores)
            assert (got[a][keep:] == ref_slots[a][keep:]).all(), a
    plan.close()
    t.free()


def coded_bits(t, a, n_bits):
    """The code bits of allocation a, mi_lte_dlsch_encode_3gpp_nl with N_L = 2: the tap is descrambled, so the scrambling sequence drops out"""
    from openlte_amd import synth
    al = t.allocs[a]
    return synth.dlsch_encode_3gpp(t.payload(a), n_bits, dm.QM[al.mod_type], al.tx_mode, al.rv_idx, N_SOFT, 8, n_l=2)


@pytest.mark.parametrize("name", ["A", "B", "C"])
def test_noiseless_signs_and_decode(ctx, name):
    """snr_db >= 200: every MAXLOG soft bit has the sign of its code bit (positive: 0), and every transport block decodes."""
    import openlte_amd as m
    t, _ = make(ctx, name, 300.0, seed=41)
    plan = t.plan(N_SOFT)
    plan.set_demapper(m.DEMAP_MAXLOG, 0.0)
    h = decode(t, plan)
    for a, al in enumerate(t.allocs):
        e = plan.soft_bits(a)
        want = coded_bits(t, a, len(e))
        wrong = np.flatnonzero(np.where(want == 1, e >= 0, e <= 0))
        print("allocation %d: %d soft bits, smallest magnitude %d, %d with the wrong sign" % (a, len(e), np.abs(e).min(), len(wrong)))
        assert len(wrong) == 0, (a, wrong[:8], e[wrong[:8]])
        assert h["st"][a] == 0 and (h["rows"][a, :al.tbs] == t.payload(a)).all(), a
    plan.close()
    t.free()


def rate_unmatch_ref(ref, ref_phy, es, lay, al, n_soft):
    d = np.zeros(3 * (lay["K"] + 4), np.float32)
    ref.ref_rate_unmatch_turbo(ref_phy, es.copy(), len(es), lay["K"], lay["C"], al.tx_mode, n_soft, 8, 0, al.rv_idx, d)
    return d


def test_code_block_concatenation_with_nl2(ctx, ref, ref_phy):
    """A two-block 64QAM allocation whose symbol pairs do not split evenly (19 PRB of a 25-RB two-port cell in subframe 0, one of them half
    inside the PBCH window: M_symb / 2 is odd), so that its N_L = 2 layout differs from its N_L = 1 layout: every block of the _cb_soft tap is
    the reference's rate un-matching of soft bits [off_r, off_r + E_r) of the N_L = 2 layout, and at 30 dB the payload decodes."""
    import openlte_amd as m
    prbs = list(range(0, 10)) + list(range(16, 25))
    t = TxD(ctx, 25, 2, [0], [17], [[mk(0, 3, 6200, prbs, 0x71, rv=1)]], N_SOFT, 2, 30.0, seed=51)
    plan = t.plan(N_SOFT)
    plan.set_demapper(m.DEMAP_MAXLOG, 0.0)
    h = decode(t, plan)
    al, e = t.allocs[0], plan.soft_bits(0)
    one, two = m.dlsch_layout(al.tbs, len(e), 6, 2, 1, N_SOFT, 8, n_l=1), m.dlsch_layout(al.tbs, len(e), 6, 2, 1, N_SOFT, 8, n_l=2)
    print("G %d: N_L = 1 %s, N_L = 2 %s" % (len(e), one["E"], two["E"]))
    assert two["C"] == 2 and (len(e) // 12) % 2 == 1 and one["E"] != two["E"] and one["off"] != two["off"]
    blocks = plan.cb_soft(0)
    assert blocks.shape == (2, 3 * (two["K"] + 4))
    for r in range(2):
        d = rate_unmatch_ref(ref, ref_phy, e[two["off"][r]:two["off"][r] + two["E"][r]].astype(np.float32), two, al, N_SOFT)
        assert (blocks[r] == np.where(d == NULL, 0, np.clip(d, -127, 127)).astype(np.int8)).all(), r
        d1 = rate_unmatch_ref(ref, ref_phy, e[one["off"][r]:one["off"][r] + one["E"][r]].astype(np.float32), one, al, N_SOFT)
        assert (blocks[r] != np.where(d1 == NULL, 0, np.clip(d1, -127, 127)).astype(np.int8)).any(), r
    assert h["st"][0] == 0 and h["cb_ok"][0] == 3 and (h["rows"][0, :al.tbs] == t.payload(0)).all()
    plan.close()
    t.free()


def test_thirteen_blocks_decode(ctx):
    """The largest transport block (75376 bits, 13 code blocks) on 100 PRB of a two-port cell at 30 dB, under both demappers"""
    import openlte_amd as m
    t = TxD(ctx, 100, 2, [3], [42], [[mk(0, 3, 75376, range(100), 0x72)]], N_SOFT, 1, 30.0, seed=52, gain=(1.0, 1.0))
    plan = t.plan(N_SOFT)
    for mode in (m.DEMAP_MAXLOG, m.DEMAP_REF):
        plan.set_demapper(mode, 0.0)
        h = decode(t, plan)
        print("demapper %d: status %d, cb_ok %#x, %d bit errors" % (mode, h["st"][0], h["cb_ok"][0], (h["rows"][0, :75376] != t.payload(0)).sum()))
        if mode == m.DEMAP_MAXLOG:
            assert h["st"][0] == 0 and h["cb_ok"][0] == (1 << 13) - 1 and (h["rows"][0, :75376] == t.payload(0)).all()
    plan.close()
    t.free()


def gather_sums_nl2(ref, ref_phy, plan, a, al, n_soft):
    """test_harq_gpu.gather_sums over the N_L = 2 layout: the exact integer sums [C, 3 (K + 4)] of allocation a's soft bits per decoder position"""
    import openlte_amd as m
    e = plan.soft_bits(a)
    lay = m.dlsch_layout(al.tbs, len(e), dm.QM[al.mod_type], al.tx_mode, al.rv_idx, n_soft, 8, n_l=2)
    n = 3 * (lay["K"] + 4)
    d = rate_unmatch_ref(ref, ref_phy, np.ones(lay["N_cb"], np.float32), lay, al, n_soft)
    nnn = int((d != NULL).sum())
    v = np.zeros((lay["C"], n), np.int64)
    for r in range(lay["C"]):
        es = e[lay["off"][r]:lay["off"][r] + lay["E"][r]].astype(np.float32)
        for c0 in range(0, len(es), nnn):
            d = rate_unmatch_ref(ref, ref_phy, np.ascontiguousarray(es[c0:c0 + nnn]), lay, al, n_soft)
            v[r] += np.where(d == NULL, 0, d).astype(np.int64)
    return v


def harq_units(rv):
    """25 RB, two ports: a two-block 64QAM grant next to a QPSK one, and a 16QAM grant in subframe 5 astride the sync window"""
    return [3, 5], [17, 301], [[mk(0, 3, tbs(20, 18), range(0, 18), 0x61, rv=rv), mk(0, 1, tbs(9, 7), range(18, 25), 0x62, rv=rv)],
                               [mk(1, 2, tbs(14, 12), range(5, 17), 0x63, rv=rv), mk(1, 3, tbs(20, 8), range(17, 25), 0x64, rv=rv)]]


def test_harq_on_the_shared_pool(ctx, ref, ref_phy):
    """MAXLOG through mi_lte_pdsch_decode_run_harq: a first transmission is the plain run byte for byte; after rv 0 and then rv 2 the int16
    buffer is the sat16 chain over the two runs' exact sums; the same pool serves a single-port 3GPP plan of the context in between."""
    import openlte_amd as m
    n_soft = 125184
    pool = ctx.harq_pool(12)
    model, payload = {}, None
    for k, rv in enumerate((0, 2)):
        sfs, cells, per_unit = harq_units(rv)
        t = TxD(ctx, 25, 2, sfs, cells, per_unit, n_soft, 2, 6.0 + k, seed=60 + k, payload=payload)
        payload = t.tx
        plan = t.plan(n_soft)
        plan.set_demapper(m.DEMAP_MAXLOG, 0.0)
        n = plan.n_alloc
        if k == 0:
            plain = decode(t, plan)
            e_plain = [plan.soft_bits(a) for a in range(n)]
            first = decode(t, plan, pool, list(range(4, 4 + n)), True)
            assert ctx.last_kernels().startswith("k_pdsch_demod_llr_txd:1,k_dl3_desc:1,k_harq_bind:1,k_harq_rm:1,")
            assert (first["st"] == plain["st"]).all() and (first["rows"] == plain["rows"]).all() and (first["cb_ok"] == plain["cb_ok"]).all()
            for a in range(n):
                assert (first["cb_soft"][a] == plain["cb_soft"][a]).all() and (plan.soft_bits(a) == e_plain[a]).all(), a
        h = decode(t, plan, pool, list(range(n)), k == 0)
        for a, al in enumerate(t.allocs):
            v = gather_sums_nl2(ref, ref_phy, plan, a, al, n_soft)
            model[a] = sat16(sat16(v) if k == 0 else model[a] + sat16(v))
            got = pool.soft(a)
            assert got.shape == model[a].shape and (got == model[a]).all(), (k, a)
            assert (h["cb_soft"][a] == np.clip(model[a], -127, 127)).all(), (k, a)
            assert pool.state(a)["n_tx"] == k + 1
        if k == 0:  # a single-port plan of the same context on the pool's other buffers
            s = Tx(ctx, 25, [3], [17], [[mk(0, 2, tbs(14, 12), range(5, 17), 0x65, txm=1)]], n_soft, 2, 20.0, seed=70)
            sp = s.plan(n_soft)
            want = decode(s, sp)
            got = decode(s, sp, pool, [8], True)
            assert ctx.last_kernels().startswith("k_pdsch_demod:1,k_dl3_desc:1,k_harq_bind:1,k_harq_rm:1,")
            assert (got["st"] == want["st"]).all() and (got["rows"] == want["rows"]).all() and pool.state(8)["n_tx"] == 1
            assert all(pool.state(a)["n_tx"] == 1 for a in range(n))
            sp.close()
            s.free()
        plan.close()
        t.free()
    assert max(int(np.abs(v).max()) for v in model.values()) > 127
    pool.close()


def test_opt_in_is_inert(ctx):
    """MAXLOG and back to REF: soft bits, output rows, verdicts and cb_soft of the plan that never opted in, byte for byte.  A single-port 3GPP
    plan lists the kernels it listed before."""
    import openlte_amd as m
    t, _ = make(ctx, "C", 9.0, seed=3)
    plain, other = t.plan(N_SOFT), t.plan(N_SOFT)
    want = decode(t, plain)
    assert ctx.last_kernels() == "k_pdsch_demod:1,k_dl3_desc:1,k_dl3_rm_i8:1,k_bcjr_* per block size,k_dl3_cb_finish:1,k_dl3_tb_finish:1"
    want_e = [plain.soft_bits(a) for a in range(plain.n_alloc)]
    other.set_demapper(m.DEMAP_MAXLOG, 0.0)
    decode(t, other)
    assert ctx.last_kernels() == "k_pdsch_demod_llr_txd:1,k_dl3_desc:1,k_dl3_rm_i8:1,k_bcjr_* per block size,k_dl3_cb_finish:1,k_dl3_tb_finish:1"
    assert any((other.soft_bits(a) != want_e[a]).any() for a in range(plain.n_alloc))
    other.set_demapper(m.DEMAP_REF, 123.0)
    got = decode(t, other)
    assert ctx.last_kernels().startswith("k_pdsch_demod:1,")
    assert (got["st"] == want["st"]).all() and (got["rows"] == want["rows"]).all() and (got["cb_ok"] == want["cb_ok"]).all()
    for a in range(plain.n_alloc):
        assert (other.soft_bits(a) == want_e[a]).all() and (got["cb_soft"][a] == want["cb_soft"][a]).all(), a
    for p in (plain, other):
        p.close()
    t.free()
    s = Tx(ctx, 25, [3], [17], [[mk(0, 2, tbs(14, 12), range(5, 17), 0x65, txm=1)]], N_SOFT, 2, 20.0, seed=70)
    sp = s.plan(N_SOFT)
    decode(s, sp)
    assert ctx.last_kernels() == "k_pdsch_demod:1,k_dl3_desc:1,k_dl3_rm_i8:1,k_bcjr_* per block size,k_dl3_cb_finish:1,k_dl3_tb_finish:1"
    sp.set_demapper(m.DEMAP_MAXLOG, 0.0)
    decode(s, sp)
    assert ctx.last_kernels() == "k_pdsch_demod_llr:1,k_dl3_desc:1,k_dl3_rm_i8:1,k_bcjr_* per block size,k_dl3_cb_finish:1,k_dl3_tb_finish:1"
    sp.close()
    s.free()


def sweep_point(ctx, name, snr_db):
    """One class of profiles/txdiv_llr_sweep.txt at one SNR, with the sweep's seeds (tools/txdiv_llr_sweep.py)"""
    import txdiv_llr_sweep as sw
    sfs, cells, allocs = sw.class_units(name, 16)
    return TxD(ctx, sw.N_RB, sw.N_ANT, sfs, cells, [[al] for al in allocs], sw.N_SOFT, sw.CFI, float(snr_db), seed=sw.point_seed(name, snr_db),
               gain=sw.CLASSES[name][3])


def decoded(t, h):
    return np.array([h["st"][a] == 0 and (h["rows"][a, :al.tbs] == t.payload(a)).all() for a, al in enumerate(t.allocs)])


def test_value_of_the_soft_decisions(ctx):
    """The value point of profiles/txdiv_llr_sweep.txt.  Rule "window": at VALUE_SNR_DB and 1 dB under it MAXLOG decodes every transport block
    of VALUE_CLASS, and at VALUE_SNR_DB and 1 dB over it the default demapper none.  Rule "largest_difference" (no class of the sweep has such
    a window): at VALUE_SNR_DB MAXLOG decodes strictly more blocks than the default demapper."""
    import openlte_amd as m
    if VALUE_RULE == "window":
        points = ((VALUE_SNR_DB - 1, (m.DEMAP_MAXLOG,)), (VALUE_SNR_DB, (m.DEMAP_MAXLOG, m.DEMAP_REF)), (VALUE_SNR_DB + 1, (m.DEMAP_REF,)))
    else:
        points = ((VALUE_SNR_DB, (m.DEMAP_MAXLOG, m.DEMAP_REF)),)
    for snr, modes in points:
        t = sweep_point(ctx, VALUE_CLASS, snr)
        plan = t.plan(N_SOFT)
        n_ok = {}
        for mode in modes:
            plan.set_demapper(mode, 0.0)
            ok = decoded(t, decode(t, plan))
            n_ok[mode] = int(ok.sum())
            print("%d dB, demapper %d: %d of %d transport blocks decoded" % (snr, mode, ok.sum(), len(ok)))
            if VALUE_RULE == "window":
                assert ok.all() if mode == m.DEMAP_MAXLOG else not ok.any(), (snr, mode, ok)
        if VALUE_RULE != "window":
            assert n_ok[m.DEMAP_MAXLOG] > n_ok[m.DEMAP_REF], n_ok
        plan.close()
        t.free()


def test_all_zero_grid(ctx):
    """An all-zero grid and estimate: zero soft bits with the default run's e_len, gains 0 and finite, status 2, no CRC bit"""
    import openlte_amd as m
    t, _ = make(ctx, "B", 20.0, seed=8)
    plan = t.plan(N_SOFT)
    decode(t, plan)
    e_len = [len(plan.soft_bits(b)) for b in range(plan.n_alloc)]
    t.d_sub.zero()
    plan.set_demapper(m.DEMAP_MAXLOG, 0.0)
    h = decode(t, plan)
    g = plan.llr_gain()
    assert all(len(plan.soft_bits(b)) == e_len[b] and not plan.soft_bits(b).any() for b in range(plan.n_alloc))
    assert np.isfinite(g).all() and (g == 0).all(), g
    assert (h["st"] == 2).all() and not h["cb_ok"].any() and not any(b.any() for b in h["cb_soft"])
    plan.close()
    t.free()


def test_refusals_leave_everything_usable(ctx):
    """Each refusal of mi_lte_pdsch_plan_create_3gpp_txdiv and mi_lte_pdsch_alloc_decodable_3gpp_txdiv; a plan made before them runs as before
    after each; mi_lte_pdsch_plan_create_3gpp still refuses two ports."""
    import openlte_amd as m
    L = ctx.L
    t, _ = make(ctx, "C", 20.0, seed=9)
    plan = t.plan(N_SOFT)
    plan.set_demapper(m.DEMAP_MAXLOG, 0.0)
    want = decode(t, plan)
    want_e = [plan.soft_bits(a) for a in range(plan.n_alloc)]
    dl = m.DlschCfg(N_SOFT, 8)

    def same():
        got = decode(t, plan)
        assert ctx.last_kernels().startswith("k_pdsch_demod_llr_txd:1,")
        assert (got["st"] == want["st"]).all() and (got["rows"] == want["rows"]).all()
        assert all((plan.soft_bits(a) == want_e[a]).all() for a in range(plan.n_alloc))

    def create(fn, cfg, allocs):
        arr = (m.PdschAlloc * len(allocs))(*allocs)
        h = C.c_void_p()
        rc = fn(ctx.h, C.byref(cfg), 1, C.byref(dl), C.cast(arr, C.c_void_p), len(allocs), C.byref(h))
        if rc == 0:
            L.mi_lte_pdsch_plan_destroy(ctx.h, h)
        return rc

    txd, good = L.mi_lte_pdsch_plan_create_3gpp_txdiv, mk(0, 3, 6200, range(25), 0x100)
    cfg1, cfg2, cfg3, cfg4 = (m.DlCfg(512, 25, n, 0) for n in (1, 2, 3, 4))
    assert create(txd, cfg2, [good]) == 0 and create(txd, cfg4, [good]) == 0
    ok = lambda cfg, al: L.mi_lte_pdsch_alloc_decodable_3gpp_txdiv(C.byref(cfg), C.byref(dl), C.byref(al), 1)
    assert ok(cfg2, good) == 1 and ok(cfg4, good) == 1
    for cfg, al, rc in ((cfg1, good, ERR_UNSUPPORTED), (cfg3, good, ERR_INVALID), (m.DlCfg(512, 25, 2, m.CE_COMPACT), good, ERR_UNSUPPORTED),
                        (cfg2, mk(0, 3, 6200, range(25), 0x100, txm=1), ERR_UNSUPPORTED), (cfg2, mk(0, 3, 6200, range(25), 0x100, txm=3), ERR_UNSUPPORTED),
                        (cfg4, mk(0, 0, 6200, range(25), 0x100), ERR_UNSUPPORTED), (cfg2, mk(0, 3, 6128, range(25), 0x100), ERR_UNSUPPORTED),
                        (cfg2, mk(0, 3, 75384, range(25), 0x100), ERR_UNSUPPORTED), (cfg2, mk(0, 3, 6200, [25], 0x100), ERR_INVALID)):
        assert create(txd, cfg, [good, al]) == rc, (cfg.N_ant, al.tx_mode, al.mod_type, al.tbs)
        assert ok(cfg, al) == 0
        same()
    assert create(L.mi_lte_pdsch_plan_create_3gpp, cfg2, [good]) == ERR_UNSUPPORTED
    assert create(L.mi_lte_pdsch_plan_create_3gpp, cfg1, [mk(0, 3, 6200, range(25), 0x100, txm=1)]) == 0
    assert L.mi_lte_pdsch_plan_set_decoder(plan.h, m.TURBO_REF, 8, 1) == ERR_UNSUPPORTED
    assert L.mi_lte_pdsch_plan_set_decoder(plan.h, m.TURBO_BCJR, 8, 0) == ERR_INVALID
    same()
    plan.close()
    t.free()
