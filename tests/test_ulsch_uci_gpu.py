"""GPU: HARQ-ACK, RI and CQI multiplexed on PUSCH in the 3GPP transport-block mode (mi_lte_pusch_plan_create_3gpp_uci; 36.212 5.2.2.6-5.2.2.8,
scrambling 36.211 5.3.1).  The demodulator is the plain 3GPP plan's, byte for byte; k_ulsch_uci_gather and k_ulsch_uci_decide are integer
work and are pinned exactly to a numpy restatement of the placement and decision rules (test_ulsch_uci_cpu: written from the rules, not from
the library's map); the code blocks behind them to the reference's rate un-matching run as ULSCH and to the plain-C BCJR model, as in
test_ulsch3gpp_gpu; the whole chain to the transmitted transport blocks and control bits."""
import ctypes as C

import numpy as np
import pytest

from test_dlsch3gpp_cpu import tbs_table
from test_dlsch3gpp_gpu import expect_from_blocks
from test_ulsch3gpp_cpu import CHAN_ULSCH
from test_ulsch3gpp_gpu import FFT, QM, ULC
from test_ulsch_uci_cpu import ACK_CQI, ACK_WALK, RI_WALK, gold, place, uci, walk_cells

pytestmark = pytest.mark.gpu

ERR_INVALID, ERR_UNSUPPORTED = -1, -4


def tbs_above(n_prb, lo):
    """the smallest transport block size of N_prb's column of 36.213 Table 7.1.7.2.1-1 above lo"""
    return int(min(v for v in tbs_table()[:, n_prb - 1] if v > lo))


def tbs_at_most(n_prb, hi):
    return int(max(v for v in tbs_table()[:, n_prb - 1] if v <= hi))


class Grant:
    """One allocation with its control information: the descriptor and the values the UE sends"""

    def __init__(self, mod, size, n_prb, prb0, rnti, u=None, ack=(), ri=(), rv=0, seed=0):
        self.mod, self.tbs, self.n_prb, self.prb0, self.rnti, self.rv = mod, size, n_prb, prb0, rnti, rv
        self.u, self.ack, self.ri = u if u is not None else uci(), list(ack), list(ri)
        assert len(self.ack) == self.u.O_ack and len(self.ri) == self.u.O_ri
        self.cqi = np.random.default_rng(1000 + seed).integers(0, 2, self.u.Q_cqi).astype(np.uint8)


class UciUnits:
    """test_ulsch3gpp_gpu.Units with control information: one grant per unit on one cell, through the generator and the front end"""

    def __init__(self, ctx, n_rb, cell, grants, snr_db, seed, clean=False):
        import openlte_amd as m
        from openlte_amd import synth
        self.ctx, self.cfg, self.ul, self.g = ctx, m.DlCfg(FFT[n_rb], n_rb, 1, 0), m.UlCfg(*ULC), grants
        n = len(grants)
        self.sfs, self.cells = [(3 * k + 1) % 10 for k in range(n)], [cell] * n
        self.allocs = [m.make_alloc(k, g.mod, g.tbs, list(range(g.prb0, g.prb0 + g.n_prb)), g.rnti, rv_idx=g.rv) for k, g in enumerate(grants)]
        self.ucis = [g.u for g in grants]
        chan = dict(gain=(1.0, 1.0), max_delay=0, snr_db=200.0) if clean else dict(max_delay=3, snr_db=snr_db)
        self.iq, self.tx = synth.ul_units_3gpp(self.cfg, self.ul, self.sfs, self.cells, self.allocs, 1, uci=self.ucis, ack=[g.ack for g in grants],
                                               ri=[g.ri for g in grants], cqi=[g.cqi for g in grants], peak=100.0, seed=seed, **chan)
        _, self.d_sub = ctx.ul_frontend(self.cfg, self.iq.reshape(-1, 2), np.arange(n) * self.iq.shape[1], keep=True)

    def plan(self, with_uci=True):
        return self.ctx.pusch_plan_3gpp(self.cfg, self.ul, self.sfs, self.cells, self.allocs, uci=self.ucis if with_uci else None)

    def sent(self, k):
        return self.tx[k, 0, :self.g[k].tbs]

    def c_init(self, k):
        return (self.g[k].rnti << 14) | (self.sfs[k] << 9) | self.cells[k]

    def free(self):
        self.d_sub.free()


# ---- rules 6 and 7, restated

def gather_py(soft, g):
    """rule 7: (data [G], cqi [Q_cqi], erased flags of both) from the demodulator's transposed soft bits"""
    Qm, M = QM[g.mod], 12 * g.n_prb
    kind, own, under, stream, G = place(g.n_prb, Qm, g.u.Qp_ack, g.u.Qp_ri, g.u.Q_cqi)
    s, gone = soft.reshape(12 * M, Qm).copy(), np.zeros((12 * M, Qm), bool)
    r, c = walk_cells(M, g.u.Qp_ack, ACK_WALK)
    s[r * 12 + c], gone[r * 12 + c] = 0, True
    run, gone = s[stream].reshape(-1), gone[stream].reshape(-1)
    assert len(run) == G + g.u.Q_cqi
    return run[g.u.Q_cqi:], run[:g.u.Q_cqi], gone[g.u.Q_cqi:], gone[:g.u.Q_cqi]


def sums_py(soft, g, O, Qp, walk, c):
    """rule 6: S[3] of one control stream from the soft bits 0 and 1 of its symbols; c: the scrambling sequence"""
    Qm, M = QM[g.mod], 12 * g.n_prb
    s = soft.reshape(M, 12, Qm).astype(np.int64)
    r, col = walk_cells(M, Qp, walk)
    u0, u1, n = s[r, col, 0], s[r, col, 1], np.arange(Qp)
    if O == 1:
        i0 = (col * M + r) * Qm
        return [int((u0 + np.where(c[i0] == c[i0 + 1], u1, -u1)).sum()), 0, 0]
    if O == 2:
        return [int(u0[(2 * n) % 3 == j].sum() + u1[(2 * n + 1) % 3 == j].sum()) for j in range(3)]
    return [0, 0, 0]


def decide_py(O, S):
    if O == 1:
        return [int(S[0] < 0), 0]
    if O == 2:
        metric = [(1 - 2 * o0) * S[0] + (1 - 2 * o1) * S[1] + (1 - 2 * (o0 ^ o1)) * S[2] for o0 in (0, 1) for o1 in (0, 1)]
        h = int(np.argmax(metric))  # (the first maximum)
        return [h >> 1, h & 1]
    return [0, 0]


def check_gather_and_sums(un, plan, rec, k):
    g, soft = un.g[k], plan.soft_bits(k)
    data, cqi, _, _ = gather_py(soft, g)
    got_d, got_c = plan.data_soft(k), plan.cqi_soft(k)
    assert got_d.shape == data.shape and got_c.shape == cqi.shape
    assert (got_d == data).all() and (got_c == cqi).all(), k
    c = gold(un.c_init(k), len(soft))
    for name, O, Qp, walk in (("ack", g.u.O_ack, g.u.Qp_ack, ACK_WALK), ("ri", g.u.O_ri, g.u.Qp_ri, RI_WALK)):
        S = sums_py(soft, g, O, Qp, walk, c)
        print("alloc %d %s: O %d Q' %d sums %s -> %s" % (k, name, O, Qp, rec[k]["S_" + name], rec[k][name]))
        assert rec[k]["S_" + name] == S, (k, name)
        assert rec[k][name] == decide_py(O, S), (k, name)
    return data


# ---- gather and decisions

def exact_grants():
    return [Grant(1, 16, 1, 3, 0x101, uci(1, 48, 1, 48, 0), [1], [0], seed=1),                      # both regions full: rows of 4 data cells
            Grant(2, tbs_at_most(2, 400), 2, 5, 0x102, uci(1, 7, 2, 5, 40), [0], [1, 1], rv=1, seed=2),  # partial RI row
            Grant(3, tbs_at_most(3, 500), 3, 0, 0x103, uci(2, 100, 2, 6, 6 * 200), [1, 0], [0, 1], rv=2, seed=3),  # ACK over CQI (rows 11-16)
            Grant(1, tbs_at_most(2, 150), 2, 9, 0x104),                                              # no control information
            Grant(3, tbs_above(10, 6120), 10, 2, 0x105, uci(2, 12, 0, 0, 0), [1, 1], seed=5),        # two code blocks
            Grant(2, tbs_at_most(12, 1500), 12, 1, 0x106, uci(1, 4 * 144, 1, 4 * 144 - 1, 4 * 300), [0], [1], rv=3, seed=6)]  # several tiles, every row with RI


def test_gather_decisions_and_code_blocks_exact(ctx, port, ref, ref_phy):
    """15 dB, six grants in one plan (see exact_grants): the demodulator's soft bits equal a plain 3GPP plan's byte for byte; data_soft and
    cqi_soft equal the numpy gather with zeros at the erasures; the records' sums and bits equal the numpy sums and rule 6's decisions;
    cb_soft equals the reference's rate un-matching (ULSCH, N_codeblocks = C) of data_soft; status, bits and cb_ok equal the BCJR model's;
    the grant without control information decodes exactly as in the plain plan."""
    import openlte_amd as m
    un = UciUnits(ctx, 25, 33, exact_grants(), 15.0, seed=41)
    assert un.g[4].tbs > 6120 and m.ulsch_layout(un.g[4].tbs, 0, 2)["C"] == 2
    p_uci, p_plain = un.plan(), un.plan(with_uci=False)
    st0, bits0 = p_plain.run(un.d_sub)
    ok0, plain_soft = p_plain.cb_ok(), [p_plain.soft_bits(k) for k in range(len(un.g))]
    st, bits = p_uci.run(un.d_sub)
    ok, rec = p_uci.cb_ok(), p_uci.uci_results()
    kinds = set()
    for k, g in enumerate(un.g):
        Qm = QM[g.mod]
        assert p_uci.soft_bits(k).tobytes() == plain_soft[k].tobytes(), k
        data = check_gather_and_sums(un, p_uci, rec, k)
        kinds |= set(np.unique(m.ulsch_uci_map(g.n_prb, Qm, g.u)[0]))
        lay = m.ulsch_layout(g.tbs, len(data), Qm, g.rv)
        nc, K = lay["C"], lay["K"]
        blocks = p_uci.cb_soft(k)
        assert blocks.shape == (nc, 3 * (K + 4))
        c_bits = np.zeros((nc, K), np.uint8)
        for r in range(nc):
            es = data[lay["off"][r]:lay["off"][r] + lay["E"][r]].astype(np.float32)
            d = np.zeros(3 * (K + 4), np.float32)
            ref.ref_rate_unmatch_turbo(ref_phy, es.copy(), lay["E"][r], K, nc, 1, 1, 1, CHAN_ULSCH, g.rv, d)
            assert (blocks[r] == np.where(d == 10000.0, 0, np.clip(d, -127, 127)).astype(np.int8)).all(), (k, r)
            port.lo_turbo_decode_bcjr(np.ascontiguousarray(blocks[r].astype(np.int16)), K, 8, 1, c_bits[r])
        want_bits, want_st, want_mask = expect_from_blocks(c_bits, g.tbs)
        assert (bits[k] == want_bits).all() and (st[k], ok[k]) == (want_st, want_mask), (k, st[k], ok[k], want_st, want_mask)
    assert ACK_CQI in kinds
    assert rec[3] == {"ack": [0, 0], "ri": [0, 0], "S_ack": [0, 0, 0], "S_ri": [0, 0, 0]}
    assert (st[3], ok[3]) == (st0[3], ok0[3]) and bits[3].tobytes() == bits0[3].tobytes()
    assert p_uci.data_soft(3).tobytes() == plain_soft[3].tobytes() and p_uci.cqi_soft(3).shape == (0,)
    print("status with control information %s, plain plan on the same subframes %s" % (list(st), list(st0)))
    p_uci.close()
    p_plain.close()
    un.free()


def test_all_zero_descriptors_decode_as_the_plain_plan(ctx):
    """A plan whose descriptors are all zero on units without control information: bits, status and cb_ok byte-identical to pusch_plan_3gpp
    without uci; its records are zero."""
    un = UciUnits(ctx, 25, 9, [Grant(2, tbs_above(10, 6120), 20, 0, 0x111, rv=1), Grant(3, tbs_at_most(6, 2000), 6, 4, 0x112), Grant(1, tbs_at_most(10, 1000), 10, 7, 0x113)],
                  14.0, seed=43)
    p_uci, p_plain = un.plan(), un.plan(with_uci=False)
    a, b = p_uci.run(un.d_sub), p_plain.run(un.d_sub)
    assert a[0].tobytes() == b[0].tobytes() and all(x.tobytes() == y.tobytes() for x, y in zip(a[1], b[1]))
    assert p_uci.cb_ok().tobytes() == p_plain.cb_ok().tobytes()
    assert all(r == {"ack": [0, 0], "ri": [0, 0], "S_ack": [0, 0, 0], "S_ri": [0, 0, 0]} for r in p_uci.uci_results())
    p_uci.close()
    p_plain.close()
    un.free()


def test_gather_and_sums_at_99_prb(ctx):
    """The largest grant (99 PRB 64QAM, 85 536 soft bits, 84 tiles), noiseless: gather and sums exact, every soft bit kept with its sign."""
    g = Grant(3, int(tbs_table()[20][98]), 99, 0, 0x121, uci(1, 50, 2, 37, 6 * 500), [1], [1, 0], seed=7)
    un = UciUnits(ctx, 100, 301, [g], 0, seed=44, clean=True)
    plan = un.plan()
    st, bits = plan.run(un.d_sub)
    check_gather_and_sums(un, plan, plan.uci_results(), 0)
    check_signs(un, plan, 0)
    assert st[0] == 0 and (bits[0] == un.sent(0)).all()
    plan.close()
    un.free()


# ---- end to end

def check_signs(un, plan, k, strict=True):
    """the sign of every soft bit that no ACK symbol erased is the sent coded bit's; strict (noiseless): none of them is 0, every erased one is"""
    from openlte_amd import synth
    g = un.g[k]
    _, _, gone_d, gone_c = gather_py(plan.soft_bits(k), g)
    data, cqi = plan.data_soft(k), plan.cqi_soft(k)
    f = synth.ulsch_encode_3gpp(un.sent(k), len(data), QM[g.mod], g.rv)
    assert ((cqi < 0) == (g.cqi == 1))[~gone_c].all(), k
    if strict:
        assert ((data < 0) == (f == 1))[~gone_d].all(), k
        assert (data[~gone_d] != 0).all() and (cqi[~gone_c] != 0).all() and (data[gone_d] == 0).all() and (cqi[gone_c] == 0).all(), k
    return int(gone_d.sum()), int(gone_c.sum())


def end_to_end_grants():
    """QPSK / 16QAM / 64QAM at a code rate <= 0.6 after control, and the two-block grant; O = 1 and 2; both values of every control bit"""
    gr = [Grant(1, 0, 6, 0, 0x131, uci(1, 8, 1, 4, 40), [1], [0], seed=11),
          Grant(2, 0, 5, 8, 0x132, uci(2, 10, 2, 6, 80), [0, 1], [1, 0], rv=1, seed=12),
          Grant(3, 0, 4, 14, 0x133, uci(1, 9, 1, 5, 600), [0], [1], seed=13),  # (the CQI ends in row 8 of 48: no ACK over it)
          Grant(3, tbs_above(10, 6120), 10, 3, 0x134, uci(2, 12, 2, 7, 0), [1, 0], [0, 1], seed=14),
          Grant(2, 0, 3, 20, 0x135, uci(2, 40, 2, 11, 4 * 340), [1, 1], [0, 0], rv=2, seed=15)]  # ACK over CQI (36 rows; the CQI reaches row 28)
    import openlte_amd as m
    for g in gr:
        if g.tbs == 0:
            left = m.ulsch_uci_G(g.n_prb, QM[g.mod], g.u) - QM[g.mod] * g.u.Qp_ack  # what no ACK symbol erases
            g.tbs = tbs_at_most(g.n_prb, int(0.6 * left) - 24)
    return gr


@pytest.mark.parametrize("clean", [False, True])
def test_end_to_end(ctx, clean):
    """30 dB (and noiseless): every transport block passes and equals the sent bits, every ACK and RI bit equals the sent one and its sums
    have the sent bits' signs, every CQI soft bit that no ACK erased has its coded bit's sign.  Noiseless: every data and CQI soft bit is
    non-zero with the right sign, every erased one exactly 0."""
    import openlte_amd as m
    un = UciUnits(ctx, 25, 77, end_to_end_grants(), 30.0, seed=45, clean=clean)
    plan = un.plan()
    st, bits = plan.run(un.d_sub)
    rec, ok = plan.uci_results(), plan.cb_ok()
    seen = {n: set() for n in ("a0", "a1", "r0", "r1")}
    n_gone_c = 0
    for k, g in enumerate(un.g):
        assert st[k] == 0 and (bits[k] == un.sent(k)).all(), (k, g.tbs, st[k], ok[k])
        assert ok[k] == (1 << m.ulsch_layout(g.tbs, 0, 2)["C"]) - 1
        print("alloc %d: tbs %d ack %s (sent %s) S %s, ri %s (sent %s) S %s" % (k, g.tbs, rec[k]["ack"], g.ack, rec[k]["S_ack"], rec[k]["ri"], g.ri, rec[k]["S_ri"]))
        for name, sent, O in (("ack", g.ack, g.u.O_ack), ("ri", g.ri, g.u.O_ri)):
            assert rec[k][name][:O] == sent, (k, name)
            S, w = rec[k]["S_" + name], sent if O == 1 else [sent[0], sent[1], sent[0] ^ sent[1]]
            assert all((S[j] < 0) == bool(w[j]) and S[j] != 0 for j in range(len(w))), (k, name, S)
            for j in range(O):
                seen[name[0] + str(j)].add(sent[j])
        n_gone_c += check_signs(un, plan, k, strict=clean)[1]
    assert all(v == {0, 1} for v in seen.values()), seen
    assert n_gone_c > 0 and {g.mod for g in un.g} == {1, 2, 3} and {g.u.O_ack for g in un.g} == {1, 2}
    plan.close()
    un.free()


# ---- refusals, last_kernels

def test_refusals_at_plan_creation(ctx):
    """Every refusal of a descriptor through pusch_plan_3gpp(uci=..), a descriptor on a reference-mode plan, and the taps on plans without
    control information -- each followed by a run of a good plan."""
    import openlte_amd as m
    un = UciUnits(ctx, 25, 5, [Grant(2, tbs_at_most(6, 1000), 6, 0, 0x141, uci(1, 8, 1, 4, 40), [1], [1], seed=21)], 30.0, seed=46)
    good = un.plan()

    def still_runs():
        st, bits = good.run(un.d_sub)
        assert st[0] == 0 and (bits[0] == un.sent(0)).all() and good.uci_results()[0]["ack"] == [1, 0]

    M = 72
    bad = [(uci(3, 4), ERR_INVALID), (uci(0, 0, 3, 4), ERR_INVALID), (uci(1, 4 * M + 1), ERR_INVALID), (uci(0, 0, 2, 4 * M + 1), ERR_INVALID),
           (uci(0, 4), ERR_INVALID), (uci(2, 0), ERR_INVALID), (uci(0, 0, 0, 4), ERR_INVALID), (uci(0, 0, 1, 0), ERR_INVALID),
           (uci(Q_cqi=42), ERR_INVALID),                          # not a multiple of Q_m = 4
           (uci(Q_cqi=4 * 12 * M), ERR_INVALID),                  # G = 0
           (uci(0, 0, 1, 4 * M, 4 * 8 * M), ERR_INVALID)]         # G = 0 behind a full RI region
    for u, want in bad:
        with pytest.raises(m.MiLteError) as e:
            ctx.pusch_plan_3gpp(un.cfg, un.ul, un.sfs, un.cells, un.allocs, uci=[u])
        assert e.value.args[1] == want, (u.O_ack, u.Qp_ack, u.O_ri, u.Qp_ri, u.Q_cqi)
        assert "control information" in str(e.value)
        still_runs()
    two = [m.make_alloc(0, 3, tbs_above(10, 6120), list(range(10)), 0x142)]
    with pytest.raises(m.MiLteError) as e:  # one symbol for two code blocks
        ctx.pusch_plan_3gpp(un.cfg, un.ul, un.sfs, un.cells, two, uci=[uci(Q_cqi=6 * (1440 - 1))])
    assert e.value.args[1] == ERR_INVALID
    with pytest.raises(m.MiLteError) as e:  # a transport block the layout refuses (filler bits), whatever the descriptor
        ctx.pusch_plan_3gpp(un.cfg, un.ul, un.sfs, un.cells, [m.make_alloc(0, 2, 6128, list(range(20)), 0x143)], uci=[uci(1, 4)])
    assert e.value.args[1] == ERR_UNSUPPORTED
    still_runs()
    one = [m.make_alloc(0, 1, 1544, list(range(10)), 0x144)]
    with pytest.raises(m.MiLteError) as e:  # the reference-mode plans have no control information
        ctx.pusch_plan(un.cfg, un.ul, un.sfs, un.cells, one, uci=[uci(1, 4)])
    assert e.value.args[1] == ERR_UNSUPPORTED
    p_ref, p_plain = ctx.pusch_plan(un.cfg, un.ul, un.sfs, un.cells, one), un.plan(with_uci=False)
    L, p, n = ctx.L, C.c_void_p(), C.c_uint32()
    for pl in (p_ref, p_plain):
        assert L.mi_lte_pusch_plan_uci_results(pl.h, C.byref(p)) == ERR_INVALID
        assert L.mi_lte_pusch_plan_cqi_soft(pl.h, 0, C.byref(p), C.byref(n)) == ERR_INVALID
        assert L.mi_lte_pusch_plan_data_soft(pl.h, 0, C.byref(p), C.byref(n)) == ERR_INVALID
        pl.close()
    assert L.mi_lte_pusch_plan_data_soft(good.h, 1, C.byref(p), C.byref(n)) == ERR_INVALID  # allocation index past the plan
    still_runs()
    good.close()
    un.free()


def test_last_kernels_names_the_new_kernels_for_a_uci_plan_only(ctx):
    un = UciUnits(ctx, 25, 6, [Grant(1, tbs_at_most(6, 500), 6, 0, 0x151, uci(1, 8), [0], seed=31)], 30.0, seed=47)
    p_uci, p_plain = un.plan(), un.plan(with_uci=False)
    p_uci.run(un.d_sub)
    assert ctx.last_kernels().startswith("k_pusch_demod:1,k_ulsch_uci_gather:1,k_ulsch_uci_decide:1,k_dl3_desc:1,")
    p_plain.run(un.d_sub)
    lk = ctx.last_kernels()
    assert lk.startswith("k_pusch_demod:1,k_dl3_desc:1,") and "k_ulsch_uci" not in lk
    p_uci.close()
    p_plain.close()
    un.free()
