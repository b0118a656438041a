"""GPU: HARQ soft combining on the 3GPP PUSCH plans (mi_lte_pusch_decode_run_harq), the uplink counterpart of test_harq_gpu on the pool
both directions share.  A first transmission is the plain run byte for byte; the int16 buffer after every transmission is the sat16 chain
over the reference's own rate un-matching run as ULSCH (N_codeblocks = C); the decode of the combined blocks is the plain-C BCJR
model's; two transmissions that cannot be decoded alone recover the payload together; the flush rules -- a buffer a PDSCH plan with a
limited soft buffer wrote included -- and the refusals hold; and what the noise-referenced gain buys over the automatic one when the
transmissions differ (profiles/pusch_harq_sweep.txt)."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

from test_dlsch3gpp_cpu import tbs_table
from test_dlsch3gpp_gpu import alloc as dl_alloc, tbs
from test_harq_gpu import NULL, Tx as DlTx, decode as dl_decode, model_decode, pool_bytes, sat16
from test_ulsch3gpp_cpu import CHAN_ULSCH
from test_ulsch3gpp_gpu import FFT, QM, ULC, grant
from test_ulsch_uci_cpu import uci
from test_ulsch_uci_gpu import exact_grants

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))

pytestmark = pytest.mark.gpu

ERR_INVALID, ERR_UNSUPPORTED = -1, -4


class Tx:
    """One transmission: uplink units of one cell from the 3GPP transmitter (optionally the caller's payload, optionally with control
    information: ucis one descriptor per allocation, ctrl the values sent) through the front end, on the device."""

    def __init__(self, ctx, n_rb, sfs, cell, per_unit, snr_db, seed, payload=None, ucis=None, ctrl=None, gain=(0.5, 1.5)):
        import openlte_amd as m
        from openlte_amd import synth
        self.ctx, self.cfg, self.ul = ctx, m.DlCfg(FFT[n_rb], n_rb, 1, 0), m.UlCfg(*ULC)
        self.sfs, self.cells, self.n_alloc = list(sfs), [cell] * len(sfs), len(per_unit[0])
        self.allocs = [a for u in per_unit for a in u]
        self.ucis = ucis
        kw = {} if ucis is None else dict(uci=ucis, **ctrl)
        iq, self.tx = synth.ul_units_3gpp(self.cfg, self.ul, self.sfs, self.cells, self.allocs, self.n_alloc, gain=gain, max_delay=3, snr_db=snr_db,
                                          peak=100.0, seed=seed, payload=payload, **kw)
        _, self.d_sub = ctx.ul_frontend(self.cfg, iq.reshape(-1, 2), np.arange(len(self.sfs)) * iq.shape[1], keep=True)

    def payload(self, a):
        return self.tx[a // self.n_alloc, a % self.n_alloc, :self.allocs[a].tbs]

    def plan(self):
        return self.ctx.pusch_plan_3gpp(self.cfg, self.ul, self.sfs, self.cells, self.allocs, uci=self.ucis)

    def free(self):
        self.d_sub.free()


def decode(t, plan, pool=None, bufs=None, new_data=False):
    """One run (HARQ when pool is given): status, the full output rows, cb_ok, every allocation's cb_soft, and the control records of a
    plan that has them."""
    import openlte_amd as m
    ctx = t.ctx
    d_out, d_st = ctx.alloc(plan.n_alloc * plan.out_stride), ctx.alloc(4 * plan.n_alloc)
    d_out.zero()
    try:
        if pool is None:
            plan.run_dev(t.d_sub, d_out, d_st)
        else:
            plan.run_harq_dev(pool, m.harq_binds(plan.n_alloc, bufs, new_data), t.d_sub, d_out, d_st)
        st = d_st.download(np.int32)
        rows = d_out.download(np.uint8).reshape(plan.n_alloc, plan.out_stride)
    finally:
        d_out.free()
        d_st.free()
    res = {"st": st, "rows": rows, "cb_ok": plan.cb_ok(), "cb_soft": [plan.cb_soft(a) for a in range(plan.n_alloc)], "kernels": ctx.last_kernels()}
    if t.ucis is not None:
        res["uci"] = plan.uci_results()
    return res


def run_rc(ctx, plan, pool, binds, t):
    """mi_lte_pusch_decode_run_harq's return code (binds: a ctypes array, or None for a NULL binding)."""
    d_out, d_st = ctx.alloc(plan.n_alloc * plan.out_stride), ctx.alloc(4 * plan.n_alloc)
    try:
        return ctx.L.mi_lte_pusch_decode_run_harq(ctx.h, plan.h, pool.h, None if binds is None else C.cast(binds, C.c_void_p), t.d_sub.ptr,
                                                  d_out.ptr, d_st.ptr)
    finally:
        ctx.sync()
        d_out.free()
        d_st.free()


def data_run(t, plan, a):
    """the soft bits rate un-matching reads: the gathered data run of a plan with control information, the demodulator's otherwise"""
    return plan.data_soft(a) if t.ucis is not None else plan.soft_bits(a)


def gather_sums(ref, ref_phy, e, al):
    """test_harq_gpu.gather_sums for the uplink: the exact integer sums v [C, 3 (K + 4)] of the data run e per decoder position from the
    reference's rate un-matcher run as ULSCH with N_codeblocks = C, in chunks of one pass round the circular buffer."""
    import openlte_amd as m
    lay = m.ulsch_layout(al.tbs, len(e), QM[al.mod_type], al.rv_idx)
    nc, K = lay["C"], lay["K"]
    n = 3 * (K + 4)
    d = np.zeros(n, np.float32)
    ref.ref_rate_unmatch_turbo(ref_phy, np.ones(lay["N_cb"], np.float32), lay["N_cb"], K, nc, 1, 1, 1, CHAN_ULSCH, al.rv_idx, d)
    nnn = int((d != NULL).sum())  # non-NULL positions of the circular buffer
    v = np.zeros((nc, n), np.int64)
    for r in range(nc):
        es = e[lay["off"][r]:lay["off"][r] + lay["E"][r]].astype(np.float32)
        for c0 in range(0, len(es), nnn):
            chunk = np.ascontiguousarray(es[c0:c0 + nnn])
            d = np.zeros(n, np.float32)
            ref.ref_rate_unmatch_turbo(ref_phy, chunk.copy(), len(chunk), K, nc, 1, 1, 1, CHAN_ULSCH, al.rv_idx, d)
            v[r] += np.where(d == NULL, 0, d).astype(np.int64)
    return v, lay


def same(h, plain, what):
    assert (h["st"] == plain["st"]).all(), what
    assert (h["rows"] == plain["rows"]).all(), what
    assert (h["cb_ok"] == plain["cb_ok"]).all(), what
    assert all((x == y).all() for x, y in zip(h["cb_soft"], plain["cb_soft"])), what
    assert h.get("uci") == plain.get("uci"), what


def first_tx_batches(ctx):
    """A 25-RB batch of one to three code blocks per transport block at 12 dB (test_ulsch3gpp_gpu's: some pass, some fail), and
    test_ulsch_uci_gpu's six grants with control information at 15 dB."""
    per_unit = [[grant(0, 2, 15, 20, 0, 0x81, rv=0)], [grant(1, 2, 15, 24, 0, 0x82, rv=1)], [grant(2, 3, 26, 24, 1, 0x83, rv=0)],
                [grant(3, 1, 9, 10, 7, 0x84, rv=2)], [grant(4, 2, 15, 12, 3, 0x85, rv=3)], [grant(5, 3, 22, 6, 18, 0x86, rv=2)]]
    plain = Tx(ctx, 25, [0, 5, 3, 8, 1, 6], 17, per_unit, 12.0, seed=5)
    import openlte_amd as m
    gr = exact_grants()
    allocs = [[m.make_alloc(k, g.mod, g.tbs, list(range(g.prb0, g.prb0 + g.n_prb)), g.rnti, rv_idx=g.rv)] for k, g in enumerate(gr)]
    ctrl = dict(ack=[g.ack for g in gr], ri=[g.ri for g in gr], cqi=[g.cqi for g in gr])
    with_uci = Tx(ctx, 25, [(3 * k + 1) % 10 for k in range(len(gr))], 33, allocs, 15.0, seed=41, ucis=[g.u for g in gr], ctrl=ctrl)
    return plain, with_uci


def test_first_transmission_is_the_plain_run(ctx):
    """From an empty buffer (NEW_DATA, or an empty buffer without it), bound and unbound allocations mixed: rows, d_status, cb_ok, cb_soft and
    the control records equal the plain run's byte for byte under BCJR x 8, BCJR_EARLY and BCJR_BLOCK, with the default demapper and with
    MAXLOG, on a plan without and a plan with control information; last_kernels is the plain run's prefix and the HARQ kernels."""
    import openlte_amd as m
    pool = ctx.harq_pool(8, max_tbs=17568)
    fails = 0
    for t in first_tx_batches(ctx):
        plan = t.plan()
        n = plan.n_alloc
        bufs = [None if a % 3 == 0 else 7 - a for a in range(n)]
        new_data = [a % 3 == 1 for a in range(n)]
        for demap in (m.DEMAP_REF, m.DEMAP_MAXLOG):
            plan.set_demapper(demap, 0.0)
            for mode, n_iter in ((m.TURBO_BCJR, 8), (m.TURBO_BCJR_EARLY, 8), (m.TURBO_BCJR_BLOCK, 6)):
                plan.set_decoder(mode, n_iter, 1)
                plain = decode(t, plan)
                pool.reset()
                if mode == m.TURBO_BCJR_EARLY:  # NEW_DATA over a buffer that holds another transmission: flushed first
                    decode(t, plan, pool, bufs, False)
                h = decode(t, plan, pool, bufs, new_data if mode != m.TURBO_BCJR_EARLY else [b is not None for b in bufs])
                same(h, plain, (demap, mode))
                head = plain["kernels"].split(",k_dl3_desc:1,")[0]
                assert head.startswith("k_pusch_demod_llr:1" if demap == m.DEMAP_MAXLOG else "k_pusch_demod:1"), head
                assert (t.ucis is not None) == ("k_ulsch_uci_gather:1" in head)
                assert h["kernels"].startswith(head + ",k_dl3_desc:1,k_harq_bind:1,k_harq_rm:1,") and h["kernels"].endswith(",k_harq_commit:1"), h["kernels"]
                for a in range(n):
                    if bufs[a] is not None:
                        st = pool.state(bufs[a])
                        assert st["n_tx"] == 1 and st["tbs"] == t.allocs[a].tbs and st["status"] == plain["st"][a], (demap, mode, a, st)
                        assert (np.clip(pool.soft(bufs[a]), -127, 127) == plain["cb_soft"][a]).all(), (demap, mode, a)
                fails += int((plain["st"] != 0).sum())
        for b in {0, 1, 2, 3, 4, 5, 6, 7} - {x for x in bufs if x is not None}:
            assert pool.state(b)["n_tx"] == 0 and not pool.soft_raw(b).any()
        plan.close()
        t.free()
    assert fails > 0  # (the batches have failing blocks, so the verdicts compared are not all 0)
    pool.close()


SIZE_A, SIZE_B = 6200, 73712  # two code blocks (I_TBS 15 on 20 PRB); thirteen (I_TBS 26 on 99 PRB)


def retx(ctx, k, payload):
    """Transmission k (rv 0, 2, 3, 1) of two transport blocks, each in its own cell: SIZE_A on a 25-RB cell, SIZE_B on 96 PRB of a 100-RB
    cell.  Transmission 2 changes both subframes, modulations and N_prb; transmission 3 carries control information on both."""
    import openlte_amd as m
    rv = (0, 2, 3, 1)[k]
    sf_a, mod_a, prb_a, n_a = [(1, 2, 0, 20), (4, 2, 3, 20), (6, 3, 10, 12), (2, 2, 5, 20)][k]
    sf_b, mod_b, prb_b, n_b = [(3, 3, 0, 96), (7, 3, 2, 96), (8, 2, 5, 90), (9, 3, 4, 96)][k]
    al_a = m.make_alloc(0, mod_a, SIZE_A, list(range(prb_a, prb_a + n_a)), 0x401, rv_idx=rv)
    al_b = m.make_alloc(0, mod_b, SIZE_B, list(range(prb_b, prb_b + n_b)), 0x402, rv_idx=rv)
    kw_a = kw_b = {}
    if k == 3:
        kw_a = dict(ucis=[uci(2, 12, 1, 8, 4 * 30)], ctrl=dict(ack=[[1, 0]], ri=[[1]], cqi=[np.arange(120) % 2]))
        kw_b = dict(ucis=[uci(1, 40, 2, 64, 6 * 500)], ctrl=dict(ack=[[1]], ri=[[0, 1]], cqi=[(np.arange(3000) // 3) % 2]))
    ta = Tx(ctx, 25, [sf_a], 17, [[al_a]], 8.0 + 2 * k, seed=40 + k, payload=None if payload is None else payload[0], **kw_a)
    tb = Tx(ctx, 100, [sf_b], 301, [[al_b]], 8.0 + 2 * k, seed=50 + k, payload=None if payload is None else payload[1], **kw_b)
    return ta, tb


def test_buffer_pinned_to_reference(ctx, port, ref, ref_phy):
    """Four transmissions of the same payloads (rv 0, 2, 3, 1, each with its own seed and noise; one in other subframes with other
    modulations and N_prb; one with control information, where rate un-matching reads the gathered data run): after each, pool.soft(buf)
    is the sat16 chain over the reference's rate un-matching, cb_soft is clamp127 of it, the decode is the BCJR model's on those blocks,
    and the state steps n_tx 1..4 with the expected tbs and N_cb = K_w.  The two-block transport block runs under MAXLOG with the
    noise-referenced gain, the thirteen-block one under the default demapper."""
    import openlte_amd as m
    pool = ctx.harq_pool(4)
    bufs = [2, 0]
    payload, model = None, [None, None]
    for k in range(4):
        txs = retx(ctx, k, payload)
        if payload is None:
            payload = [t.tx for t in txs]
        for i, t in enumerate(txs):
            al = t.allocs[0]
            plan = t.plan()
            if i == 0:
                plan.set_demapper(m.DEMAP_MAXLOG, 0.0)
                plan.set_llr_noise(8.0)
            h = decode(t, plan, pool, [bufs[i]], False)
            v, lay = gather_sums(ref, ref_phy, data_run(t, plan, 0), al)
            assert lay["C"] == (2, 13)[i] and lay["N_cb"] == 3 * ((lay["K"] + 4 + 31) // 32 * 32)
            model[i] = sat16(sat16(v) if model[i] is None else model[i] + sat16(v))
            got = pool.soft(bufs[i])
            assert got.shape == model[i].shape and (got == model[i]).all(), (k, i, int((got != model[i]).sum()))
            assert (h["cb_soft"][0] == np.clip(model[i], -127, 127)).all(), (k, i)
            want_bits, want_st, want_mask = model_decode(port, np.clip(model[i], -127, 127), lay["K"], al.tbs)
            assert (h["rows"][0, :al.tbs] == want_bits).all() and (h["st"][0], h["cb_ok"][0]) == (want_st, want_mask), (k, i)
            st = pool.state(bufs[i])
            assert (st["n_tx"], st["tbs"], st["C"], st["K"], st["N_cb"], st["status"]) == (k + 1, al.tbs, lay["C"], lay["K"], lay["N_cb"], h["st"][0])
            print("transmission %d, %d blocks: status %d, cb_ok %#x, largest |buffer| %d" % (k, lay["C"], h["st"][0], h["cb_ok"][0], np.abs(model[i]).max()))
            plan.close()
            t.free()
    assert all(int(np.abs(m_).max()) > 127 for m_ in model)  # the int16 buffer holds more than the decoder's int8 range
    assert not pool.soft_raw(1).any() and not pool.soft_raw(3).any()
    pool.close()


def rate_above_one_units():
    """Eight 16QAM transport blocks in a 100-RB cell, one per unit, N_prb 96 down to 2, each the size of its column of 36.213 Table
    7.1.7.2.1-1 whose B' = tbs + 24 (+ 24 per block when segmented) is nearest G / 0.95: each transmission carries about 0.95 B' coded bits
    (test_harq_gpu.rate_above_one_units' reason: far fewer, and rv 2 alone can come out as a wrong block whose CRCs pass)."""
    import openlte_amd as m
    n_prbs = [96, 50, 24, 10, 6, 4, 3, 2]
    sfs = [1, 2, 3, 4, 6, 7, 8, 9]
    per_unit = []
    for u, n in enumerate(n_prbs):
        G = 144 * n * 4

        def b_prime(size):
            nc = m.ulsch_layout(int(size), 0, 2)["C"]
            return size + 24 + (24 * nc if nc > 1 else 0)

        size = min((int(s) for s in tbs_table()[:, n - 1]), key=lambda s: abs(G / b_prime(s) - 0.95))
        assert 0.9 <= G / b_prime(size) < 1.0, (n, size, G)
        per_unit.append([m.make_alloc(u, 2, size, list(range(n)), 0x500 + u)])
    return sfs, per_unit


@pytest.mark.parametrize("demap", ["ref", "maxlog_noise"])
def test_combining_decodes_what_one_transmission_cannot(ctx, demap):
    """30 dB, code rate above 1 per transmission: every single transmission fails (plain, and HARQ with NEW_DATA); rv 0 then rv 2, through
    two plans created and destroyed in turn while the pool lives on, decode every block to the sent payload."""
    import openlte_amd as m
    sfs, per_unit = rate_above_one_units()
    pool = ctx.harq_pool(16)
    n = len(per_unit)
    payload = None
    for k, rv in enumerate((0, 2)):
        pu = [[m.make_alloc(a.unit, a.mod_type, a.tbs, list(range(a.N_prb)), a.rnti, rv_idx=rv) for a in row] for row in per_unit]
        t = Tx(ctx, 100, sfs, 222, pu, 30.0, seed=60 + k, payload=payload)
        if payload is None:
            payload = t.tx
        plan = t.plan()
        if demap == "maxlog_noise":
            plan.set_demapper(m.DEMAP_MAXLOG, 0.0)
            plan.set_llr_noise(8.0)
        plain = decode(t, plan)
        assert max(m.ulsch_layout(al.tbs, 0, 2)["C"] for al in t.allocs) >= 9 and min(m.ulsch_layout(al.tbs, 0, 2)["C"] for al in t.allocs) == 1
        assert (plain["st"] != 0).all(), plain["st"]
        alone = decode(t, plan, pool, list(range(8, 8 + n)), True)
        assert (alone["st"] != 0).all(), alone["st"]
        h = decode(t, plan, pool, list(range(n)), k == 0)
        if k == 0:
            assert (h["st"] != 0).all()
        else:
            assert (h["st"] == 0).all(), h["st"]
            for a, al in enumerate(t.allocs):
                assert (h["rows"][a, :al.tbs] == t.payload(a)).all(), a
                assert pool.state(a)["n_tx"] == 2 and pool.state(a)["status"] == 0
        plan.close()
        t.free()
    pool.close()


def test_flush_rules(ctx):
    """NEW_DATA gives the single-transmission buffer and n_tx = 1; another tbs without NEW_DATA flushes; reset(buf) and reset() empty the
    buffers; a run whose allocations are all unbound leaves every pool byte alone; a buffer a PDSCH plan with a limited soft buffer wrote
    is flushed by a PUSCH plan of the same tbs (N_cb differs); and the pool serves plans of one, three and one allocations in turn."""
    import openlte_amd as m
    size1, size2 = tbs(15, 50), tbs(13, 50)
    pool = ctx.harq_pool(3)

    def tx(size, k, n_prb=50):
        al = m.make_alloc(0, 2, size, list(range(n_prb)), 0x601, rv_idx=(0, 2, 3, 1)[k % 4])
        return Tx(ctx, 100, [1 + k], 77, [[al]], 15.0, seed=70 + k)

    t0, t1 = tx(size1, 0), tx(size1, 1)
    p0, p1 = t0.plan(), t1.plan()
    decode(t0, p0, pool, [0])
    decode(t1, p1, pool, [0])
    assert pool.state(0)["n_tx"] == 2
    decode(t1, p1, pool, [1])  # the single-transmission buffer of t1 in buffer 1
    single = pool.soft(1)
    decode(t1, p1, pool, [0], True)
    assert pool.state(0)["n_tx"] == 1 and (pool.soft(0) == single).all()
    # another tbs, no NEW_DATA
    t2 = tx(size2, 2)
    p2 = t2.plan()
    decode(t2, p2, pool, [0])
    st = pool.state(0)
    assert st["n_tx"] == 1 and st["tbs"] == size2
    decode(t2, p2, pool, [2], True)
    single2 = pool.soft(2)
    assert (pool.soft(0) == single2).all()
    # a run with every allocation unbound: the pool's bytes do not change
    before = pool_bytes(pool)
    decode(t2, p2, pool, [None])
    for (s0, st0), (s1, st1) in zip(before, pool_bytes(pool)):
        assert (s0 == s1).all() and st0 == st1
    # a PDSCH plan of the same tbs with a limited soft buffer wrote buffer 0: another N_cb, so the PUSCH plan flushes it
    n_soft = 125184
    td = DlTx(ctx, 100, [4], [77], [[dl_alloc(0, 2, size2, 0, 50, 0x601)]], n_soft, 1, 15.0, seed=75)
    pd = td.plan(n_soft)
    dl_decode(td, pd, pool, [0], True)
    dl_decode(td, pd, pool, [0])
    st = pool.state(0)
    k_w = 3 * ((st["K"] + 4 + 31) // 32 * 32)
    assert st["n_tx"] == 2 and st["tbs"] == size2 and st["N_cb"] < k_w, st
    decode(t2, p2, pool, [0])
    st = pool.state(0)
    assert st["n_tx"] == 1 and st["tbs"] == size2 and st["N_cb"] == k_w, st
    assert (pool.soft(0) == single2).all()
    decode(t2, p2, pool, [0])
    assert pool.state(0)["n_tx"] == 2 and (pool.soft(0) == sat16(2 * single2.astype(np.int64))).all()
    pd.close()
    td.free()
    # reset(buf), then reset()
    assert pool.soft_raw(0).any() and pool.soft_raw(1).any()
    pool.reset(0)
    assert pool.state(0)["n_tx"] == 0 and not pool.soft_raw(0).any() and pool.soft(0).size == 0
    assert pool.state(1)["n_tx"] == 1 and pool.soft_raw(1).any()
    pool.reset()
    for b in range(3):
        assert pool.state(b) == {"tbs": 0, "C": 0, "K": 0, "N_cb": 0, "n_tx": 0, "status": 0} and not pool.soft_raw(b).any()
    decode(t1, p1, pool, [1])  # after a reset, the next transmission starts from an empty buffer
    assert pool.state(1)["n_tx"] == 1 and (pool.soft(1) == single).all()
    # plans of 1, 3 and 1 allocations in turn on the one pool (its binding block grows and is then used in part)
    three = [[m.make_alloc(0, 2, size2, list(range(0, 30)), 0x611, rv_idx=2), m.make_alloc(0, 1, tbs(9, 10), list(range(30, 40)), 0x612),
              m.make_alloc(0, 3, tbs(22, 6), list(range(40, 46)), 0x613, rv_idx=1)]]
    t3 = Tx(ctx, 100, [5], 77, three, 15.0, seed=79)
    p3 = t3.plan()
    h3 = decode(t3, p3, pool, [2, None, 0], True)
    plain3 = decode(t3, p3)
    same({k: v for k, v in h3.items() if k != "kernels"}, {k: v for k, v in plain3.items() if k != "kernels"}, "three allocations")
    assert (pool.state(2)["n_tx"], pool.state(2)["tbs"], pool.state(0)["n_tx"], pool.state(0)["tbs"]) == (1, size2, 1, tbs(22, 6))
    assert pool.state(1)["n_tx"] == 1 and (pool.soft(1) == single).all()
    held = pool_bytes(pool)
    decode(t0, p0, pool, [1])  # the same tbs as buffer 1 holds (t1's): combined
    assert pool.state(1)["n_tx"] == 2
    decode(t0, p0, pool, [1], True)
    first = pool.soft(1)
    decode(t1, p1, pool, [1])
    assert pool.state(1)["n_tx"] == 2 and (pool.soft(1) == sat16(first.astype(np.int64) + single)).all()
    now = pool_bytes(pool)
    for b in (0, 2):
        assert (held[b][0] == now[b][0]).all() and held[b][1] == now[b][1], b
    for p in (p0, p1, p2, p3):
        p.close()
    for t in (t0, t1, t2, t3):
        t.free()
    pool.close()


def test_saturation(ctx, ref, ref_phy):
    """The smallest tbs over 96 PRB at 64QAM (hundreds of repeats per position), three times: the buffer equals the sat16 model and sits at
    the int16 rails (32767, -32768); cb_soft is +-127 everywhere."""
    import openlte_amd as m
    pool = ctx.harq_pool(1, max_tbs=16)
    model = payload = None
    for k in range(3):
        al = m.make_alloc(0, 3, 16, list(range(2, 98)), 0x701, rv_idx=(0, 2, 3)[k])
        t = Tx(ctx, 100, [2 + k], 9, [[al]], 30.0, seed=80 + k, payload=payload)
        payload = t.tx
        plan = t.plan()
        h = decode(t, plan, pool, [0], k == 0)
        v, lay = gather_sums(ref, ref_phy, plan.soft_bits(0), al)
        model = sat16(v) if model is None else sat16(model + sat16(v))
        got = pool.soft(0)
        assert (got == model).all(), (k, int((got != model).sum()))
        assert (np.abs(h["cb_soft"][0]) == 127).all(), k
        assert pool.state(0)["n_tx"] == k + 1
        plan.close()
        t.free()
    assert ((model == 32767) | (model == -32768)).all() and (model == 32767).any() and (model == -32768).any()
    pool.close()


def test_refusals(ctx):
    """Every refusal returns before anything is launched and leaves pool and plan usable: a plan of mi_lte_pusch_plan_create (UNSUPPORTED); a
    NULL binding, buf >= n_buf, one buf bound twice, a tbs past the pool's max_tbs (INVALID_ARG).  Each is followed by a correct run."""
    import openlte_amd as m
    per_unit = [[m.make_alloc(0, 2, tbs(15, 50), list(range(50)), 0x801)], [m.make_alloc(1, 3, tbs(22, 96), list(range(2, 98)), 0x803)]]
    assert per_unit[1][0].tbs > per_unit[0][0].tbs
    t = Tx(ctx, 100, [1, 6], 345, per_unit, 30.0, seed=90)
    plan = t.plan()
    pool = ctx.harq_pool(4)
    small = ctx.harq_pool(2, max_tbs=tbs(15, 50))
    n_tx = {}

    def good(p, bufs):
        h = decode(t, plan, p, bufs)
        assert (h["st"] == 0).all(), h["st"]
        for a, b in enumerate(bufs):
            if b is not None:
                n_tx[(id(p), b)] = n_tx.get((id(p), b), 0) + 1
                assert p.state(b)["n_tx"] == n_tx[(id(p), b)], (a, b)

    good(pool, [0, 1])
    ref_plan = ctx.pusch_plan(t.cfg, t.ul, [1], [345], [m.make_alloc(0, 1, tbs(9, 10), list(range(10)), 0x805)])
    assert run_rc(ctx, ref_plan, pool, m.harq_binds(1, [0]), t) == ERR_UNSUPPORTED
    ref_plan.close()
    good(pool, [0, 1])
    assert run_rc(ctx, plan, pool, None, t) == ERR_INVALID
    good(pool, [0, 1])
    assert run_rc(ctx, plan, pool, m.harq_binds(2, [0, 4]), t) == ERR_INVALID
    good(pool, [0, 1])
    assert run_rc(ctx, plan, pool, m.harq_binds(2, [3, 3]), t) == ERR_INVALID
    good(pool, [0, 1])
    assert run_rc(ctx, plan, small, m.harq_binds(2, [0, 1]), t) == ERR_INVALID  # the second grant exceeds max_tbs
    good(small, [0, None])
    assert small.state(1)["n_tx"] == 0
    d_out, d_st = ctx.alloc(plan.n_alloc * plan.out_stride), ctx.alloc(4 * plan.n_alloc)
    binds = m.harq_binds(2, [0, 1])
    assert ctx.L.mi_lte_pusch_decode_run_harq(ctx.h, plan.h, None, C.cast(binds, C.c_void_p), t.d_sub.ptr, d_out.ptr, d_st.ptr) == ERR_INVALID
    d_out.free()
    d_st.free()
    good(pool, [0, 1])
    small.close()
    pool.close()
    plan.close()
    t.free()


# profiles/pusch_harq_sweep.txt (16 transport blocks per point, the sweep's seeds, rv 0 then rv 2 combined, BCJR x 8).  No class has a point
# where the noise-referenced gain decodes every block there and 1 dB under it while the automatic gain decodes none there and 1 dB over it
# (DESIGN.md section 8's window rule): the two curves lie 2 dB apart and both rise from 0 to 16 within 1 dB, so the window is one step short
# in 16qam_25prb_plus8db (N 16 / 16 from 1 dB on; A 0 / 16 up to 2 dB, 14 / 16 at 3 dB) and in 16qam_96prb_plus8db (N from 3 dB on; A 0 up to
# 4 dB, 12 at 5 dB).  So, as the issue sets for that case, the test runs the point of the largest difference -- the first of them:
#   16qam_25prb_plus8db   SNR 1    R 0    A 0    N4 16    N8 16    N16 16
# at scale 8, the header's convention, and asserts that N decodes at least as many blocks as A and strictly more than R.
VALUE_CLASS, VALUE_SNR_DB, VALUE_SCALE = "16qam_25prb_plus8db", 1, 8


def test_value_noise_gain_against_automatic_gain_and_default_demapper(ctx):
    """The point of the largest difference of profiles/pusch_harq_sweep.txt with the sweep's seeds: two combined transmissions, the second
    8 dB above the first; MAXLOG under the noise-referenced gain decodes at least as many transport blocks as under the automatic gain and
    strictly more than the default demapper."""
    import pusch_harq_sweep as sw
    p = sw.Point(ctx, VALUE_CLASS, float(VALUE_SNR_DB), 16)
    n_ok = {mode: int(p.decoded(mode).sum()) for mode in ("R", "A", "N%d" % VALUE_SCALE)}
    p.close()
    print("%s at %d dB: %s of 16 transport blocks decoded" % (VALUE_CLASS, VALUE_SNR_DB, n_ok))
    assert n_ok["N%d" % VALUE_SCALE] >= n_ok["A"] and n_ok["N%d" % VALUE_SCALE] > n_ok["R"], n_ok
