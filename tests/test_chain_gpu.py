"""GPU parity: PDSCH demodulation + DL-SCH decode (HIP) vs the oracle.

Stage parity is exact: the oracle's own rx_symb / rx_ce arrays are uploaded, so RE extraction,
pre-decoding, de-mapping, descrambling, rate un-matching, turbo decoding and CRC all see the same
inputs as the oracle and must produce identical bytes (16/64QAM and the decoder are integer work;
the equaliser is IEEE add/mul/div in the reference's order).  End-to-end parity (own front end) is
checked on decoded bits and return codes."""
import ctypes as C

import numpy as np
import pytest

import lte_testdata as td

pytestmark = pytest.mark.gpu


def upload_oracle_subframe(ctx, s, n_ant):
    a = np.concatenate([s.arr("rx_symb_re").ravel(), s.arr("rx_symb_im").ravel(), s.arr("rx_ce_re")[:n_ant].ravel(),
                        s.arr("rx_ce_im")[:n_ant].ravel()]).astype(np.float32)
    return a


def oracle_pdsch(port, lc, s, alloc, cfi, cell, n_ant):
    from oracle import pyoracle as po
    out, n = np.zeros(6200, np.uint8), C.c_uint32()
    soft, ns = np.zeros(max(20000, 6 * 168 * alloc.N_prb + 64), np.int8), C.c_uint32()
    la = td.to_lo_alloc(alloc)
    err = port.lo_pdsch_channel_decode(C.byref(lc), C.byref(s), C.byref(la), cfi, cell, n_ant, out, C.byref(n),
                                       soft.ctypes.data_as(C.c_void_p), C.byref(ns))
    c = np.zeros(ns.value, np.uint8)
    port.lo_prs_c((alloc.rnti << 14) | (s.num << 9) | cell, ns.value, c)
    desc = (soft[:ns.value].astype(np.int16) * (1 - 2 * c.astype(np.int16))).astype(np.int8)
    return err, out[:n.value].copy(), desc


@pytest.mark.parametrize("mod,tbs,nprb,snr", [(3, 3240, 12, 300), (3, 3240, 12, 18), (2, 1384, 8, 300), (2, 1384, 8, 12),
                                              (1, 680, 8, 300), (1, 680, 8, 6), (3, 1064, 4, 300), (3, 2024, 8, 25)])
def test_pdsch_stage_parity_exact(ctx, port, mod, tbs, nprb, snr):
    import openlte_amd as m
    from openlte_amd import synth
    cfg = m.DlCfg(2048, 100, 1, 0)
    sfs, cells = [1, 5, 0, 9], [17, 301, 503, 44]
    allocs = []
    for u in range(4):
        allocs += td.small_allocs(u, 100, mod, tbs, nprb, rnti=0x100 + u, first=45 if u in (1, 2) else 3 * u)
    iq, tx = synth.dl_units(cfg, sfs, cells, allocs, 1, snr_db=snr, max_delay=3, seed=tbs + snr)
    subs, want = [], []
    for u in range(4):
        lc, s = td.oracle_frontend(port, 2048, 100, 1, iq[u], sfs[u], cells[u])
        subs.append(upload_oracle_subframe(ctx, s, 1))
        want.append(oracle_pdsch(port, lc, s, allocs[u], 2, cells[u], 1))
    d_sub = ctx.to_device(np.concatenate(subs))
    plan = ctx.pdsch_plan(cfg, 2, allocs)
    st, bits = plan.run(d_sub, sfs, cells)
    for u in range(4):
        err, out, desc = want[u]
        e = plan.soft_bits(u)
        # every modulation, QPSK's graded soft values included: the equaliser is IEEE arithmetic in the reference's order, the quadrant
        # is the reference's (signs away from the axes, its atan2f comparisons next to them) and sqrtf is correctly rounded, so the
        # bytes are identical -- measured on 441 240 QPSK soft bits from 300 dB down to 0 dB SNR: none differ (tools/diag_qpsk.py)
        assert e.shape == desc.shape and (e == desc).all(), "soft bits differ (unit %d): %d" % (u, int((e != desc).sum()))
        assert st[u] == err, (u, st[u], err)
        if err == 0:
            assert (bits[u] == out).all()
            if snr >= 300:
                assert (bits[u] == tx[u, 0, :tbs]).all()
    plan.close()
    d_sub.free()


def test_w4_full_chain_end_to_end(ctx, port):
    """20 MHz, 9 allocations per subframe (8 x 12 PRB TBS 3240 + 4 PRB TBS 1064), 64QAM,
    own front end -> own PDSCH chain; every allocation must decode to the transmitted bits, and to the
    oracle's verdict."""
    import openlte_amd as m
    from openlte_amd import synth
    cfg = m.DlCfg(2048, 100, 1, 0)
    n = 6
    sfs, cells = [1, 2, 3, 4, 6, 7], [0, 17, 100, 301, 404, 503]
    allocs = []
    for u in range(n):
        allocs += td.w4_allocs(u)
    iq, tx = synth.dl_units(cfg, sfs, cells, allocs, 9, snr_db=30, max_delay=4, seed=99)
    ul = iq.shape[1]
    d_iq = ctx.to_device(iq.reshape(-1, 2))
    d_start = ctx.to_device((np.arange(n) * ul).astype(np.uint64))
    d_sf, d_cell = ctx.to_device(np.asarray(sfs, np.uint32)), ctx.to_device(np.asarray(cells, np.uint32))
    d_sub = ctx.alloc(n * ctx.subframe_floats(1) * 4)
    ctx.dl_frontend_dev(cfg, d_iq, None, d_start, d_sf, d_cell, n, d_sub)
    plan = ctx.pdsch_plan(cfg, 2, allocs)
    st, bits = plan.run(d_sub, sfs, cells)
    assert (st == 0).all(), st
    for u in range(n):
        lc, s = td.oracle_frontend(port, 2048, 100, 1, iq[u], sfs[u], cells[u])
        for a in range(9):
            k = u * 9 + a
            assert (bits[k] == tx[u, a, :allocs[k].tbs]).all()
            err, out, _ = oracle_pdsch(port, lc, s, allocs[k], 2, cells[u], 1)
            assert err == st[k] and (out == bits[k]).all()
    plan.close()
    for b in (d_iq, d_start, d_sf, d_cell, d_sub):
        b.free()


def test_big_allocation_soft_combining(ctx, port):
    """SURVEY 8d W4, "big" variant: one 100-PRB 64QAM allocation, E = 82 800 soft bits for K = 6016 -- 4.6 laps of the circular
    buffer, i.e. heavy soft combining.  The unmodified reference cannot run it (its scratch arrays hold 10 000 soft bits), so the
    checker is `oracle_big` -- the reference compiled through the sed of oracle/ref/Makefile that only enlarges those literals
     -- on its own receive grid; the restatement with scratch sized from the allocation must agree with both."""
    import fuzz_cases as fz
    import openlte_amd as m
    from openlte_amd import synth
    from oracle import pyoracle
    big = pyoracle.ref_big()
    if big is None:
        pytest.skip("oracle/_ref/libref_oracle_big.so not built (needs /root/reference)")
    cfg = m.DlCfg(2048, 100, 1, 0)
    sfs, cells = [1, 8], [17, 404]
    allocs = [m.make_alloc(u, 3, 5992, list(range(100)), 0x100 + u) for u in range(2)]
    for snr in (30, 14, 4):  # parity at every SNR (at 4 dB both sides fail the CRC); clean decode where the channel allows
        iq, tx = synth.dl_units(cfg, sfs, cells, allocs, 1, snr_db=snr, max_delay=4, seed=1234 + snr)
        cases = [fz.make_case(2048, 100, 1, cells[u], sfs[u], 2, 3, 5992, list(range(100)), 0x100 + u) for u in range(2)]
        r = fz.run_ref_dl(big, cases, iq=fz.pad_units(iq))
        for u in range(2):
            al = [m.make_alloc(0, 3, 5992, list(range(100)), 0x100 + u)]
            plan = ctx.pdsch_plan(cfg, 2, al)
            d_sub = ctx.to_device(np.ascontiguousarray(r["planes"][u, :4]).reshape(-1))
            st, bits = plan.run(d_sub, [sfs[u]], [cells[u]])
            assert r["n_soft"][u] == 82800
            assert (plan.soft_bits(0)[:82800] == r["soft"][u, :82800]).all()
            assert (st[0] == 0) == (r["rc"][u] == 0) and (st[0] != 0 or (bits[0] == r["bits"][u, :5992]).all())
            if snr >= 14:
                assert st[0] == 0 and (bits[0] == tx[u, 0, :5992]).all(), (snr, u)
            # the restatement on its own grid: the same verdict and block (its front end differs from the reference's by float rounding)
            lc, s = td.oracle_frontend(port, 2048, 100, 1, iq[u], sfs[u], cells[u])
            err, out, desc = oracle_pdsch(port, lc, s, al[0], 2, cells[u], 1)
            assert len(desc) == 82800 and (err == 0) == (st[0] == 0) and (err != 0 or (out == bits[0]).all())
            plan.close()
            d_sub.free()

@pytest.mark.parametrize("mod,tbs,nprb", [(1, 1000, 50), (2, 2024, 60), (1, 256, 40)])
def test_staged_soft_combining(ctx, port, mod, tbs, nprb):
    """Several laps of the circular buffer with the allocation's soft bits staged in LDS (E well below the staging limit): QPSK sums of
    soft values (the quantiser table path), 16QAM sums of +-127 (block maxima of 254, 381, ...)."""
    import openlte_amd as m
    from openlte_amd import synth
    cfg = m.DlCfg(2048, 100, 1, 0)
    sf, cell = 6, 77
    allocs = [m.make_alloc(0, mod, tbs, list(range(20, 20 + nprb)), 0x222)]
    for snr in (20, 2):
        iq, tx = synth.dl_units(cfg, [sf], [cell], allocs, 1, snr_db=snr, max_delay=4, seed=99 + snr)
        lc, s = td.oracle_frontend(port, 2048, 100, 1, iq[0], sf, cell)
        d_sub = ctx.to_device(upload_oracle_subframe(ctx, s, 1))
        plan = ctx.pdsch_plan(cfg, 2, allocs)
        st, bits = plan.run(d_sub, [sf], [cell])
        err, out, desc = oracle_pdsch(port, lc, s, allocs[0], 2, cell, 1)
        assert len(desc) < 40000 and len(desc) > 3 * (tbs + 28) * 2  # at least two laps, staged
        assert (plan.soft_bits(0)[:len(desc)] == desc).all()
        assert st[0] == err and (err != 0 or (bits[0] == out).all())
        if snr >= 20:
            assert err == 0 and (bits[0] == tx[0, 0, :tbs]).all()
        plan.close()
        d_sub.free()



def test_two_port_stage_parity(ctx, port):
    """Transmit-diversity combiner path (N_ant = 2) on a single-port capture: garbage in, but the
    same garbage out as the oracle -- exercises the reference's |h|^4 normaliser (quirk Q4)."""
    import openlte_amd as m
    from openlte_amd import synth
    cfg1 = m.DlCfg(2048, 100, 1, 0)
    allocs = td.small_allocs(0, 100, 3, 2024, 8)
    iq, _ = synth.dl_units(cfg1, [3], [42], allocs, 1, snr_db=25, seed=5)
    lc, s = td.oracle_frontend(port, 2048, 100, 2, iq[0], 3, 42)
    err, out, desc = oracle_pdsch(port, lc, s, allocs[0], 2, 42, 2)
    cfg = m.DlCfg(2048, 100, 2, 0)
    d_sub = ctx.to_device(upload_oracle_subframe(ctx, s, 2))
    plan = ctx.pdsch_plan(cfg, 2, allocs)
    st, bits = plan.run(d_sub, [3], [42])
    e = plan.soft_bits(0)
    assert e.shape == desc.shape and (e == desc).all()
    assert st[0] == err
    plan.close()
    d_sub.free()


def test_multi_block_transport_blocks_are_rejected(ctx):
    import openlte_amd as m
    cfg = m.DlCfg(2048, 100, 1, 0)
    with pytest.raises(m.MiLteError):
        ctx.pdsch_plan(cfg, 2, [m.make_alloc(0, 3, 6200, list(range(50)), 1)])


def test_w4_chain_batch_property(ctx):
    """Size-independent property at batch scale (BASELINE config 4, 4096 subframes x 9 allocations = 36 864 transport blocks, more
    than one launch wave of every kernel): every allocation passes its CRC and decodes to exactly the transmitted bits."""
    import openlte_amd as m
    from openlte_amd import synth
    cfg = m.DlCfg(2048, 100, 1, 0)
    U, n = 48, 4096
    sfs = np.array([[1, 2, 3, 4, 6, 7, 8, 9][i % 8] for i in range(U)], np.uint32)
    cells = ((np.arange(U) * 37) % 504).astype(np.uint32)
    allocs = []
    for u in range(U):
        allocs += td.w4_allocs(u)
    iq, tx = synth.dl_units(cfg, sfs, cells, allocs, 9, snr_db=30.0, max_delay=8, seed=2024)
    idx = np.arange(n) % U
    ul = iq.shape[1]
    d_iq = ctx.to_device(iq[idx].reshape(-1, 2))
    d_start = ctx.to_device((np.arange(n) * ul).astype(np.uint64))
    d_sf, d_cell = ctx.to_device(sfs[idx]), ctx.to_device(cells[idx])
    d_sub = ctx.alloc(n * ctx.subframe_floats(1) * 4)
    ctx.dl_frontend_dev(cfg, d_iq, None, d_start, d_sf, d_cell, n, d_sub)
    all_allocs = []
    for i in range(n):
        all_allocs += td.w4_allocs(i)
    plan = ctx.pdsch_plan(cfg, 2, all_allocs)
    d_out, d_st = ctx.alloc(n * 9 * plan.out_stride), ctx.alloc(n * 9 * 4)
    plan.run_dev(d_sub, d_sf, d_cell, d_out, d_st)
    st = d_st.download(np.int32)
    bits = d_out.download(np.uint8).reshape(n * 9, plan.out_stride)
    assert (st == 0).all(), int((st != 0).sum())
    want = np.zeros_like(bits)
    for a in range(9):
        t = 3240 if a < 8 else 1064
        want[a::9, :t] = tx[idx, a, :t]
        assert (bits[a::9, :t] == want[a::9, :t]).all(), a
    plan.close()
    for b in (d_iq, d_start, d_sf, d_cell, d_sub, d_out, d_st):
        b.free()


@pytest.mark.parametrize("n_ant", [2, 4])
def test_multi_port_transmit_diversity_end_to_end(ctx, ref, n_ant):
    """A real 2- / 4-port cell: CRS on every port and a transmit-diversity PDSCH from the reference's own transmitter, each
    antenna through its own channel, summed and quantised to int8.  (a) stage parity: fed the reference's received grid and
    estimates, the combiner / de-mapper / descrambler / decoder give the reference's soft bits and transport block exactly;
    (b) end to end through the library's own front end the transport block is the transmitted one."""
    import ctypes as C
    import openlte_amd as m
    from oracle import pyoracle as po
    cap = td.multi_port_capture(ref, n_ant)
    fft, nrb, cell, sf, cfi, tbs, prbs, msg, iq, la, phy = (cap[k] for k in ("fft", "nrb", "cell", "sf", "cfi", "tbs", "prbs", "msg", "iq", "la", "phy"))
    n_samp = 30720
    # the reference's receiver on the same int8-valued samples
    i_f = np.ascontiguousarray(np.concatenate([np.zeros(sf * n_samp, np.float32), iq[:, 0].astype(np.float32)]))
    q_f = np.ascontiguousarray(np.concatenate([np.zeros(sf * n_samp, np.float32), iq[:, 1].astype(np.float32)]))
    rx = ref.ref_subframe_new()
    assert ref.ref_get_dl_subframe_and_ce(phy, i_f, q_f, 0, sf, cell, n_ant, rx) == 0
    out, n = np.zeros(6200, np.uint8), C.c_uint32()
    rc = ref.ref_pdsch_channel_decode(phy, rx, C.byref(la), cfi, cell, n_ant, out, C.byref(n))
    assert rc == 0 and (out[:tbs] == msg).all(), "the reference does not decode its own %d-port transmission" % n_ant
    want_soft = np.ctypeslib.as_array(ref.ref_pdsch_descramb_bits_ptr(phy), shape=(12 * 12 * 12 * 4,)).copy()
    cfg = m.DlCfg(fft, nrb, n_ant, 0)
    alloc = [m.make_alloc(0, 2, tbs, prbs, 0x2345, 0, 2)]
    # (a) stage parity on the reference's grid
    grid = np.concatenate([po.ref_subframe_view(ref, rx, 0).ravel(), po.ref_subframe_view(ref, rx, 1).ravel(),
                           po.ref_subframe_view(ref, rx, 2, True)[:n_ant].ravel(), po.ref_subframe_view(ref, rx, 3, True)[:n_ant].ravel()]).astype(np.float32)
    d_sub = ctx.to_device(grid)
    plan = ctx.pdsch_plan(cfg, cfi, alloc)
    st, bits = plan.run(d_sub, [sf], [cell])
    e = plan.soft_bits(0)
    assert st[0] == 0 and (bits[0] == out[:tbs]).all()
    assert (e == want_soft[:len(e)].astype(np.int8)).all(), "soft bits differ from the reference's"
    d_sub.free()
    # (b) end to end through the library's front end
    got = ctx.dl_frontend(cfg, iq, [0], [sf], [cell])
    d_sub = ctx.to_device(np.ascontiguousarray(got[0], np.float32))
    st, bits = plan.run(d_sub, [sf], [cell])
    assert st[0] == 0 and (bits[0] == msg).all()
    plan.close()
    d_sub.free()
    ref.ref_subframe_free(rx)
    ref.ref_phy_free(phy)


@pytest.mark.parametrize("fft,nrb,n_ant", [(128, 6, 1), (256, 15, 2), (512, 25, 1), (1024, 50, 4), (2048, 75, 2)])
def test_every_bandwidth_end_to_end(ctx, ref, fft, nrb, n_ant):
    """The other five LTE bandwidths (FFT 128 ... 2048, 6 ... 75 resource blocks; 1, 2 or 4 ports): a 64QAM allocation from the reference's
    transmitter through the library's front end and PDSCH chain decodes to the transmitted block, and -- on the reference's own
    received grid -- to the reference's soft bits exactly."""
    import ctypes as C
    import openlte_amd as m
    from oracle import pyoracle as po
    n_sym = 3 if nrb <= 10 else 2  # PDCCH symbols (the helper's "cfi" argument is that count)
    cap = td.multi_port_capture(ref, n_ant, seed=fft, fft=fft, nrb=nrb, cell=(7 * nrb) % 504, sf=7, cfi=n_sym, mod=3, tbs=1064,
                                prbs=list(range(1, 6)))  # 5 PRB x 64QAM: E >= 3(K + 4) in every configuration
    n_samp, sf, cell, cfi, tbs, iq, la, phy = 30720 * fft // 2048, cap["sf"], cap["cell"], cap["cfi"], cap["tbs"], cap["iq"], cap["la"], cap["phy"]
    i_f = np.ascontiguousarray(np.concatenate([np.zeros(sf * n_samp, np.float32), iq[:, 0].astype(np.float32)]))
    q_f = np.ascontiguousarray(np.concatenate([np.zeros(sf * n_samp, np.float32), iq[:, 1].astype(np.float32)]))
    rx = ref.ref_subframe_new()
    assert ref.ref_get_dl_subframe_and_ce(phy, i_f, q_f, 0, sf, cell, n_ant, rx) == 0
    out, n = np.zeros(6200, np.uint8), C.c_uint32()
    assert ref.ref_pdsch_channel_decode(phy, rx, C.byref(la), n_sym, cell, n_ant, out, C.byref(n)) == 0 and (out[:tbs] == cap["msg"]).all()
    cfg = m.DlCfg(fft, nrb, n_ant, 0)
    alloc = [m.make_alloc(0, 3, tbs, cap["prbs"], 0x2345, 0, 1 if n_ant == 1 else 2)]
    plan = ctx.pdsch_plan(cfg, n_sym, alloc)
    grid = np.concatenate([po.ref_subframe_view(ref, rx, 0).ravel(), po.ref_subframe_view(ref, rx, 1).ravel(),
                           po.ref_subframe_view(ref, rx, 2, True)[:n_ant].ravel(), po.ref_subframe_view(ref, rx, 3, True)[:n_ant].ravel()]).astype(np.float32)
    d_sub = ctx.to_device(grid)
    st, bits = plan.run(d_sub, [sf], [cell])
    e = plan.soft_bits(0)
    want = np.ctypeslib.as_array(ref.ref_pdsch_descramb_bits_ptr(phy), shape=(len(e),)).astype(np.int8)
    assert (e == want).all() and st[0] == 0 and (bits[0] == out[:tbs]).all()
    d_sub.free()
    got = ctx.dl_frontend(cfg, iq, [0], [sf], [cell])
    d_sub = ctx.to_device(np.ascontiguousarray(got[0], np.float32))
    st, bits = plan.run(d_sub, [sf], [cell])
    assert st[0] == 0 and (bits[0] == cap["msg"]).all()
    plan.close()
    d_sub.free()
    ref.ref_subframe_free(rx)
    ref.ref_phy_free(phy)


@pytest.mark.parametrize("rv,mod,tbs,nprb", [(1, 3, 3240, 12), (2, 2, 2024, 12), (3, 1, 680, 8), (2, 3, 1064, 4)])
def test_redundancy_versions(ctx, ref, rv, mod, tbs, nprb):
    """HARQ redundancy versions 1-3 (the circular buffer is read from another start column; the reference decodes each transmission
    on its own, without combining): exact soft bits and the same verdict / bits as the compiled reference."""
    import ctypes as C
    import openlte_amd as m
    from oracle import pyoracle as po
    cap = td.multi_port_capture(ref, 1, seed=10 * rv + mod, mod=mod, tbs=tbs, prbs=list(range(20, 20 + nprb)), rv=rv, noise=2.0)
    n_samp, sf, cell, iq, la, phy = 30720, cap["sf"], cap["cell"], cap["iq"], cap["la"], cap["phy"]
    i_f = np.ascontiguousarray(np.concatenate([np.zeros(sf * n_samp, np.float32), iq[:, 0].astype(np.float32)]))
    q_f = np.ascontiguousarray(np.concatenate([np.zeros(sf * n_samp, np.float32), iq[:, 1].astype(np.float32)]))
    rx = ref.ref_subframe_new()
    assert ref.ref_get_dl_subframe_and_ce(phy, i_f, q_f, 0, sf, cell, 1, rx) == 0
    out, n = np.zeros(6200, np.uint8), C.c_uint32()
    rc = ref.ref_pdsch_channel_decode(phy, rx, C.byref(la), 2, cell, 1, out, C.byref(n))
    cfg = m.DlCfg(2048, 100, 1, 0)
    plan = ctx.pdsch_plan(cfg, 2, [m.make_alloc(0, mod, tbs, cap["prbs"], 0x2345, rv, 1)])
    grid = np.concatenate([po.ref_subframe_view(ref, rx, 0).ravel(), po.ref_subframe_view(ref, rx, 1).ravel(),
                           po.ref_subframe_view(ref, rx, 2, True)[:1].ravel(), po.ref_subframe_view(ref, rx, 3, True)[:1].ravel()]).astype(np.float32)
    d_sub = ctx.to_device(grid)
    st, bits = plan.run(d_sub, [sf], [cell])
    e = plan.soft_bits(0)
    want = np.ctypeslib.as_array(ref.ref_pdsch_descramb_bits_ptr(phy), shape=(len(e),)).astype(np.int8)
    assert (e == want).all()
    assert (st[0] == 0) == (rc == 0)
    if rc == 0:
        assert (bits[0] == out[:tbs]).all()
    plan.close()
    d_sub.free()
    ref.ref_subframe_free(rx)
    ref.ref_phy_free(phy)


@pytest.mark.parametrize("tbs,mod,nprb", [(672, 1, 8), (1376, 2, 8), (2000, 3, 8), (680, 1, 8), (3200, 3, 12)])
def test_filler_bit_transport_blocks_same_verdict_as_reference(ctx, ref, tbs, mod, nprb):
    """F > 0 (tbs + 24 is not a turbo block size): the reference fails its own noise-free transmission with LIBLTE_ERROR_DECODE_FAIL
    because its receiver does not treat the filler positions as NULL (liblte_phy.cc:9826-9829, :11404).  Drop-in means
    the same verdict, and the same soft bits on the way there; tbs = 680 (F = 0) is the control that decodes."""
    import ctypes as C
    import openlte_amd as m
    from oracle import pyoracle as po
    cap = td.multi_port_capture(ref, 1, seed=tbs, mod=mod, tbs=tbs, prbs=list(range(30, 30 + nprb)), noise=0.0)
    sf, cell, iq, la, phy = cap["sf"], cap["cell"], cap["iq"], cap["la"], cap["phy"]
    i_f = np.ascontiguousarray(np.concatenate([np.zeros(sf * 30720, np.float32), iq[:, 0].astype(np.float32)]))
    q_f = np.ascontiguousarray(np.concatenate([np.zeros(sf * 30720, np.float32), iq[:, 1].astype(np.float32)]))
    rx = ref.ref_subframe_new()
    assert ref.ref_get_dl_subframe_and_ce(phy, i_f, q_f, 0, sf, cell, 1, rx) == 0
    out, n = np.zeros(6200, np.uint8), C.c_uint32()
    rc = ref.ref_pdsch_channel_decode(phy, rx, C.byref(la), 2, cell, 1, out, C.byref(n))
    assert (rc == 0) == (tbs == 680) and rc in (0, 2)
    cfg = m.DlCfg(2048, 100, 1, 0)
    plan = ctx.pdsch_plan(cfg, 2, [m.make_alloc(0, mod, tbs, cap["prbs"], 0x2345, 0, 1)])
    grid = np.concatenate([po.ref_subframe_view(ref, rx, 0).ravel(), po.ref_subframe_view(ref, rx, 1).ravel(),
                           po.ref_subframe_view(ref, rx, 2, True)[:1].ravel(), po.ref_subframe_view(ref, rx, 3, True)[:1].ravel()]).astype(np.float32)
    d_sub = ctx.to_device(grid)
    st, bits = plan.run(d_sub, [sf], [cell])
    e = plan.soft_bits(0)
    want = np.ctypeslib.as_array(ref.ref_pdsch_descramb_bits_ptr(phy), shape=(len(e),)).astype(np.int8)
    assert (e == want).all()
    assert st[0] == rc, (st[0], rc)
    if rc == 0:
        assert (bits[0] == out[:tbs]).all() and (bits[0] == cap["msg"]).all()
    plan.close()
    d_sub.free()
    ref.ref_subframe_free(rx)
    ref.ref_phy_free(phy)


def test_compact_estimate_form_is_bit_identical(ctx, port):
    """MI_LTE_CE_COMPACT (the form bench.py's chain runs in): the estimator stops after the frequency direction and the demodulator runs
    the reference's time interpolation (liblte_phy.cc:6119-6190) for its own resource elements.  Same arithmetic in the same order, so
    every soft bit, verdict and decoded bit must equal the full form's -- on W4 subframes, on subframes 0 and 5 (PBCH / PSS / SSS
    windows), with QPSK / 16QAM / 64QAM, with different PRBs in the two slots and at an SNR where blocks fail -- and the oracle's."""
    import openlte_amd as m
    from openlte_amd import synth
    cfg_f, cfg_c = m.DlCfg(2048, 100, 1, m.IQ_I8), m.DlCfg(2048, 100, 1, m.IQ_I8 | m.CE_COMPACT)
    sfs, cells = [0, 5, 3, 9, 6, 1], [0, 17, 100, 301, 404, 503]
    for case, snr in (("w4", 30.0), ("w4", 21.0), ("mixed", 25.0)):
        allocs = []
        for u in range(len(sfs)):
            if case == "w4":
                allocs += td.w4_allocs(u)
            else:
                allocs += [m.make_alloc(u, 1, 680, list(range(0, 8)), 0x200), m.make_alloc(u, 2, 1384, list(range(40, 48)), 0x201),
                           m.make_alloc(u, 3, 2024, list(range(50, 58)), 0x202, prbs_slot1=list(range(70, 78))),
                           m.make_alloc(u, 1, 1000, list(range(10, 40)), 0x203), m.make_alloc(u, 3, 1064, [99, 98, 97, 96], 0x204)]
        n_al = len(allocs) // len(sfs)
        iq, tx = synth.dl_units(cfg_f, sfs, cells, allocs, n_al, snr_db=snr, max_delay=5, seed=int(snr) + n_al)
        n, ul = len(sfs), iq.shape[1]
        d_iq = ctx.to_device(iq.reshape(-1, 2))
        d_start = ctx.to_device((np.arange(n) * ul).astype(np.uint64))
        d_sf, d_cell = ctx.to_device(np.asarray(sfs, np.uint32)), ctx.to_device(np.asarray(cells, np.uint32))
        res = []
        for cfg in (cfg_f, cfg_c):
            d_sub = ctx.alloc(n * ctx.subframe_floats(1) * 4)
            d_sub.zero()
            ctx.dl_frontend_dev(cfg, d_iq, None, d_start, d_sf, d_cell, n, d_sub)
            plan = ctx.pdsch_plan(cfg, 2, allocs)
            st, bits = plan.run(d_sub, sfs, cells)
            res.append((st.copy(), [b.copy() for b in bits], [plan.soft_bits(a).copy() for a in range(len(allocs))]))
            plan.close()
            d_sub.free()
        (st_f, bits_f, e_f), (st_c, bits_c, e_c) = res
        assert (st_f == st_c).all(), (case, snr)
        for a in range(len(allocs)):
            assert e_f[a].shape == e_c[a].shape and (e_f[a] == e_c[a]).all(), (case, snr, a, int((e_f[a] != e_c[a]).sum()))
            assert (bits_f[a] == bits_c[a]).all(), (case, snr, a)
        if case == "w4":  # and the oracle's verdicts / bits (the oracle's allocation has one PRB list for both slots)
            if snr >= 30:  # everything decodes except where the PBCH / PSS / SSS window of subframes 0 and 5 punctures an allocation below rate 1/3
                assert (st_c[18:] == 0).all()
            for u in (0, 3):
                lc, s = td.oracle_frontend(port, 2048, 100, 1, iq[u], sfs[u], cells[u])
                for a in range(9):
                    k = u * 9 + a
                    err, out, _ = oracle_pdsch(port, lc, s, allocs[k], 2, cells[u], 1)
                    assert err == st_c[k] and (err != 0 or (out == bits_c[k]).all()), (snr, u, a)
        for b in (d_iq, d_start, d_sf, d_cell):
            b.free()


@pytest.mark.parametrize("fft,nrb", [(128, 6), (256, 15), (512, 25), (1024, 50), (2048, 75)])
def test_compact_estimate_form_on_every_bandwidth(ctx, fft, nrb):
    """The compact estimate form (one wavefront per CRS symbol in the estimator, time interpolation in the demodulator) against the full
    form on the other five LTE bandwidths: soft bits, verdicts and decoded bits identical."""
    import openlte_amd as m
    from openlte_amd import synth
    cfg_f, cfg_c = m.DlCfg(fft, nrb, 1, m.IQ_I8), m.DlCfg(fft, nrb, 1, m.IQ_I8 | m.CE_COMPACT)
    sfs, cells = [0, 5, 2, 7], [3, 120, 251, 502]
    allocs = []
    w = max(1, min(6, nrb // 3))
    for u in range(len(sfs)):
        allocs += [m.make_alloc(u, 1, 72 if nrb < 15 else 224, list(range(0, w)), 0x500),
                   m.make_alloc(u, 3, 256 if nrb < 15 else 776, list(range(nrb - w, nrb)), 0x501),
                   m.make_alloc(u, 2, 152 if nrb < 15 else 504, list(range(nrb // 2 - w // 2, nrb // 2 - w // 2 + w)), 0x502)]  # across the sync window
    iq, tx = synth.dl_units(cfg_f, sfs, cells, allocs, 3, snr_db=22.0, max_delay=3, seed=fft)
    n, ul = len(sfs), iq.shape[1]
    d_iq = ctx.to_device(iq.reshape(-1, 2))
    d_start = ctx.to_device((np.arange(n) * ul).astype(np.uint64))
    d_sf, d_cell = ctx.to_device(np.asarray(sfs, np.uint32)), ctx.to_device(np.asarray(cells, np.uint32))
    res = []
    for cfg in (cfg_f, cfg_c):
        d_sub = ctx.alloc(n * ctx.subframe_floats(1) * 4)
        d_sub.zero()
        ctx.dl_frontend_dev(cfg, d_iq, None, d_start, d_sf, d_cell, n, d_sub)
        plan = ctx.pdsch_plan(cfg, 2, allocs)
        st, bits = plan.run(d_sub, sfs, cells)
        res.append((st.copy(), [b.copy() for b in bits], [plan.soft_bits(a).copy() for a in range(len(allocs))]))
        plan.close()
        d_sub.free()
    (st_f, bits_f, e_f), (st_c, bits_c, e_c) = res
    assert (st_f == st_c).all()
    for a in range(len(allocs)):
        assert e_f[a].shape == e_c[a].shape and (e_f[a] == e_c[a]).all(), (a, int((e_f[a] != e_c[a]).sum()))
        assert (bits_f[a] == bits_c[a]).all(), a
    assert (st_c == 0).sum() >= len(allocs) // 2
    for b in (d_iq, d_start, d_sf, d_cell):
        b.free()


def test_compact_estimate_form_is_single_port_only(ctx):
    import openlte_amd as m
    with pytest.raises(m.MiLteError):
        ctx.pdsch_plan(m.DlCfg(2048, 100, 2, m.IQ_I8 | m.CE_COMPACT), 2, td.small_allocs(0, 100, 3, 2024, 8))


def test_packed_output_equals_the_unpacked_bits(ctx):
    """mi_lte_pdsch_plan_set_output(packed): eight bits per byte, first bit most significant -- np.packbits of the one-bit-per-byte output,
    for several block sizes and modulations, in both decoder modes."""
    import openlte_amd as m
    from openlte_amd import synth
    cfg = m.DlCfg(2048, 100, 1, m.IQ_I8 | m.CE_COMPACT)
    sfs, cells = [2, 8], [10, 499]
    allocs = []
    for u in range(2):
        allocs += [m.make_alloc(u, 3, 3240, list(range(0, 12)), 0x300), m.make_alloc(u, 3, 2024, list(range(12, 20)), 0x301),
                   m.make_alloc(u, 2, 1384, list(range(30, 38)), 0x302), m.make_alloc(u, 1, 680, list(range(40, 48)), 0x303),
                   m.make_alloc(u, 3, 1064, list(range(96, 100)), 0x304)]
    iq, tx = synth.dl_units(cfg, sfs, cells, allocs, 5, snr_db=28, max_delay=4, seed=3)
    d_iq = ctx.to_device(iq.reshape(-1, 2))
    d_start = ctx.to_device((np.arange(2) * iq.shape[1]).astype(np.uint64))
    d_sf, d_cell = ctx.to_device(np.asarray(sfs, np.uint32)), ctx.to_device(np.asarray(cells, np.uint32))
    d_sub = ctx.alloc(2 * ctx.subframe_floats(1) * 4)
    ctx.dl_frontend_dev(cfg, d_iq, None, d_start, d_sf, d_cell, 2, d_sub)
    for mode in (m.TURBO_REF, m.TURBO_BCJR):
        plan = ctx.pdsch_plan(cfg, 2, allocs)
        if mode == m.TURBO_BCJR:
            plan.set_decoder(m.TURBO_BCJR, 6, 0)
        st, bits = plan.run(d_sub, sfs, cells)
        stride_bytes = plan.out_stride
        plan.set_packed(True)
        assert plan.out_stride == ((3240 // 8 + 63) // 64) * 64 and stride_bytes == ((3240 + 63) // 64) * 64
        d_out, d_st = ctx.alloc(len(allocs) * plan.out_stride), ctx.alloc(4 * len(allocs))
        d_out.zero()
        plan.run_dev(d_sub, d_sf, d_cell, d_out, d_st)
        st_p = d_st.download(np.int32)
        raw = d_out.download(np.uint8).reshape(len(allocs), plan.out_stride)
        assert (st_p == st).all()
        for a, al in enumerate(allocs):
            assert (raw[a, :al.tbs // 8] == np.packbits(bits[a])).all(), (mode, a)
            if st[a] == 0:
                assert (np.unpackbits(raw[a, :al.tbs // 8]) == tx[a // 5, a % 5, :al.tbs]).all()
        assert (st == 0).all()
        plan.close()
        d_out.free(); d_st.free()
    for b in (d_iq, d_start, d_sf, d_cell, d_sub):
        b.free()


@pytest.mark.parametrize("n_units,chunk,lanes", [(40, 16, 3), (64, 32, 2), (7, 8, 1)])
def test_host_batch_pipeline_equals_the_device_resident_chain(ctx, n_units, chunk, lanes):
    """mi_lte_dl_pipeline: int8 units from pinned host memory, chunks overlapped on several lanes, packed transport blocks and
    verdicts back in host memory -- identical to what the device-resident batch path produces for the same units, including a ragged
    last chunk."""
    import openlte_amd as m
    from openlte_amd import synth
    cfg = m.DlCfg(2048, 100, 1, m.IQ_I8 | m.CE_COMPACT)
    U = 8
    sfs_u = np.array([1, 2, 3, 4, 6, 7, 8, 9], np.uint32)
    cells_u = ((np.arange(U) * 61 + 5) % 504).astype(np.uint32)
    allocs_u = []
    for u in range(U):
        allocs_u += td.w4_allocs(u)
    iq_u, tx = synth.dl_units(cfg, sfs_u, cells_u, allocs_u, 9, snr_db=30, max_delay=6, seed=n_units)
    idx = (np.arange(n_units) * 3) % U
    pipe = m.DlPipeline(0, cfg, 2, td.w4_allocs(0), chunk, lanes)
    assert pipe.unit_samples == iq_u.shape[1]
    h_iq, h_sf, h_cell = m.HostBuffer((n_units, iq_u.shape[1], 2), np.int8), m.HostBuffer((n_units,), np.uint32), m.HostBuffer((n_units,), np.uint32)
    h_out, h_st = m.HostBuffer((n_units * 9, pipe.out_stride), np.uint8), m.HostBuffer((n_units * 9,), np.int32)
    h_iq.arr[:], h_sf.arr[:], h_cell.arr[:] = iq_u[idx], sfs_u[idx], cells_u[idx]
    h_out.arr[:], h_st.arr[:] = 0xEE, -7
    for _ in range(2):  # a second run over the same lanes: nothing is left over from the first
        pipe.run(h_iq.arr, h_sf.arr, h_cell.arr, n_units, h_out.arr, h_st.arr)
    # the device-resident path on the same units
    d_iq = ctx.to_device(iq_u[idx].reshape(-1, 2))
    d_start = ctx.to_device((np.arange(n_units) * iq_u.shape[1]).astype(np.uint64))
    d_sf, d_cell = ctx.to_device(sfs_u[idx]), ctx.to_device(cells_u[idx])
    d_sub = ctx.alloc(n_units * ctx.subframe_floats(1) * 4)
    ctx.dl_frontend_dev(cfg, d_iq, None, d_start, d_sf, d_cell, n_units, d_sub)
    all_allocs = []
    for i in range(n_units):
        all_allocs += td.w4_allocs(i)
    plan = ctx.pdsch_plan(cfg, 2, all_allocs)
    st, bits = plan.run(d_sub, sfs_u[idx], cells_u[idx])
    assert (h_st.arr == st).all() and (st == 0).all()
    for k in range(n_units * 9):
        t = all_allocs[k].tbs
        assert (np.unpackbits(h_out.arr[k, :t // 8]) == bits[k]).all(), k
        assert (bits[k] == tx[idx[k // 9], k % 9, :t]).all()
    plan.close()
    pipe.close()
    for b in (d_iq, d_start, d_sf, d_cell, d_sub):
        b.free()
    for b in (h_iq, h_sf, h_cell, h_out, h_st):
        b.free()


def test_random_allocations_stage_parity(ctx, port):
    """Seeded random PDSCH geometries at 20 MHz -- cell, subframe (0 and 5 included: PBCH / PSS / SSS windows), control-region size,
    modulation, allocation width and position, RNTI, transport block size (some punctured: E < 3(K+4), where both sides fail their CRC) --
    against the oracle on the oracle's own received grid: soft bits, verdict and decoded bits identical; and the same allocations
    through the library's own front end in the full and the compact estimate form: identical to each other."""
    import openlte_amd as m
    from openlte_amd import synth
    rng = np.random.default_rng(20260926)
    sizes = [k - 24 for k in td.ALL_K if k - 24 >= 16]
    cfg_f, cfg_c = m.DlCfg(2048, 100, 1, m.IQ_I8), m.DlCfg(2048, 100, 1, m.IQ_I8 | m.CE_COMPACT)
    n_ok = 0
    for case in range(28):
        cell, sf, cfi, mod = int(rng.integers(0, 504)), int(rng.integers(0, 10)), int(rng.integers(1, 4)), int(rng.integers(1, 4))
        n_prb = int(rng.integers(1, 21))
        first = int(rng.integers(0, 100 - n_prb + 1))
        if case % 4 == 0:  # across the sync window of subframes 0 / 5
            sf, first = (0, 5)[case // 4 % 2], int(rng.integers(40, 50))
        qm = (2, 4, 6)[mod - 1]
        e_ub = n_prb * 12 * (14 - cfi) * qm
        fit = [t for t in sizes if 3 * (t + 28) <= e_ub * (1.3 if case % 7 == 3 else 0.9) and t + 24 <= 6144]
        if not fit:
            continue
        tbs = int(fit[int(rng.integers(max(0, len(fit) - 6), len(fit)))])
        rnti = int(rng.integers(1, 0xFFF0))
        alloc = [m.make_alloc(0, mod, tbs, list(range(first, first + n_prb)), rnti)]
        snr = float(rng.choice([30.0, 18.0, 8.0]))
        iq, tx = synth.dl_units(cfg_f, [sf], [cell], alloc, 1, n_pdcch_symbs=cfi, snr_db=snr, max_delay=5, seed=case)
        lc, s = td.oracle_frontend(port, 2048, 100, 1, iq[0], sf, cell)
        err, out, desc = oracle_pdsch(port, lc, s, alloc[0], cfi, cell, 1)
        d_sub = ctx.to_device(upload_oracle_subframe(ctx, s, 1))
        plan = ctx.pdsch_plan(cfg_f, cfi, alloc)
        st, bits = plan.run(d_sub, [sf], [cell])
        e = plan.soft_bits(0)
        assert e.shape == desc.shape and (e == desc).all(), (case, cell, sf, cfi, mod, n_prb, first, tbs)
        assert st[0] == err and (err != 0 or (bits[0] == out).all()), (case, st[0], err)
        n_ok += err == 0
        plan.close()
        d_sub.free()
        # own front end, both estimate forms
        res = []
        d_iq, d_start = ctx.to_device(iq.reshape(-1, 2)), ctx.to_device(np.zeros(1, np.uint64))
        d_sf, d_cell = ctx.to_device(np.array([sf], np.uint32)), ctx.to_device(np.array([cell], np.uint32))
        for cfg in (cfg_f, cfg_c):
            d_sub = ctx.alloc(ctx.subframe_floats(1) * 4)
            d_sub.zero()
            ctx.dl_frontend_dev(cfg, d_iq, None, d_start, d_sf, d_cell, 1, d_sub)
            plan = ctx.pdsch_plan(cfg, cfi, alloc)
            st2, bits2 = plan.run(d_sub, [sf], [cell])
            res.append((int(st2[0]), bits2[0].copy(), plan.soft_bits(0).copy()))
            plan.close()
            d_sub.free()
        assert res[0][0] == res[1][0] and (res[0][1] == res[1][1]).all() and (res[0][2] == res[1][2]).all(), case
        for b in (d_iq, d_start, d_sf, d_cell):
            b.free()
    assert n_ok >= 10  # most cases decode; the punctured and the low-SNR ones fail on both sides alike


@pytest.mark.parametrize("fft,nrb,n_ant", [(128, 6, 1), (256, 15, 2), (512, 25, 4), (1024, 50, 2), (2048, 75, 1), (2048, 100, 4)])
def test_random_allocations_other_bandwidths_and_ports(ctx, port, fft, nrb, n_ant):
    """The same seeded random geometries on the other bandwidths and with the 2- / 4-port transmit-diversity combiner (on a single-port
    capture: garbage in, but the oracle's garbage out -- the reference's |h|^4 normaliser, quirk Q4, and the layer de-mapper are what is
    exercised): soft bits, verdict and bits equal the oracle's on the oracle's grid."""
    import openlte_amd as m
    from openlte_amd import synth
    rng = np.random.default_rng(fft * 7 + n_ant)
    sizes = [k - 24 for k in td.ALL_K if k - 24 >= 16]
    cfg1, cfg = m.DlCfg(fft, nrb, 1, m.IQ_I8), m.DlCfg(fft, nrb, n_ant, m.IQ_I8)
    done = 0
    for case in range(14):
        cell, cfi, mod = int(rng.integers(0, 504)), int(rng.integers(1, 4)), int(rng.integers(1, 4))
        sf = int(rng.integers(0, 10)) if case % 3 else (0, 5)[case // 3 % 2]  # subframes 0 / 5 for every port count (M_ap % 4 == 0 always: test_fuzz_cpu.py)
        n_sym = cfi + (1 if nrb <= 10 else 0)
        n_prb = int(rng.integers(1, min(nrb, 16) + 1))
        first = int(rng.integers(0, nrb - n_prb + 1))
        e_ub = n_prb * 12 * (14 - n_sym) * (2, 4, 6)[mod - 1]
        fit = [t for t in sizes if 3 * (t + 28) <= e_ub * 0.85]
        if not fit:
            continue
        tbs = int(fit[int(rng.integers(max(0, len(fit) - 5), len(fit)))])
        alloc = [m.make_alloc(0, mod, tbs, list(range(first, first + n_prb)), int(rng.integers(1, 0xFFF0)), 0, 1 if n_ant == 1 else 2)]
        iq, tx = synth.dl_units(cfg1, [sf], [cell], alloc, 1, n_pdcch_symbs=n_sym, snr_db=25.0, max_delay=2, seed=case)
        lc, s = td.oracle_frontend(port, fft, nrb, n_ant, iq[0], sf, cell)
        err, out, desc = oracle_pdsch(port, lc, s, alloc[0], n_sym, cell, n_ant)
        d_sub = ctx.to_device(upload_oracle_subframe(ctx, s, n_ant))
        plan = ctx.pdsch_plan(cfg, n_sym, alloc)
        st, bits = plan.run(d_sub, [sf], [cell])
        e = plan.soft_bits(0)
        assert e.shape == desc.shape and (e == desc).all(), (case, cell, sf, cfi, mod, n_prb, first, tbs, int((e[:min(len(e), len(desc))] != desc[:min(len(e), len(desc))]).sum()))
        assert st[0] == err and (err != 0 or (bits[0] == out).all()), (case, st[0], err)
        if n_ant == 1 and err == 0:
            assert (bits[0] == tx[0, 0, :tbs]).all()
        plan.close()
        d_sub.free()
        done += 1
    assert done >= 8


@pytest.mark.parametrize("tx_mode,tbs,nprb,mod,rv", [(3, 5992, 100, 3, 0), (4, 5352, 70, 2, 2), (3, 6120, 100, 3, 1), (1, 6120, 100, 3, 3), (8, 4584, 40, 3, 0)])
def test_limited_soft_buffer_and_redundancy_versions_on_large_blocks(ctx, port, tx_mode, tbs, nprb, mod, rv):
    """Transmission modes 3 / 4 / 8 halve the soft buffer (K_MIMO = 2, liblte_phy.cc:11381-11386): for the largest code blocks N_cb drops
    below K_w and the circular buffer wraps early -- the rank tables' odd combinations -- here with every redundancy version and heavy
    repetition (one 40-100 PRB allocation for one code block).  Checker: the restatement, whose scratch is sized from the allocation
    (the unmodified reference caps an allocation at 10 000 soft bits)."""
    import openlte_amd as m
    from openlte_amd import synth
    cfg = m.DlCfg(2048, 100, 1, 0)
    sf, cell = 7, 250
    rx_alloc = [m.make_alloc(0, mod, tbs, list(range(nprb)), 0x321, rv, tx_mode)]  # the host transmitter maps on one port whatever the mode and
    for snr in (30, 6):                                                           # takes its soft-buffer size from it, like the receiver
        iq, tx = synth.dl_units(cfg, [sf], [cell], rx_alloc, 1, snr_db=snr, max_delay=4, seed=tbs + rv)
        lc, s = td.oracle_frontend(port, 2048, 100, 1, iq[0], sf, cell)
        err, out, desc = oracle_pdsch(port, lc, s, rx_alloc[0], 2, cell, 1)
        d_sub = ctx.to_device(upload_oracle_subframe(ctx, s, 1))
        plan = ctx.pdsch_plan(cfg, 2, rx_alloc)
        st, bits = plan.run(d_sub, [sf], [cell])
        assert (plan.soft_bits(0)[:len(desc)] == desc).all()
        assert st[0] == err and (err != 0 or (bits[0] == out).all()), (snr, st[0], err)
        if err == 0:  # (the K = 6144 block with half a soft buffer fails in the reference's decoder even at 30 dB: punctured, and its interleaver wraps)
            assert (bits[0] == tx[0, 0, :tbs]).all(), (tx_mode, tbs)
        plan.close()
        d_sub.free()


@pytest.mark.parametrize("tbs,mod,nprb", [(16, 1, 1), (32, 1, 2), (48, 2, 1), (104, 1, 2), (152, 3, 1), (256, 1, 4), (296, 2, 3), (440, 1, 6)])
def test_tiny_transport_blocks(ctx, port, tbs, mod, nprb):
    """The smallest code blocks (K = 40 ... 464), half of them with K % 16 == 8: the last unit of the per-code-block kernels holds eight
    positions, which is its own path in the rate un-matching gather, the vote and the CRC (whose weights are derived from one table
    entry: the short unit starts from a negative exponent).  Soft bits, verdict and decoded bits against the oracle at three SNRs."""
    import openlte_amd as m
    from openlte_amd import synth
    K = tbs + 24
    assert K in td.ALL_K
    cfg = m.DlCfg(2048, 100, 1, m.IQ_I8)
    n_ok = 0
    for k, snr in enumerate((30.0, 12.0, 4.0)):
        cell, sf, first = 17 + 31 * k, (1, 4, 8)[k], 20 + 7 * k
        alloc = [m.make_alloc(0, mod, tbs, list(range(first, first + nprb)), 0x200 + k)]
        iq, tx = synth.dl_units(cfg, [sf], [cell], alloc, 1, n_pdcch_symbs=2, snr_db=snr, max_delay=4, seed=tbs + k)
        lc, s = td.oracle_frontend(port, 2048, 100, 1, iq[0], sf, cell)
        err, out, desc = oracle_pdsch(port, lc, s, alloc[0], 2, cell, 1)
        d_sub = ctx.to_device(upload_oracle_subframe(ctx, s, 1))
        plan = ctx.pdsch_plan(cfg, 2, alloc)
        st, bits = plan.run(d_sub, [sf], [cell])
        e = plan.soft_bits(0)
        assert e.shape == desc.shape and (e == desc).all(), (tbs, snr)
        assert st[0] == err and (err != 0 or (bits[0] == out).all()), (tbs, snr, st[0], err)
        if err == 0:
            assert (bits[0] == tx[0, 0, :tbs]).all()
            n_ok += 1
        plan.close()
        d_sub.free()
    assert n_ok >= 1, tbs  # the 30 dB case decodes


def _ulp_ladder(x, steps):
    """float32 neighbours of x: x stepped by each entry of `steps` ulps"""
    out = []
    for k in steps:
        v = np.float32(x)
        for _ in range(abs(k)):
            v = np.nextafter(v, np.float32(np.inf if k > 0 else -np.inf), dtype=np.float32)
        out.append(v)
    return np.array(out, np.float32)


@pytest.mark.parametrize("form", ["full", "compact", "two_port"])
@pytest.mark.parametrize("mod", [2, 3])
def test_qam_decisions_next_to_the_thresholds(ctx, ref, port, mod, form):
    """16QAM / 64QAM hard decisions are taken without the equaliser's divisions (phy_dev.hpp qam_neg_bits_nodiv); next to a threshold the
    kernel divides as the reference does (liblte_phy.cc:7680-7690 -> :9573-9659).  Here every resource element of the allocations holds a
    symbol whose real or imaginary part, after the reference's own equaliser arithmetic, lands 0-3 ulp either side of a de-mapper
    threshold (0, 2/sqrt(42), 4/sqrt(42), 6/sqrt(42); 0, 2/sqrt(10)), with three kinds of channel estimate: 1 (the quotient IS the
    received value), 2 (exact halving) and random gains (the quotient rounds wherever it rounds).  Soft bits must equal the reference's
    on all of them -- in the full estimate form, in the compact form (magnitude / phase rows, time interpolation in the demodulator) and
    through the two-port combiner."""
    import ctypes as C
    import openlte_amd as m
    from oracle import pyoracle as po
    rng = np.random.default_rng(100 * mod + len(form))
    n_ant = 2 if form == "two_port" else 1
    cell, sf, cfi = 77, 3, 2
    t = 2 / np.sqrt(42.0) if mod == 3 else 2 / np.sqrt(10.0)
    thr = [np.float32(0.0)] + [np.float32(k * t) for k in ((1, 2, 3) if mod == 3 else (1,))]  # liblte_phy.cc:9514-9517
    ladder = np.concatenate([_ulp_ladder(s * th, range(-3, 4)) for th in thr for s in (1, -1)] +
                            [np.array([0.0, -0.0, 1e-45, -1e-45, 1e-38, -1e-38], np.float32)])
    # the grid: y = target * gain, gain per sub-carrier constant over the subframe (the compact form interpolates it in time)
    gains = np.ones(1200, np.float32)
    gains[400:800] = 2.0
    gains[800:] = rng.uniform(0.3, 3.0, 400).astype(np.float32)
    kind = rng.integers(0, 3, (14, 1200))  # 0: both parts next to a threshold, 1: the real part only, 2: the imaginary part only
    free = rng.uniform(-1.3, 1.3, (2, 14, 1200)).astype(np.float32)
    tgt_re = np.where(kind == 2, free[0], rng.choice(ladder, (14, 1200))).astype(np.float32)
    tgt_im = np.where(kind == 1, free[1], rng.choice(ladder, (14, 1200))).astype(np.float32)
    y_re = np.zeros((16, 1200), np.float32)
    y_im = np.zeros((16, 1200), np.float32)
    y_re[:14], y_im[:14] = tgt_re * gains, tgt_im * gains  # exact for gains 1 and 2
    ce_re = np.zeros((4, 16, 1200), np.float32)
    ce_im = np.zeros((4, 16, 1200), np.float32)
    ce_re[0, :14] = gains  # port 0: (gain, 0); port 1 (two_port): 0, so the combiner's normaliser is gain^2 -> sqrt -> gain^2 again
    phy = ref.ref_phy_new(4, cell, n_ant, 100)
    rx = ref.ref_subframe_new()
    ref.ref_subframe_set_num(rx, sf)
    po.ref_subframe_view(ref, rx, 0)[:], po.ref_subframe_view(ref, rx, 1)[:] = y_re, y_im
    po.ref_subframe_view(ref, rx, 2, True)[:], po.ref_subframe_view(ref, rx, 3, True)[:] = ce_re, ce_im
    tbs = {2: 1384, 3: 2024}[mod]
    allocs = [m.make_alloc(0, mod, tbs, list(range(p, p + 10)), 0x300 + p, 0, 2 if n_ant == 2 else 1) for p in range(0, 100, 10)]
    if form == "compact":
        cfg = m.DlCfg(2048, 100, 1, m.IQ_I8 | m.CE_COMPACT)
        h_m, h_a = np.zeros((16, 1200), np.float32), np.zeros((16, 1200), np.float32)
        h_m[:5] = gains  # magnitude rows at the five CRS symbols, phase 0
        grid = np.concatenate([y_re.ravel(), y_im.ravel(), h_m.ravel(), h_a.ravel()])
    else:
        cfg = m.DlCfg(2048, 100, n_ant, 0)
        grid = np.concatenate([y_re.ravel(), y_im.ravel(), ce_re[:n_ant].ravel(), ce_im[:n_ant].ravel()])
    d_sub = ctx.to_device(grid.astype(np.float32))
    plan = ctx.pdsch_plan(cfg, cfi, allocs)
    plan.run(d_sub, [sf], [cell])
    n_sym = 0
    for a, al in enumerate(allocs):
        la = td.to_lo_alloc(al)
        out, n = np.zeros(6200, np.uint8), C.c_uint32()
        ref.ref_pdsch_channel_decode(phy, rx, C.byref(la), cfi, cell, n_ant, out, C.byref(n))  # (the verdict is a CRC failure: the bits are not a code word)
        e = plan.soft_bits(a)
        want = np.ctypeslib.as_array(ref.ref_pdsch_descramb_bits_ptr(phy), shape=(len(e),)).astype(np.int8)
        assert len(e) >= 10 * 12 * 10 * (4 if mod == 2 else 6) and (e == want).all(), (a, int((e != want).sum()))
        n_sym += len(e) // (4 if mod == 2 else 6)
    assert n_sym > 13000
    plan.close()
    d_sub.free()
    ref.ref_subframe_free(rx)
    ref.ref_phy_free(phy)


@pytest.mark.parametrize("form", ["full", "compact", "two_port"])
def test_qpsk_soft_values_next_to_an_integer(ctx, ref, port, form):
    """QPSK soft bits are (int)(127 (1 - dist)), dist the distance to the quadrant's constellation point (liblte_phy.cc:9541-9556 ->
    get_soft_decision :13880-13900).  The kernels take the hardware's 1-ulp square root and fall back to the correctly rounded one only
    where 127 (1 - dist) is within 2^-13 of an integer (phy_dev.hpp soft_decision_127) -- the only place the root's last bit can show.  Here
    every resource element holds a symbol for which that product lands within a few float steps of an integer k = 2 .. 126 (both sides of
    it), or sits at / beyond the distance cap, or on the constellation point itself; channel estimates 1, 2 and random gains as in the QAM
    test above.  Soft bits must equal the reference's on all of them."""
    import ctypes as C
    import openlte_amd as m
    from oracle import pyoracle as po
    rng = np.random.default_rng(31 + len(form))
    n_ant = 2 if form == "two_port" else 1
    cell, sf, cfi = 91, 6, 1
    r2 = np.float32(1 / np.sqrt(2.0))
    n = 14 * 1200
    # per element: quadrant, integer k, direction (pointing out of the origin's side so the quadrant holds), a step of -8 .. 8 floats
    sgn = rng.choice(np.array([-1.0, 1.0]), (2, n))
    k = rng.integers(2, 127, n)
    phi = rng.uniform(0.02, np.pi / 2 - 0.02, n)
    dist = 1.0 - k / 127.0
    d_im = (dist * np.sin(phi)).astype(np.float32)  # the imaginary offset as a float; the real one solved for in float64
    d_re = np.sqrt(np.maximum(dist * dist - d_im.astype(np.float64) ** 2, 0.0))
    x_re = (r2 + d_re).astype(np.float32)
    x_im = (r2 + d_im).astype(np.float32)
    steps = rng.integers(-8, 9, n)
    for s in range(1, 9):
        x_re = np.where(steps >= s, np.nextafter(x_re, np.float32(np.inf), dtype=np.float32), x_re)
        x_re = np.where(steps <= -s, np.nextafter(x_re, np.float32(-np.inf), dtype=np.float32), x_re)
    # how close did that get?  (the reference's own float chain, restated)
    e_re, e_im = x_re - r2, x_im - r2
    v = np.float32(127) * (np.float32(1) - np.minimum(np.sqrt(e_re * e_re + e_im * e_im, dtype=np.float32), np.float32(1 - 1 / 120)))
    near = np.abs(v - np.rint(v)) < 2.0 ** -13
    assert near.mean() > 0.9, near.mean()
    special = rng.integers(0, 40, n)  # one in 40 each: on the constellation point; at the distance cap; far beyond it
    x_re = np.where(special == 0, r2, x_re)
    x_im = np.where(special == 0, r2, x_im)
    cap = np.float32(1 - 1 / 120)
    x_re = np.where(special == 1, r2 + cap, x_re).astype(np.float32)
    x_im = np.where(special == 1, r2, x_im).astype(np.float32)
    x_re = np.where(special == 2, r2 + np.float32(1.7), x_re).astype(np.float32)
    tgt_re = (x_re * sgn[0]).astype(np.float32).reshape(14, 1200)
    tgt_im = (x_im * sgn[1]).astype(np.float32).reshape(14, 1200)
    gains = np.ones(1200, np.float32)
    gains[600:900] = 2.0
    gains[900:] = rng.uniform(0.3, 3.0, 300).astype(np.float32)
    y_re = np.zeros((16, 1200), np.float32)
    y_im = np.zeros((16, 1200), np.float32)
    y_re[:14], y_im[:14] = tgt_re * gains, tgt_im * gains  # exact for gains 1 and 2
    ce_re = np.zeros((4, 16, 1200), np.float32)
    ce_im = np.zeros((4, 16, 1200), np.float32)
    ce_re[0, :14] = gains
    phy = ref.ref_phy_new(4, cell, n_ant, 100)
    rx = ref.ref_subframe_new()
    ref.ref_subframe_set_num(rx, sf)
    po.ref_subframe_view(ref, rx, 0)[:], po.ref_subframe_view(ref, rx, 1)[:] = y_re, y_im
    po.ref_subframe_view(ref, rx, 2, True)[:], po.ref_subframe_view(ref, rx, 3, True)[:] = ce_re, ce_im
    allocs = [m.make_alloc(0, 1, 256, list(range(p, p + 10)), 0x500 + p, 0, 2 if n_ant == 2 else 1) for p in range(0, 100, 10)]
    if form == "compact":
        cfg = m.DlCfg(2048, 100, 1, m.IQ_I8 | m.CE_COMPACT)
        h_m, h_a = np.zeros((16, 1200), np.float32), np.zeros((16, 1200), np.float32)
        h_m[:5] = gains
        grid = np.concatenate([y_re.ravel(), y_im.ravel(), h_m.ravel(), h_a.ravel()])
    else:
        cfg = m.DlCfg(2048, 100, n_ant, 0)
        grid = np.concatenate([y_re.ravel(), y_im.ravel(), ce_re[:n_ant].ravel(), ce_im[:n_ant].ravel()])
    d_sub = ctx.to_device(grid.astype(np.float32))
    plan = ctx.pdsch_plan(cfg, cfi, allocs)
    plan.run(d_sub, [sf], [cell])
    n_sym, values = 0, set()
    for a, al in enumerate(allocs):
        la = td.to_lo_alloc(al)
        out, nb = np.zeros(6200, np.uint8), C.c_uint32()
        ref.ref_pdsch_channel_decode(phy, rx, C.byref(la), cfi, cell, n_ant, out, C.byref(nb))  # (the verdict is a CRC failure: the bits are not a code word)
        e = plan.soft_bits(a)
        want = np.ctypeslib.as_array(ref.ref_pdsch_descramb_bits_ptr(phy), shape=(len(e),)).astype(np.int8)
        assert len(e) >= 10 * 12 * 10 * 2 and (e == want).all(), (a, int((e != want).sum()), np.flatnonzero(e != want)[:8], e[e != want][:8], want[e != want][:8])
        n_sym += len(e) // 2
        values |= set(np.abs(e).tolist())
    assert n_sym > 13000 and len(values) > 100  # (the whole range of soft values took part)
    plan.close()
    d_sub.free()
    ref.ref_subframe_free(rx)
    ref.ref_phy_free(phy)
