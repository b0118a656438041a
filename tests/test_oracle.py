"""CPU tests: the plain-C oracle against (a) the reference compiled in place (where available) and
(b) the committed golden fixtures generated from that reference build."""
import os

import numpy as np
import pytest

import lte_testdata as td

GOLD = os.path.join(os.path.dirname(__file__), "golden")


def golden_cases(name):
    z = np.load(os.path.join(GOLD, name))
    keys = sorted({k.rsplit("_", 1)[0] for k in z.files})
    return z, keys


def test_port_matches_golden_turbo_ref(port):
    """Pins the restatement on machines without /root/reference."""
    z, keys = golden_cases("turbo_ref.npz")
    assert len(keys) >= 9
    for key in keys:
        K = int(key.split("_")[0][1:])
        soft, want = z[key + "_soft"], z[key + "_bits"]
        got = td.oracle_turbo_ref(port, soft, K)
        assert (np.packbits(got, axis=-1) == want).all(), key


@td.on_both_boxes
@pytest.mark.parametrize("K", [40, 48, 200, 512, 1024, 3584, 4224, 6016, 6080, 6144])
def test_port_turbo_ref_vs_reference(port, ref, ref_phy, K, box):
    """Differential test against the compiled reference, incl. uint32-overflow sizes."""
    for kind in ("clean", "awgn0.5", "awgn0.8", "int"):
        tx, soft = td.turbo_blocks(port, K, 3, kind, seed=K)
        for b in range(3):
            d = np.ascontiguousarray(soft[b], dtype=np.float32)
            a, c = np.zeros(K, np.uint8), np.zeros(K, np.uint8)
            ref.ref_turbo_decode(ref_phy, d.copy(), 3 * (K + 4), a)
            port.lo_turbo_decode_ref(d.copy(), K, c)
            assert (a == c).all(), (K, kind, b)


@td.on_both_boxes
def test_port_all_188_block_sizes_vs_reference(port, ref, ref_phy, box):
    from oracle.pyoracle import port as _p  # noqa: F401
    rng = np.random.default_rng(5)
    sizes = list(range(40, 513, 8)) + list(range(528, 1025, 16)) + list(range(1056, 2049, 32)) + list(range(2112, 6145, 64))
    assert len(sizes) == 188
    for K in sizes:
        c = rng.integers(0, 2, K).astype(np.uint8)
        d1, d2 = np.zeros(3 * (K + 4), np.uint8), np.zeros(3 * (K + 4), np.uint8)
        ref.ref_turbo_encode(ref_phy, c, K, d1)
        port.lo_turbo_encode(c, K, d2)
        assert (d1 == d2).all(), K
        x = (1 - 2 * d1.reshape(3, K + 4).astype(np.float32)) + 0.6 * rng.standard_normal((3, K + 4)).astype(np.float32)
        d = np.ascontiguousarray(x.T.reshape(-1))
        a, b = np.zeros(K, np.uint8), np.zeros(K, np.uint8)
        ref.ref_turbo_decode(ref_phy, d.copy(), 3 * (K + 4), a)
        port.lo_turbo_decode_ref(d.copy(), K, b)
        assert (a == b).all(), K


@td.on_both_boxes
def test_port_siso_and_fb_vs_reference(port, ref, ref_phy, box):
    rng = np.random.default_rng(11)
    for K in (40, 1024, 6144):
        x = rng.integers(-127, 128, 2 * K).astype(np.int8)
        x[rng.random(2 * K) < 0.1] = 0
        a, b = np.zeros(K + 16, np.int8), np.zeros(K + 16, np.int8)
        ref.ref_viterbi_siso(ref_phy, x, 2 * K, a)
        port.lo_viterbi_siso(x, K, b)
        assert (a[:K] == b[:K]).all()
        y = rng.integers(-127, 128, K).astype(np.int8)
        fa, fb = np.zeros(K + 8, np.int8), np.zeros(K + 8, np.int8)
        ref.ref_conv_encode_soft_g03(ref_phy, y, K, fa[1:])
        fa[0] = 127
        port.lo_fb_soft(y, K, fb)
        assert (fa[:K] == fb[:K]).all()


@td.on_both_boxes
def test_port_prs_crc_crs_vs_reference(port, ref, box):
    rng = np.random.default_rng(2)
    for c_init in (0, 1, 0x1234567, (0x1234 << 14) | (3 << 9) | 17, 2**31 - 1):
        a, b = np.zeros(3000, np.uint32), np.zeros(3000, np.uint8)
        ref.ref_generate_prs_c(c_init, 3000, a)
        port.lo_prs_c(c_init, 3000, b)
        assert (a == b).all()
    for n in (16, 40, 3240, 6120):
        bits = rng.integers(0, 2, n).astype(np.uint8)
        a, b = np.zeros(24, np.uint8), np.zeros(24, np.uint8)
        ref.ref_calc_crc24a(bits, n, a)
        port.lo_crc24a(bits, n, b)
        assert (a == b).all()
    for ns, l, cell in ((0, 0, 0), (7, 4, 17), (19, 1, 503)):
        a = [np.zeros(220, np.float32) for _ in range(4)]
        ref.ref_generate_crs(ns, l, cell, a[0], a[1])
        port.lo_generate_crs(ns, l, cell, a[2], a[3])
        assert (a[0] == a[2]).all() and (a[1] == a[3]).all()


@td.on_both_boxes
def test_port_rate_unmatch_vs_reference(port, ref, ref_phy, box):
    """Restated ratematch round trip (liblte/manual_tests/ratematch_test.cc:58-251) + element-wise
    comparison with the reference incl. puncturing, repetition (soft combining), rv, C, tx_mode."""
    rng = np.random.default_rng(3)
    for K in (40, 104, 512, 1088, 3264, 6016, 6144):
        D = K + 4
        for (rv, C_, M, txm, chan, ratio) in ((0, 1, 4, 2, 0, 3.0), (1, 1, 8, 1, 0, 2.1), (2, 2, 8, 3, 0, 4.7),
                                             (3, 1, 8, 1, 0, 3.3), (0, 1, 1, 1, 2, 3.0)):
            E = int(ratio * D) // 2 * 2
            e = rng.integers(-127, 128, E).astype(np.float32)
            a, b = np.full(3 * D, -7, np.float32), np.full(3 * D, -7, np.float32)
            n_soft = 250368 if chan == 0 else 1
            na = ref.ref_rate_unmatch_turbo(ref_phy, e.copy(), E, K, C_, txm, n_soft, M, chan, rv, a)
            nb = port.lo_rate_unmatch_turbo(e.copy(), E, D, C_, txm, n_soft, M, chan, rv, b)
            assert na == nb == 3 * D
            assert (a == b).all(), (K, rv, C_, M, txm, chan, ratio)
        # round trip with the TX side, error-free channel, G = 3D (ratematch_test.cc)
        c = rng.integers(0, 2, K).astype(np.uint8)
        d = np.zeros(3 * D, np.uint8)
        port.lo_turbo_encode(c, K, d)
        e8a, e8b = np.zeros(3 * D, np.uint8), np.zeros(3 * D, np.uint8)
        ref.ref_rate_match_turbo(ref_phy, d.copy(), 3 * D, 1, 2, 250368, 4, 0, 0, 3 * D, e8a)
        port.lo_rate_match_turbo(d, 3 * D, 1, 2, 250368, 4, 0, 0, 3 * D, e8b)
        assert (e8a == e8b).all()
        back = np.zeros(3 * D, np.float32)
        port.lo_rate_unmatch_turbo((1.0 - 2.0 * e8b).astype(np.float32), 3 * D, D, 1, 2, 250368, 4, 0, 0, back)
        rx = (back.reshape(D, 3).T < 0).astype(np.uint8).reshape(-1)
        if 250368 // 4 >= 3 * (D + 28):  # the manual test skips K where N_cb != K_w
            assert (rx == d).all()


@td.on_both_boxes
def test_port_demapper_vs_reference(port, ref, box):
    rng = np.random.default_rng(4)
    M = 4000
    re = (rng.standard_normal(M) * 0.8).astype(np.float32)
    im = (rng.standard_normal(M) * 0.8).astype(np.float32)
    for mod, q in ((0, 1), (1, 2), (2, 4), (3, 6)):
        a, b = np.zeros(q * M, np.int8), np.zeros(q * M, np.int8)
        na = ref.ref_modulation_demapper(re, im, M, mod, a)
        nb = port.lo_modulation_demapper(re, im, M, mod, b)
        assert na == nb == q * M and (a == b).all(), mod


@td.on_both_boxes
def test_port_pre_decoder_vs_reference(port, ref, box):
    rng = np.random.default_rng(6)
    for n_ant, M_ap in ((1, 1000), (2, 1000), (4, 1000), (4, 998)):
        cap = 5000
        y = [rng.standard_normal(M_ap + 8).astype(np.float32) for _ in range(2)]
        h = [rng.standard_normal(4 * cap).astype(np.float32) for _ in range(2)]
        xa = [np.zeros(10000, np.float32) for _ in range(2)]
        xb = [np.zeros(10000, np.float32) for _ in range(2)]
        import ctypes as C
        ml = C.c_uint32()
        ref.ref_pre_decoder_dl(y[0], y[1], h[0], h[1], cap, M_ap, n_ant, xa[0], xa[1], C.byref(ml))
        mb = port.lo_pre_decoder_dl(y[0], y[1], h[0], h[1], cap, M_ap, n_ant, xb[0], xb[1])
        assert ml.value == mb
        assert (xa[0] == xb[0]).all() and (xa[1] == xb[1]).all()


def test_bcjr_model_decodes_and_segments(port):
    """The plain-C model of the BCJR mode (the mode's specification): decodes BPSK/AWGN at Eb/N0 ~ 2.7 dB error free,
    with the exact 3GPP interleaver on a uint32-overflow size too, and cuts long blocks into up to 8 segments."""
    import ctypes as C
    port.lo_bcjr_n_seg.restype = C.c_uint32
    assert [port.lo_bcjr_n_seg(K) for K in (40, 512, 1024, 2048, 3264, 6144)] == [1, 1, 2, 4, 1, 8]
    rng = np.random.default_rng(4)
    for K, spec in ((512, 0), (2048, 0), (6144, 1)):
        tx = rng.integers(0, 2, K).astype(np.uint8)
        d = np.zeros(3 * (K + 4), np.uint8)
        if spec:  # encode with the 3GPP-exact interleaver: re-interleave by hand around the constituent encoders
            import openlte_amd.synth as synth
            _, soft8 = synth.turbo_soft_blocks(K, 1, flip=0.0, amp=8, seed=9, ref_wrap=False)
            txs, _ = synth.turbo_soft_blocks(K, 1, flip=0.0, amp=8, seed=9, ref_wrap=False)
            x = soft8[0].astype(np.float64) / 8.0
            tx = txs[0]
        else:
            port.lo_turbo_encode(np.ascontiguousarray(tx), K, d)
            x = np.ascontiguousarray((1.0 - 2.0 * d.reshape(3, K + 4)).T).reshape(-1)
        y = x + 0.9 * rng.standard_normal(x.shape)
        llr = np.clip(np.round(y * 8 / 0.81), -127, 127).astype(np.int16)
        out = np.zeros(K, np.uint8)
        port.lo_turbo_decode_bcjr(np.ascontiguousarray(llr), K, 8, spec, out)
        assert (out == tx).all(), (K, spec)


def test_bcjr_block_model_segments_and_decodes(port):
    """The model of MI_LTE_TURBO_BCJR_BLOCK (one code block per wavefront): the batch model with the alpha recursion restarting every
    lo_bcjr_block_seg_len(K) steps -- a whole number of 32-step beta blocks per lane, at most 64 segments -- still decodes."""
    assert [port.lo_bcjr_block_seg_len(K) for K in (40, 2048, 2112, 4096, 4160, 6144)] == [32, 32, 64, 64, 96, 96]
    assert all((K + port.lo_bcjr_block_seg_len(K) - 1) // port.lo_bcjr_block_seg_len(K) <= 64 for K in td.ALL_K)
    rng = np.random.default_rng(8)
    for K in (40, 1088, 6016):
        tx = rng.integers(0, 2, K).astype(np.uint8)
        d = np.zeros(3 * (K + 4), np.uint8)
        port.lo_turbo_encode(np.ascontiguousarray(tx), K, d)
        x = np.ascontiguousarray((1.0 - 2.0 * d.reshape(3, K + 4)).T).reshape(-1)
        y = x + 0.9 * rng.standard_normal(x.shape)
        llr = np.clip(np.round(y * 8 / 0.81), -127, 127).astype(np.int16)
        out = np.zeros(K, np.uint8)
        port.lo_turbo_decode_bcjr_block(np.ascontiguousarray(llr), K, 8, 0, out)
        assert (out == tx).all(), K


def _ref_vs_port_subframe(port, ref, iq_unit, sf, cell, n_ant):
    """Both CPU front ends on one int8 unit -> (ref phy, ref subframe, port cfg, port subframe)."""
    import ctypes as C
    from oracle import pyoracle as po
    i_f = np.ascontiguousarray(np.concatenate([np.zeros(sf * 30720, np.float32), iq_unit[:, 0].astype(np.float32)]))
    q_f = np.ascontiguousarray(np.concatenate([np.zeros(sf * 30720, np.float32), iq_unit[:, 1].astype(np.float32)]))
    phy, rx = ref.ref_phy_new(4, cell, n_ant, 100), ref.ref_subframe_new()
    assert ref.ref_get_dl_subframe_and_ce(phy, i_f, q_f, 0, sf, cell, n_ant, rx) == 0
    lc, s = td.oracle_frontend(port, 2048, 100, n_ant, iq_unit, sf, cell)
    return phy, rx, lc, s


@td.on_both_boxes
def test_port_w4_subframe_front_end_and_pdsch_decode_vs_reference(port, ref, box):
    """The two composite functions of the restatement that the GPU stage-parity and smoke tests check against, pinned directly on
    the headline configuration (20 MHz, 1 port, CFI 2, 8 x 12 PRB TBS 3240 + 1 x 4 PRB TBS 1064, 64QAM):
    lo_get_dl_subframe_and_ce vs liblte_phy_get_dl_subframe_and_ce (liblte_phy.cc:5905; float stage: both sit on a float64 DFT,
    so they agree to rounding) and lo_pdsch_channel_decode vs liblte_phy_pdsch_channel_decode (:3690) fed the SAME received grid:
    soft bits, decoded bits, bit count and return code identical for every allocation."""
    import ctypes as C
    import openlte_amd as m
    from openlte_amd import synth
    from oracle import pyoracle as po
    cfg = m.DlCfg(2048, 100, 1, 0)
    sfs, cells = [3, 8], [42, 301]
    allocs = td.w4_allocs(0) + td.w4_allocs(1)
    for snr in (30.0, 21.0):
        iq, tx = synth.dl_units(cfg, sfs, cells, allocs, 9, snr_db=snr, max_delay=6, seed=int(snr))
        for u in range(2):
            phy, rx, lc, s = _ref_vs_port_subframe(port, ref, iq[u], sfs[u], cells[u], 1)
            for which, name in ((0, "rx_symb_re"), (1, "rx_symb_im")):
                a, b = po.ref_subframe_view(ref, rx, which)[:15], s.arr(name)[:15]
                assert np.linalg.norm(a - b) <= 1e-6 * np.linalg.norm(a), name
            for which, name in ((2, "rx_ce_re"), (3, "rx_ce_im")):
                a, b = po.ref_subframe_view(ref, rx, which, True)[0, :14], s.arr(name)[0, :14]
                assert np.linalg.norm(a - b) <= 1e-5 * np.linalg.norm(a) and np.abs(a - b).max() <= 1e-4 * np.abs(a).max(), name
            # the same grid into both decoders: copy the reference's received symbols and estimates into the restatement's struct
            s.arr("rx_symb_re")[:] = po.ref_subframe_view(ref, rx, 0)
            s.arr("rx_symb_im")[:] = po.ref_subframe_view(ref, rx, 1)
            s.arr("rx_ce_re")[:] = po.ref_subframe_view(ref, rx, 2, True)
            s.arr("rx_ce_im")[:] = po.ref_subframe_view(ref, rx, 3, True)
            n_ok = 0
            for a in range(9):
                al = allocs[u * 9 + a]
                la = td.to_lo_alloc(al)
                o1, n1, o2, n2 = np.zeros(6200, np.uint8), C.c_uint32(), np.zeros(6200, np.uint8), C.c_uint32()
                soft, ns = np.zeros(20000, np.int8), C.c_uint32()
                rc1 = ref.ref_pdsch_channel_decode(phy, rx, C.byref(la), 2, cells[u], 1, o1, C.byref(n1))
                rc2 = port.lo_pdsch_channel_decode(C.byref(lc), C.byref(s), C.byref(la), 2, cells[u], 1, o2, C.byref(n2), soft.ctypes.data_as(C.c_void_p), C.byref(ns))
                want_soft = np.ctypeslib.as_array(ref.ref_pdsch_soft_bits_ptr(phy), shape=(ns.value,))
                assert ns.value == (9936 if a < 8 else 3312) and (soft[:ns.value] == want_soft).all(), (snr, u, a)
                assert rc1 == rc2 and n1.value == n2.value and (o1[:n1.value] == o2[:n2.value]).all(), (snr, u, a, rc1, rc2)
                n_ok += rc1 == 0 and bool((o1[:al.tbs] == tx[u, a, :al.tbs]).all())
            assert n_ok == 9 or snr < 25
            ref.ref_subframe_free(rx)
            ref.ref_phy_free(phy)


@td.on_both_boxes
@pytest.mark.parametrize("tbs,mod,nprb", [(672, 1, 8), (1376, 2, 8), (2000, 3, 8), (680, 1, 8)])
def test_port_filler_bit_transport_blocks_vs_reference(port, ref, tbs, mod, nprb, box):
    """Transport blocks whose size + 24 is not a turbo block size (F > 0 filler bits).  The reference's transmitter skips the fillers
    when rate matching but its receiver does not treat them as NULL (uint8 filler markers never equal RX_NULL_BIT,
    liblte_phy.cc:9826-9829, :11404), so it fails its own noise-free loopback with LIBLTE_ERROR_DECODE_FAIL; tbs = 680 (F = 0) is the
    control.  The restatement must give the reference's verdict, bit count and soft bits."""
    import ctypes as C
    cap = td.multi_port_capture(ref, 1, seed=tbs, mod=mod, tbs=tbs, prbs=list(range(30, 30 + nprb)), noise=0.0)
    sf, cell, iq, la, phy = cap["sf"], cap["cell"], cap["iq"], cap["la"], cap["phy"]
    phy2, rx, lc, s = _ref_vs_port_subframe(port, ref, iq, sf, cell, 1)
    o1, n1, o2, n2 = np.zeros(6200, np.uint8), C.c_uint32(), np.zeros(6200, np.uint8), C.c_uint32()
    rc1 = ref.ref_pdsch_channel_decode(phy, rx, C.byref(la), 2, cell, 1, o1, C.byref(n1))
    s.arr("rx_symb_re")[:], s.arr("rx_symb_im")[:] = np.ctypeslib.as_array(ref.ref_subframe_ptr(rx, 0), shape=(16, 1200)), np.ctypeslib.as_array(ref.ref_subframe_ptr(rx, 1), shape=(16, 1200))
    s.arr("rx_ce_re")[:], s.arr("rx_ce_im")[:] = np.ctypeslib.as_array(ref.ref_subframe_ptr(rx, 2), shape=(4, 16, 1200)), np.ctypeslib.as_array(ref.ref_subframe_ptr(rx, 3), shape=(4, 16, 1200))
    rc2 = port.lo_pdsch_channel_decode(C.byref(lc), C.byref(s), C.byref(la), 2, cell, 1, o2, C.byref(n2), None, None)
    assert rc1 == rc2, (rc1, rc2)
    if tbs == 680:
        assert rc1 == 0 and (o1[:tbs] == cap["msg"]).all() and (o2[:tbs] == cap["msg"]).all()
    else:
        assert rc1 == 2  # LIBLTE_ERROR_DECODE_FAIL, noise-free
    ref.ref_subframe_free(rx)
    ref.ref_phy_free(phy)
    ref.ref_phy_free(phy2)


def test_bcjr_model_stays_inside_int16(port):
    """The kernels run two code blocks per lane on packed 16-bit arithmetic with no saturation; the model flags any intermediate that
    would leave int16.  Every one of the 188 block sizes (the segment lengths, and with them how far alpha and beta run between two
    normalisations' starting points, depend on K), both models (k_bcjr_block keeps its boundary states in int16 too), both interleavers,
    and the inputs that move the metrics most: +-127 with random signs, uniform noise, all +127 and all -127."""
    import ctypes as C
    port.lo_bcjr_range_ok.restype = C.c_int
    assert port.lo_bcjr_range_ok() == 1
    assert len(td.ALL_K) == 188

    def case(K):
        rng = np.random.default_rng(K)
        n = 3 * (K + 4)
        inputs = ((127 * (1 - 2 * rng.integers(0, 2, n))).astype(np.int16), rng.integers(-127, 128, n).astype(np.int16),
                  np.full(n, 127, np.int16), np.full(n, -127, np.int16))
        out = np.zeros(K, np.uint8)
        for soft in inputs:
            for model in (port.lo_turbo_decode_bcjr, port.lo_turbo_decode_bcjr_block):
                for spec in (0, 1):
                    model(np.ascontiguousarray(soft), K, 8, spec, out)
        return K, port.lo_bcjr_range_ok()  # (the flag is sticky and shared: the first size listed is near, not at, the one that cleared it)

    left = [K for K, ok in td.parallel_map(case, td.ALL_K, threads=max(1, min(16, len(os.sched_getaffinity(0))))) if ok != 1]
    assert port.lo_bcjr_range_ok() == 1 and not left, "an intermediate left int16; flag seen cleared after K = %s" % left[:8]


def test_closed_forms_of_the_two_float_sites_the_kernels_shortcut():
    """k_turbo_prep / k_turbo_perm replace two of the reference's float expressions by integer closed forms when the block maximum is the
    one saturated soft values produce: q(d) = (int8)(d * 127 / max) with max = 254 is d / 2 towards zero (liblte_phy.cc:10645-10664), and
    (int8)(127 * (w / W)) is w >> 1 for W = 254 and w for W = 127 (:10498-10524).  Exhaustive check in IEEE float32 (numpy rounds like the
    reference's SSE code and like the un-contracted device code)."""
    f = np.float32
    d = np.arange(-254, 255)
    assert ((d.astype(f) * f(127.0) / f(254.0)).astype(np.int32) == np.trunc(d / 2).astype(np.int32)).all()
    w = np.arange(0, 255)
    assert ((f(127.0) * (w.astype(f) / f(254.0))).astype(np.int32) == (w >> 1)).all()
    w = np.arange(0, 128)
    assert ((f(127.0) * (w.astype(f) / f(127.0))).astype(np.int32) == w).all()

def test_traceback_by_composition_of_state_maps_equals_the_serial_walk():
    """k_turbo_siso_small does not walk the reference's traceback (liblte_phy.cc:10483-10527): one step of it sends state s at time t+1 to
    2*(s & 3) + (compare bit of pair s & 3 at time t), a map of the 8 states onto themselves that depends on that step's four bits only,
    and maps compose associatively -- so a suffix scan over the steps gives every state at once.  The rule itself, in numpy: the serial
    walk against the suffix composition (doubling, as the kernel's scan does), on random compare bits and every end state."""
    rng = np.random.default_rng(5)
    for K in (8, 40, 64, 100, 528):
        bits = rng.integers(0, 2, (K, 4))
        maps = np.array([[2 * (s & 3) + bits[t, s & 3] for s in range(8)] for t in range(K)])  # f_t[s]
        # suffix composition G_t = f_t o f_{t+1} o ... o f_{K-1}, by doubling: G_t <- G_t o G_{t+d}
        G = maps.copy()
        d = 1
        while d < K:
            nxt = np.vstack([G[d:], np.tile(np.arange(8), (d, 1))])  # the identity past the end
            G = np.take_along_axis(G, nxt, axis=1)                  # (G_t o G_{t+d})[s] = G_t[G_{t+d}[s]]
            d *= 2
        for end in range(8):
            cur, serial = end, []
            for t in range(K - 1, -1, -1):
                cur = 2 * (cur & 3) + bits[t, cur & 3]
                serial.append(cur)
            assert (G[:, end] == np.array(serial[::-1])).all(), (K, end)

def _siso_states_on_lanes_model(x, y):
    """k_turbo_siso_small's arithmetic in numpy, for one trellis: four lanes, lane j holding the metrics of states j and j + 4 as int16
    (modulo 2^16), the branch terms (c, u) of acs_step2 (turbo.hip) per lane class, the compare bits of the four state pairs per step, the
    first strict minimum of the end metrics relative to state 0, and the traceback as a suffix composition of state maps.  Returns the sign
    decisions (True = the reference's "+" branch) -- the magnitudes are not the trellis kernel's business (k_turbo_prep makes them)."""
    K = len(x)
    X = np.zeros(4, np.int16)  # states 0..3
    Y = np.zeros(4, np.int16)  # states 4..7
    bits = np.zeros((K, 4), np.int64)
    with np.errstate(over="ignore"):
        for t in range(K):
            xi, yi = int(x[t]), int(y[t])
            m0, my = (-1 if xi < 0 else 0), (-1 if yi < 0 else 0)
            mx = m0 ^ my
            nmx = ~mx
            uP, uQ = ((xi + yi) << 1) & nmx, ((xi - yi) << 1) & mx
            c4 = (m0 & 8) - 4
            P2, Q2 = c4 & nmx, c4 & mx
            c = np.array([P2, Q2, -Q2, -P2], np.int16)   # lanes 0..3: states 0 (4), 1 (5), 2 (6), 3 (7)
            u = np.array([uP, uQ, -uQ, -uP], np.int16)
            pm = np.concatenate([X, Y])                  # what the quad_perm moves + byte permutes fetch: (PM[2j], PM[2j+1])
            a, b = pm[0::2].copy(), pm[1::2].copy()
            n = (b - a).astype(np.int16)
            bits[t] = n < 0
            X = np.where((n - c).astype(np.int16) < 0, (b + u).astype(np.int16), (a - u).astype(np.int16))
            Y = np.where((n + c).astype(np.int16) < 0, (b - u).astype(np.int16), (a + u).astype(np.int16))
        pm = np.concatenate([X, Y])
        best, end = 0, 0
        for st in range(1, 8):
            d = int(np.int16(pm[st] - pm[0]))
            if d < best:
                best, end = d, st
    maps = np.array([[2 * (s & 3) + bits[t, s & 3] for s in range(8)] for t in range(K)])
    G, d = maps.copy(), 1
    while d < K:
        nxt = np.vstack([G[d:], np.tile(np.arange(8), (d, 1))])
        G = np.take_along_axis(G, nxt, axis=1)
        d *= 2
    st = G[:, end]                                  # state at t
    nx = np.concatenate([st[1:], [end]])            # state at t + 1
    return (nx < st) | ((nx == st) & (nx == 0))


def test_states_on_lanes_siso_model_vs_the_restatement(port):
    """The arithmetic k_turbo_siso_small is built on (int16 metrics modulo 2^16, two states per lane with opposite branch signs, the
    composition traceback) against lo_viterbi_siso -- itself pinned to the reference above -- on inputs with a code word underneath, on
    noise, and on +-127 without a code word (the widest metric spread)."""
    rng = np.random.default_rng(21)
    for K, kind in ((40, "noise"), (104, "pm127"), (528, "noise"), (528, "sparse"), (1024, "pm127")):
        if kind == "noise":
            v = rng.integers(-127, 128, 2 * K)
        elif kind == "pm127":
            v = 127 * (1 - 2 * rng.integers(0, 2, 2 * K))
        else:
            v = rng.integers(-127, 128, 2 * K) * (rng.random(2 * K) < 0.3)
        v = v.astype(np.int8)
        out = np.zeros(K + 16, np.int8)
        port.lo_viterbi_siso(v, K, out)
        pos = _siso_states_on_lanes_model(v[0::2], v[1::2])
        w = np.abs(v[0::2].astype(np.int64)) + np.abs(v[1::2].astype(np.int64))
        mag = (np.float32(127) * (w.astype(np.float32) / np.float32(w.max()))).astype(np.int8) if w.max() else np.zeros(K, np.int8)
        want = np.where(pos, mag, -mag).astype(np.int8)
        assert (want == out[:K]).all(), (K, kind, int((want != out[:K]).sum()))


def _full_trellis_max_log_map(llr, K, pi, n_iter=8, scale=0.75):
    """Textbook max-log-MAP turbo decoding in float64, batch-vectorised: full-block alpha and beta recursions (no windows, no
    next-iteration initialisation, no fixed point), exact termination, extrinsic scaling 0.75.  llr: [n, 3(K+4)] in the reference's
    interleaved layout, positive = bit 0.  RSC: state s = 4 r1 + 2 r2 + r3, a = u ^ r2 ^ r3, next = 4a + (s >> 1), z = a ^ r1 ^ r3."""
    n = llr.shape[0]
    d = llr.reshape(n, K + 4, 3).astype(np.float64)
    ls1, lp1, lp2 = d[:, :K, 0], d[:, :K, 1], d[:, :K, 2]
    x = d[:, K:, :].reshape(n, 12)
    tails = ((x[:, [0, 2, 4]], x[:, [1, 3, 5]]), (x[:, [6, 8, 10]], x[:, [7, 9, 11]]))
    ls2 = ls1[:, pi]
    nxt = np.zeros((8, 2), int)
    par = np.zeros((8, 2), int)
    for s in range(8):
        r1, r2, r3 = s >> 2, (s >> 1) & 1, s & 1
        for u in (0, 1):
            a = u ^ r2 ^ r3
            nxt[s, u], par[s, u] = 4 * a + (s >> 1), a ^ r1 ^ r3
    NEG = -1e9

    def siso(ls, lp, la, tail):
        g = np.zeros((n, K, 8, 2))  # branch metric of the edge leaving state s with input u
        for s in range(8):
            for u in (0, 1):
                g[:, :, s, u] = (0.5 if u == 0 else -0.5) * (ls + la) + (0.5 if par[s, u] == 0 else -0.5) * lp
        alpha = np.full((n, K + 1, 8), NEG)
        alpha[:, 0, 0] = 0
        for t in range(K):
            new = np.full((n, 8), NEG)
            for s in range(8):
                for u in (0, 1):
                    new[:, nxt[s, u]] = np.maximum(new[:, nxt[s, u]], alpha[:, t, s] + g[:, t, s, u])
            alpha[:, t + 1] = new - new.max(axis=1, keepdims=True)
        beta = np.full((n, 8), NEG)  # through the three termination steps back from state 0: only the a = 0 edges exist
        beta[:, 0] = 0
        for k in (2, 1, 0):
            new = np.full((n, 8), NEG)
            for s in range(8):
                r1, r2, r3 = s >> 2, (s >> 1) & 1, s & 1
                u = r2 ^ r3  # the input that makes a = 0
                z = r1 ^ r3
                new[:, s] = beta[:, s >> 1] + (0.5 if u == 0 else -0.5) * tail[0][:, k] + (0.5 if z == 0 else -0.5) * tail[1][:, k]
            beta = new
        ext = np.zeros((n, K))
        app = np.zeros((n, K))
        for t in range(K - 1, -1, -1):
            m0 = np.full(n, NEG)
            m1 = np.full(n, NEG)
            new = np.full((n, 8), NEG)
            for s in range(8):
                e0 = g[:, t, s, 0] + beta[:, nxt[s, 0]]
                e1 = g[:, t, s, 1] + beta[:, nxt[s, 1]]
                m0 = np.maximum(m0, alpha[:, t, s] + e0)
                m1 = np.maximum(m1, alpha[:, t, s] + e1)
                new[:, s] = np.maximum(e0, e1)
            beta = new - new.max(axis=1, keepdims=True)
            app[:, t] = m0 - m1
            ext[:, t] = scale * (app[:, t] - ls[:, t] - la[:, t])
        return ext, app
    la1 = np.zeros((n, K))
    inv = np.argsort(pi)
    for _ in range(n_iter):
        e1, _ = siso(ls1, lp1, la1, tails[0])
        e2, app2 = siso(ls2, lp2, e1[:, pi], tails[1])
        la1 = e2[:, inv]
    return (app2[:, inv] < 0).astype(np.uint8)


def test_bcjr_models_lose_little_against_a_full_trellis_max_log_map(port):
    """The two fixed-point specifications of the BCJR modes trade windows, next-iteration initialisation, int8 half-resolution
    extrinsics and (block mode) 32-96 step alpha restarts for speed; "the kernels equal the model bit for bit" says nothing about what
    that costs in error rate.  This pins it: at the decoding threshold (K = 1088, rate 1/3, BPSK, 8 iterations, where the textbook
    float decoder still loses a few blocks in a hundred) neither model may lose more blocks than the textbook decoder does 0.2 dB
    further down (the loss is at most 0.2 dB), plus a small-sample allowance."""
    K, n = 1088, 160
    pi = np.zeros(K, np.uint16)
    port.lo_qpp_map_spec(K, pi)
    pi = pi.astype(int)
    rng = np.random.default_rng(2026)
    tx = rng.integers(0, 2, (n, K)).astype(np.uint8)
    code = np.zeros((n, 3 * (K + 4)), np.float64)
    for b in range(n):
        dd = np.zeros(3 * (K + 4), np.uint8)
        port.lo_turbo_encode(np.ascontiguousarray(tx[b]), K, dd)  # (K = 1088 is not one of the wrapped-interleaver sizes: ref map == spec map)
        code[b] = (1.0 - 2.0 * dd.reshape(3, K + 4)).T.reshape(-1)
    noise = rng.standard_normal(code.shape)
    bler = {}
    for snr_db in (-4.3, -4.1):  # Es/N0 per coded bit (rate 1/3: Eb/N0 = this + 4.77 dB, i.e. 0.47 and 0.67 dB)
        sigma = 10 ** (-snr_db / 20) / np.sqrt(2)
        y = code + sigma * noise
        llr_f = 2 * y / sigma ** 2
        q = np.clip(np.round(llr_f * 8.0), -127, 127)  # the int8 channel LLRs the kernels take (1/8 resolution)
        ref_bits = _full_trellis_max_log_map(q / 8.0, K, pi)
        i16 = np.ascontiguousarray(q.astype(np.int16))
        out = np.zeros(K, np.uint8)
        e_model = e_block = 0
        for b in range(n):
            port.lo_turbo_decode_bcjr(i16[b], K, 8, 1, out)
            e_model += int((out != tx[b]).any())
            port.lo_turbo_decode_bcjr_block(i16[b], K, 8, 1, out)
            e_block += int((out != tx[b]).any())
        bler[snr_db] = (int((ref_bits != tx).any(axis=1).sum()), e_model, e_block)
    lo, hi = bler[-4.3], bler[-4.1]   # measured when written: textbook 31 / 7 blocks of 160 lost, batch model 45 / 14, block model 56 / 25
    assert 10 < lo[0] < n // 2 and hi[0] < lo[0], bler   # both points sit on the textbook decoder's waterfall
    assert hi[1] <= lo[0] and hi[2] <= lo[0] + 2, bler    # 0.2 dB up, the models lose no more blocks than the textbook decoder lost below: <= 0.2 dB
    assert hi[1] <= hi[0] + 12 and lo[1] <= lo[0] + 24, bler  # and the batch model stays within a few blocks of it at the same point


def test_timing_fft_stand_in_agrees_with_the_parity_one(ref):
    """oracle/ref/fftw_shim_f32.c (single precision: what bench.py's cpu_baseline legs time) against fftw_shim.c (float64 radix-2: what
    every parity test uses) THROUGH the reference's own front ends: the downlink grid and estimates of a 20 MHz subframe
    (liblte_phy_get_dl_subframe_and_ce: 2048-point transforms), the uplink grid (liblte_phy_get_ul_subframe) and the PRACH
    root spectra made at init (839-point transforms: the mixed-radix / generic-prime path).  Single-precision rounding apart."""
    from oracle import pyoracle as po
    fast = po.ref_f32fft()
    if fast is None:
        pytest.skip("oracle/_ref/libref_oracle_f32fft.so not built")
    rng = np.random.default_rng(5)
    n = 30720 + 4400
    i_f = np.ascontiguousarray(rng.integers(-90, 91, n).astype(np.float32))
    q_f = np.ascontiguousarray(rng.integers(-90, 91, n).astype(np.float32))
    outs = []
    for R in (ref, fast):
        phy, rx = R.ref_phy_new(4, 77, 2, 100), R.ref_subframe_new()
        assert R.ref_get_dl_subframe_and_ce(phy, i_f, q_f, 0, 0, 77, 2, rx) == 0
        dl = [po.ref_subframe_view(R, rx, w)[:14].copy() for w in (0, 1)] + [po.ref_subframe_view(R, rx, w, True)[:2, :14].copy() for w in (2, 3)]
        assert R.ref_get_ul_subframe(phy, i_f, q_f, rx) == 0
        ul = [po.ref_subframe_view(R, rx, w)[:14].copy() for w in (0, 1)]
        R.ref_ul_init_prach(phy, 22, 0, 0, 1, 0)
        roots = []
        for r in range(min(R.ref_prach_n_roots(phy), 3)):
            a, b = np.zeros(839, np.float32), np.zeros(839, np.float32)
            R.ref_get_prach_root_fft(phy, r, a, b)
            roots += [a, b]
        outs.append(dl + ul + roots)
    for a, b in zip(*outs):
        assert np.linalg.norm(a) > 0 and np.linalg.norm(a - b) <= 3e-6 * np.linalg.norm(a)
    # the transform itself at the sizes the uplink's transform pre-decoding uses (12 * N_prb with N_prb = 2^a 3^b 5^c: radix 4 / 2 / 3 / 5
    # passes), both directions, against numpy's float64 FFT
    import ctypes as C
    c64 = np.ctypeslib.ndpointer(np.complex64, flags="C_CONTIGUOUS")
    for L in (ref, fast):
        L.fftwf_plan_dft_1d.restype = C.c_void_p
        L.fftwf_plan_dft_1d.argtypes = [C.c_int, c64, c64, C.c_int, C.c_uint]
        L.fftwf_execute.argtypes = [C.c_void_p]
        L.fftwf_destroy_plan.argtypes = [C.c_void_p]
    for n in (1, 2, 3, 8, 12, 24, 36, 60, 72, 108, 128, 180, 300, 512, 600, 1024, 1200, 1536, 7 * 11 * 4):
        x = (rng.standard_normal(n) + 1j * rng.standard_normal(n)).astype(np.complex64)
        for sign in (-1, 1):
            want = np.fft.fft(x.astype(np.complex128)) if sign < 0 else np.fft.ifft(x.astype(np.complex128)) * n
            for L in (ref, fast):
                y = np.zeros(n, np.complex64)
                plan = L.fftwf_plan_dft_1d(n, x, y, sign, 0)
                L.fftwf_execute(plan)
                L.fftwf_destroy_plan(plan)
                assert np.linalg.norm(y - want) <= 2e-6 * max(np.linalg.norm(want), 1e-30), (n, sign, L is fast)


@td.on_both_boxes
def test_demappers_atan2f_is_the_host_libms(port, box):
    """phy_dev.hpp's ref_atan2f (what the de-mappers decide QPSK / BPSK quadrants and PUCCH 1b regions on) against libm's atan2f on
    this host, bit for bit: arbitrary bit patterns (NaNs, infinities, zeros, denormals), pairs within 2^-60 .. 2^-1 of either axis and of
    the diagonals, moderate values.  The reference compares the float angle with 0, +-pi/2, pi (and +-pi/4, 3pi/4) in double, so one ulp
    of difference at those values is another quadrant (the soak's one differing soft bit in 320 000 cases)."""
    import ctypes as C
    import openlte_amd as m
    L = m.load_library()
    f32p = np.ctypeslib.ndpointer(np.float32, flags="C_CONTIGUOUS")
    L.mi_lte_model_atan2f.argtypes = [f32p, f32p, f32p, C.c_size_t]
    port.lo_libm_atan2f.argtypes = [f32p, f32p, f32p, C.c_uint64]
    rng = np.random.default_rng(17)
    n = 3_000_000

    def unit(k):  # random floats in [0.5, 1) with random signs
        return (rng.integers(0, 1 << 23, k, dtype=np.uint32) | np.uint32(0x3F000000) | (rng.integers(0, 2, k, dtype=np.uint32) << np.uint32(31))).view(np.float32)

    sets = []
    a, b = rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32).view(np.float32), rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32).view(np.float32)
    sets.append((a, b))
    small = np.ldexp(unit(n), -rng.integers(1, 61, n)).astype(np.float32)
    x = unit(n)
    sets.append((x * small, x))          # next to the real axis (both signs of both)
    sets.append((x, x * small))          # next to the imaginary axis
    d = (1.0 + rng.integers(-128, 129, n) * 1e-7).astype(np.float32) * rng.choice(np.array([-1.0, 1.0], np.float32), n)
    sets.append((x * d, x))              # next to the diagonals
    sets.append(((rng.integers(-2000, 2001, n) / 977.0).astype(np.float32), (rng.integers(-2000, 2001, n) / 1021.0).astype(np.float32)))
    sets.append((np.array([-1.0715198516845703e+00 * 0 + 4.047898727321808e-08, 0.0, -0.0, 0.0, -0.0, np.inf, -np.inf, np.nan, 1.0], np.float32),
                 np.array([-1.0715198516845703, -1.0, -1.0, 1.0, 0.0, -np.inf, np.inf, 1.0, np.nan], np.float32)))
    for y, xx in sets:
        y, xx = np.ascontiguousarray(y, np.float32), np.ascontiguousarray(xx, np.float32)
        got, want = np.zeros(len(y), np.float32), np.zeros(len(y), np.float32)
        assert L.mi_lte_model_atan2f(y, xx, got, len(y)) == 0
        port.lo_libm_atan2f(y, xx, want, len(y))
        same = (got.view(np.uint32) == want.view(np.uint32)) | (np.isnan(got) & np.isnan(want))
        assert same.all(), (y[~same][:4], xx[~same][:4], got[~same][:4], want[~same][:4])
    # the soak's symbol: below pi (second quadrant) with libm, above it with a few-ulp atan2f
    assert got[0].view(np.uint32) == 0x40490FDA


def test_port_two_port_front_end_vs_golden_from_reference(port):
    """The restatement's two-port front end on a capture from the reference's own two-port transmitter, against what the compiled
    reference made of it when the fixture was generated (tools/gen_golden.py two_port): symbol rows and both ports' estimate rows."""
    import os
    z = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "dl_two_port_units.npz"))
    _, s = td.oracle_frontend(port, 2048, 100, 2, z["iq"][0], int(z["sfs"][0]), int(z["cells"][0]))
    rel = lambda a, b: np.linalg.norm(a - b) / np.linalg.norm(b)
    assert rel(s.arr("rx_symb_re")[:14], z["symb_re"]) < 1e-5 and rel(s.arr("rx_symb_im")[:14], z["symb_im"]) < 1e-5
    for p in range(2):
        assert rel(s.arr("rx_ce_re")[p, :14], z["ce_re"][p]) < 1e-4 and rel(s.arr("rx_ce_im")[p, :14], z["ce_im"][p]) < 1e-4
        assert np.hypot(z["ce_re"][p], z["ce_im"][p]).mean() > 0.1  # a real second port: its estimate is a channel, not noise around zero


def test_prach_root_sets_vs_reference(ref):
    """The physical roots of a cell's 64 preambles (prach_sets.hpp: prach_root_set -- what mi_lte_prach_plan_create correlates against and the
    library's transmitter draws from) against what liblte_phy_ul_init leaves in LIBLTE_PHY_STRUCT, over formats 0 and 4 (1-3 share format 0's
    tables), every zeroCorrelationZoneConfig, both sets, and root indices that include the ends of the logical root tables: same number of
    roots, same root for every one that lies inside the reference's table.  Where the set runs past the table the reference indexes past it
    (liblte_phy.cc:7168-7171: whatever follows the array names the root) and the library continues at index 0 (36.211 5.7.2) -- there the
    count must still agree whenever the wrapped roots have as many cyclic shifts as the reference's stray ones (always, in the unrestricted
    set), and the wrapped roots must be the table's first entries."""
    import ctypes as C
    import openlte_amd as m
    from oracle import pyoracle as po
    if not hasattr(ref, "ref_get_prach_root_seq"):
        pytest.skip("oracle/_ref predates ref_get_prach_root_seq (rebuild it: make -C oracle/ref)")
    L = m.load_library()
    L.mi_lte_prach_root_set.argtypes = [C.POINTER(m.PrachCfg), np.ctypeslib.ndpointer(np.uint32, flags="C_CONTIGUOUS"), C.POINTER(C.c_uint32)]
    table4 = [(i // 2 + 1) if i % 2 == 0 else 139 - (i + 1) // 2 for i in range(138)]  # 36.211 table 5.7.2-5
    n_cmp = n_wrap = n_refused = 0
    re, im = np.zeros(839, np.float32), np.zeros(839, np.float32)
    for fmt, n_idx, n_zc, zmax in ((0, 838, 839, 16), (4, 138, 139, 7)):
        roots = sorted(set([0, 1, 2, 7, 22, 129, 300, 411, 836, 837] + list(range(n_idx - 70, n_idx, 9)) + [n_idx - 3, n_idx - 2, n_idx - 1]) & set(range(n_idx)))
        for root in roots:
            for zczc in range(zmax):
                for hs in (0, 1):
                    if (root * 7 + zczc * 3 + hs) % 4 and root < n_idx - 70:  # (the reference's init costs 0.1 s: a quarter of the inner grid, all of the table's end)
                        continue
                    pc = m.PrachCfg(root, fmt, zczc, hs, 0)
                    u = np.zeros(64, np.uint32)
                    n = C.c_uint32(0)
                    rc = L.mi_lte_prach_root_set(C.byref(pc), u, C.byref(n))
                    if rc != 0:  # configurations the reference cannot process (it divides by zero -- SIGFPE -- or indexes past its N_cs table): refused
                        n_refused += 1
                        continue
                    if hs and root + n.value > n_idx:  # restricted-set arithmetic on whatever follows the reference's table may divide by zero: not run
                        n_wrap += 1
                        continue
                    phy = ref.ref_phy_new(po.FS_ENUM[128], 1, 1, 6)
                    try:
                        assert ref.ref_ul_init_prach(phy, 1, root, fmt, zczc, hs) == 0
                        n_ref = ref.ref_prach_n_roots(phy)
                        inside = min(n.value, n_idx - root)
                        for r in range(min(inside, n_ref)):
                            ref.ref_get_prach_root_seq(phy, r, re, im)
                            u_ref = int(round(-np.arctan2(float(im[1]), float(re[1])) * n_zc / (2 * np.pi))) % n_zc  # x_u(1) = exp(-2 pi i u / N_zc)
                            assert u_ref == int(u[r]), (fmt, root, zczc, hs, r, u_ref, int(u[r]))
                        if root + n.value <= n_idx:
                            assert n_ref == n.value, (fmt, root, zczc, hs, n_ref, n.value)
                            n_cmp += 1
                        else:
                            n_wrap += 1
                            want = [(table4[i] if fmt == 4 else None) for i in range(n.value - inside)]
                            if fmt == 4:
                                assert [int(x) for x in u[inside:n.value]] == want, (root, zczc, hs, u[:n.value].tolist())
                            if not hs:
                                assert n_ref == n.value, (fmt, root, zczc, n_ref, n.value)
                    finally:
                        ref.ref_phy_free(phy)
    assert n_cmp > 200 and n_wrap > 20, (n_cmp, n_wrap, n_refused)
