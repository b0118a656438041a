"""GPU: the PDSCH plans' 3GPP transport-block mode (mi_lte_pdsch_plan_create_3gpp): transport blocks of 1..13 code blocks, 36.212
segmentation / CRC24B / code-block concatenation.  The reference cannot decode these (its C > 1 path is broken), so each stage
is pinned to what specifies it: rate un-matching to the reference's own liblte_phy_rate_unmatch_turbo with N_codeblocks = C, the decode to
the plain-C model of the BCJR decoder the plan ran, the assembly to a numpy desegmentation with both CRCs, and the whole chain to the
transmitted bits (mi_lte_synth_dl_units_3gpp_i8)."""
import ctypes as C

import numpy as np
import pytest

from test_dlsch3gpp_cpu import crc, tbs_table

pytestmark = pytest.mark.gpu

ERR_INVALID, ERR_UNSUPPORTED = -1, -4
G_A, G_B = 0x1864CFB, 0x1800063
FFT = {6: 128, 25: 512, 100: 2048}


def tbs(itbs, n_prb):
    return int(tbs_table()[itbs][n_prb - 1])


def alloc(unit, mod, size, prb0, n_prb, rnti, rv=0, txm=1):
    import openlte_amd as m
    return m.make_alloc(unit, mod, size, list(range(prb0, prb0 + n_prb)), rnti, rv_idx=rv, tx_mode=txm)


def run_cells(ctx, n_rb, sfs, cells, per_unit, n_soft, cfi, snr_db, seed, decoders=((1, 8),), packed=False):
    """Synthesise the units (3GPP transmitter), run the front end and ONE 3GPP plan over all of them, once per decoder.
    Returns (allocs, tx, plan, [(status, bits, cb_ok) per decoder])."""
    import openlte_amd as m
    from openlte_amd import synth
    cfg = m.DlCfg(FFT[n_rb], n_rb, 1, 0)
    n = len(sfs)
    allocs = [a for u in range(n) for a in per_unit[u]]
    iq, tx = synth.dl_units_3gpp(cfg, sfs, cells, allocs, len(per_unit[0]), n_soft, n_pdcch_symbs=cfi, snr_db=snr_db, max_delay=4, seed=seed)
    ul = iq.shape[1]
    d_iq = ctx.to_device(iq.reshape(-1, 2))
    d_start = ctx.to_device((np.arange(n) * ul).astype(np.uint64))
    d_sf, d_cell = ctx.to_device(np.asarray(sfs, np.uint32)), ctx.to_device(np.asarray(cells, np.uint32))
    d_sub = ctx.alloc(n * ctx.subframe_floats(1) * 4)
    ctx.dl_frontend_dev(cfg, d_iq, None, d_start, d_sf, d_cell, n, d_sub)
    plan = ctx.pdsch_plan_3gpp(cfg, cfi, allocs, n_soft)
    if packed:
        plan.set_packed(True)
    res = []
    for mode, n_iter in decoders:
        plan.set_decoder(mode, n_iter, 1)
        st, bits = plan.run(d_sub, sfs, cells)
        res.append((st, bits, plan.cb_ok()))
    for b in (d_iq, d_start, d_sf, d_cell, d_sub):
        b.free()
    return allocs, tx, plan, res


def expect_from_blocks(c_bits, size):
    """numpy desegmentation + CRCs of a transport block's decoded code blocks [C, K]: (payload bits, status, cb_ok mask)."""
    n_cb, K = c_bits.shape
    if n_cb == 1:
        ok_a = not crc(c_bits[0], G_A).any()  # the block with its CRC24A appended divides by the generator
        return c_bits[0, :size], 0 if ok_a else 2, 1 if ok_a else 0
    b = np.concatenate([c_bits[r, :K - 24] for r in range(n_cb)])
    ok_a = not crc(b, G_A).any()
    mask = sum(1 << r for r in range(n_cb) if not crc(c_bits[r], G_B).any())
    return b[:size], 0 if (ok_a and mask == (1 << n_cb) - 1) else 2, mask


def test_refusals(ctx):
    """The documented errors: BPSK, F != 0, tbs past the table, two ports (create); REF and the wrapped interleaver (set_decoder).
    A reference-mode plan refuses the multi-block sizes as before (duplicates, does not replace, tests/test_chain_gpu.py's check)."""
    import openlte_amd as m
    L, cfg, cfg2 = ctx.L, m.DlCfg(2048, 100, 1, 0), m.DlCfg(2048, 100, 2, 0)
    dl = m.DlschCfg(1237248, 8)

    def create(c, allocs):
        arr = (m.PdschAlloc * len(allocs))(*allocs)
        h = C.c_void_p()
        rc = L.mi_lte_pdsch_plan_create_3gpp(ctx.h, C.byref(c), 1, C.byref(dl), C.cast(arr, C.c_void_p), len(allocs), C.byref(h))
        if rc == 0:
            L.mi_lte_pdsch_plan_destroy(ctx.h, h)
        return rc

    def create_ref(allocs):
        arr = (m.PdschAlloc * len(allocs))(*allocs)
        h = C.c_void_p()
        rc = L.mi_lte_pdsch_plan_create(ctx.h, C.byref(cfg), 1, C.cast(arr, C.c_void_p), len(allocs), C.byref(h))
        if rc == 0:
            L.mi_lte_pdsch_plan_destroy(ctx.h, h)
        return rc

    good = alloc(0, 3, 75376, 0, 100, 0x100)
    assert create(cfg, [good]) == 0
    assert L.mi_lte_pdsch_alloc_decodable_3gpp(C.byref(cfg), C.byref(dl), C.byref(good), 1) == 1
    assert L.mi_lte_pdsch_alloc_decodable(C.byref(cfg), C.byref(good), 1) == 0
    refused = [alloc(0, 3, 6128, 0, 100, 0x100), alloc(0, 3, 75384, 0, 100, 0x100), alloc(0, 0, 6200, 0, 100, 0x100)]
    for bad in refused:
        assert create(cfg, [good, bad]) == ERR_UNSUPPORTED, bad.tbs
        assert L.mi_lte_pdsch_alloc_decodable_3gpp(C.byref(cfg), C.byref(dl), C.byref(bad), 1) == 0
    assert create(cfg2, [good]) == ERR_UNSUPPORTED
    for size in (75376, 36696, 18336, 6200, 6128, 75384):  # the reference-mode plan: unchanged
        assert create_ref([alloc(0, 3, size, 0, 100, 0x100)]) == ERR_UNSUPPORTED, size
    plan = ctx.pdsch_plan_3gpp(cfg, 1, [good], 1237248)
    assert L.mi_lte_pdsch_plan_set_decoder(plan.h, m.TURBO_REF, 8, 1) == ERR_UNSUPPORTED
    assert L.mi_lte_pdsch_plan_set_decoder(plan.h, m.TURBO_BCJR, 8, 0) == ERR_INVALID
    assert plan.out_stride >= 75376
    plan.close()


def noisy_batch():
    """100 RB: C in {1, 2, 3, 6, 13}, rv 0-3, subframes 0 and 5, K_MIMO 1 and 2, QPSK / 16QAM / 64QAM; N_soft small enough that every
    multi-block size's soft buffer is limited (N_cb < K_w); an SNR at which some blocks fail."""
    per_unit = [
        [alloc(0, 2, 18336, 0, 50, 0x101, rv=1), alloc(0, 1, 6200, 50, 50, 0x102, rv=2)],
        [alloc(1, 3, 36696, 0, 40, 0x103, rv=3), alloc(1, 2, 12216, 40, 60, 0x104, rv=0, txm=4)],
        [alloc(2, 3, 75376, 0, 90, 0x105, rv=0), alloc(2, 1, 1032, 90, 10, 0x106, rv=2)],
        [alloc(3, 1, 6200, 0, 30, 0x107, rv=1), alloc(3, 3, 18336, 30, 70, 0x108, rv=3)],
    ]
    return [0, 5, 3, 8], [17, 301, 42, 503], per_unit


def check_blocks_exact(port, ref, ref_phy, plan, allocs, res, n_soft):
    """The three stages of every allocation of a plan that ran under BCJR x 8 and BCJR_BLOCK x 6 (res, in that order) against what
    specifies them: cb_soft against the reference's rate un-matching, the output row / status / cb_ok against the plain-C models' decisions
    on those blocks + the numpy desegmentation.  Returns ([(C, K, soft buffer limited) per allocation], passes, failures)."""
    import openlte_amd as m
    n_fail = n_pass = 0
    seen = []
    for a, al in enumerate(allocs):
        e = plan.soft_bits(a)
        Qm = {1: 2, 2: 4, 3: 6}[al.mod_type]
        lay = m.dlsch_layout(al.tbs, len(e), Qm, al.tx_mode, al.rv_idx, n_soft, 8)
        nc, K = lay["C"], lay["K"]
        seen.append((nc, K, lay["N_cb"] < 96 * ((K + 4 + 31) // 32)))
        blocks = plan.cb_soft(a)
        assert blocks.shape == (nc, 3 * (K + 4))
        for r in range(nc):
            es = e[lay["off"][r]:lay["off"][r] + lay["E"][r]].astype(np.float32)
            d = np.zeros(3 * (K + 4), np.float32)
            ref.ref_rate_unmatch_turbo(ref_phy, es.copy(), lay["E"][r], K, nc, al.tx_mode, n_soft, 8, 0, al.rv_idx, d)
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
    """Every block's cb_soft equals the reference's rate un-matching (N_codeblocks = C) of the tap's soft bits [off_r, off_r + E_r), mapped
    by the decoder's rule (NULL -> 0, sums saturated to +-127); the output row, status and cb_ok equal the desegmentation + CRC24B / CRC24A
    of the plain-C models' decisions on those blocks (BCJR x 8: lo_turbo_decode_bcjr; BCJR_BLOCK x 6: lo_turbo_decode_bcjr_block)."""
    import openlte_amd as m
    n_soft = 125184
    sfs, cells, per_unit = noisy_batch()
    allocs, tx, plan, res = run_cells(ctx, 100, sfs, cells, per_unit, n_soft, 2, 11.0, seed=5 + packed,
                                      decoders=((m.TURBO_BCJR, 8), (m.TURBO_BCJR_BLOCK, 6)), packed=packed)
    seen, n_pass, n_fail = check_blocks_exact(port, ref, ref_phy, plan, allocs, res, n_soft)
    seen_c, limited = {nc for nc, K, lim in seen}, sum(lim for nc, K, lim in seen)
    assert seen_c >= {1, 2, 3, 6, 13} and limited >= 6
    assert n_pass > 0 and n_fail > 0, (n_pass, n_fail)
    plan.close()


def segment_class_batch():
    """100 RB grants whose code blocks fall in the segment classes of k_bcjr_half that noisy_batch (K = 3136, 5824: one segment; 6144:
    eight) does not reach: n_seg = 2 (9912 -> 2 x 4992, 12576 -> 3 x 4224), n_seg = 4 (10680 -> 2 x 5376, 12960 -> 3 x 4352, 17568 ->
    3 x 5888), and one-block grants whose K = tbs + 24 is a ragged n_seg = 2 size (992, 1120, 1504, 1888: K < kpad64(K), the last segment
    ends short) or the ragged n_seg = 4 one (2016).  Code rates from ~0.4 (QPSK: decodes at any SNR the test runs at) to ~1 (64QAM on
    too few PRBs: cannot decode), the rest in between; rv 0-3."""
    per_unit = [
        [alloc(0, 2, 9912, 0, 30, 0x111, rv=1), alloc(0, 3, 12576, 30, 35, 0x112, rv=0), alloc(0, 1, 1096, 65, 10, 0x113, rv=2)],
        [alloc(1, 3, 10680, 0, 30, 0x114, rv=0), alloc(1, 1, 968, 30, 6, 0x115, rv=2), alloc(1, 3, 9912, 36, 12, 0x116, rv=0)],
        [alloc(2, 2, 12960, 0, 40, 0x117, rv=3), alloc(2, 3, 17568, 40, 50, 0x118, rv=0), alloc(2, 3, 1480, 90, 2, 0x119, rv=1)],
        [alloc(3, 2, 1864, 0, 5, 0x11A, rv=1), alloc(3, 3, 1992, 5, 6, 0x11B, rv=0), alloc(3, 1, 10680, 11, 60, 0x11C, rv=3)],
    ]
    return [0, 5, 3, 8], [17, 301, 42, 503], per_unit


def test_rate_unmatch_decode_and_assembly_exact_at_the_other_segment_classes(ctx, port, ref, ref_phy):
    """test_rate_unmatch_decode_and_assembly_exact's three checks on a plan whose code blocks the batch kernels cut into 2 and 4 segments
    (full and ragged), under BCJR x 8 and BCJR_BLOCK x 6, at an SNR where some transport blocks pass and some fail.  N_soft of UE
    category 1: the three-block sizes' soft buffers are limited, the two-block ones' are not."""
    import openlte_amd as m
    port.lo_bcjr_n_seg.restype = C.c_uint32
    n_soft = 250368
    sfs, cells, per_unit = segment_class_batch()
    allocs, tx, plan, res = run_cells(ctx, 100, sfs, cells, per_unit, n_soft, 2, 11.0, seed=23,
                                      decoders=((m.TURBO_BCJR, 8), (m.TURBO_BCJR_BLOCK, 6)))
    seen, n_pass, n_fail = check_blocks_exact(port, ref, ref_phy, plan, allocs, res, n_soft)
    classes = {(int(port.lo_bcjr_n_seg(K)), nc, K % 64 != 0) for nc, K, lim in seen}  # (n_seg, C, ragged last segment)
    print("3GPP segment classes: (C, K, limited) per grant %s, status per grant %s / %s, cb_ok %s / %s"
          % (seen, list(res[0][0]), list(res[1][0]), list(res[0][2]), list(res[1][2])))
    assert classes >= {(2, 2, False), (2, 3, False), (4, 2, False), (4, 3, False), (2, 1, True), (4, 1, True)}, classes
    assert {K for nc, K, lim in seen} >= {4992, 4224, 5376, 4352, 5888, 992, 1120, 1504, 1888, 2016}
    assert any(lim for nc, K, lim in seen) and not all(lim for nc, K, lim in seen)
    assert n_pass > 0 and n_fail > 0, (n_pass, n_fail)
    plan.close()


def check_end_to_end(allocs, tx, res, n_alloc):
    for i, (st, bits, cb_ok) in enumerate(res):
        for k, al in enumerate(allocs):
            assert st[k] == 0, ("decoder #%d" % i, k, al.tbs, st[k], cb_ok[k], int((bits[k] != tx[k // n_alloc, k % n_alloc, :al.tbs]).sum()))
            assert (bits[k] == tx[k // n_alloc, k % n_alloc, :al.tbs]).all(), k
            assert cb_ok[k] == (1 << m_blocks(al.tbs)) - 1


def m_blocks(size):
    import openlte_amd as m
    return m.dlsch_layout(size, 0, 2)["C"]


@pytest.mark.parametrize("n_rb", [6, 25, 100])
def test_end_to_end_mixed_batch(ctx, n_rb):
    """30 dB, every transport block equals its transmitted bits with status 0 under BCJR x 8, BCJR_EARLY (its output is BCJR's with the
    iterations its tile pair ran, which the model comparison above does not cover: checked here end to end) and BCJR_BLOCK.  The largest
    size of the 25- and 100-RB cells, one-block sizes, several sizes in one plan, subframes 0 and 5.  The grants near code rate 1 (I_TBS 26)
    use rv 0, the one redundancy version that carries the systematic bits; the lower-rate ones cover rv 1-3."""
    import openlte_amd as m
    dec = ((m.TURBO_BCJR, 8), (m.TURBO_BCJR_EARLY, 8), (m.TURBO_BCJR_BLOCK, 8))
    if n_rb == 6:  # one-block sizes only.  Not subframes 0 / 5, where the PBCH and the sync signals take most of the band; I_TBS 25, not the
        # largest 6-RB size: I_TBS 26 is code rate 0.89 behind the two-symbol control region of a 6-RB cell and missed its CRC at 30 dB
        cfi, units = 2, [(3, 11, 3, tbs(25, 6), 0, 6, 0), (7, 250, 1, tbs(9, 6), 0, 6, 1)]
    elif n_rb == 25:  # the largest 25-RB size in subframe 5 (code rate 0.86): behind subframe 0's PBCH it is 0.92, where one of the three
        # decoders left three bit errors at 30 dB; subframe 0 carries a two-block 16QAM grant
        cfi, units = 1, [(0, 3, 2, tbs(15, 25), 0, 25, 1), (5, 77, 3, tbs(26, 25), 0, 25, 0), (2, 400, 2, tbs(15, 10), 7, 10, 1),
                         (4, 9, 1, tbs(9, 25), 0, 25, 2)]
    else:
        cfi, units = 1, [(0, 0, 3, tbs(26, 100), 0, 100, 0), (5, 123, 3, tbs(26, 50), 0, 50, 0), (1, 502, 2, tbs(15, 60), 20, 60, 2),
                         (6, 7, 1, tbs(9, 50), 50, 50, 3), (9, 8, 1, tbs(9, 38), 3, 38, 1)]
    sfs, cells = [u[0] for u in units], [u[1] for u in units]
    per_unit = [[alloc(i, mod, size, prb0, n_prb, 0x200 + i, rv=rv)] for i, (_, _, mod, size, prb0, n_prb, rv) in enumerate(units)]
    allocs, tx, plan, res = run_cells(ctx, n_rb, sfs, cells, per_unit, 1237248, cfi, 30.0, seed=n_rb, decoders=dec)
    check_end_to_end(allocs, tx, res, 1)
    assert max(m_blocks(a.tbs) for a in allocs) == {6: 1, 25: 3, 100: 13}[n_rb]
    plan.close()
