"""CPU: the host arithmetic of the PDCCH's 3GPP mode (include/mi_lte.h: "PDCCH, 3GPP mode") -- the UE-specific search spaces of 36.213 9.1.1,
the C-RNTI format 0 / 1A unpacker against a packer written here from the header's field list, and the any-DCI control-region generator
against the format-1A one it shares its body with."""
import ctypes as C

import numpy as np
import pytest

ERR_INVALID = -1
M_OF_L = {1: 6, 2: 6, 4: 2, 8: 2}


# ---- 36.213 9.1.1, restated

def y_k(rnti, sf):
    y = np.asarray(rnti, np.int64)
    for _ in range(sf + 1):
        y = (39827 * y) % 65537
    return y


def space(rnti, sf, n_cce, L):
    """the first CCEs of the RNTI's candidates, duplicates kept; [] when no candidate fits"""
    nl = n_cce // L
    if nl == 0:
        return []
    y = int(y_k(rnti, sf))
    return [L * ((y + m) % nl) for m in range(M_OF_L[L])]


def test_search_space_equals_the_recurrence():
    import openlte_amd as m
    lib = m.load_library()
    rng = np.random.default_rng(9)
    rntis = [int(r) for r in rng.integers(1, 0x10000, 200)] + [1, 0xFFFF, 0xFFF3]
    out, n = np.zeros(6, np.uint32), C.c_uint32()
    for L in (1, 2, 4, 8):
        for sf in range(10):
            y = y_k(rntis, sf)
            for n_cce in range(89):
                nl = n_cce // L
                for k, r in enumerate(rntis):
                    assert lib.mi_lte_pdcch_search_space(r, sf, n_cce, L, out, C.byref(n)) == 0
                    if nl == 0:
                        assert n.value == 0, (r, sf, n_cce, L)
                        continue
                    want = [L * ((int(y[k]) + i) % nl) for i in range(M_OF_L[L])]
                    assert out[:n.value].tolist() == want, (r, sf, n_cce, L)
    # the binding, the 1.4 MHz cell with two CCEs, and duplicates kept as the formula yields them
    assert m.pdcch_search_space(0x1234, 3, 2, 4) == [] and m.pdcch_search_space(0x1234, 3, 2, 8) == []
    assert m.pdcch_search_space(0x1234, 3, 2, 2) == [0] * 6
    assert m.pdcch_search_space(0x1234, 3, 20, 1) == space(0x1234, 3, 20, 1)


def test_search_space_refusals():
    import openlte_amd as m
    lib = m.load_library()
    out, n = np.zeros(6, np.uint32), C.c_uint32()
    for rnti, sf, n_cce, L in [(0, 0, 20, 1), (0x10000, 0, 20, 1), (5, 10, 20, 1), (5, 0, 20, 0), (5, 0, 20, 3), (5, 0, 20, 16)]:
        assert lib.mi_lte_pdcch_search_space(rnti, sf, n_cce, L, out, C.byref(n)) == ERR_INVALID, (rnti, sf, n_cce, L)
    lib.mi_lte_pdcch_search_space.argtypes = [C.c_uint32] * 4 + [C.c_void_p, C.c_void_p]
    try:
        assert lib.mi_lte_pdcch_search_space(5, 0, 20, 1, None, C.addressof(n)) == ERR_INVALID
        assert lib.mi_lte_pdcch_search_space(5, 0, 20, 1, out.ctypes.data, None) == ERR_INVALID
    finally:
        lib.mi_lte_pdcch_search_space.argtypes = [C.c_uint32] * 4 + [np.ctypeslib.ndpointer(np.uint32, flags="C_CONTIGUOUS"), C.POINTER(C.c_uint32)]
    with pytest.raises(m.MiLteError):
        m.pdcch_search_space(0, 0, 20, 1)


# ---- the C-RNTI format 0 / 1A layout, packed here from the header's field list

def riv_bits(n_rb):
    return (n_rb * (n_rb + 1) // 2 - 1).bit_length()


def riv_of(n_rb, start, length):
    """36.213 7.1.6.3 / 8.1"""
    return n_rb * (length - 1) + start if length - 1 <= n_rb // 2 else n_rb * (n_rb - length + 1) + (n_rb - 1 - start)


def pack(fields, pad):
    """[(value, width)] -> (payload, n_bits), first field in the most significant bits, `pad` zero bits behind"""
    v, n = 0, 0
    for val, w in fields:
        assert 0 <= val < (1 << w)
        v, n = (v << w) | val, n + w
    return v << pad, n + pad


def pack_1a(n_rb, start, length, mcs, harq, ndi, rv, tpc, distributed=0, pad=0):
    return pack([(1, 1), (distributed, 1), (riv_of(n_rb, start, length), riv_bits(n_rb)), (mcs, 5), (harq, 3), (ndi, 1), (rv, 2), (tpc, 2)], pad)


def pack_0(n_rb, start, length, mcs, ndi, tpc, cs, cqi, hop=0, pad=1):
    return pack([(0, 1), (hop, 1), (riv_of(n_rb, start, length), riv_bits(n_rb)), (mcs, 5), (ndi, 1), (tpc, 2), (cs, 3), (cqi, 1)], pad)


TBS_SPOT = {(0, 1): 16, (0, 2): 32, (0, 6): 152, (26, 1): 712, (9, 25): 4008, (26, 100): 75376}  # 36.213 table 7.1.7.2.1-1, [I_TBS, N_prb]


def pairs(n_rb, rng):
    every = [(s, ln) for ln in range(1, n_rb + 1) for s in range(n_rb - ln + 1)]
    if n_rb <= 25:
        return every
    return [every[i] for i in rng.choice(len(every), 2000, replace=False)]


@pytest.mark.parametrize("n_rb", [6, 25, 100])
def test_unpack_round_trip(n_rb):
    import openlte_amd as m
    rng = np.random.default_rng(n_rb)
    lib, plan_cfg = m.load_library(), m.DlCfg({6: 128, 25: 512, 100: 2048}[n_rb], n_rb, 1, 0)
    cases = [(s, ln, int(rng.integers(0, 32))) for s, ln in pairs(n_rb, rng)]
    cases += [(s, ln, mcs) for mcs in range(32) for s, ln in [(0, 1), (n_rb - 1, 1), (0, n_rb), (1, n_rb // 2 + 1), (n_rb // 3, n_rb // 2)]]  # every MCS
    layouts = {}
    for s, ln, mcs in cases:
        harq, ndi, rv, tpc, cs, cqi = (int(x) for x in rng.integers(0, [8, 2, 4, 4, 8, 2]))
        rnti, n_ant = int(rng.integers(0x3D, 0xFFF4)), int(rng.choice([1, 2, 4]))
        # format 1A
        payload, n_bits = pack_1a(n_rb, s, ln, mcs, harq, ndi, rv, tpc, pad=int(rng.integers(0, 3)))
        rc, d = m.dci_0_1a_unpack_crnti(payload, n_bits, rnti, n_rb, n_ant)
        assert (d.format, d.flag, d.riv, d.rb_start, d.N_prb) == (1, 0, riv_of(n_rb, s, ln), s, ln), (s, ln, mcs)
        assert (d.mcs, d.harq, d.ndi, d.rv, d.tpc) == (mcs, harq, ndi, rv, tpc)
        assert rc == (4 if mcs >= 29 else 0)
        assert d.alloc.rnti == rnti and d.alloc.N_prb == ln
        assert list(d.alloc.prb[0][:ln]) == list(range(s, s + ln)) == list(d.alloc.prb[1][:ln])
        if rc == 0:
            i_tbs = mcs if mcs <= 9 else mcs - 1 if mcs <= 16 else mcs - 2
            assert d.alloc.mod_type == (1 if mcs <= 9 else 2 if mcs <= 16 else 3)
            assert (d.alloc.rv_idx, d.alloc.tx_mode, d.alloc.unit, d.alloc.n_pdcch_symbs) == (rv, 1 if n_ant == 1 else 2, 0, 0)
            assert d.alloc.tbs > 0 and d.alloc.tbs % 8 == 0
            if (i_tbs, ln) in TBS_SPOT:
                assert d.alloc.tbs == TBS_SPOT[(i_tbs, ln)]
            if n_ant == 1:  # (the 3GPP PDSCH plans are single-port) the allocation is one mi_lte_pdsch_plan_create_3gpp accepts as it is
                assert lib.mi_lte_pdsch_alloc_decodable_3gpp(C.byref(plan_cfg), C.byref(m.DlschCfg(1237248, 8)), C.byref(d.alloc), 2) == 1, (s, ln, mcs)
            key = (i_tbs, ln)
            if key not in layouts:  # the size is one of the table's: the 3GPP transport-block layout takes it
                layouts[key] = m.dlsch_layout(d.alloc.tbs, 0, 2 * d.alloc.mod_type, tx_mode=d.alloc.tx_mode)
                assert layouts[key]["C"] * layouts[key]["K"] >= d.alloc.tbs + 24
        else:
            assert d.alloc.tbs == 0
        # format 0
        payload, n_bits = pack_0(n_rb, s, ln, mcs, ndi, tpc, cs, cqi, hop=harq & 1, pad=1 + int(rng.integers(0, 2)))
        rc, d = m.dci_0_1a_unpack_crnti(payload, n_bits, rnti, n_rb, n_ant)
        assert (d.format, d.flag, d.riv, d.rb_start, d.N_prb) == (0, harq & 1, riv_of(n_rb, s, ln), s, ln), (s, ln, mcs)
        assert (d.mcs, d.ndi, d.tpc, d.cyclic_shift, d.cqi_request) == (mcs, ndi, tpc, cs, cqi)
        assert rc == (4 if mcs >= 29 else 0)
        assert d.alloc.rnti == rnti and d.alloc.N_prb == ln and list(d.alloc.prb[0][:ln]) == list(range(s, s + ln))


def test_unpack_both_riv_branches_are_covered():
    """The pairs of the round trip reach both branches of the RIV rule at every bandwidth, and every RIV below N (N + 1) / 2 is some pair's."""
    for n_rb in (6, 25):
        rivs = {riv_of(n_rb, s, ln) for ln in range(1, n_rb + 1) for s in range(n_rb - ln + 1)}
        assert rivs == set(range(n_rb * (n_rb + 1) // 2))
        assert any(ln - 1 > n_rb // 2 for ln in range(1, n_rb + 1))


def test_unpack_what_has_no_transport_block_and_refusals():
    import openlte_amd as m
    lib = m.load_library()
    # a distributed assignment: the fields come back, no PRB list, 4
    payload, n_bits = pack_1a(25, 3, 4, 7, 1, 1, 2, 3, distributed=1)
    rc, d = m.dci_0_1a_unpack_crnti(payload, n_bits, 0x4321, 25, 2)
    assert rc == 4 and (d.format, d.flag, d.rb_start, d.N_prb, d.mcs, d.rv) == (1, 1, 3, 4, 7, 2) and d.alloc.N_prb == 0 and d.alloc.tbs == 0
    # a RIV past the last pair's
    payload, n_bits = pack([(1, 1), (0, 1), (21, 5), (0, 5), (0, 3), (0, 1), (0, 2), (0, 2)], 0)
    rc, d = m.dci_0_1a_unpack_crnti(payload, n_bits, 0x4321, 6, 1)
    assert rc == 4 and d.riv == 21 and d.N_prb == 0 and d.alloc.N_prb == 0
    good, n_good = pack_1a(25, 3, 4, 7, 1, 1, 2, 3)
    out = m.DciCrnti()
    for payload, n_bits, rnti, n_rb, n_ant in [(good, n_good, 0, 25, 1), (good, n_good, 0x10000, 25, 1), (good, n_good, 5, 0, 1), (good, n_good, 5, 111, 1),
                                               (good, n_good, 5, 25, 3), (good, 12, 5, 25, 1), (good, 65, 5, 25, 1), (good, 0, 5, 25, 1)]:
        assert lib.mi_lte_dci_0_1a_unpack_crnti(payload, n_bits, rnti, n_rb, n_ant, C.byref(out)) == ERR_INVALID, (n_bits, rnti, n_rb, n_ant)
    assert lib.mi_lte_dci_0_1a_unpack_crnti(good, n_good, 5, 25, 1, None) == ERR_INVALID


# ---- the any-DCI generator against the format-1A one

DCI_1A_BITS = {6: 21, 15: 22, 25: 25, 50: 27, 75: 27, 100: 28}


@pytest.mark.parametrize("n_ant", [1, 2, 4])
@pytest.mark.parametrize("fft,n_rb", [(128, 6), (512, 25)])
def test_synth_records_equal_the_format_1a_generator(fft, n_rb, n_ant):
    import openlte_amd as m
    from openlte_amd import synth
    rng = np.random.default_rng(fft + n_ant)
    n = 6
    cfg = m.DlCfg(fft, n_rb, n_ant, 0)
    sfs, cells, cfis = rng.integers(0, 10, n), rng.integers(0, 504, n), rng.integers(1, 4, n)
    size = DCI_1A_BITS[n_rb]
    dcis, recs = [], []
    for u in range(n):
        n_symbs = int(cfis[u]) + (1 if n_rb <= 10 else 0)
        n_cce = m.load_library().mi_lte_get_n_cce(n_rb, int(np.ceil(n_rb / 8.0)), n_symbs, n_ant)
        lst, rl = [], []
        for a in range(int(rng.integers(0, 5))):
            if rng.random() < 0.25:
                lst.append((0, 0, 0, 0, 0))  # an unused slot
                continue
            n_prb = int(rng.integers(1, n_rb // 2 + 2))
            t = (int(rng.choice([0xFFFF, 0xFFFE, 7, 0x3C])), int(rng.integers(0, 27)), n_prb, int(rng.integers(0, n_rb - n_prb + 1)), int(rng.integers(0, 4)))
            lst.append(t)
            if 4 * a + 4 <= n_cce:  # (the format-1A generator sends nothing on a candidate without all its CCEs)
                payload, n_bits = pack([(1, 1), (0, 1), (n_rb * (t[2] - 1) + t[3], riv_bits(n_rb)), (t[1], 5), (0, 3), (0, 1), (t[4], 2), (1, 2)], 0)
                rl.append((t[0], 4, 4 * a, size, payload << (size - n_bits)))
        dcis.append(lst)
        recs.append(rl)
    want = synth.ctrl_grids(cfg, sfs, cells, cfis, dcis, snr_db=9.0, seed=fft + n_ant)
    got = synth.ctrl_grids_dci(cfg, sfs, cells, cfis, recs, snr_db=9.0, seed=fft + n_ant)
    assert sum(len(r) for r in recs) > 0
    assert want.tobytes() == got.tobytes()


def test_synth_records_refusals():
    import openlte_amd as m
    from openlte_amd import synth
    cfg = m.DlCfg(512, 25, 2, 0)
    lib = m.load_library()
    n_cce = lib.mi_lte_get_n_cce(25, 4, 3, 2)
    assert n_cce == 20
    ok = [(0x100, 4, 4, 27, 5), (0x101, 2, 8, 27, 6), (0x102, 1, 19, 41, 7), (0x103, 8, 8 + 8 * 0, 41, 1)]
    with pytest.raises(m.MiLteError):  # the L = 8 record lies over the L = 2 one
        synth.ctrl_grids_dci(cfg, [0], [7], [3], [ok])
    synth.ctrl_grids_dci(cfg, [0], [7], [3], [ok[:3]])
    for bad in [(0x100, 4, 20, 27, 5), (0x100, 8, 16, 27, 5), (0x100, 1, 20, 27, 5),      # past the last CCE
                (0x100, 3, 0, 27, 5), (0x100, 4, 2, 27, 5), (0x10000, 4, 0, 27, 5), (0x100, 4, 0, 0, 5), (0x100, 4, 0, 65, 5)]:
        with pytest.raises(m.MiLteError):
            synth.ctrl_grids_dci(cfg, [0], [7], [3], [[bad]])
    with pytest.raises(m.MiLteError):  # two records on one CCE
        synth.ctrl_grids_dci(cfg, [0], [7], [3], [[(0x100, 1, 5, 27, 5), (0x101, 1, 5, 27, 5)]])
    with pytest.raises(m.MiLteError):  # CFI 1: 3 CCEs only
        synth.ctrl_grids_dci(cfg, [0], [7], [1], [[(0x100, 4, 0, 27, 5)]])
    with pytest.raises(m.MiLteError):  # more records per unit than the generator takes
        synth.ctrl_grids_dci(cfg, [0], [7], [3], [[(0x100 + i, 1, i, 27, 5) for i in range(9)]])
