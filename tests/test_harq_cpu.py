"""CPU: the host side of HARQ soft combining in the 3GPP transport-block mode.  The payload transmitter
(mi_lte_synth_dl_units_3gpp_payload_i8) against the seeded generator it extends, and the pool's buffer size (mi_lte_harq_buffer_bytes)
against 36.212 segmentation restated in numpy.  No GPU."""
import ctypes as C

import numpy as np
import pytest

from test_dlsch3gpp_cpu import all_tbs, seg, tbs_table

ERR_INVALID = -1
FFT = {6: 128, 15: 256, 25: 512, 50: 1024, 100: 2048}


def alloc(mod, size, prb0, n_prb, rnti, rv=0, txm=1):
    import openlte_amd as m
    return m.make_alloc(0, mod, size, list(range(prb0, prb0 + n_prb)), rnti, rv_idx=rv, tx_mode=txm)


def tbs(itbs, n_prb):
    return int(tbs_table()[itbs][n_prb - 1])


# (N_rb, [(subframe, cell)], per unit: [(mod, I_TBS, prb0, N_prb, rv, tx_mode)]): C = 1 .. 13 over the cases, rv 0 .. 3 in each
CASES = [
    (6, [(3, 11), (7, 250)], [[(1, 9, 0, 6, 0, 1)], [(2, 15, 0, 6, 3, 1)]]),
    (25, [(0, 3), (5, 77), (2, 400)], [[(2, 15, 0, 25, 1, 1)], [(3, 26, 0, 25, 2, 4)], [(2, 15, 7, 10, 3, 1)]]),
    (100, [(0, 0), (5, 123), (1, 502), (6, 7)], [[(3, 26, 0, 100, 0, 1)], [(3, 26, 0, 50, 1, 1)], [(2, 15, 20, 60, 2, 4)], [(1, 9, 50, 50, 3, 1)]]),
    (50, [(9, 8), (4, 33)], [[(3, 20, 0, 30, 2, 1), (1, 5, 30, 20, 1, 1)], [(3, 24, 0, 48, 0, 1), (1, 9, 48, 2, 3, 1)]]),
]


def build_case(n_rb, units, per_unit):
    return [[alloc(mod, tbs(itbs, n_prb), prb0, n_prb, 0x300 + 10 * u + k, rv=rv, txm=txm)
             for k, (mod, itbs, prb0, n_prb, rv, txm) in enumerate(specs)] for u, specs in enumerate(per_unit)]


@pytest.mark.parametrize("case", range(len(CASES)))
def test_payload_transmitter_matches_generator(case):
    """Given the bits the seeded generator drew, the payload transmitter writes the generator's IQ byte for byte; another payload changes it."""
    import openlte_amd as m
    from openlte_amd import synth
    n_rb, units, per_unit = CASES[case]
    allocs2d = build_case(n_rb, units, per_unit)
    allocs = [a for row in allocs2d for a in row]
    n_alloc = len(allocs2d[0])
    cfg = m.DlCfg(FFT[n_rb], n_rb, 1, 0)
    sfs, cells = [u[0] for u in units], [u[1] for u in units]
    n_soft = 125184 if case % 2 else 1237248
    iq, tx = synth.dl_units_3gpp(cfg, sfs, cells, allocs, n_alloc, n_soft, snr_db=20.0, seed=31 + case)
    iq2, tx2 = synth.dl_units_3gpp(cfg, sfs, cells, allocs, n_alloc, n_soft, snr_db=20.0, seed=31 + case, payload=tx)
    assert (iq2 == iq).all()
    assert (tx2 == tx).all()
    flipped = tx.copy()
    flipped[0, 0, 0] ^= 1
    iq3, _ = synth.dl_units_3gpp(cfg, sfs, cells, allocs, n_alloc, n_soft, snr_db=20.0, seed=31 + case, payload=flipped)
    assert (iq3 != iq).any()
    # a retransmission: the same payload with another rv and another seed differs from the first transmission
    allocs_rv = [alloc(a.mod_type, a.tbs, a.prb[0][0], a.N_prb, a.rnti, rv=(a.rv_idx + 2) % 4, txm=a.tx_mode) for a in allocs]
    iq4, _ = synth.dl_units_3gpp(cfg, sfs, cells, allocs_rv, n_alloc, n_soft, snr_db=20.0, seed=32 + case, payload=tx)
    assert (iq4 != iq).any()


def test_payload_cases_cover_sizes_and_rvs():
    """The cases above cover C = 1, 2, 3, 6 (or more) and 13, and every rv."""
    import openlte_amd as m
    cs, rvs = set(), set()
    for n_rb, units, per_unit in CASES:
        for row in build_case(n_rb, units, per_unit):
            for a in row:
                cs.add(m.dlsch_layout(a.tbs, 0, 2)["C"])
                rvs.add(a.rv_idx)
    assert {1, 2, 3, 13} <= cs and max(cs) == 13 and len(cs) >= 5, cs
    assert rvs == {0, 1, 2, 3}


def test_payload_transmitter_refusals():
    """NULL payload, a tbs past the payload stride, and the generator's own refusals (two ports, a tbs outside the 3GPP mode)."""
    import openlte_amd as m
    from openlte_amd import synth
    L = synth._lib()
    cfg, cfg2 = m.DlCfg(512, 25, 1, 0), m.DlCfg(512, 25, 2, 0)
    dl = m.DlschCfg(1237248, 8)
    ch = synth.SynthChannel(0.5, 1.5, 4.0, 30.0, 100.0, 1)
    iq = np.zeros((1, synth.unit_len(512), 2), np.int8)
    sf, cell = np.zeros(1, np.uint32), np.full(1, 7, np.uint32)

    def call(c, allocs, payload, stride, dlsch=dl):
        arr = (m.PdschAlloc * len(allocs))(*allocs)
        return L.mi_lte_synth_dl_units_3gpp_payload_i8(C.byref(c), 1, sf, cell, 2, C.cast(arr, C.c_void_p), len(allocs),
                                                        None if dlsch is None else C.byref(dlsch), C.byref(ch),
                                                        None if payload is None else payload.ctypes.data, stride, iq)

    size = tbs(15, 25)
    good = alloc(2, size, 0, 25, 0x101)
    pay = np.zeros(size, np.uint8)
    assert call(cfg, [good], pay, size) == 0
    assert call(cfg, [good], None, size) == ERR_INVALID
    assert call(cfg, [good], pay, size - 8) == ERR_INVALID
    assert call(cfg, [good], pay, size, dlsch=None) == ERR_INVALID
    assert call(cfg2, [good], pay, size) == ERR_INVALID
    bad = alloc(2, 6128, 0, 25, 0x101)  # F != 0: outside the 3GPP mode
    assert call(cfg, [bad], np.zeros(6128, np.uint8), 6128) == ERR_INVALID
    with pytest.raises(ValueError):
        synth.dl_units_3gpp(cfg, [0], [7], [good], 1, 1237248, payload=np.zeros((2, 1, size), np.uint8))


def test_harq_buffer_bytes_matches_numpy():
    """mi_lte_harq_buffer_bytes(max_tbs) = 2 * the largest C * 3 (K + 4) over the table's sizes <= max_tbs, for every size of the table as
    max_tbs, the values between them and past the end; 0 below the smallest size."""
    import openlte_amd as m
    sizes = all_tbs()
    foot = np.array([seg(t)[0] * 3 * (seg(t)[1] + 4) for t in sizes], np.int64)
    run_max = np.maximum.accumulate(foot)
    for i, t in enumerate(sizes):
        assert m.harq_buffer_bytes(t) == 2 * run_max[i], t
        assert m.harq_buffer_bytes(t + 1) == 2 * run_max[i], t
        if i > 0:
            assert m.harq_buffer_bytes(t - 1) == 2 * run_max[i - 1], t
    assert m.harq_buffer_bytes(0) == 0 and m.harq_buffer_bytes(sizes[0] - 1) == 0
    assert m.harq_buffer_bytes(0xFFFFFFFF) == 2 * run_max[-1] == 2 * 13 * 3 * (5824 + 4)
