"""CPU: the float64 model of the PDCCH search's control-region de-mapper (pdcch_ctrl_model) on its own and against the library's host
tables -- what test_pdcch_ctrl_model_gpu then holds k_pdcch_search_demod to.  No GPU."""
import numpy as np
import pytest

import pdcch_ctrl_cases as pc
import pdcch_ctrl_model as pm

CAP_SHARE = 0.01  # of a case's bits may be close calls (a condition on the inputs)
CASE_IDX = list(range(len(pc.CASES)))


def n_bits_of(refs):
    return sum(len(r["soft"]) for r in refs)


# ---- the model alone

@pytest.mark.parametrize("i", CASE_IDX, ids=pc.IDS)
def test_model_round_trip_without_noise(i):
    """modulator -> float64 decoder: the CFI and every bit of every CCE come back, no magnitude below 64 (the condition the clean batches'
    channel seeds were chosen for)"""
    _, bits = pc.batch(i, "clean")
    for u, r in enumerate(pc.reference(i, "clean")):
        cell, sf, cfi = pc.ALL[i][3][u]
        assert r["cfi"] == cfi and r["n_cce"] == len(bits[u])
        assert (r["pcfich"]["soft"] < 0).tolist() == pm.CFI_WORDS[cfi - 1].astype(bool).tolist() and np.abs(r["pcfich"]["soft"]).min() >= 64
        assert (np.sign(r["soft"]) == 1 - 2 * bits[u].reshape(-1).astype(np.int64)).all()
        assert len(r["soft"]) == 0 or np.abs(r["soft"]).min() >= 64


@pytest.mark.parametrize("i", pc.IDX_36211, ids=pc.IDS_36211)
def test_model_round_trip_with_the_numbering_of_36211(i):
    """the cases for MI_LTE_PDCCH_SEARCH_36211_REGS: the round trip holds, and the default tables put these cells' CCEs elsewhere"""
    n_rb, n_ant, n_g, units = pc.ALL[i]
    _, bits = pc.batch(i, "clean", "36.211")
    n_other = 0
    for u, r in enumerate(pc.reference(i, "clean", numbering="36.211")):
        cell, sf, cfi = units[u]
        assert r["cfi"] == cfi and r["n_cce"] == len(bits[u]) > 0
        assert (np.sign(r["soft"]) == 1 - 2 * bits[u].reshape(-1).astype(np.int64)).all()
        a, b = (pm.geometry(n_rb, n_ant, cell, pm.N_G[n_g], pc.n_symbs(n_rb, cfi), nb) for nb in ("library", "36.211"))
        n_other += a[0] != b[0] or bool((a[1] != b[1]).any())
    assert n_other >= len(units) - 1


def test_dci_encoder_round_trip():
    """the DCI encoder against the independent decoder pieces of the CQI tests: un-matching, three-lap Viterbi, CRC16 syndrome = RNTI"""
    from test_pdcch_search_gpu import crc16_syndrome
    from test_ulsch_cqi_cpu import unmatch, viterbi3
    for rnti, L, n_bits, payload in [(0x1234, 1, 27, 0x5A5A5A5), (0xFFFF, 4, 41, 0x123456789A), (1, 8, 64, (1 << 64) - 3), (0x8001, 2, 8, 0x81)]:
        e = pm.dci_encode(payload, n_bits, rnti, L)
        assert e.shape == (72 * L,)
        c = viterbi3(unmatch(127 * (1 - 2 * e.astype(np.int64)), n_bits + 16)[None, :])
        assert int(crc16_syndrome(c, n_bits)[0]) == rnti
        assert sum(int(b) << (n_bits - 1 - k) for k, b in enumerate(c[0, :n_bits])) == payload


# ---- the tables against the library

def legal_n_symbs(n_rb):
    return (2, 3, 4) if n_rb <= 10 else (1, 2, 3, 4)


@pytest.mark.parametrize("n_rb", [6, 15, 25, 50, 75, 100])
def test_tables_equal_the_library(n_rb):
    """every cell, port count, N_g and region size: the PCFICH's elements, CCEs 0 .. 15 as the six candidates (with the same ones incomplete)
    and N_cce"""
    import openlte_amd as m
    lib = m.load_library()
    for n_ant in (1, 2, 4):
        for g in pm.N_G.values():
            for ns in legal_n_symbs(n_rb):
                for cell in range(504):
                    n_cce, cce_re, pc_re = pm.geometry(n_rb, n_ant, cell, g, ns)
                    l_pc, l_cand = m.pdcch_re_tables(n_rb, n_ant, cell, float(g), ns)
                    assert (l_pc == pc_re).all(), (n_ant, g, ns, cell)
                    assert (l_cand == pm.candidate_table(n_cce, cce_re)).all(), (n_ant, g, ns, cell)
                    if n_cce or not (n_ant == 4 and ns == 1):  # (where the formula's N_reg is negative the reference's unsigned count is not a count)
                        assert lib.mi_lte_get_n_cce(n_rb, pm.n_group(n_rb, g), ns, n_ant) == n_cce, (n_ant, g, ns, cell)
                    # every CCE, as a search plan holds them: the default tables and those of MI_LTE_PDCCH_SEARCH_36211_REGS
                    l_n, l_re = m.pdcch_cce_tables(n_rb, n_ant, cell, float(g), ns)
                    assert l_n == n_cce and (l_re == cce_re).all(), (n_ant, g, ns, cell)
                    n_cce, cce_re, _ = pm.geometry(n_rb, n_ant, cell, g, ns, "36.211")
                    l_n, l_re = m.pdcch_cce_tables(n_rb, n_ant, cell, float(g), ns, regs_36211=True)
                    assert l_n == n_cce and (l_re == cce_re).all(), (n_ant, g, ns, cell)


def test_cce_tables_refusals():
    import ctypes as C
    import openlte_amd as m
    lib = m.load_library()
    n, out = C.c_uint32(), np.zeros(36 * 128, np.uint32)
    assert lib.mi_lte_pdcch_cce_tables(25, 2, 7, 1.0, 3, m.PDCCH_SEARCH_36211_REGS, C.byref(n), out, 128) == 0 and n.value == 20
    assert lib.mi_lte_pdcch_cce_tables(25, 2, 7, 1.0, 3, 0, C.byref(n), out[:36], 1) == 0 and n.value == 20  # (n_max cuts the copy, not the count)
    for args in [(26, 2, 7, 1.0, 3, 0), (25, 3, 7, 1.0, 3, 0), (25, 2, 504, 1.0, 3, 0), (25, 2, 7, 0.0, 3, 0), (25, 2, 7, 2.5, 3, 0), (25, 2, 7, 1.0, 0, 0),
                 (25, 2, 7, 1.0, 5, 0), (25, 2, 7, 1.0, 3, 1), (25, 2, 7, 1.0, 3, 4)]:
        assert lib.mi_lte_pdcch_cce_tables(*args, C.byref(n), out, 128) == -1, args
    assert lib.mi_lte_pdcch_cce_tables(25, 2, 7, 1.0, 3, 0, None, out, 128) == -1


@pytest.mark.parametrize("n_rb", [6, 25, 100])
def test_where_the_library_numbering_departs_from_36211(n_rb):
    """The library's numbering is 36.211's except in the two respects the header names: a PHICH group numbered past a PCFICH group that wrapped
    round the band's edge, and N_reg with four ports and a one-symbol region.  Everywhere else the two geometries are the same tables."""
    n_dep = 0
    for n_ant in (1, 2, 4):
        for g in pm.N_G.values():
            for ns in legal_n_symbs(n_rb):
                for cell in range(0, 504, 5):
                    same_phich = sorted(pm.phich_regs(n_rb, cell, g, "library")) == sorted(pm.phich_regs(n_rb, cell, g, "36.211"))
                    a, b = pm.geometry(n_rb, n_ant, cell, g, ns), pm.geometry(n_rb, n_ant, cell, g, ns, numbering="36.211")
                    same = a[0] == b[0] and (a[1] == b[1]).all()
                    if same_phich and not (n_ant == 4 and ns == 1):
                        assert same, (n_ant, g, ns, cell)
                    n_dep += not same
                    regs = pm.phich_regs(n_rb, cell, g, "36.211")  # 6.9.3 itself never puts a PHICH group on a PCFICH group or on another's
                    assert len(set(regs)) == len(regs) and not set(regs) & set(pm.pcfich_regs(n_rb, cell))
    assert n_dep > 0


# ---- float32 against float64, and what the comparison can resolve

def test_the_deltas_are_eight_times_the_measured_gap():
    gv, gx = (max(a, b) for a, b in zip(pm.measure_f32_gap(pc.all_subframes("noisy")), pm.measure_f32_gap(pc.all_subframes("low"))))
    print("largest |v32 - v64| %.3e, largest |x32 - x64| / |x| %.3e" % (gv, gx))
    assert 0.98 * pm.MEASURED_V <= gv <= 1.0001 * pm.MEASURED_V and 0.98 * pm.MEASURED_X <= gx <= 1.0001 * pm.MEASURED_X
    assert pm.DELTA_V == 8 * pm.MEASURED_V and pm.DELTA_X == 8 * pm.MEASURED_X


@pytest.mark.parametrize("kind", ["noisy", "low"])
@pytest.mark.parametrize("i", CASE_IDX, ids=pc.IDS)
def test_cap_holds_for_float32_numpy(i, kind):
    """the header's formula in numpy float32 against float64: equal but for close calls, which stay under the cap; the PCFICH decision equal"""
    want, got = pc.reference(i, kind), pc.reference(i, kind, None, True)
    n_close = 0
    for w, g in zip(want, got):
        assert g["cfi"] == w["cfi"] and g["n_cce"] == w["n_cce"]
        if w["n_cce"]:
            nc, bad = pm.compare(g["soft"], w)
            n_close += nc
            assert len(bad) == 0, bad[:8]
    assert n_close <= CAP_SHARE * n_bits_of(want)
    if kind == "noisy":
        assert sum(int((~w["sat"]).sum()) for w in want if w["n_cce"]) >= 0.5 * n_bits_of(want)


def applies(variant, i):
    n_rb, n_ant, _, units = pc.CASES[i]
    if variant == "swap4":
        return n_ant == 4
    if variant in ("own_est", "norm2"):
        return n_ant > 1
    if variant == "freq_first":
        return any(pc.n_symbs(n_rb, cfi) > 1 for _, _, cfi in units)
    return True


@pytest.mark.parametrize("variant", pm.VARIANTS)
def test_each_wrong_variant_is_resolved(variant):
    """swapped in for the right decoder, every wrong variant fails the comparison of the soft-value test in every case it applies to: it
    differs from the float64 decoder by more than a close call allows on more bits than the cap admits close calls"""
    n_cases = 0
    for i in CASE_IDX:
        if not applies(variant, i):
            continue
        want, wrong = pc.reference(i, "noisy"), pc.reference(i, "noisy", variant)
        n_bad = 0
        for w, g in zip(want, wrong):
            if not w["n_cce"]:
                continue
            n_bad += len(pm.compare(g["soft"], w)[1]) if g["n_cce"] == w["n_cce"] else len(w["soft"])
        assert n_bad > CAP_SHARE * n_bits_of(want), (variant, pc.IDS[i], n_bad, n_bits_of(want))
        n_cases += 1
    assert n_cases >= 5
