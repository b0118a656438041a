"""CPU: the host arithmetic of the PUSCH plans' 3GPP transport-block mode.  mi_lte_ulsch_layout against mi_lte_dlsch_layout with a soft
buffer no block reaches and against a restatement of 36.212 5.2.2.5 (N_cb = K_w); its transmitter mi_lte_ulsch_encode_3gpp block by block
against the compiled reference's CRC, turbo encoder and rate matcher run as channel type ULSCH with N_codeblocks = C; and the unit
generator's two forms against each other where they must coincide.  No GPU."""
import numpy as np
import pytest

import lte_testdata as td
from test_dlsch3gpp_cpu import all_tbs, crc, crc24b, seg, tbs_table, turbo_encode_exact

CHAN_ULSCH = 2  # LIBLTE_PHY_CHAN_TYPE_ULSCH
BIG_N_SOFT = 0xFFFFFFFF  # with M_dl_harq = 1: N_IR / 13 is far above the largest K_w (18 528)


def layout_ul_py(tbs, G, Qm, rv):
    """36.212 5.2.2.3-5.2.2.5: the segmentation of 5.1.2, N_cb = K_w, E_r of 5.1.4.1.2 with N_L = 1."""
    C, K, B, Bp = seg(tbs)
    R = -(-(K + 4) // 32)
    K_w = 96 * R
    k0 = R * (2 * -(-K_w // (8 * R)) * rv + 2)
    Gp = G // Qm
    gam = Gp % C
    E = [Qm * (Gp // C) if r <= C - gam - 1 else Qm * -(-Gp // C) for r in range(C)]
    return {"C": C, "K": K, "B": B, "N_cb": K_w, "k0": k0, "E": E, "off": [sum(E[:r]) for r in range(C)]}


def test_layout_vs_dlsch_layout_and_36212():
    """Every size of Table 7.1.7.2.1-1 x Q_m 2/4/6 x rv 0-3 at the G of a few PRB counts (G = 12 * 12 N_prb * Q_m, N_prb one the transform
    pre-decoder has a plan for): mi_lte_ulsch_layout = mi_lte_dlsch_layout with an unlimited buffer = the restatement."""
    from openlte_amd import dlsch_layout, ulsch_layout
    sizes = all_tbs()
    assert len(sizes) == 178
    n = 0
    for i, tbs in enumerate(sizes):
        for Qm in (2, 4, 6):
            for rv in range(4):
                for prb in (2, 24, (3, 20, 45, 99)[(i + rv) % 4]):
                    G = 12 * 12 * prb * Qm
                    got = ulsch_layout(tbs, G, Qm, rv)
                    assert got == dlsch_layout(tbs, G, Qm, 1, rv, BIG_N_SOFT, 1), (tbs, G, Qm, rv)
                    assert got == layout_ul_py(tbs, G, Qm, rv), (tbs, G, Qm, rv)
                    assert sum(got["E"]) == G and got["N_cb"] == 96 * ((got["K"] + 4 + 31) // 32)
                    n += 1
    assert n == 178 * 12 * 3


def test_layout_known_answers_and_refusals():
    from openlte_amd import ulsch_layout, MiLteError
    t = tbs_table()
    for (itbs, prb), tbs, C, K in (((15, 20), 6200, 2, 3136), ((15, 24), 7224, 2, 3648), ((26, 24), 17568, 3, 5888), ((26, 99), 73712, 13, 5696)):
        assert int(t[itbs][prb - 1]) == tbs
        lay = ulsch_layout(tbs, 12 * 12 * prb * 6, 6)
        assert (lay["C"], lay["K"], lay["B"]) == (C, K, tbs + 24), tbs
    for tbs in (6128, 100, 75384, 0):  # filler bits, past the table, empty
        with pytest.raises(MiLteError) as e:
            ulsch_layout(tbs, 1200, 2)
        assert e.value.args[1] == -4, tbs
    for args in ((6200, 1201, 2), (6200, 1200, 3), (6200, 1200, 2, 4)):  # G not a multiple of Q_m, Q_m 3, rv 4
        with pytest.raises(MiLteError) as e:
            ulsch_layout(*args)
        assert e.value.args[1] == -1


ENCODE_CASES = [(c, rv) for c in ((3240, 6, 12), (6200, 4, 20), (7224, 2, 24), (17568, 6, 24), (73712, 6, 99)) for rv in range(4)]


@pytest.mark.parametrize("case,rv", ENCODE_CASES)
def test_encode_vs_reference_block_by_block(ref, ref_phy, case, rv):
    """C in {1, 2, 3, 13} x rv 0-3: CRC24A against the reference's calc_crc, every block's turbo code against its turbo_encode (where it
    evaluates the interleaver without overflow) and its E_r bits against liblte_phy_rate_match_turbo with ULSCH and N_codeblocks = C."""
    from openlte_amd import ulsch_layout, synth
    tbs, Qm, prb = case
    rng = np.random.default_rng(tbs + rv)
    G = 12 * 12 * prb * Qm
    bits = rng.integers(0, 2, tbs).astype(np.uint8)
    e = synth.ulsch_encode_3gpp(bits, G, Qm, rv)
    lay = ulsch_layout(tbs, G, Qm, rv)
    C, K = lay["C"], lay["K"]
    assert C == {3240: 1, 6200: 2, 7224: 2, 17568: 3, 73712: 13}[tbs]
    p = np.zeros(24, np.uint8)
    ref.ref_calc_crc24a(bits.copy(), tbs, p)
    assert (p == crc(bits, 0x1864CFB)).all()
    b = np.concatenate([bits, p])
    nb = K if C == 1 else K - 24
    for r in range(C):
        c = b[r * nb:(r + 1) * nb]
        if C > 1:
            c = np.concatenate([c, crc24b(c)])
        assert len(c) == K
        d = turbo_encode_exact(c, K)
        if K not in td.OVERFLOW_K:
            d_ref = np.zeros(3 * (K + 4), np.uint8)
            assert ref.ref_turbo_encode(ref_phy, c.copy(), K, d_ref) == 3 * (K + 4)
            assert (d_ref == d).all(), (tbs, r)
        want = np.zeros(lay["E"][r], np.uint8)
        ref.ref_rate_match_turbo(ref_phy, d.copy(), 3 * (K + 4), C, 1, 1, 1, CHAN_ULSCH, rv, lay["E"][r], want)
        got = e[lay["off"][r]:lay["off"][r] + lay["E"][r]]
        assert (got == want).all(), (tbs, r)


def test_units_3gpp_equal_the_reference_mode_generator_on_a_single_block():
    """One code block whose tbs + 24 is a turbo size the reference interleaves without overflow: the two generators differ in nothing, so
    with one seed they write the same IQ and the same bits; and the 3GPP one accepts what the other refuses."""
    import openlte_amd as m
    from openlte_amd import synth
    cfg, ul = m.DlCfg(512, 25, 1, 0), m.UlCfg(3, 0, 0, 2, 1)
    sizes = [(1, 1096, 6, 0), (2, 2664, 8, 1), (3, 3240, 10, 2)]  # K = 1120, 2688, 3264
    assert all(t + 24 in td.ALL_K and t + 24 not in td.OVERFLOW_K for _, t, _, _ in sizes)
    allocs = [m.make_alloc(u, mod, tbs, list(range(3 * u, 3 * u + n_prb)), 0x40 + u, rv_idx=rv) for u, (mod, tbs, n_prb, rv) in enumerate(sizes)]
    sfs, cells = [1, 4, 8], [21, 21, 21]
    iq_a, tx_a = synth.ul_units(cfg, ul, sfs, cells, allocs, 1, snr_db=12.0, seed=9)
    iq_b, tx_b = synth.ul_units_3gpp(cfg, ul, sfs, cells, allocs, 1, snr_db=12.0, seed=9)
    assert iq_a.any() and (iq_a == iq_b).all() and (tx_a == tx_b).all()
    two = [m.make_alloc(0, 2, 6200, list(range(20)), 0x50)]
    with pytest.raises(m.MiLteError):
        synth.ul_units(cfg, ul, [0], [21], two, 1)
    iq, tx = synth.ul_units_3gpp(cfg, ul, [0], [21], two, 1)
    assert iq.any() and tx.shape == (1, 1, 6200)
    with pytest.raises(m.MiLteError):  # BPSK is outside the mode
        synth.ul_units_3gpp(cfg, ul, [0], [21], [m.make_alloc(0, 0, 1096, list(range(6)), 0x51)], 1)
