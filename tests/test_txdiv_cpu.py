"""CPU: the host arithmetic of the transmit-diversity mode of the 3GPP PDSCH plans (include/mi_lte.h, "PDSCH, 3GPP mode: transmit diversity on 2
or 4 ports"): mi_lte_dlsch_layout_nl against a restatement of 36.212 5.1.2 / 5.1.4.1.2 with N_L, mi_lte_txdiv_precode against the matrices of
36.211 6.3.4.3, the combiner of tests/demap_llr_model.py against both (it returns the symbols, its w is the stated one, and the noise on
t / w has variance sigma^2 / w), and the generator's refusals and payload hand-back.  No GPU."""
import ctypes as C

import numpy as np
import pytest

import demap_llr_model as tm
from test_dlsch3gpp_cpu import all_tbs, seg

ERR_INVALID, ERR_UNSUPPORTED = -1, -4
N_SOFT = 1237248


def layout_py(tbs, G, Qm, n_l, kmimo, rv, n_soft, m_harq):
    """36.212 5.1.2 (segmentation) and 5.1.4.1.2 (soft buffer; G' = G / (N_L Q_m), gamma = G' mod C, E_r) restated"""
    C_, K, B, Bp = seg(tbs)
    R = -(-(K + 4) // 32)
    K_w = 96 * R
    N_ir = n_soft // (kmimo * min(m_harq, 8))
    N_cb = min(N_ir // C_, K_w)
    k0 = R * (2 * -(-N_cb // (8 * R)) * rv + 2)
    Gp = G // (n_l * Qm)
    gam = Gp % C_
    E = [n_l * Qm * (Gp // C_) if r <= C_ - gam - 1 else n_l * Qm * -(-Gp // C_) for r in range(C_)]
    return {"C": C_, "K": K, "B": B, "N_cb": N_cb, "k0": k0, "E": E, "off": [sum(E[:r]) for r in range(C_)]}


def test_layout_nl_is_36212_for_every_table_size():
    """Every size of Table 7.1.7.2.1-1 x Q_m in {2, 4, 6} x N_L in {1, 2} x four G, two of them with G' mod C != 0 whenever C > 1; the N_L = 1
    results are mi_lte_dlsch_layout's."""
    from openlte_amd import dlsch_layout
    n = ragged = 0
    for tbs in all_tbs():
        C_ = seg(tbs)[0]
        for Qm in (2, 4, 6):
            for n_l in (1, 2):
                u = n_l * Qm
                for Gp in (C_ * 40, C_ * 40 + 1, 13 * 700 + C_ - 1, 15000 // u):
                    G = Gp * u
                    for rv, txm in ((0, 2), (3, 4)):
                        got = dlsch_layout(tbs, G, Qm, txm, rv, N_SOFT, 8, n_l=n_l)
                        assert got == layout_py(tbs, G, Qm, n_l, 2 if txm == 4 else 1, rv, N_SOFT, 8), (tbs, G, Qm, n_l)
                        assert sum(got["E"]) == G and all(e % u == 0 for e in got["E"])
                        if n_l == 1:
                            assert got == dlsch_layout(tbs, G, Qm, txm, rv, N_SOFT, 8)
                        n += 1
                        ragged += Gp % C_ != 0
    assert n == 178 * 3 * 2 * 4 * 2 and ragged > n // 8


def test_layout_nl_differs_from_nl1_where_the_pairs_do_not_split_evenly():
    """Two blocks, M_symb / 2 odd: N_L = 2 keeps the odd pair whole in the second block"""
    from openlte_amd import dlsch_layout
    one, two = dlsch_layout(6200, 6 * 3002, 6, 2, n_l=1), dlsch_layout(6200, 6 * 3002, 6, 2, n_l=2)
    assert one["E"] == [6 * 1501, 6 * 1501] and two["E"] == [6 * 1500, 6 * 1502] and two["off"] == [0, 9000]


def test_layout_nl_refusals():
    import openlte_amd as m
    L = m.load_library()
    from openlte_amd.lib import DlschLayout
    out, dl = DlschLayout(), m.DlschCfg(N_SOFT, 8)
    call = lambda tbs, G, Qm, n_l, rv=0: L.mi_lte_dlsch_layout_nl(tbs, G, Qm, n_l, 2, rv, C.byref(dl), C.byref(out))
    assert call(3240, 1200, 6, 2) == 0
    assert call(3240, 1200, 6, 0) == ERR_INVALID and call(3240, 1200, 6, 3) == ERR_INVALID
    assert call(3240, 1206, 6, 2) == ERR_INVALID and call(3240, 1206, 6, 1) == 0  # G a multiple of N_L Q_m
    assert call(3240, 1200, 6, 2, rv=4) == ERR_INVALID and call(3240, 1200, 5, 2) == ERR_INVALID
    assert call(75384, 1200, 6, 2) == ERR_UNSUPPORTED and call(6128, 1200, 6, 2) == ERR_UNSUPPORTED
    assert L.mi_lte_dlsch_layout_nl(3240, 1200, 6, 2, 2, 0, None, C.byref(out)) == ERR_INVALID


def precode_np(n_ant, d):
    """36.211 6.3.3.3 (x_l(i) = d(N_ant i + l)) and the matrices of 6.3.4.3, written out"""
    s = 1 / np.sqrt(2)
    y = np.zeros((n_ant, len(d)), np.complex128)
    if n_ant == 2:
        x0, x1 = d[0::2], d[1::2]
        y[0, 0::2], y[1, 0::2] = s * x0, -s * np.conj(x1)
        y[0, 1::2], y[1, 1::2] = s * x1, s * np.conj(x0)
        return y
    x0, x1, x2, x3 = d[0::4], d[1::4], d[2::4], d[3::4]
    y[0, 0::4], y[2, 0::4] = s * x0, -s * np.conj(x1)
    y[0, 1::4], y[2, 1::4] = s * x1, s * np.conj(x0)
    y[1, 2::4], y[3, 2::4] = s * x2, -s * np.conj(x3)
    y[1, 3::4], y[3, 3::4] = s * x3, s * np.conj(x2)
    return y


@pytest.mark.parametrize("n_ant", [2, 4])
def test_precode_is_36211(n_ant):
    from openlte_amd import synth
    rng = np.random.default_rng(n_ant)
    d = (rng.standard_normal(48) + 1j * rng.standard_normal(48)).astype(np.complex64)
    got = synth.txdiv_precode(n_ant, d)
    assert got.shape == (n_ant, 48)
    assert np.abs(got - precode_np(n_ant, d.astype(np.complex128))).max() < 2e-7 * np.abs(d).max()
    if n_ant == 4:
        assert not got[1:4:2, 0::4].any() and not got[0:3:2, 2::4].any()  # the resting ports
    import openlte_amd as m
    for bad_ant, n in ((1, 48), (3, 48), (2, 47), (4, 46)):
        with pytest.raises(m.MiLteError):
            synth.txdiv_precode(bad_ant, d[:n])


def through_channel(rng, n_ant, d, sigma2=0.0):
    """The precoded symbols through a pair-constant random channel per port, plus noise: (ya, yb, ha, hb) per element pair"""
    from openlte_amd import synth
    y = synth.txdiv_precode(n_ant, d.astype(np.complex64)).astype(np.complex128)
    n_pair = len(d) // 2
    h = (rng.standard_normal((n_ant, n_pair)) + 1j * rng.standard_normal((n_ant, n_pair))) * rng.uniform(0.3, 1.5, (n_ant, 1))
    rx = (np.repeat(h, 2, axis=1) * y).sum(0)
    rx = rx + np.sqrt(sigma2 / 2) * (rng.standard_normal(len(d)) + 1j * rng.standard_normal(len(d)))
    pa, pb = tm.pair_ports(n_pair, n_ant)
    k = np.arange(n_pair)
    return rx[0::2], rx[1::2], h[pa, k], h[pb, k]


@pytest.mark.parametrize("n_ant", [2, 4])
def test_combiner_returns_the_symbols(n_ant):
    """t / w = d and w = (|h_pa|^2 + |h_pb|^2) / 2 through a noiseless channel that is constant over each pair"""
    rng = np.random.default_rng(10 + n_ant)
    d = (rng.standard_normal(240) + 1j * rng.standard_normal(240)).astype(np.complex64).astype(np.complex128)
    ya, yb, ha, hb = through_channel(rng, n_ant, d)
    t0, w0, t1, w1 = tm.combine(ya, yb, ha, hb, ha, hb)
    want_w = (np.abs(ha) ** 2 + np.abs(hb) ** 2) / 2
    assert np.allclose(w0, want_w, rtol=1e-14) and np.allclose(w1, want_w, rtol=1e-14)
    assert np.abs(t0 / w0 - d[0::2]).max() < 1e-6 and np.abs(t1 / w1 - d[1::2]).max() < 1e-6  # (the precoder's float rounding)


@pytest.mark.parametrize("n_ant", [2, 4])
def test_noise_variance_of_the_symbol_estimate(n_ant):
    """White noise of variance sigma^2 per resource element leaves noise of variance sigma^2 / w on t / w.  N draws: a symbol's estimate has
    relative standard deviation 1 / sqrt(N) (|x|^2 of a complex Gaussian) and the mean over the independent symbols 1 / sqrt(N n); both are
    held to five standard deviations, the method of tests/test_pusch_llr_cpu.py."""
    rng = np.random.default_rng(20 + n_ant)
    n_sym, N, sigma2 = 48, 20000, 0.37
    d = np.zeros(n_sym, np.complex128)
    ya, yb, ha, hb = through_channel(rng, n_ant, d)  # the channel alone
    w = (np.abs(ha) ** 2 + np.abs(hb) ** 2) / 2
    assert w.max() / w.min() > 4
    na = np.sqrt(sigma2 / 2) * (rng.standard_normal((N, n_sym // 2)) + 1j * rng.standard_normal((N, n_sym // 2)))
    nb = np.sqrt(sigma2 / 2) * (rng.standard_normal((N, n_sym // 2)) + 1j * rng.standard_normal((N, n_sym // 2)))
    t0, w0, t1, w1 = tm.combine(na, nb, ha[None], hb[None], ha[None], hb[None])
    ratio = np.concatenate([(np.abs(t0 / w0) ** 2).mean(0) / (sigma2 / w), (np.abs(t1 / w1) ** 2).mean(0) / (sigma2 / w)])
    per_sample, pooled = 5 / np.sqrt(N), 5 / np.sqrt(N * n_sym)
    print("%d ports: worst symbol off by %.3g (bound %.3g), mean by %.3g (bound %.3g)" % (n_ant, np.abs(ratio - 1).max(), per_sample, abs(ratio.mean() - 1), pooled))
    assert np.abs(ratio - 1).max() < per_sample and abs(ratio.mean() - 1) < pooled
    assert abs((np.abs(t0) ** 2).mean() / (sigma2 * w.mean()) - 1) < 0.05  # (t itself carries sigma^2 w)


def units(n_ant, txm=2, mod=2, size=3240):
    import openlte_amd as m
    cfg = m.DlCfg(512, 25, n_ant, 0)
    return cfg, [m.make_alloc(0, mod, size, list(range(4, 16)), 0x77, tx_mode=txm)]


def test_generator_refusals():
    import openlte_amd as m
    from openlte_amd import synth
    cfg, allocs = units(2)
    iq, tx = synth.dl_units_3gpp_txdiv(cfg, [3], [42], allocs, 1, N_SOFT)
    assert iq.any() and tx.shape == (1, 1, 3240)
    for n_ant, txm, mod, size in ((1, 2, 2, 3240), (3, 2, 2, 3240), (2, 1, 2, 3240), (2, 3, 2, 3240), (4, 2, 0, 3240), (2, 2, 2, 6128), (2, 2, 2, 75384)):
        cfg, allocs = units(n_ant, txm, mod, size)
        with pytest.raises(m.MiLteError) as e:
            synth.dl_units_3gpp_txdiv(cfg, [3], [42], allocs, 1, N_SOFT)
        assert e.value.args[1] == ERR_INVALID, (n_ant, txm, mod, size)
    cfg, allocs = units(2)
    allocs[0].prb[1][3] = 25
    with pytest.raises(m.MiLteError):
        synth.dl_units_3gpp_txdiv(cfg, [3], [42], allocs, 1, N_SOFT)
    L = synth._lib()
    ch = synth.SynthChannel(1, 1, 0, 30, 100, 1)
    sf, cell = np.array([3], np.uint32), np.array([42], np.uint32)
    arr = (m.PdschAlloc * 1)(*units(2)[1])
    assert L.mi_lte_synth_dl_units_3gpp_txdiv_i8(C.byref(units(2)[0]), 1, sf, cell, 2, C.cast(arr, C.c_void_p), 1, None, C.byref(ch), None, 3240,
                                                 np.zeros((synth.unit_len(512), 2), np.int8), None) == ERR_INVALID


@pytest.mark.parametrize("n_ant", [2, 4])
def test_payload_comes_back_and_keeps_the_stream(n_ant):
    """The caller's payload is what h_tx_bits holds; given the bits a run without payload drew, the samples are the same byte for byte; the
    single-port generator's stream does not move."""
    from openlte_amd import synth
    cfg, allocs = units(n_ant)
    iq, tx = synth.dl_units_3gpp_txdiv(cfg, [3, 5], [42, 7], allocs * 2, 1, N_SOFT, snr_db=12.0, seed=4)
    iq2, tx2 = synth.dl_units_3gpp_txdiv(cfg, [3, 5], [42, 7], allocs * 2, 1, N_SOFT, snr_db=12.0, seed=4, payload=tx)
    assert (tx2 == tx).all() and (iq2 == iq).all()
    mine = np.random.default_rng(1).integers(0, 2, (2, 1, 3300), dtype=np.uint8)
    iq3, tx3 = synth.dl_units_3gpp_txdiv(cfg, [3, 5], [42, 7], allocs * 2, 1, N_SOFT, snr_db=12.0, seed=4, payload=mine)
    assert (tx3 == mine[:, :, :3240]).all() and (iq3 != iq).any()
