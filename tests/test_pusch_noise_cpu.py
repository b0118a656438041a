"""CPU: the DMRS noise estimate of the 3GPP PUSCH plans as include/mi_lte.h states it (tests/pusch_demod_model.py, the float64
restatement the GPU test holds the kernel to): unbiased on a channel with a timing offset, the spread the header quotes, the edges; and the
uplink payload transmitter (mi_lte_synth_ul_units_3gpp_payload_i8) against the seeded generators it extends.  No GPU."""
import ctypes as C

import numpy as np
import pytest

import pusch_demod_model as nm
from test_ulsch_uci_cpu import uci, units_case

ERR_INVALID = -1


def channel(rng, n_prb, s2, n):
    """n draws of t [2, M] = h exp(-2 pi i 4 k / 2048) + CN(0, s2), |h| uniform in 0.5 .. 1.5 with a random phase, one h per draw and slot"""
    M = 12 * n_prb
    h = rng.uniform(0.5, 1.5, (n, 2, 1)) * np.exp(2j * np.pi * rng.uniform(0, 1, (n, 2, 1)))
    ramp = np.exp(-2j * np.pi * 4 * np.arange(M) / 2048)
    w = np.sqrt(s2 / 2) * (rng.standard_normal((n, 2, M)) + 1j * rng.standard_normal((n, 2, M)))
    return h * ramp + w, h


@pytest.mark.parametrize("s2", [1.0, 0.01])
def test_unbiased(s2):
    """25 PRB, 400 seeded draws: |mean(sigma2_hat / sigma2) - 1| <= 0.015 (the standard error of the mean is 1.36 / sqrt(500) / 20 = 0.003)."""
    rng = np.random.default_rng(2025 + int(100 * s2))
    t, _ = channel(rng, 25, s2, 400)
    ratio = np.array([nm.sigma2_t(x) for x in t]) / s2
    print("sigma2 %g: mean ratio %.4f, standard deviation %.4f" % (s2, ratio.mean(), ratio.std(ddof=1)))
    assert abs(ratio.mean() - 1) <= 0.015, ratio.mean()


@pytest.mark.parametrize("n_prb", [1, 6, 25, 96])
def test_spread(n_prb):
    """The sample standard deviation of sigma2_hat / sigma2 over 400 draws is <= 1.6 / sqrt(20 N_prb) (neighbouring second differences
    share samples: the header's 1.36 / sqrt(20 N_prb), not 1 / sqrt)."""
    rng = np.random.default_rng(77 + n_prb)
    t, _ = channel(rng, n_prb, 0.25, 400)
    ratio = np.array([nm.sigma2_t(x) for x in t]) / 0.25
    root = 1.0 / np.sqrt(20 * n_prb)
    print("%2d PRB: standard deviation %.4f = %.3f / sqrt(20 N_prb)" % (n_prb, ratio.std(ddof=1), ratio.std(ddof=1) / root))
    assert ratio.std(ddof=1) <= 1.6 * root


def test_noiseless_linear_phase_channel():
    """No noise, a timing offset of 4 samples: sigma2_hat <= 1e-6 |h|^2 (the second difference leaves (2 pi 4 / 2048)^4 |h|^2 per term)."""
    rng = np.random.default_rng(5)
    for n_prb in (1, 25, 96):
        t, h = channel(rng, n_prb, 0.0, 8)
        for x, hh in zip(t, h):
            s = nm.sigma2_t(x)
            assert 0 <= s <= 1e-6 * float(np.abs(hh).min() ** 2), (n_prb, s)
    assert nm.sigma2_t(np.zeros((2, 24), np.complex128)) == 0.0


def test_non_contiguous_prb_list_equals_its_prbs_one_by_one():
    """A hopping, non-contiguous allocation on random planes: the estimate over the list equals the mean of the single-PRB estimates (S is
    a sum over resource blocks and no difference crosses a boundary), and differs from that of the contiguous list of the same length."""
    import openlte_amd as m
    rng = np.random.default_rng(11)
    planes = rng.standard_normal((2, 16, 1200)).astype(np.float32)
    prbs0, prbs1 = [3, 4, 9, 17, 18, 40], [50, 7, 8, 30, 2, 99]
    M = 12 * len(prbs0)
    dmrs = np.exp(2j * np.pi * rng.uniform(0, 1, (2, M)))
    dmrs = np.stack([dmrs[0].real, dmrs[0].imag, dmrs[1].real, dmrs[1].imag]).astype(np.float32)
    al = m.make_alloc(0, 1, 16, prbs0, 0x10, prbs_slot1=prbs1)
    whole = nm.sigma2(planes, al, dmrs)
    parts = []
    for j, (p0, p1) in enumerate(zip(prbs0, prbs1)):
        one = m.make_alloc(0, 1, 16, [p0], 0x10, prbs_slot1=[p1])
        parts.append(nm.sigma2(planes, one, dmrs[:, 12 * j:12 * j + 12]))
    assert abs(whole - np.mean(parts)) <= 1e-12 * whole, (whole, np.mean(parts))
    other = nm.sigma2(planes, m.make_alloc(0, 1, 16, list(range(3, 9)), 0x10), dmrs)
    assert abs(other - whole) > 1e-3 * whole


def test_gain_rules():
    """(float)(scale / (float)sigma2); 0 for sigma2 0, infinite or NaN and for a quotient past float."""
    assert nm.gain(8.0, np.float32(0.5)) == 16.0
    assert nm.gain(8.0, 0.0) == 0.0 and nm.gain(8.0, np.inf) == 0.0 and nm.gain(8.0, np.nan) == 0.0
    assert nm.gain(1e30, 1e-30) == 0.0
    assert nm.gain(3.0, np.float32(0.1)) == float(np.float32(3.0 / np.float64(np.float32(0.1))))


# ---- the payload transmitter

def uci_case():
    us = [uci(1, 4, 0, 0, 0), uci(2, 6, 1, 3, 40), uci(), uci(0, 0, 2, 8, 0)]
    return us, dict(ack=[[1], [0, 1], [], []], ri=[[], [1], [], [1, 1]], cqi=[[], np.arange(40) % 2, [], []])


@pytest.mark.parametrize("with_uci", [False, True])
def test_payload_transmitter_matches_generator(with_uci):
    """Given the bits the seeded generator drew, the payload transmitter writes the generator's IQ byte for byte, with and without control
    information; another payload changes it; the same payload at another rv and seed is another signal."""
    import openlte_amd as m
    from openlte_amd import synth
    cfg, ul, sfs, cells, allocs = units_case()
    kw = {}
    if with_uci:
        us, vals = uci_case()
        kw = dict(uci=us, **vals)
    iq, tx = synth.ul_units_3gpp(cfg, ul, sfs, cells, allocs, 2, snr_db=14.0, seed=11, **kw)
    iq2, tx2 = synth.ul_units_3gpp(cfg, ul, sfs, cells, allocs, 2, snr_db=14.0, seed=11, payload=tx, **kw)
    assert iq.any() and iq2.tobytes() == iq.tobytes() and tx2.tobytes() == tx.tobytes()
    wide = np.concatenate([tx, np.ones((2, 2, 5), np.uint8)], 2)  # a stride above the largest tbs
    iq2w, tx2w = synth.ul_units_3gpp(cfg, ul, sfs, cells, allocs, 2, snr_db=14.0, seed=11, payload=wide, **kw)
    assert iq2w.tobytes() == iq.tobytes() and tx2w.tobytes() == tx.tobytes()
    flipped = tx.copy()
    flipped[1, 1, 0] ^= 1
    iq3, _ = synth.ul_units_3gpp(cfg, ul, sfs, cells, allocs, 2, snr_db=14.0, seed=11, payload=flipped, **kw)
    assert (iq3[1] != iq[1]).any() and iq3[0].tobytes() == iq[0].tobytes()
    allocs_rv = [m.make_alloc(a.unit, a.mod_type, a.tbs, [a.prb[0][i] for i in range(a.N_prb)], a.rnti, rv_idx=(a.rv_idx + 2) % 4) for a in allocs]
    iq4, tx4 = synth.ul_units_3gpp(cfg, ul, sfs, cells, allocs_rv, 2, snr_db=14.0, seed=12, payload=tx, **kw)
    assert (iq4 != iq).any() and tx4.tobytes() == tx.tobytes()


def test_payload_transmitter_refusals():
    """A NULL payload, a tbs past the payload's stride, and what the siblings refuse: BPSK, a tbs outside the 3GPP mode, a bad grid, a
    descriptor mi_lte_ulsch_uci_G refuses, a transport block the remaining G cannot carry."""
    import openlte_amd as m
    from openlte_amd import synth
    L = synth._lib()
    cfg, ul = m.DlCfg(512, 25, 1, 0), m.UlCfg(3, 0, 0, 2, 1)
    ch = synth.SynthChannel(0.5, 1.5, 4.0, 30.0, 100.0, 1)
    iq = np.zeros((1, synth.ul_unit_len(512), 2), np.int8)
    sf, cell = np.zeros(1, np.uint32), np.full(1, 21, np.uint32)
    two_bytes = np.zeros(2, np.uint8)

    def call(c, allocs, payload, stride, u=None, cqi=None, cqi_stride=0):
        arr = (m.PdschAlloc * len(allocs))(*allocs)
        u_arr = None if u is None else (m.UlschUci * len(u))(*u)
        return L.mi_lte_synth_ul_units_3gpp_payload_i8(C.byref(c), C.byref(ul), 1, sf, cell, C.cast(arr, C.c_void_p), len(allocs), C.byref(ch),
                                                        None if u is None else C.cast(u_arr, C.c_void_p),
                                                        None if u is None else two_bytes.ctypes.data, None if u is None else two_bytes.ctypes.data,
                                                        None if cqi is None else cqi.ctypes.data, cqi_stride,
                                                        None if payload is None else payload.ctypes.data, stride, iq)

    good = m.make_alloc(0, 2, 6200, list(range(10)), 0x50)
    pay = np.zeros(6200, np.uint8)
    assert call(cfg, [good], pay, 6200) == 0
    assert call(cfg, [good], pay, 6200, u=[uci(1, 12)]) == 0
    assert call(cfg, [good], None, 6200) == ERR_INVALID
    assert call(cfg, [good], pay, 6192) == ERR_INVALID
    assert call(m.DlCfg(500, 25, 1, 0), [good], pay, 6200) == ERR_INVALID
    assert call(cfg, [m.make_alloc(0, 0, 72, [0], 0x51)], pay, 6200) == ERR_INVALID                # BPSK
    assert call(cfg, [m.make_alloc(0, 2, 6128, list(range(10)), 0x52)], pay, 6200) == ERR_INVALID  # F != 0
    assert call(cfg, [good], pay, 6200, u=[uci(3, 4)]) == ERR_INVALID                               # O_ack > 2
    big = np.zeros(4 * 1439, np.uint8)
    assert call(cfg, [good], pay, 6200, u=[uci(Q_cqi=4 * 1439)], cqi=big, cqi_stride=len(big)) != 0  # one symbol left for two code blocks
    with pytest.raises(ValueError):
        synth.ul_units_3gpp(cfg, ul, [0], [21], [good], 1, payload=np.zeros((2, 1, 6200), np.uint8))
    with pytest.raises(m.MiLteError):
        synth.ul_units_3gpp(cfg, ul, [0], [21], [good], 1, payload=np.zeros((1, 1, 6000), np.uint8))
