"""CPU: the claims behind the 3GPP PUSCH plans' receive-antenna combining (include/mi_lte.h, "PUSCH, 3GPP mode: receive-antenna combining")
and its float64 model tests/pusch_demod_model.py: one antenna is the single-antenna models to the last bit; the same grid on every antenna
is the single-antenna symbol with n_rx times the reliability and the same noise estimate; with independent noise per antenna the combined
symbol's noise variance is sigma^2 / rho_s and the noise estimate is unbiased with 1 / sqrt(n_rx) of the single-antenna spread; the
restatement of the launch's LDS and S_par rule gives today's values for one antenna and the limits the header names for two and four; the
float32 restatement of the combiner stays inside the hard gate; the synthetic antenna captures are antenna-major.  No GPU."""
import numpy as np
import pytest

import pusch_demod_cases as pc
import pusch_demod_model as nm
import pusch_demod_model as pm
from pusch_demod_cases import rx_view as rxm
from test_pusch_llr_cpu import selective_channel
from test_pusch_noise_cpu import channel


@pytest.mark.parametrize("n_prb", [1, 6, 25])
def test_one_antenna_is_the_single_antenna_models(n_prb):
    """a list of one antenna: every function equals what it gives for the bare unit's planes exactly"""
    c = pc.case(n_prb, 0)
    one = [c.planes]
    assert np.array_equal(rxm.h_polar(one, c.al, c.dmrs)[0], pm.h_polar(c.planes, c.al, c.dmrs))
    assert np.array_equal(rxm.combined(one, c.al, c.dmrs), pm.equalised(c.planes, c.al, c.dmrs))
    assert np.array_equal(rxm.equalise_predecode(one, c.al, c.dmrs), pm.equalise_predecode(c.planes, c.al, c.dmrs))
    got, want = rxm.rho(one, c.al, c.dmrs), pm.rho_of(pm.h_polar(c.planes, c.al, c.dmrs))
    assert all(np.array_equal(g, w) for g, w in zip(got, want))
    assert rxm.sigma2(one, c.al, c.dmrs) == nm.sigma2(c.planes, c.al, c.dmrs)
    assert np.abs(rxm.combined(one, c.al, c.dmrs)).min() > 0


@pytest.mark.parametrize("n_rx", [2, 4])
def test_the_same_grid_on_every_antenna(n_rx):
    """z is the single-antenna z to 1e-12 relative, rho is n_rx times and sigma2 the same as with one antenna"""
    c = pc.case(6, 1)
    many = [c.planes] * n_rx
    z1, z = pm.equalised(c.planes, c.al, c.dmrs), rxm.combined(many, c.al, c.dmrs)
    assert np.abs(z - z1).max() <= 1e-12 * np.abs(z1).max()
    r1, r = pm.rho_of(pm.h_polar(c.planes, c.al, c.dmrs))[0], rxm.rho(many, c.al, c.dmrs)[0]
    assert np.allclose(r, n_rx * r1, rtol=1e-12, atol=0)
    s1, s = nm.sigma2(c.planes, c.al, c.dmrs), rxm.sigma2(many, c.al, c.dmrs)
    assert s1 > 0 and abs(s - s1) <= 1e-12 * s1


def test_a_zero_antenna_drops_out():
    """an all-zero grid next to a live one: h_r = 0, so z and rho are the live antenna's and sigma2 is half its estimate; all zero: rho 0"""
    c = pc.case(6, 0)
    dead = np.zeros_like(c.planes)
    assert not rxm.h_polar([dead], c.al, c.dmrs).any()
    for pair in ([c.planes, dead], [dead, c.planes]):
        assert np.array_equal(rxm.combined(pair, c.al, c.dmrs), pm.equalised(c.planes, c.al, c.dmrs))
        assert np.array_equal(rxm.rho(pair, c.al, c.dmrs)[0], pm.rho_of(pm.h_polar(c.planes, c.al, c.dmrs))[0])
        assert rxm.sigma2(pair, c.al, c.dmrs) == nm.sigma2(c.planes, c.al, c.dmrs) / 2
    assert not rxm.rho([dead, dead], c.al, c.dmrs)[0].any() and rxm.sigma2([dead, dead], c.al, c.dmrs) == 0.0


@pytest.mark.parametrize("n_rx,M", [(2, 12), (2, 72), (4, 72), (2, 300)])
def test_noise_variance_after_combining_and_idft(n_rx, M):
    """test_pusch_llr_cpu's Monte Carlo with n_rx antennas: white noise of variance sigma^2 per sub-carrier and antenna, combined with
    conj(h_r) / P and put through the 1 / sqrt(M) inverse DFT, has variance sigma^2 / rho on every sample, rho = M / sum_k 1 / P_k.  The
    combined noise on sub-carrier k is complex normal of variance sigma^2 / P_k, so that test's two bounds hold with P in place of |h|^2:
    5 / sqrt(N) per sample and 5 sqrt(sum 1 / P^2) / sum 1 / P / sqrt(N) for the mean."""
    rng = np.random.default_rng(300 + 10 * M + n_rx)
    h = np.stack([selective_channel(rng, M) for _ in range(n_rx)])
    P = rxm.power(h[:, None, :])[0]
    rho = M / (1 / P).sum()
    sigma2, N = 0.37, 20000
    z = np.zeros((N, M), np.complex128)
    for r in range(n_rx):
        n = np.sqrt(sigma2 / 2) * (rng.standard_normal((N, M)) + 1j * rng.standard_normal((N, M)))
        z += n * np.conj(h[r])[None, :]
    x = np.fft.ifft(z / P[None, :], axis=1) * np.sqrt(M)
    var = (np.abs(x) ** 2).mean(0)
    want = sigma2 / rho
    per_sample, pooled = 5 / np.sqrt(N), 5 * np.sqrt((1 / P ** 2).sum()) / (1 / P).sum() / np.sqrt(N)
    print("n_rx %d, M %d: rho %.4g, variance %.5g against %.5g, worst sample off by %.3g (bound %.3g), mean by %.3g (bound %.3g)"
          % (n_rx, M, rho, var.mean(), want, np.abs(var / want - 1).max(), per_sample, abs(var.mean() / want - 1), pooled))
    assert np.abs(var / want - 1).max() < per_sample
    assert abs(var.mean() / want - 1) < pooled
    w0 = np.abs(h[0]) ** 2  # one antenna alone is noisier: the combiner's rho is more than any single antenna's
    assert rho > M / (1 / w0).sum()


@pytest.mark.parametrize("n_rx", [2, 4])
def test_noise_estimate_mean_and_spread(n_rx):
    """6 PRB, N = 1600 draws of test_pusch_noise_cpu's channel per antenna (another gain and phase per antenna, the same noise power).
    Mean of sigma2_hat / sigma2: 1 within 4 standard errors of the mean (the sample's own).  Spread: the estimate is the mean of n_rx
    independent single-antenna estimates, so its standard deviation is 1 / sqrt(n_rx) of theirs; a sample standard deviation of N
    near-normal values (each estimate sums 120 terms) has relative standard error 1 / sqrt(2 (N - 1)), the ratio of two independent ones
    sqrt(2) times that, and the ratio is held to 4 of those: 10 %."""
    N, n_prb, s2 = 1600, 6, 0.25
    rng = np.random.default_rng(900 + n_rx)
    ts = [channel(rng, n_prb, s2, N)[0] for _ in range(n_rx)]
    single = np.array([nm.sigma2_t(x) for x in channel(rng, n_prb, s2, N)[0]]) / s2
    many = np.array([rxm.sigma2_t([t[k] for t in ts]) for k in range(N)]) / s2
    se = many.std(ddof=1) / np.sqrt(N)
    ratio = many.std(ddof=1) * np.sqrt(n_rx) / single.std(ddof=1)
    bound = 4 * np.sqrt(2) / np.sqrt(2 * (N - 1))
    print("n_rx %d: mean ratio %.4f (standard error %.4f), standard deviation %.4f against %.4f with one antenna: sqrt(n_rx) x ratio %.3f (bound +-%.3f)"
          % (n_rx, many.mean(), se, many.std(ddof=1), single.std(ddof=1), ratio, bound))
    assert abs(many.mean() - 1) <= 4 * se
    assert abs(ratio - 1) <= bound


def test_lds_and_s_par_rule():
    """One antenna: the restatement gives today's S_par (pusch_demod_model.s_par) and the noise-referenced launch's LDS at every planned
    size and modulation.  Two antennas: every planned size fits 160 KiB at today's S_par, 144 224 bytes at 99 PRB of 64QAM.  Four: the
    steps and limits the header names -- with 64QAM S_par 3 up to 65 PRB, 2 up to 70, 1 up to 76, refused from 78; with QPSK 3 up to 66,
    2 up to 72, 1 up to 78, refused from 80 -- and 25 PRB fits by a wide margin."""
    for n in pc.planned_sizes():
        for q in (2, 4, 6):
            M, W = 12 * n, rxm.words(n, q)
            S = pc.s_par(M)
            assert rxm.s_par(1, M, W) == S
            today = 4 * 9 * M + 8 * M * (1 + 2 * S) + 4 * W  # uplink.hip's run function: est | tw, buf A, buf B | words_max + 1 words
            assert rxm.lds_bytes(1, M, W, S) == (today + 7) // 8 * 8 + 4 * 12 * 8 + 12 * 4 + 4 * 8
            assert rxm.s_par(2, M, W) == S and rxm.lds_bytes(2, M, W, S) <= rxm.LDS_LIMIT
    assert rxm.lds_bytes(2, 1188, rxm.words(99, 6), 2) == 144224
    assert rxm.lds_bytes(1, 1188, rxm.words(99, 6), 2) == 144224 - 36 * 1188
    four = {q: {n: rxm.s_par(4, 12 * n, rxm.words(n, q)) for n in pc.planned_sizes()} for q in (2, 6)}
    assert [four[6][n] for n in (34, 35, 36, 65, 66, 70, 72, 76, 78, 99)] == [6, 6, 3, 3, 2, 2, 1, 1, 0, 0]
    assert [four[2][n] for n in (66, 68, 72, 74, 78, 80, 99)] == [3, 2, 2, 1, 1, 0, 0]
    assert all(four[q][n] == pc.s_par(12 * n) for q in (2, 6) for n in pc.planned_sizes() if n <= 65)
    assert four[6][25] == 6 and rxm.lds_bytes(4, 300, rxm.words(25, 6), 6) < rxm.LDS_LIMIT // 2
    assert rxm.threads(96) == 192 and rxm.threads(108) == 256


@pytest.mark.parametrize("n_prb,n_rx", [(1, 2), (6, 4), (25, 2)])
def test_float32_restatement_sits_inside_the_hard_gate(n_prb, n_rx):
    """the combiner's float operations and the float32 transform against the float64 model on the GPU tests' kind of input: under a tenth
    of the hard gates, so the tight gate (8 x this) is the one that binds; and the gapped PRB lists are what they claim to be"""
    c = rxm.case(n_prb, n_rx)
    prb = [[c.al.prb[b][i] for i in range(n_prb)] for b in range(2)]
    assert all(len(set(p)) == n_prb and max(p) < pc.N_RB for p in prb) and (n_prb == 1 or prb[0] != prb[1])
    assert n_prb == 1 or all(max(p) - min(p) >= n_prb for p in prb)  # a gap
    l2, el = rxm.float32_floor(((n_prb, n_rx, 0, 1),))
    print("%d PRB, %d antennas: float32 restatement rel-L2 %.3g, elementwise / RMS %.3g" % (n_prb, n_rx, l2, el))
    assert 0 < l2 < 0.1 * pc.TOL_SYMB and 0 < el < pc.TOL_SYMB
    g = rxm.gates(((n_prb, n_rx, 0, 1),))
    assert g == (pc.GATE_FACTOR * l2, pc.GATE_FACTOR * el)


def test_antenna_captures_are_antenna_major():
    """synth.ul_units_3gpp_rx: antenna r of unit u at r * ant_stride + u, each antenna ul_units_3gpp of the same payload with its own seed,
    the units in between zero"""
    from openlte_amd import synth
    from test_ulsch_uci_cpu import units_case
    cfg, ul, sfs, cells, allocs = units_case()
    n = len(sfs)
    iq, tx = synth.ul_units_3gpp_rx(cfg, ul, sfs, cells, allocs, 2, 2, ant_stride=n + 1, seeds=(5, 9), seed=3, snr_db=14.0)
    assert iq.shape[0] == 2 * (n + 1) and not iq[n].any() and not iq[2 * n + 1].any()
    for r, seed in enumerate((5, 9)):
        one, tx1 = synth.ul_units_3gpp(cfg, ul, sfs, cells, allocs, 2, snr_db=14.0, seed=seed, payload=tx)
        assert one.any() and iq[r * (n + 1):r * (n + 1) + n].tobytes() == one.tobytes() and tx1.tobytes() == tx.tobytes()
    assert (iq[:n] != iq[n + 1:2 * n + 1]).any()
    with pytest.raises(ValueError):
        synth.ul_units_3gpp_rx(cfg, ul, sfs, cells, allocs, 2, 2, ant_stride=n - 1)
