"""CPU: the claims behind the 3GPP PUSCH plans' max-log demapper (include/mi_lte.h, "PUSCH, 3GPP mode: max-log soft-decision demapping") and
its float64 model tests/pusch_demod_model.py: the noise variance after zero forcing and the 1 / sqrt(M) inverse DFT is sigma^2 / rho_s; the
piecewise-linear LLR with w = rho_s is the brute-force max-log LLR over the whole constellation; the automatic gain's degenerate cases."""
import numpy as np
import pytest

import demap_llr_model as dm
import pusch_demod_model as pm


def selective_channel(rng, M, taps=4):
    """a random frequency-selective channel over M sub-carriers: a few paths with delays up to half the allocation's inverse DFT length, so
    |h|^2 varies by more than 6 dB inside the allocation"""
    d = rng.integers(0, M // 2 + 1, taps)
    a = (rng.standard_normal(taps) + 1j * rng.standard_normal(taps)) / np.sqrt(2 * taps)
    k = np.arange(M)
    return (a[None, :] * np.exp(-2j * np.pi * k[:, None] * d[None, :] / M)).sum(1)


@pytest.mark.parametrize("M", [12, 72, 300])
def test_noise_variance_after_zero_forcing_and_idft(M):
    """White noise of variance sigma^2 per sub-carrier, divided by h_k and put through the 1 / sqrt(M) inverse DFT, has variance sigma^2 / rho
    on every time-domain sample, rho = M / sum_k 1 / |h_k|^2 (the model's rho_of).  N draws: a sample's estimate has relative standard
    deviation 1 / sqrt(N) (|x|^2 of a complex Gaussian), the mean over the M samples sqrt(sum 1 / |h|^4) / sum 1 / |h|^2 / sqrt(N) by Parseval;
    both are held to five standard deviations."""
    rng = np.random.default_rng(100 + M)
    h = selective_channel(rng, M)
    w = np.abs(h) ** 2
    assert w.max() / w.min() > 4
    rho, w_min, w_mean = pm.rho_of(np.tile(h, (12, 1)))
    assert np.allclose(rho, M / (1 / w).sum(), rtol=1e-12) and np.allclose(w_min, w.min()) and np.isclose(w_mean, w.mean())
    sigma2, N = 0.37, 20000
    n = np.sqrt(sigma2 / 2) * (rng.standard_normal((N, M)) + 1j * rng.standard_normal((N, M)))
    x = np.fft.ifft(n / h[None, :], axis=1) * np.sqrt(M)  # numpy's ifft divides by M: times sqrt(M) is the 1 / sqrt(M) transform
    var = (np.abs(x) ** 2).mean(0)
    want = sigma2 / rho[0]
    per_sample, pooled = 5 / np.sqrt(N), 5 * np.sqrt((1 / w ** 2).sum()) / (1 / w).sum() / np.sqrt(N)
    print("M %d: rho %.4g (mean |h|^2 %.4g), variance %.5g against %.5g, worst sample off by %.3g (bound %.3g), mean by %.3g (bound %.3g)"
          % (M, rho[0], w.mean(), var.mean(), want, np.abs(var / want - 1).max(), per_sample, abs(var.mean() / want - 1), pooled))
    assert np.abs(var / want - 1).max() < per_sample
    assert abs(var.mean() / want - 1) < pooled
    assert abs(sigma2 / w.mean() / want - 1) > 10 * pooled  # (the arithmetic mean of the channel power would be the wrong weight)


@pytest.mark.parametrize("mod", [1, 2, 3])
def test_piecewise_form_is_the_brute_force_llr_with_w_rho(mod):
    """g L of the model -- llr_axis with t = rho_s x and w = rho_s, through its scrambling and transposition -- equals g rho_s (min over the
    symbols with bit 1 of |x - s|^2 - min over those with bit 0) over the full constellation, for symbols spread well past its corners."""
    rng = np.random.default_rng(7 + mod)
    M, q = 24, pm.QM[mod]
    xs = ((rng.standard_normal((12, M)) + 1j * rng.standard_normal((12, M))) * 0.9).astype(np.complex64)
    rho = rng.uniform(0.05, 3.0, 12).astype(np.float32)
    g, c_init = 40.25, 0x1234567
    got = pm.demap(xs, rho, mod, c_init, gain=g)
    assert got.gain == g and got.bytes.shape == (12 * M * q,)
    want = np.zeros((12, M, q))
    for s in range(12):
        want[s] = g * dm.brute_llr(xs[s].astype(np.complex128), np.full(M, float(rho[s])), mod)
    c = dm.gold(c_init, 12 * M * q).reshape(12, M, q)
    want = np.where(c == 1, -want, want).transpose(1, 0, 2).reshape(-1)
    assert np.abs(got.x - want).max() <= 1e-9 * (1 + np.abs(want).max())
    assert (got.bytes == dm.soft_byte(got.x)).all() and (np.abs(got.bytes) == 127).any() and (np.abs(got.bytes) < 127).any()


def test_automatic_gain_and_degenerate_cases():
    """g = (float)(T / (4 A^2 rhobar)) on the mean of the twelve floats; 0 for a mean that is 0, infinite or NaN and for a gain past the float
    range; rho_s = 0 where a symbol has a zero or non-finite estimate; a zero rho_s or a NaN symbol gives zero bytes."""
    rho = np.linspace(0.5, 1.6, 12).astype(np.float32)
    for mod in (1, 2, 3):
        g = pm.auto_gain(rho, mod, 16)
        assert g == float(np.float32(16 / (dm.FOUR_A2[mod] * rho.astype(np.float64).mean())))
        # a noiseless innermost point at the mean reliability: its least reliable bit lands on T
        x = np.full((12, 1), dm.A[mod] * (1 + 1j), np.complex64)
        r = pm.demap(x, np.full(12, rho.astype(np.float64).mean(), np.float32), mod, 0, gain=0.0, T=16)
        assert abs(np.abs(r.x).min() - 16) < 1e-4
    assert pm.auto_gain(np.zeros(12, np.float32), 3, 16) == 0.0
    for bad in (np.inf, np.nan):
        r = rho.copy()
        r[5] = bad
        assert pm.auto_gain(r, 2, 16) == 0.0
    assert pm.auto_gain(np.full(12, 1e-38, np.float32), 3, 16) == 0.0  # 16 / (4 / 42 * 1e-38) is past the float range
    assert pm.auto_gain(np.full(12, 1e-36, np.float32), 3, 16) > 0
    # rho_of: a zero estimate on one sub-carrier of symbol 4, a NaN on one of symbol 9
    h = np.ones((12, 24), np.complex128)
    h[4, 3], h[9, 0] = 0, np.nan
    r, w_min, _ = pm.rho_of(h)
    assert r[4] == 0 and r[9] == 0 and (np.delete(r, [4, 9]) == 1).all() and w_min[4] == 0
    # bytes: zero where rho_s is zero, zero where the symbol is NaN, graded elsewhere
    xs = np.full((12, 24), 0.3 - 0.2j, np.complex64)
    xs[2, 7] = complex(np.nan, np.nan)
    d = pm.demap(xs, r.astype(np.float32), 3, 99, gain=40.0)
    e = d.bytes.reshape(24, 12, 6)
    assert not e[:, 4].any() and not e[:, 9].any() and not e[7, 2].any()
    keep = np.ones((24, 12), bool)
    keep[:, [4, 9]] = False
    keep[7, 2] = False
    assert (e[keep] != 0).any(-1).all()
    assert pm.demap(xs, np.zeros(12, np.float32), 3, 99, gain=0.0).gain == 0.0
