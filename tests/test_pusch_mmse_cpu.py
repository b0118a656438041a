"""CPU: the claims behind the 3GPP PUSCH plans' MMSE equalisation (include/mi_lte.h, "PUSCH, 3GPP mode: MMSE equalisation") and its float64
model tests/pusch_demod_model.py -- the flat-channel identity with the zero-forcing noise-referenced run, w_s >= rho_s / sigma2, the limit
s2 -> 0, the error variance nu_s / (1 - nu_s) of the unbiased symbol, the degenerate inputs, the conditions the GPU tests' caps rest on --
and the multipath generator mi_lte_synth_ul_units_3gpp_paths_i8."""
import ctypes as C

import numpy as np
import pytest

import demap_llr_model as dm
import pusch_demod_model as nm
import pusch_demod_model as pm
from pusch_demod_cases import mmse_view as mm, rx_view as rxm

ALL_KEYS = tuple(k for n_rx in (1, 2, 4) for k in mm.gpu_keys(n_rx))
FLAT_KEYS = {n_rx: tuple((n, n_rx, 6, mod) for n, mod in ((1, 1), (6, 2), (10, 3))) for n_rx in (1, 2, 4)}


def two_path_h(rng, M, n_rx, a=1.0, d=4, N=512):
    k = np.arange(M)
    return np.stack([np.exp(1j * rng.uniform(-np.pi, np.pi)) * (1 + a * np.exp(1j * rng.uniform(-np.pi, np.pi)) * np.exp(-2j * np.pi * k * d / N))
                     for _ in range(n_rx)]) / np.sqrt(1 + a * a)


@pytest.mark.parametrize("n_rx", [1, 2, 4])
def test_flat_channel_is_the_zero_forcing_noise_referenced_run(n_rx):
    """P the same on every sub-carrier: (t, w) of the MMSE model equal g (rho x, rho) of the zero-forcing model with g = 1 / s2, to 1e-12"""
    rng = np.random.default_rng(10 + n_rx)
    M, s2 = 72, 0.23
    P = np.full((12, M), 1.7 * n_rx)
    num = rng.standard_normal((12, M)) + 1j * rng.standard_normal((12, M))
    z, nu, w, rho_tap = mm.mmse(num, P, s2)
    t, w = mm.tw(mm.predecode(z), nu, w)
    z0, rho0 = mm.zf(num, P)
    t0, w0 = (rho0 / s2)[:, None] * mm.predecode(z0), rho0 / s2
    assert np.abs(t - t0).max() <= 1e-12 * np.abs(t0).max() and np.abs(w / w0 - 1).max() <= 1e-12
    assert np.abs(rho_tap / rho0 - 1).max() <= 1e-12 and np.allclose(nu, s2 / (P[:, 0] + s2), rtol=1e-12)


def test_w_is_never_below_zero_forcings_reliability():
    """w_s >= rho_s / sigma2 on every symbol of every case of the GPU tests' table, for 1, 2 and 4 antennas, and strictly above on these
    two-path planes"""
    for k in ALL_KEYS:
        t = mm.expected(k)
        assert (t["w"] >= t["rho_zf"] / t["s2"]).all() and (t["rho"] >= t["rho_zf"]).all(), k
        assert (t["w"] > 1.001 * t["rho_zf"] / t["s2"]).all(), k


@pytest.mark.parametrize("n_rx", [1, 2, 4])
def test_small_noise_limit_is_zero_forcing(n_rx):
    """s2 = 1e-12 of the mean power: z and w s2 agree with zero forcing's z and rho_s to 1e-6"""
    rng = np.random.default_rng(20 + n_rx)
    M = 240
    h = two_path_h(rng, M, n_rx, a=0.5)
    P = np.tile((np.abs(h) ** 2).sum(0), (12, 1))
    num = (rng.standard_normal((12, M)) + 1j * rng.standard_normal((12, M))) * np.sqrt(P)
    s2 = 1e-12 * P.mean()
    z, nu, w, rho_tap = mm.mmse(num, P, s2)
    z0, rho0 = mm.zf(num, P)
    assert np.abs(z - z0).max() <= 1e-6 * np.abs(z0).max() and np.abs(w * s2 / rho0 - 1).max() <= 1e-6 and (rho_tap >= rho0).all()


@pytest.mark.parametrize("n_rx,snr_db", [(1, 10.0), (2, 5.0)])
def test_error_variance_of_the_unbiased_symbol(n_rx, snr_db):
    """Two equal-power paths 4 samples apart (N 512, 20 PRB): over N draws of unit-energy QPSK symbols and white noise the variance of
    x / (1 - nu) - d is nu / (1 - nu) on every sample.  Bounds as test_pusch_llr_cpu's for sigma^2 / rho_s: five standard deviations,
    1 / sqrt(N) per sample and sqrt(sum c_k^2) / sum c_k / sqrt(N) for the mean, c_k the error power per sub-carrier (Parseval)."""
    rng = np.random.default_rng(30 + n_rx)
    M, N = 240, 20000
    h = two_path_h(rng, M, n_rx, a=1.0)
    P = (np.abs(h) ** 2).sum(0)
    assert P.max() / P.min() > 4
    s2 = P.mean() / n_rx / 10 ** (snr_db / 10)
    d = ((1 - 2 * rng.integers(0, 2, (N, M))) + 1j * (1 - 2 * rng.integers(0, 2, (N, M)))) / np.sqrt(2)
    D = np.fft.fft(d, axis=1) / np.sqrt(M)
    num = np.zeros((N, M), complex)
    for r in range(n_rx):
        y = h[r][None, :] * D + np.sqrt(s2 / 2) * (rng.standard_normal((N, M)) + 1j * rng.standard_normal((N, M)))
        num += y * np.conj(h[r])[None, :]
    z, nu, w, _ = mm.mmse(num, np.tile(P, (N, 1)), s2)
    assert np.allclose(nu, nu[0]) and 0 < nu[0] < 1
    nu = float(nu[0])
    e = mm.predecode(z) / (1 - nu) - d
    var, want = (np.abs(e) ** 2).mean(0), nu / (1 - nu)
    q = 1 / (P + s2)
    c = np.abs(q * P - (1 - nu)) ** 2 + s2 * q * q * P  # residual interference and noise per sub-carrier
    assert np.isclose(c.mean(), nu * (1 - nu), rtol=1e-9)
    per_sample, pooled = 5 / np.sqrt(N), 5 * np.sqrt((c ** 2).sum()) / c.sum() / np.sqrt(N)
    print("%d antennas at %g dB: nu %.4g, variance %.5g against %.5g, worst sample off by %.3g (bound %.3g), mean by %.3g (bound %.3g); zero forcing %.4g"
          % (n_rx, snr_db, nu, var.mean(), want, np.abs(var / want - 1).max(), per_sample, abs(var.mean() / want - 1), pooled, s2 / mm.zf(num[:12], np.tile(P, (12, 1)))[1][0]))
    assert np.abs(var / want - 1).max() < per_sample
    assert abs(var.mean() / want - 1) < pooled
    assert s2 * (1 / P).mean() > want * (1 + 10 * pooled)  # (zero forcing's sigma2 / rho_s lies above it, by more than the estimate's spread)


def test_degenerate_inputs():
    """Zero grids (s2 = 0: q infinite, nu not a number), P = 0 with s2 > 0 (nu = 1), s2 = 0 on a live channel (nu = 0): w = 0, t = 0 and
    all-zero bytes; a dead antenna adds nothing to numerator and P and halves s2."""
    M = 72
    zero = np.zeros((12, M))
    for P, s2 in ((zero, 0.0), (zero, 0.3), (zero + 1.2, 0.0), (zero + 1.2, np.nan), (zero + 1.2, np.inf)):
        z, nu, w, rho_tap = mm.mmse(zero + 0j, P, s2)
        t, w = mm.tw(mm.predecode(z), nu, w)
        assert not w.any() and not t.any(), (P[0, 0], s2, nu)
    assert (mm.mmse(zero + 0j, zero, 0.3)[1].astype(np.float32) == 1.0).all()
    x = (np.random.default_rng(1).standard_normal((12, M)) * (1 + 1j)).astype(np.complex64)
    for nu in (0.0, 1.0, -0.5, 1.5, np.nan, np.inf):
        out = mm.demap(x, np.full(12, nu, np.float32), 2, 0x1234, 8.0)
        assert not out.bytes.any(), nu
    assert mm.demap(x, np.full(12, 0.4, np.float32), 2, 0x1234, 8.0).bytes.any()
    k = (6, 2, 3, 2)
    c = mm.case(*k)
    live = mm.taps([c.planes[0]], c.al, c.dmrs)
    dead = mm.taps([c.planes[0], np.zeros_like(c.planes[0])], c.al, c.dmrs)
    assert np.isclose(dead["s2"], live["s2"] / 2, rtol=1e-12) and np.array_equal(dead["P"], live["P"])
    both = mm.taps([np.zeros_like(c.planes[0])] * 2, c.al, c.dmrs)
    assert both["s2"] == 0 and not both["w"].any()


def test_gpu_cases_are_not_vacuous():
    """What the GPU tests' caps rest on.  Every two-path case has nu_s between 0.05 and 0.9 on every symbol (graded LLRs, no clamp at
    either end), and nu_s spans more than a factor of two over the table.  On the flat planes P varies by float rounding alone, and the two
    float64 models -- MMSE, and zero forcing under the noise-referenced gain -- give byte streams that differ in no byte."""
    lo, hi = 1.0, 0.0
    for k in ALL_KEYS:
        nu = mm.expected(k)["nu"]
        assert (nu > 0.05).all() and (nu < 0.9).all(), (k, nu)
        lo, hi = min(lo, nu.min()), max(hi, nu.max())
    print("nu_s over the GPU cases: %.3g .. %.3g" % (lo, hi))
    assert hi >= 2 * lo
    for n_rx, keys in FLAT_KEYS.items():
        for k in keys:
            c, t = mm.flat_case(*k), mm.expected(k, flat=True)
            assert t["P"].max() / t["P"].min() - 1 < 1e-6 and 0.05 < t["nu"].min() and t["nu"].max() < 0.9
            scale = 8.0
            a = mm.demap(t["x"].astype(np.complex64), t["nu"].astype(np.float32), k[3], c.c_init, scale)
            b = pm.demap(t["x_zf"].astype(np.complex64), t["rho_zf"].astype(np.float32), k[3], c.c_init, gain=nm.gain(scale, np.float32(t["s2"])))
            print("flat %s: %d bytes, %d differ, %d distinct values" % (k, len(a.bytes), (a.bytes != b.bytes).sum(), len(np.unique(a.bytes))))
            assert (a.bytes == b.bytes).all() and len(np.unique(a.bytes)) > 32, k


# ---- the generator

def _cell25():
    import openlte_amd as m
    return m.DlCfg(512, 25, 1, 0), m.UlCfg(3, 0, 0, 2, 1)


def test_one_path_is_the_payload_generator():
    import openlte_amd as m
    from openlte_amd import synth
    cfg, ul = _cell25()
    allocs = [m.make_alloc(0, 2, 1000, list(range(2, 12)), 0x77), m.make_alloc(0, 1, 120, list(range(3, 5)), 0x78)]
    pl = np.random.default_rng(3).integers(0, 2, (2, 1, 1000), dtype=np.uint8)
    kw = dict(payload=pl, snr_db=12.0, seed=9, max_delay=3)
    want, _ = synth.ul_units_3gpp(cfg, ul, [2, 7], [11, 11], allocs, 1, **kw)
    for amps in ([1.0], [3.7]):
        got, tx = synth.ul_units_3gpp(cfg, ul, [2, 7], [11, 11], allocs, 1, paths=([0], amps), **kw)
        assert got.tobytes() == want.tobytes() and (tx == pl).all()
    two, _ = synth.ul_units_3gpp(cfg, ul, [2, 7], [11, 11], allocs, 1, paths=([0, 4], [1.0, 0.5]), **kw)
    assert two.tobytes() != want.tobytes() and np.abs(two.astype(int)).max() <= 127


def test_generator_refusals():
    import openlte_amd as m
    from openlte_amd import synth
    cfg, ul = _cell25()
    al = (m.PdschAlloc * 1)(m.make_alloc(0, 1, 120, [3, 4], 0x78))
    pl, iq = np.zeros(120, np.uint8), np.zeros((synth.ul_unit_len(512), 2), np.int8)
    ch = synth.SynthChannel(1.0, 1.0, 0.0, 20.0, 100.0, 1)
    sf, cell = np.array([1], np.uint32), np.array([5], np.uint32)

    def call(paths):
        return synth._lib().mi_lte_synth_ul_units_3gpp_paths_i8(C.byref(cfg), C.byref(ul), 1, sf, cell, C.cast(al, C.c_void_p), 1, C.byref(ch), None, None,
                                                                None, None, 0, pl.ctypes.data, 120, paths, iq)

    def P(n, delays, amps):
        return C.byref(synth.SynthPaths(n, (C.c_uint32 * 4)(*delays), (C.c_double * 4)(*amps)))

    assert call(P(2, [0, 4, 0, 0], [1, 0.5, 0, 0])) == 0 and call(P(4, [0, 1, 2, 3], [1, 1, 1, 1])) == 0 and call(P(2, [0, 3, 0, 0], [0, 1, 0, 0])) == 0
    bad = [P(0, [0] * 4, [1] * 4), P(5, [0] * 4, [1] * 4), P(2, [1, 4, 0, 0], [1, 1, 0, 0]), P(2, [0, 4, 0, 0], [1, -0.5, 0, 0]),
           P(2, [0, 4, 0, 0], [1, float("nan"), 0, 0]), P(2, [0, 4, 0, 0], [float("inf"), 1, 0, 0]), P(2, [0, 4, 0, 0], [0, 0, 1, 1]), None]
    for k, p in enumerate(bad):
        assert call(p) == -1, k
    with pytest.raises(ValueError):
        synth.ul_units_3gpp(cfg, ul, [1], [5], [al[0]], 1, paths=([0] * 5, [1] * 5))


def test_two_path_capture_has_the_ripple():
    """A noiseless capture through paths 0 and d = 4 samples with amplitudes 1 and a = 0.5 (N 512, 20 PRB): the DFT of the DMRS symbol over
    the DMRS is |1 + a e^{i phi} e^{-2 pi i k d / N}|^2 up to a factor -- of the delays 1 .. 8 a mean and a sinusoid of period N / d fit
    it best for d = 4, and sqrt(min / max) is (1 - a) / (1 + a) within the int8 quantisation (uniform noise of 1 / 12 per component and
    sample: sqrt(N / 6) per bin, five of them on either extreme)."""
    import openlte_amd as m
    from openlte_amd import synth
    cfg, ul = _cell25()
    N, n_prb, a, d, sf, cell = 512, 20, 0.5, 4, 4, 21
    al = m.make_alloc(0, 2, 1000, list(range(3, 3 + n_prb)), 0x91)
    iq, _ = synth.ul_units_3gpp(cfg, ul, [sf], [cell], [al], 1, paths=([0, d], [1.0, a]), snr_db=300.0, gain=(1.0, 1.0), max_delay=0, seed=4)
    x = iq[0, :, 0].astype(np.float64) + 1j * iq[0, :, 1].astype(np.float64)
    start = 40 + 3 * N + 3 * 36  # DMRS symbol 3 of slot 0: cyclic prefixes 40, 36, 36, 36 at N = 512
    sym = x[start:start + N] * np.exp(-1j * np.pi * np.arange(N) / N)  # (the half-sub-carrier shift)
    Y = np.fft.fft(sym)
    cols = 36 + np.arange(12 * n_prb)  # grid columns of PRB 3 ..
    bins = (N - 150 + cols) % N
    r = m.ul_dmrs_pusch(ul, cell, sf, n_prb)
    H = Y[bins] / (r[0].astype(np.float64) + 1j * r[1].astype(np.float64))
    p = np.abs(H) ** 2
    k = np.arange(len(p))
    res = {}
    for dd in range(1, 9):
        A = np.stack([np.ones(len(p)), np.cos(2 * np.pi * k * dd / N), np.sin(2 * np.pi * k * dd / N)], 1)
        res[dd] = float(np.linalg.norm(p - A @ np.linalg.lstsq(A, p, rcond=None)[0]) / np.linalg.norm(p))
    print("ripple fit residual per delay: %s" % {k_: round(v, 4) for k_, v in res.items()})
    assert min(res, key=res.get) == d and res[d] < 0.02 and all(v > 3 * res[d] for dd, v in res.items() if dd != d)
    amp = np.abs(H)
    ratio, tol = amp.min() / amp.max(), 2 * 5 * np.sqrt(N / 6) / amp.max()
    print("sqrt(min / max) %.4f against %.4f, tolerance %.4f" % (ratio, (1 - a) / (1 + a), tol))
    assert abs(ratio - (1 - a) / (1 + a)) <= tol and tol < 0.1  # (a flat channel would give 1)
