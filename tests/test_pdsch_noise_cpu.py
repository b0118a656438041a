"""CPU: the downlink CRS noise estimate as include/mi_lte.h states it (tests/pdsch_noise_model.py, the float64 restatement the GPU test holds
k_dl_crs_noise to): unbiased on a constant channel, the spread the header quotes, what a timing offset leaves, the pilot geometry against the
library's own CRS mapper (mi_lte_map_crs, pinned to the reference in tests/test_cabi.py), and the host side of the new entry points.  No GPU."""
import ctypes as C

import numpy as np
import pytest

import pdsch_noise_model as nm
from fuzz_cases import BANDWIDTHS

ERR_INVALID = -1
N_SC = 1200


def crs_planes(n_rb, n_ant, sf, cell, h):
    """float64 [2, 16, 1200]: the y planes of a subframe that holds nothing but the CRS of ports 0 .. min(n_ant, 2) - 1, port p through the
    complex gain h[p] -- placed with the model's own positions and values (test_geometry_against_the_transmitter pins those)"""
    y = np.zeros((16, N_SC), complex)
    for p, i in nm.rows(n_ant):
        y[nm.SYMBOLS[i], nm.pilots(n_rb, cell, p, i)] = h[p] * nm.crs(n_rb, cell, sf, nm.SYMBOLS[i])
    return y


def with_noise(rng, y, s2):
    w = np.sqrt(s2 / 2) * (rng.standard_normal(y.shape) + 1j * rng.standard_normal(y.shape))
    return np.stack([(y + w).real, (y + w).imag])


@pytest.mark.parametrize("n_ant", [1, 2])
@pytest.mark.parametrize("n_rb", [6, 100])
def test_unbiased_and_spread(n_rb, n_ant):
    """A constant channel per port (gain 0.5 .. 1.5, random phase) plus white noise of known variance, 300 seeded draws (cells, subframes and
    variances drawn too): the mean of sigma2_hat / sigma2 lies within 4 standard errors of 1, the standard error from the draws themselves.
    Prints the measured relative standard deviation next to 1.36 / sqrt(n_rows (n_pil - 2)).  Measured (the formula's value in brackets): 6 RB 0.225 (0.215) on
    one port, 0.152 (0.152) on two; 100 RB 0.0462 (0.0483) and 0.0360 (0.0342)."""
    rng = np.random.default_rng(4000 + 10 * n_rb + n_ant)
    n_draws, ratio = 300, []
    for _ in range(n_draws):
        sf, cell, s2 = int(rng.integers(0, 10)), int(rng.integers(0, 504)), float(10 ** rng.uniform(-3, 0))
        h = rng.uniform(0.5, 1.5, 2) * np.exp(2j * np.pi * rng.random(2))
        planes = with_noise(rng, crs_planes(n_rb, n_ant, sf, cell, h), s2)
        ratio.append(nm.sigma2(planes, n_rb, n_ant, sf, cell) / s2)
    ratio = np.array(ratio)
    sd = ratio.std(ddof=1)
    se = sd / np.sqrt(n_draws)
    n_terms = len(nm.rows(n_ant)) * (2 * n_rb - 2)
    print("%3d RB, %d port(s): mean ratio %.4f (standard error %.4f), relative standard deviation %.4f, 1.36 / sqrt(%d) = %.4f"
          % (n_rb, n_ant, ratio.mean(), se, sd, n_terms, 1.36 / np.sqrt(n_terms)))
    assert abs(ratio.mean() - 1) <= 4 * se, (ratio.mean(), se)


def test_linear_phase():
    """Noise-free, unit gain, a delay of 4 samples at N_fft = 2048: every second difference is (2 cos theta - 2) t with theta = 2 pi 6 Delta / N_fft,
    so sigma2_hat = (2 - 2 cos theta)^2 / 6 = 4.894e-6, to 1e-3 relative (it holds to rounding)."""
    theta = 2 * np.pi * 6 * 4 / 2048
    want = (2 - 2 * np.cos(theta)) ** 2 / 6
    assert abs(want - 4.894e-6) <= 1e-3 * want
    ramp = np.exp(-2j * np.pi * 4 * np.arange(N_SC) / 2048)[None, :]
    for n_rb, n_ant in ((100, 1), (100, 2), (25, 2), (6, 1)):
        y = crs_planes(n_rb, n_ant, 3, 77, [1.0, 1.0]) * ramp
        got = nm.sigma2(np.stack([y.real, y.imag]), n_rb, n_ant, 3, 77)
        print("%3d RB, %d port(s): sigma2 %.6g, (2 - 2 cos theta)^2 / 6 = %.6g" % (n_rb, n_ant, got, want))
        assert abs(got - want) <= 1e-3 * want, (n_rb, n_ant, got, want)


@pytest.mark.parametrize("fft,n_rb", [(fft, n_rb) for _, fft, n_rb in BANDWIDTHS])
def test_geometry_against_the_transmitter(fft, n_rb):
    """mi_lte_map_crs on an empty grid of a two-port cell, every bandwidth, N_id_cell of every residue mod 6 (cells 0 and 503 among them),
    subframes 0 and 9: on port p's grid the model's least-squares product is 1 at every pilot of port p's rows and 0 on the other port's rows
    (that port is silent there), and sigma2 of either grid alone (one port) and of their sum (two ports) is below 1e-12.  This pins k_j, the
    bit index and the slot arithmetic."""
    import openlte_amd as m
    L = m.load_library()
    re, im = np.zeros((4, 16, N_SC), np.float32), np.zeros((4, 16, N_SC), np.float32)
    for cell in (0, 1, 2, 303, 250, 503):
        for sf in (0, 9):
            re[:], im[:] = 0, 0
            assert L.mi_lte_map_crs(n_rb, 12, sf, cell, 2, re, im) == 0
            assert np.count_nonzero(re[0, :14]) == np.count_nonzero(re[1, :14]) == 4 * 2 * n_rb
            for p in (0, 1):
                t = nm.t_ls(np.stack([re[p], im[p]]), n_rb, 2, sf, cell)
                assert t.shape == (8, 2 * n_rb)
                assert np.abs(t[4 * p:4 * p + 4] - 1).max() <= 1e-6, (cell, sf, p)
                assert not t[4 * (1 - p):4 * (1 - p) + 4].any(), (cell, sf, p)
            assert nm.sigma2(np.stack([re[0], im[0]]), n_rb, 1, sf, cell) < 1e-12
            assert nm.sigma2(np.stack([re[0] + re[1], im[0] + im[1]]), n_rb, 2, sf, cell) < 1e-12
    assert sorted(c % 6 for c in (0, 1, 2, 303, 250, 503)) == list(range(6))


def test_gain_rules():
    """(float)(scale / (float)sigma2); 0 for sigma2 0, infinite or NaN and for a quotient past float."""
    assert nm.gain(8.0, np.float32(0.5)) == 16.0
    assert nm.gain(8.0, 0.0) == 0.0 and nm.gain(8.0, np.inf) == 0.0 and nm.gain(8.0, np.nan) == 0.0
    assert nm.gain(1e30, 1e-30) == 0.0
    assert nm.gain(3.0, np.float32(0.1)) == float(np.float32(3.0 / np.float64(np.float32(0.1))))


def test_host_refusals_and_exports():
    """The three new symbols are exported; a NULL plan is refused by both plan calls, and NULL arguments by the standalone run, before
    anything touches a device."""
    import openlte_amd as m
    L = m.load_library()
    for name in ("mi_lte_dl_crs_noise_run", "mi_lte_pdsch_plan_set_llr_noise", "mi_lte_pdsch_plan_llr_noise"):
        assert hasattr(L, name), name
    p, n = C.c_void_p(), C.c_uint32()
    assert L.mi_lte_pdsch_plan_set_llr_noise(None, 8.0) == ERR_INVALID
    assert L.mi_lte_pdsch_plan_set_llr_noise(None, 0.0) == ERR_INVALID
    assert L.mi_lte_pdsch_plan_llr_noise(None, C.byref(p), C.byref(n)) == ERR_INVALID
    cfg = m.DlCfg(2048, 100, 1, 0)
    assert L.mi_lte_dl_crs_noise_run(None, C.byref(cfg), None, None, None, 1, None) == ERR_INVALID
