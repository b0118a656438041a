"""CPU: the model of the 3GPP plans' max-log soft-decision demapper (tests/demap_llr_model.py, MI_LTE_DEMAP_MAXLOG in include/mi_lte.h).  Its
piecewise-linear route is the brute-force minimum over the whole 2-D constellation; noiseless points demap to their own bits with the least
reliable one at +-T under the automatic gain; the guard band the GPU tests allow a one-step difference in stays under 1 % of the soft bits on
inputs like theirs; header, exports and the Python constants move together."""
import os
import re

import numpy as np
import pytest

import demap_llr_model as dm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_header_exports_and_constants_agree():
    import openlte_amd as m
    txt = open(os.path.join(ROOT, "include", "mi_lte.h")).read()
    L = m.load_library()
    for name in ("mi_lte_pdsch_plan_set_demapper", "mi_lte_pdsch_plan_llr_gain"):
        assert re.search(r"\bint\s+%s\(" % name, txt), name
        assert hasattr(L, name), name
    defs = {k: int(v) for k, v in re.findall(r"#define\s+MI_LTE_(DEMAP_\w+)\s+(\d+)u?\b", txt)}
    assert defs == {"DEMAP_REF": m.DEMAP_REF, "DEMAP_MAXLOG": m.DEMAP_MAXLOG, "DEMAP_AUTO_T": m.DEMAP_AUTO_T}
    assert (m.DEMAP_REF, m.DEMAP_MAXLOG) == (0, 1) and 1 <= m.DEMAP_AUTO_T <= 127
    # refusals that need no device: a NULL plan
    assert L.mi_lte_pdsch_plan_set_demapper(None, m.DEMAP_MAXLOG, 0.0) == -1
    assert L.mi_lte_pdsch_plan_llr_gain(None, None) == -1


def test_constellations_are_36211():
    """The first rows of 36.211 Tables 7.1.2-1, 7.1.3-1 and 7.1.4-1 (bit string b(i) b(i+1) .. -> I, Q in units of A), the average power, and the
    Gray property the per-axis LLR rests on."""
    rows = {1: {"00": (1, 1), "01": (1, -1), "10": (-1, 1), "11": (-1, -1)},
            2: {"0000": (1, 1), "0001": (1, 3), "0010": (3, 1), "0011": (3, 3), "0100": (1, -1), "1000": (-1, 1), "1011": (-3, 3), "1111": (-3, -3)},
            3: {"000000": (3, 3), "000001": (3, 1), "000010": (1, 3), "000011": (1, 1), "000100": (3, 5), "000101": (3, 7), "000110": (1, 5),
                "000111": (1, 7), "001000": (5, 3), "001100": (5, 5), "001111": (7, 7), "010000": (3, -3), "100000": (-3, 3), "111111": (-7, -7)}}
    for mod in (1, 2, 3):
        pts, labels = dm.constellation(mod)
        assert abs((np.abs(pts) ** 2).mean() - 1) < 1e-12
        for bits, (i, q) in rows[mod].items():
            k = int(bits, 2)
            assert "".join(map(str, labels[k])) == bits
            assert abs(pts[k] - dm.A[mod] * complex(i, q)) < 1e-12, (mod, bits)


@pytest.mark.parametrize("mod", [1, 2, 3])
def test_piecewise_route_is_the_brute_force_minimum(mod):
    """On a grid of x that holds the constellation points, every decision boundary (the even multiples of A, 0 included) and points past the
    outermost level, at several channel powers: the model's route through z and w equals w (min_S1 |x - s|^2 - min_S0 |x - s|^2) over the full
    constellation."""
    A = dm.A[mod]
    axis = np.concatenate([A * np.arange(-10, 10.01, 0.25), A * (np.arange(-8, 9, 2) + 1e-9), A * (np.arange(-8, 9, 2) - 1e-9)])
    x = (axis[:, None] + 1j * axis[None, :]).reshape(-1)
    for h in (1.0 + 0j, 0.3 - 0.4j, -1.7 + 2.2j, 1e-3j):
        hv = np.full(len(x), h)
        got = dm.llr_symbols(x * hv, hv, mod)
        want = dm.brute_llr(x, np.abs(hv) ** 2, mod)
        assert np.abs(got - want).max() <= 1e-12 * (1 + np.abs(want).max()), (mod, h)


@pytest.mark.parametrize("mod", [1, 2, 3])
def test_noiseless_points(mod):
    """Every constellation point through a flat channel: sign(L_k) is the transmitted bit (positive: 0), and under the automatic gain the least
    reliable bit of every point sits on +-T."""
    pts, labels = dm.constellation(mod)
    for h in (1.0 + 0j, 0.6 - 1.1j):
        hv = np.full(len(pts), h)
        lam = dm.llr_symbols(pts * hv, hv, mod)
        assert ((lam < 0) == (labels == 1)).all() and (lam != 0).all()
        for T in (8, 16, 48):
            g, g_exact = dm.auto_gain(np.abs(hv) ** 2, mod, T)
            assert abs(g - g_exact) <= 2.0 ** -24 * g_exact
            assert np.abs(np.abs(g_exact * lam).min(1) - T).max() < 1e-9, (mod, T)
            assert (np.abs(dm.soft_byte(g * lam)).min(1) == T).all()


def test_rounding_clamp_and_degenerate_values():
    x = np.array([0.5, 1.5, 2.5, -0.5, -1.5, 126.5, 127.4, 127.6, 1e9, -1e9, np.inf, -np.inf, np.nan, 0.0])
    assert list(dm.soft_byte(x)) == [0, 2, 2, 0, -2, 126, 127, 127, 127, -127, 0, 0, 0, 0]
    assert dm.auto_gain(np.zeros(12), 3, 16) == (0.0, 0.0) and dm.auto_gain(np.array([1.0, np.inf]), 2, 16) == (0.0, 0.0)
    assert dm.auto_gain(np.array([1.0, np.nan]), 1, 16) == (0.0, 0.0) and dm.auto_gain(np.full(4, 1e-45), 3, 16) == (0.0, 0.0)
    # w = 0 on one element: zeros for it, whatever y is (finite)
    y, h = np.array([0.3 - 2j, 1 + 1j]), np.array([0j, 1 + 0j])
    for mod in (1, 2, 3):
        lam = dm.llr_symbols(y, h, mod)
        assert (lam[0] == 0).all() and (lam[1] != 0).all()


def synthetic_unit(rng, snr_db):
    """Planes like the front end's for the GPU tests' inputs: an estimate whose power varies over the band and the symbols (two taps up to
    4 samples apart, gains 0.5 .. 1.5), unit-power symbols of the three modulations, noise at snr_db."""
    k = np.arange(dm.N_SC)[None, :]
    sym = np.arange(16)[:, None]
    g0, g1 = rng.uniform(0.5, 1.5, 2) * np.exp(2j * np.pi * rng.random(2))
    h = g0 + g1 * np.exp(-2j * np.pi * (k - 600) * 4 / 2048) * np.exp(0.02j * sym)
    planes = np.zeros((4, 16, dm.N_SC), np.float32)
    mod_of = rng.integers(1, 4, (16, dm.N_SC))
    s = np.zeros((16, dm.N_SC), complex)
    for mod in (1, 2, 3):
        pts, _ = dm.constellation(mod)
        s = np.where(mod_of == mod, pts[rng.integers(0, len(pts), s.shape)], s)
    sigma = 10 ** (-snr_db / 20) * np.sqrt((np.abs(h) ** 2).mean() / 2)
    y = h * s + sigma * (rng.standard_normal(s.shape) + 1j * rng.standard_normal(s.shape))
    planes[0], planes[1], planes[2], planes[3] = y.real, y.imag, h.real, h.imag
    return planes


@pytest.mark.parametrize("snr_db", [20.0, 5.0])
def test_guard_band_is_under_one_percent(snr_db):
    """The allocations of tests/test_demap_llr_gpu.py's 25-RB case over synthetic planes at both of its noise levels, automatic and fixed gain:
    fewer than 1 % of the soft bits lie within 2^-16 (1 + |g L|) of a rounding or clamp boundary, and the clamp is reached."""
    import openlte_amd as m
    rng = np.random.default_rng(int(snr_db))
    allocs = [m.make_alloc(0, 1, 1000, [8, 9, 10], 0x11), m.make_alloc(0, 2, 1000, [11, 12, 13], 0x12, n_pdcch_symbs=3),
              m.make_alloc(0, 3, 1000, [14, 15, 16, 17], 0x13)]
    for sf in (0, 5, 3):
        planes = synthetic_unit(rng, snr_db)
        for gain in (0.0, 40.0):
            res = dm.demap(planes, allocs, sf, 77, 25, 1, gain=gain, T=m.DEMAP_AUTO_T)
            x = np.concatenate([r.x for r in res])
            assert len(x) > 4000
            frac = dm.in_guard(x).mean()
            assert frac < 0.01, (sf, gain, frac)
            assert (np.abs(np.concatenate([r.bytes for r in res])) == 127).any()
            assert all((gain == 0 and r.gain > 0) or r.gain == gain for r in res)


def test_resource_element_counts():
    """pdsch_res: 12 symbols x 12 sub-carriers less 6 CRS positions per PRB outside subframes 0 / 5; the 6 + 6 split next to the 25-RB window."""
    import openlte_amd as m
    al = m.make_alloc(0, 1, 1000, [9, 15, 12, 0], 0x11)
    n3, n0, n5 = (len(dm.pdsch_res(al, sf, 3, 25, 2)) for sf in (3, 0, 5))
    assert n3 == 4 * 138
    # subframe 5: symbols 5 and 6 lose PRB 12 whole and half of PRBs 9 and 15; subframe 0: symbols 7-10 as well (symbol 7 holds 2 CRS per PRB)
    assert n5 == n3 - 2 * 24 and n0 == n5 - (3 * 24 + 20)
    from test_ulsch_uci_cpu import gold  # (36.211 7.2 bit by bit)
    for c_init in (0x12345, 0x7FFFFFFF, (0x101 << 14) | (5 << 9) | 301):
        assert (dm.gold(c_init, 3000) == gold(c_init, 3000)).all()
