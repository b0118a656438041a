"""CPU tests of the PHICH path: the float64 model of tests/phich_model.py against the library's transmitter (pinned to the reference) and
against itself without noise, the host arithmetic of phich_geom.cc (group count, 36.213 9.1.2 resource mapping, the plan's index table)
over its whole argument range, the margins of the GPU test's parameter sets, and the host file under the address and undefined-behaviour
sanitizers as a stand-alone program.  No GPU."""
import ctypes as C
from fractions import Fraction
import math
import os
import shutil
import subprocess

import numpy as np
import pytest

import phich_cases as pc
import phich_model as pm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BANDWIDTHS = [6, 15, 25, 50, 75, 100]
N_GS = [Fraction(1, 6), Fraction(1, 2), Fraction(1), Fraction(2)]


@pytest.mark.parametrize("n_rb", BANDWIDTHS)
def test_model_modulator_equals_the_librarys_transmitter_on_one_port(n_rb):
    """One port: what the model's modulator puts on symbol 0 at the PHICH elements is the grid mi_lte_pdcch_channel_encode writes (that
    transmitter is pinned to the reference), to float32 rounding; the model's REG positions and the library's index table are
    mi_lte_ctrl_reg_positions'.  Every N_g, cells of the three k mod 3 shifts, subframes 0 and 9."""
    import openlte_amd as m
    L = m.load_library()
    rng = np.random.default_rng(n_rb)
    for n_g in N_GS:
        n_grp = pm.n_group(n_rb, n_g)
        for cell, sf in ((0, 0), (151, 9), (302, 0), (503, 9)):
            present, hi = pm.random_pattern(rng, 1, n_grp)
            t = m.Transmitter(pc.FFT[n_rb], n_rb, cell)
            _, ph, _ = t.control(sf, 2, n_grp, present[0], hi[0])
            grid = (t.re[0, 0].astype(np.float64) + 1j * t.im[0, 0]).copy()
            t.close()
            s = pm.scramble_signs(sf, cell)
            table = m.phich_re_table(n_rb, cell, float(n_g))
            assert table.shape == (n_grp, 12) and ph.N_reg == 3 * n_grp
            k4, n4, n_reg, kk = np.zeros(4, np.uint32), np.zeros(4, np.float32), C.c_uint32(), np.zeros(75, np.uint32)
            assert L.mi_lte_ctrl_reg_positions(n_rb, cell, C.c_float(float(n_g)), k4.ctypes.data_as(C.POINTER(C.c_uint32)), n4.ctypes.data_as(C.POINTER(C.c_float)),
                                               C.byref(n_reg), kk.ctypes.data_as(C.POINTER(C.c_uint32))) == 0
            assert n_reg.value == 3 * n_grp
            for g in range(n_grp):
                k = pm.group_res(n_rb, cell, g)
                assert [6 * n for n in pm.group_regs(n_rb, cell, g)] == list(kk[3 * g:3 * g + 3]) == list(ph.k[3 * g:3 * g + 3])
                assert k == list(table[g]) and all(x % 3 != cell % 3 for x in k) and k == sorted(k[0:4]) + sorted(k[4:8]) + sorted(k[8:12])
                want = pm.modulate_group(1, g, present[0, g], hi[0, g], s)[0]
                # float32 rounding: up to eight terms added per component, every partial sum below 8, half an ulp (2^-24 x 8) per addition
                assert np.abs(grid[k] - want).max() <= 8 * 8 * 2.0 ** -24 * math.sqrt(2.0), (n_rb, n_g, cell, sf, g)


def _wrong_pair(n_ant, i, m):
    return (0, 1) if n_ant == 2 else (0, 2)


@pytest.mark.parametrize("n_ant", [1, 2, 4])
def test_noiseless_round_trip(n_ant):
    """Flat per-port gains, no noise, true estimates: a present indicator gives metric -1 (ACK) or +1 (NACK) and an absent one 0, to 1e-12,
    with random patterns and all eight sequences in one group.  The (0, 2) pairing for every quadruplet of a 4-port cell -- the PDSCH
    habit, not 36.211 6.9.2 -- must fail the same check."""
    rng = np.random.default_rng(40 + n_ant)
    worst, worst_wrong = 0.0, 0.0
    for n_rb, n_g in ((6, Fraction(2)), (25, Fraction(1)), (100, Fraction(2))):
        n_grp = pm.n_group(n_rb, n_g)
        cells, sfs = [7, 200, 503], [0, 9, 4]
        present, hi = pm.random_pattern(rng, 3, n_grp)
        sub = pm.modulate(n_rb, n_ant, cells, sfs, present, hi, rng, snr_db=None, flat=True, dtype=np.float64)
        want = np.where(present == 1, 1.0 - 2.0 * hi, 0.0)
        for u in range(3):
            metric, power, rep, dec = pm.decode(n_rb, n_ant, n_grp, cells[u], sfs[u], sub[u])
            worst = max(worst, np.abs(metric - want[u]).max())
            assert np.array_equal(dec[present[u] == 1], hi[u][present[u] == 1])
            if n_ant == 4:
                worst_wrong = max(worst_wrong, np.abs(pm.decode(n_rb, 4, n_grp, cells[u], sfs[u], sub[u], pair=_wrong_pair)[0] - want[u]).max())
    assert worst <= 1e-12
    if n_ant == 4:
        assert worst_wrong > 0.1, "the test does not see the alternation of 36.211 6.9.2"


def test_group_count():
    """mi_lte_phich_n_group on the 6 x 4 standard combinations: ceil(N_g N_rb / 8) in exact rationals and N_reg / 3 of
    mi_lte_ctrl_reg_positions; 0 for what is not standard."""
    import openlte_amd as m
    L = m.load_library()
    for n_rb in BANDWIDTHS:
        for n_g in N_GS:
            n = m.phich_n_group(n_rb, float(n_g))
            assert n == math.ceil(n_g * n_rb / 8) == pm.n_group(n_rb, n_g), (n_rb, n_g)
            k4, n4, n_reg, kk = np.zeros(4, np.uint32), np.zeros(4, np.float32), C.c_uint32(), np.zeros(75, np.uint32)
            assert L.mi_lte_ctrl_reg_positions(n_rb, 17, C.c_float(float(n_g)), k4.ctypes.data_as(C.POINTER(C.c_uint32)), n4.ctypes.data_as(C.POINTER(C.c_float)),
                                               C.byref(n_reg), kk.ctypes.data_as(C.POINTER(C.c_uint32))) == 0
            assert n_reg.value == 3 * n
    for n_rb, n_g in ((7, 1.0), (0, 1.0), (110, 1.0), (25, 0.0), (25, -1.0), (25, 2.5), (25, float("nan")), (25, float("inf"))):
        assert m.phich_n_group(n_rb, n_g) == 0, (n_rb, n_g)


def test_resource_mapping():
    """mi_lte_phich_resource over its whole argument range against 36.213 9.1.2 (N_SF = 4), and its refusals."""
    import openlte_amd as m
    L = m.load_library()
    g, s = C.c_uint32(), C.c_uint32()
    for n_grp in range(1, 26):
        for i_phich in (0, 1):
            for n_dmrs in range(8):
                for i_prb in range(110):
                    assert L.mi_lte_phich_resource(i_prb, n_dmrs, n_grp, i_phich, C.byref(g), C.byref(s)) == 0
                    assert (g.value, s.value) == ((i_prb + n_dmrs) % n_grp + i_phich * n_grp, (i_prb // n_grp + n_dmrs) % 8)
    assert m.phich_resource(0xFFFFFFFF, 7, 1, 1) == (1, (0xFFFFFFFF + 7) % 8)  # no wrap in 32 bits
    g.value, s.value = 77, 78
    assert L.mi_lte_phich_resource(5, 3, 0, 0, C.byref(g), C.byref(s)) == -1 and L.mi_lte_phich_resource(5, 8, 4, 0, C.byref(g), C.byref(s)) == -1
    assert L.mi_lte_phich_resource(5, 3, 4, 0, None, C.byref(s)) == -1 and L.mi_lte_phich_resource(5, 3, 4, 0, C.byref(g), None) == -1
    assert (g.value, s.value) == (77, 78)
    with pytest.raises(m.MiLteError):
        m.phich_resource(5, 8, 4)
    with pytest.raises(m.MiLteError):
        m.phich_re_table(25, 504, 1.0)
    with pytest.raises(m.MiLteError):
        m.phich_re_table(26, 0, 1.0)


@pytest.mark.parametrize("case", pc.CASES, ids=pc.case_id)
def test_case_margins(case):
    """Every parameter set of the GPU test: the model's |metric| is at least 0.5 on every present indicator and its decision is the
    indicator sent, so the GPU test's comparison of hard decisions leaves nothing out; the case has cells of all three shifts, a cell
    where the PCFICH moves some but not all of a group's REG numbers, subframes 0 and 9, and all eight sequences in one group."""
    present, hi, sub, model = pc.make(case)
    n_grp = pm.n_group(case["n_rb"], case["n_g"])
    assert present.shape == (len(case["cells"]), n_grp, 8) and sub.shape == (len(case["cells"]), 2 + 2 * case["n_ant"], 16, pm.N_SC)
    assert {c % 3 for c in case["cells"]} == {0, 1, 2} and {0, 9} <= set(case["sfs"]) and present[0, 0].all()
    moved = [[a != b for g in range(n_grp) for a, b in zip(pm.group_regs(case["n_rb"], c, g, raw=True), pm.group_regs(case["n_rb"], c, g))] for c in case["cells"]]
    assert any(any(x) and not all(x) for x in moved)
    for u, (metric, power, rep, dec) in enumerate(model):
        on = present[u] == 1
        assert np.abs(metric[on]).min() >= 0.5, np.abs(metric[on]).min()
        assert np.array_equal(dec[on], hi[u][on])
        assert (power > 0).all()


def test_host_arithmetic_under_address_and_undefined_behaviour_sanitizers():
    """tools/asan/run_phich_host.sh: phich_geom.cc (with pdcch_geom.cc, whose REG numbering it calls) built with g++
    -fsanitize=address,undefined into a program of its own and driven over the host functions' whole argument ranges, the refused ones
    included: no report, no failed check.  CPU build only."""
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    r = subprocess.run(["bash", os.path.join(ROOT, "tools", "asan", "run_phich_host.sh")], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "phich host driver:" in r.stdout and " 0 failures" in r.stdout and "ERROR" not in r.stderr and "runtime error" not in r.stderr, \
        (r.stdout + r.stderr)[-3000:]
