"""CPU: the PRACH detector's float64 model (prach_model) and the cases of test_prach_model_gpu.py (prach_model_cases), with the library's host
functions only.  The model is anchored to the reference -- its verdicts on the stored captures equal the ones the compiled reference
recorded -- and not to the kernels; the float32 restatement of the kernels' plan stays inside the hard gates on every case; and the
conditions on the inputs that let the GPU test demand equal arg-maxima and verdicts on every case, leaving none out, hold."""
import os

import numpy as np
import pytest

import lte_testdata as td
import prach_model as pm
import prach_model_cases as pcs


@pytest.mark.parametrize("name", list(td.PRACH_CASES))
def test_model_verdicts_equal_the_reference_s_recorded_ones(name):
    z = np.load(os.path.join(os.path.dirname(__file__), "golden", "prach_ref.npz"))
    fft, nrb, root, fmt, zczc, hs, fo = td.PRACH_CASES[name][:7]
    u = pcs.root_list((root, fmt, zczc, hs, fo))
    g = pm.Geom(fft, nrb, fmt, fo)
    iq = z[name + "_iq"]
    x = iq[..., 0].astype(np.float64) + 1j * iq[..., 1].astype(np.float64)
    _, _, stats = pm.model(x, g, pm.spectra_complex(pm.root_spectra(u, g.N_zc), g.N_zc))
    N_cs, v_max = pm.sets(u[0], zczc, hs, fmt)
    got = pm.verdict(stats, N_cs, v_max, g.N_zc)
    assert (got == z[name + "_det"]).all(), (got.tolist(), z[name + "_det"].tolist())


def test_geometry_and_sets_equal_the_library_s():
    """Geom's occasion length against the transmitter's (mi_lte_synth_prach_len = T_cp + reps T_fft + the delay room, in 16s), the root
    count against N_cs / v_max: 64 preambles need ceil(64 / (v_max + 1)) roots of an unrestricted set"""
    import openlte_amd as m
    L = m.load_library()
    for fft in pcs.N_RB:
        for fmt in range(5):
            g = pm.Geom(fft, pcs.N_RB[fft], fmt, 0)
            reps = 2 if fmt in (2, 3) else 1
            assert L.mi_lte_synth_prach_len(fft, fmt) == (g.T_cp + reps * g.T_fft + 1024 * fft // 2048 + 15) // 16 * 16
    for fmt, zs in ((0, range(16)), (4, range(7))):
        for zczc in zs:
            u = pcs.root_list((3, fmt, zczc, 0, 0))
            N_cs, v_max = pm.sets(u[0], zczc, 0, fmt)
            assert len(u) == -(-64 // (v_max + 1)), (fmt, zczc)


def test_packing_gives_odd_starts_and_a_foreign_sample_in_front():
    for c in pcs.all_cases().values():
        assert (c.occ_start % 2 == 1).all() and len(set(c.occ_start.tolist())) == len(c.occ_start)
        assert int(c.occ_start[-1]) + c.g.occasion_samples <= len(c.re) == len(c.im)
        assert (np.diff(c.occ_start.astype(np.int64)) >= c.g.occasion_samples).all()


def test_cases_cover_what_they_are_meant_to():
    cs = pcs.all_cases()
    assert {(c.g.N2, c.g.P) for c in cs.values()} == {(n, p) for n in (64, 128, 256, 512, 1024) for p in (24, 4)}
    assert {c.pc[1] for c in cs.values()} == {0, 1, 2, 3, 4}
    assert {len(c.u) for c in pcs.group("roots_own")} == {1, 64, 5} and any(c.pc[3] for c in pcs.group("roots_own"))
    assert {c.fft for c in pcs.group("float")} == {128, 2048} and all(c.is_float and np.abs(c.re - np.round(c.re)).max() > 0.4 for c in pcs.group("float"))
    assert len([c for c in cs.values() if c.fft in (128, 2048) and c.group in ("shape0", "shape4", "formats", "offsets", "roots_own", "roots_given")]) == len(pcs.group("float"))
    for c in pcs.group("offsets"):  # the kept bins at the other end of the carrier: km takes both ends of 0 .. N2 - 1 or the index wraps
        assert c.pc[4] == c.n_rb - 6 and c.g.start != pm.Geom(c.fft, c.n_rb, c.pc[1], 0).start
    km = np.concatenate([c.g.bin_index() & (c.g.N2 - 1) for c in cs.values() if c.fft in (128, 2048)])
    assert km.min() == 0 and km.max() == 1023
    for c in pcs.group("peaks"):  # the crafted peaks stand where they were put
        want = np.array(pcs.bluestein_offsets(c.pc[1]))
        assert (pcs.expected(c.name).stats[2][:, 0] == want).all()
        assert {0, 1, c.g.N_zc - 2, c.g.N_zc - 1} <= set(want.tolist())


def test_tie_case_has_exact_ties_in_the_model():
    c, = pcs.group("ties")
    e = pcs.expected(c.name)
    assert (e.power[:, 0] == e.power[:, 2]).all() and (e.power[:, 1] == 0).all() and (e.power[:, 0].max(-1) > 0).all()
    assert (e.stats[2][:, 1] == 0).all() and (e.verdict[:2, 0] == 1).all()
    # the lower of the two equal roots carries the verdict: its preamble index is below v_max + 1
    assert (e.verdict[:2, 1] <= c.v_max).all(), e.verdict.tolist()


def test_straddle_cases_straddle():
    for c in pcs.group("straddle"):
        e = pcs.expected(c.name)
        assert abs(e.ratio[0] - 1.02) <= 0.005 and abs(e.ratio[1] - 0.98) <= 0.005, e.ratio
        assert tuple(e.verdict[:, 0]) == c.detect == (1, 0)
    assert {c.fft for c in pcs.group("straddle")} == {128, 512}


def test_zero_cases_are_refused_by_the_model():
    for c in pcs.group("zeros"):
        e = pcs.expected(c.name)
        assert (e.power == 0).all() and (e.verdict == 0).all()


def test_float32_restatement_stays_inside_the_hard_gates():
    worst = np.zeros(4)
    at = [None] * 4
    for name in pcs.all_cases():
        fl = pcs.expected(name).floor
        for i in range(4):
            if fl[i] > worst[i]:
                worst[i], at[i] = fl[i], name
        assert fl[0] < pcs.TOL_L2 and fl[1] < pcs.TOL_EL and fl[2] < pcs.TOL_L2 and fl[3] < pcs.TOL_EL, (name, fl)
    gt = pcs.gates()
    print("float32 restatement, worst: x_hat rel-L2 %.3g at %s, elementwise / RMS %.3g at %s; power rel-L2 %.3g at %s, elementwise / max %.3g at %s"
          % (worst[0], at[0], worst[1], at[1], worst[2], at[2], worst[3], at[3]))
    print("tight gates: %.3g %.3g %.3g %.3g" % gt)
    assert all(abs(gt[i] - 8.0 * worst[i]) <= 1e-12 * gt[i] for i in range(4))  # none of the four is capped: they lie inside the hard gates
    assert gt[0] < pcs.TOL_L2 and gt[1] < pcs.TOL_EL and gt[2] < pcs.TOL_L2 and gt[3] < pcs.TOL_EL


def test_float32_restatement_finds_the_model_s_maxima_and_verdicts():
    for name, c in pcs.all_cases().items():
        e = pcs.expected(name)
        assert (e.floor_stats[2] == e.stats[2]).all(), name
        assert (pm.verdict(e.floor_stats, c.N_cs, c.v_max, c.g.N_zc) == e.verdict).all(), name


def test_conditions_on_the_inputs():
    """What lets the GPU test be strict on every case: the largest power of every (occasion, root) profile stands more than 1e-4 relative
    above the runner-up (ties: in the live rows), and max / (50 ave) is outside [0.9, 1.1] everywhere but in the straddle pairs.  A seed that
    violates one is changed; the conditions are not."""
    for name, c in pcs.all_cases().items():
        e = pcs.expected(name)
        if c.kind == "zeros":
            continue
        p = np.sort(e.power, axis=-1)
        top, second = p[..., -1], p[..., -2]
        live = top > 0
        assert live.all() or c.kind == "tie"
        assert (top[live] - second[live] > 1e-4 * top[live]).all(), (name, float(((top[live] - second[live]) / top[live]).min()))
        if c.kind != "straddle":
            assert ((e.ratio < 0.9) | (e.ratio > 1.1)).all(), (name, e.ratio.tolist())
