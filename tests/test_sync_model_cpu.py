"""The float64 model of the synchronisation searches (tests/sync_model.py) against what is known without a GPU: the reference's recorded
verdicts on the golden capture, the cells the synthetic captures of tests/sync_cases.py were built around, the standard's tables, and the
branches the decision-edge cases were built to reach.  The float32 restatements' distance from the model -- the floors the GPU test's tight
gates are eight times of -- is printed per family (run with -s)."""
import os

import numpy as np
import pytest

import sync_cases as sc
import sync_model as sm

FOUND = [c.name for c in sc.case_list() if c.find]


def test_golden_verdicts_equal_the_reference():
    """tests/golden/sync_ref.npz: a 1.4 MHz int8 capture and what the reference's three searches returned for it over 160 slots"""
    g = np.load(os.path.join(os.path.dirname(__file__), "golden", "sync_ref.npz"), allow_pickle=False)
    fft, n_rb = int(g["cfg"][0]), int(g["cfg"][1])
    x = g["iq"][:, 0].astype(np.float64) + 1j * g["iq"][:, 1].astype(np.float64)
    r = sm.search(x, fft, n_rb, 160)
    n = int(g["n_peaks"])
    assert r.coarse.n_peaks == n and r.coarse.symb_starts[:n].tolist() == g["symb_starts"][:n].tolist()
    # the sums are exact integers; what is left is numpy's arctan2 against atan2f, an ulp of a quotient summed over 160 slots
    assert np.abs(r.freq_offset - g["freq_offset"][:n]).max() <= 1e-6 * np.abs(g["freq_offset"][:n]).max()
    for p, pk in enumerate(r.peaks):
        assert [pk.n_id_2, pk.pss_symb] + pk.symb_starts.tolist() == g["pss"][p].tolist()
        assert abs(pk.pss_thresh - g["pss_thresh"][p]) <= 1e-4 * g["pss_thresh"][p]
        assert [int(pk.found), pk.n_id_1, pk.frame_start] == g["sss"][p].tolist()


@pytest.mark.parametrize("name", FOUND)
def test_model_finds_every_cell(name):
    c = sc.by_name(name)
    found = sm.cells_found(sc.expected(name))
    assert sc.cell_hits(c, found), (c.cells, found)


def test_standard_tables():
    """36.211 table 6.11.2.1-1 at its corners, the SSS's construction, the PSS's symmetry and constant modulus"""
    # (the table's rows of equal m1 - m0 = 1 .. 7 hold 30, 29, 28, 27, 26, 25 and 3 identities)
    assert [sm.sss_m0_m1(i) for i in (0, 1, 29, 30, 58, 59, 87, 100, 114, 165, 167)] == [(0, 1), (1, 2), (29, 30), (0, 2), (28, 30), (0, 3), (0, 4), (13, 17),
                                                                                        (0, 5), (0, 7), (2, 9)]
    seen = set()
    for k in range(3):
        d = sm.pss_seq(k)
        assert np.allclose(np.abs(d), 1) and np.allclose(d, d[::-1])  # d_u(n) = d_u(61 - n)
        for i in range(168):
            d0, d5 = sm.sss_seq(i, k)
            assert set(np.unique(d0)) | set(np.unique(d5)) <= {-1.0, 1.0}
            seen |= {d0.tobytes(), d5.tobytes()}
    assert len(seen) == 1008  # all different
    # the reference (and the library after it) takes cosf / sinf of the phase rounded to float: half an ulp of 6600 rad
    for k in range(3):
        assert np.abs(np.angle(sc.lib_pss(k).astype(np.complex128) * np.conj(sm.pss_seq(k)))).max() <= 2.45e-4


def test_sss_family_has_its_unique_maximum_at_the_sent_index():
    corr, amp = sc.sss_family_model()
    m = np.abs(corr)
    want = np.array([2 * i + h for i, k, h in sc.SSS_CASES])
    assert (m.argmax(1) == want).all()
    assert np.abs(m.max(1) / (62 * amp) - 1).max() <= 1e-9
    assert (np.sort(m, 1)[:, -2] < 0.6 * m.max(1)).all()  # unique, and far below 0.9 of it
    symb5 = sc.sss_family()[2]
    for n in range(0, len(sc.SSS_CASES), 7):  # the first-above-threshold rule finds the same one at pss_thresh = the maximum
        ss = np.zeros(7, np.uint32)
        ss[5] = symb5[n]
        found, n_id_1, _, _ = sm.sss_decide(corr[n], np.float32(m[n].max()), ss, sc.SYM_FFT)
        assert found and n_id_1 == sc.SSS_CASES[n][0]


def test_pss_family_is_found_at_its_root_shift_and_offset():
    for k, sft in sc.PSS_CASES:
        i, q, ss = sc.pss_family(k, sft)
        p = sm.pss_stage(i.astype(np.float64) + 1j * q.astype(np.float64), sc.SYM_FFT, sc.SYM_RB, ss)
        assert (p.n_id_2, p.shift, p.pss_symb, p.timing) == (k, sft, 7 * sc.PSS_SLOT + sc.PSS_SYMB, 1)
        m = np.sort(np.abs(p.fine_corr))
        assert m[-2] < 0.7 * m[-1]


@pytest.mark.parametrize("name", list(sc.EDGES))
def test_edge_cases_reach_their_branch(name):
    c, r = sc.by_name(name), sc.expected(name).coarse
    window, walk, wrapped = c.edge
    assert r.n_peaks >= 1 and (r.peaks[0], r.walk[0], r.wrapped[0]) == (window, walk, wrapped)
    N, _, cpe, n_slot, _ = sm.geom(c.fft)
    assert 0 < int(r.symb_starts[0][0]) <= N + cpe
    if window == 0:  # a peak at window 0 is not blanked itself (the walk never starts, the blanking begins a symbol later): every round finds it again
        assert r.n_peaks == 5 and r.peaks == [0] * 5


def test_other_decision_edges():
    for name in ("d_silence_i8", "d_silence_f32"):
        r = sc.expected(name)
        assert r.coarse.n_peaks == 0 and r.coarse.survivors == 0 and r.coarse.mean == 0 and not r.peaks and not r.acc.any()
    r = sc.expected("d_const")
    assert r.acc.min() == r.acc.max() == 243 == r.coarse.mean and r.coarse.survivors == 0 and r.coarse.n_peaks == 0  # '<=': equal to the mean is gated
    r = sc.expected("d_few").coarse
    assert r.survivors == 4 and r.n_peaks == 2 and sorted(r.peaks) == [392, 401]  # one window before and one after each cancelling pair
    r = sc.expected("d_two_cells")
    hits = [cell for cell, _ in sm.cells_found(r)]
    assert 150 in hits and 341 in hits and len(set(r.coarse.peaks)) == 5  # a second peak survives the blanking and yields the other cell
    r = sc.expected("b_gauss").coarse
    assert r.n_peaks == 5 and max(r.wrapped) > 0  # a later peak within n_blank / 2 of the grid's origin


def test_threshold_straddle_in_the_model():
    """family f: the sent SSS stands 2 % above 0.9 pss_thresh, and 2 % below it"""
    corr, _ = sc.sss_family_model()
    symb5 = sc.sss_family()[2]
    for n in (0, 501, 1007):
        peak = float(sm.mag32(corr[n]).max())
        ss = np.zeros(7, np.uint32)
        ss[5] = symb5[n]
        assert sm.sss_decide(corr[n], np.float32(peak / (0.9 * 0.98)), ss, sc.SYM_FFT)[0] is False
        found, n_id_1, _, _ = sm.sss_decide(corr[n], np.float32(peak / (0.9 * 1.02)), ss, sc.SYM_FFT)
        assert found and n_id_1 == sc.SSS_CASES[n][0]


def test_fine_timing_tie_in_the_model():
    """family f: offsets +1 and +2 tie to 1e-8 with the sent table (and to 1e-5 only with the standard's: sm.pss_stage)"""
    table = [sc.lib_pss(k) for k in range(3)]
    for k, sft in sc.PSS_CASES:
        i, q, ss = sc.pss_family(k, sft, True)
        x = i.astype(np.float64) + 1j * q.astype(np.float64)
        p = sm.pss_stage(x, sc.SYM_FFT, sc.SYM_RB, ss, table)
        m = np.abs(p.fine_corr)
        order = np.argsort(m)[::-1]
        assert sorted(order[:2] - 40) == [1, 2] and (m[order[0]] - m[order[1]]) <= 1e-8 * m[order[0]] and m[order[2]] < 0.5 * m[order[0]]
        assert (p.n_id_2, p.shift, p.pss_symb) == (k, sft, 7 * sc.PSS_SLOT + sc.PSS_SYMB)
        q2 = sm.pss_stage(x, sc.SYM_FFT, sc.SYM_RB, ss)
        m2 = np.sort(np.abs(q2.fine_corr))
        assert 1e-7 * m2[-1] < m2[-1] - m2[-2] < 1e-4 * m2[-1]


def test_restatement_floors_per_family():
    """What float32 in the reference's order costs against the model, per family: the GPU test's tight gates are 8 x these, case by case.
    Integer samples: the cyclic-prefix sums are exact (144 * 2 * 127^2 < 2^24)."""
    worst = {}
    for c in sc.case_list():
        if c.name[0] == "a" and c.start:
            continue  # (the same samples as the start-0 case)
        b, e = sc.build(c.name), sc.expected(c.name)
        corr32, acc32 = sc.restated(c.name)
        f = worst.setdefault(c.name[0], dict(corr=0.0, acc=0.0, rows=0.0, pss=0.0, sss=0.0))
        f["corr"] = max(f["corr"], float(sm.rel_l2(corr32, e.corr).max()))
        f["acc"] = max(f["acc"], float(sm.rel_l2(acc32, e.acc)))
        if c.fmt == "i8":
            assert (corr32 == e.corr.astype(np.complex64)).all() and (e.corr == np.round(e.corr)).all()
        for p in e.peaks[:1]:
            wins = sm.pss_windows(p.symb_starts_in, c.fft)
            f["rows"] = max(f["rows"], sc.rows_floor(b, c.fft, c.n_rb, wins, p.rows))
            seqs, z0 = sc.pss_candidates_f32(c.n_rb)
            f["pss"] = max(f["pss"], float(sm.rel_l2(sm.seq_corr_f32(p.rows.real, p.rows.imag, seqs, z0), p.corr).max()))
            seqs, z0 = sc.sss_candidates_f32(p.n_id_2, c.n_rb)
            f["sss"] = max(f["sss"], float(sm.rel_l2(sm.seq_corr_f32(p.sss_row.real, p.sss_row.imag, seqs, z0), p.sss_corr).max()))
    for fam, f in sorted(worst.items()):
        print("family %s: corr %.3g  acc %.3g  rows (stockham_f32) %.3g  PSS correlations %.3g  SSS correlations %.3g" % (fam, f["corr"], f["acc"], f["rows"],
                                                                                                                          f["pss"], f["sss"]))
        assert f["corr"] <= sc.TOL_CORR / sc.GATE_FACTOR and f["acc"] <= sc.TOL_CORR / sc.GATE_FACTOR and f["rows"] <= sc.TOL_SYMB / sc.GATE_FACTOR
        assert f["pss"] <= sc.TOL_PSS / 2 and f["sss"] <= sc.TOL_SEQ / sc.GATE_FACTOR  # (the PSS table's rounding is most of TOL_PSS by construction)
