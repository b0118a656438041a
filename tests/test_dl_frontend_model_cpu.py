"""CPU: the float64 front-end model (dl_frontend_model.py) against the port oracle on every unit of dl_frontend_cases.case_list -- symbol
rows, every port's 14-symbol estimates and the oracle's frequency-direction rows -- the coverage the list promises, the condition that no
wrap decision of a listed unit lies within 0.05 rad of +-pi, the tie family's condition, and the floors the GPU file's tight gates use.

Measured here, over the 247 downlink units of 121 cases and the 20 uplink units (least / median / worst, where the worst occurred):
  the oracle against the model
    symbol rows rel-L2         worst 3.57e-8 at rb20/1 (the float32 rounding of a float64 transform's output)
    estimates rel-L2           1.17e-7 / 1.65e-6 / 6.13e-5 at c4_15_rb100/0 (four ports, 100 RB, the steep ramp: one float32 ulp of the
                               370 rad a 59-turn unwrap reaches is 3e-5 rad, and the serial rule adds its turns one rounding at a time)
    estimates elementwise      5.16e-7 / 9.73e-6 / 2.88e-4 of |h| at c4_15_rb100/0
    magnitude rows rel-L2      6.43e-8 / 9.54e-8 / 1.34e-7 at rb6_fft512/1
    phase rows                 3.29e-7 / 6.57e-6 / 2.41e-4 rad at f32_2048_kilo/0
  the float32 radix-2 Stockham restatement against numpy's float64 FFT
    downlink symbol rows       7.0e-8 / 1.09e-7 / 1.31e-7 at rb80/0
    uplink rows                9.42e-8 / 1.23e-7 / 1.36e-7 at ul_1024_rb85/1
  least distance of a wrap decision from +-pi: 0.690 rad at f32_128_kilo/0 (the steep ramp at N = 128: steps of 2.06 rad plus noise)
  tie family: the guess from raw neighbours fails the reference's link test on 19 of 80 units
These are the floors of test_dl_frontend_model_gpu.py's tight gates (8 x, per unit and quantity); test_floors prints them again.

The coverage list asks for a partly filled last lane in the classes C = 2 and C = 3 of the wave-parallel unwrap.  With C = 2 the pilot
count 2 N_rb_dl is even, so the last populated lane is always full: the test asserts it for C = 3 (65 RB: 130 = 43 x 3 + 1) and C = 4
(97 RB: 194 = 48 x 4 + 2), and for C = 2 that the list holds sizes with fewer than 64 populated lanes and the one with exactly 64."""
import numpy as np
import pytest

import dl_frontend_cases as dc
import dl_frontend_model as dm


def all_dl_units():
    return [(c, k) for c in dc.dl_cases() for k in range(len(c.units))]


def test_case_list_is_deterministic_and_admissible():
    names = [c.name for c in dc.case_list()]
    assert len(set(names)) == len(names)
    for c in dc.case_list():
        assert c.fft in dc.FFTS and 6 <= c.n_rb <= 100 and 12 * c.n_rb < c.fft and c.n_ant in (1, 2, 4)
        assert sorted(c.order) == list(range(len(c.units)))
        for u in c.units:
            assert 0 <= u.sf <= 9 and 0 <= u.cell <= 503 and 0 <= u.d < dm.geom(c.fft)[1]


def test_coverage_of_bandwidths():
    dl = dc.dl_cases()
    for n_rb in range(6, 101):
        assert any(c.n_rb == n_rb and c.fft == dc.smallest_fft(n_rb) for c in dl), n_rb
    for fft, top in zip(dc.FFTS, (10, 21, 42, 85, 100)):
        assert dc.largest_rb(fft) == top
        for n_rb in (6, top):
            assert any(c.fft == fft and c.n_rb == n_rb for c in dl), (fft, n_rb)
            assert any(c.fft == fft and c.n_rb == n_rb for c in dc.ul_cases()), (fft, n_rb)


def test_coverage_of_ports_shifts_and_lane_classes():
    seen = {C: set() for C in (1, 2, 3, 4)}
    for c in dc.dl_cases():
        for u in c.units:
            seen[dc.lanes_class(c.n_rb)].add((c.n_ant, u.cell % 6))
    for C in seen:
        assert seen[C] == set(dc.PAIRS), (C, sorted(set(dc.PAIRS) - seen[C]))
    # a last populated lane that is only partly filled: 2 N_rb_dl is no multiple of C.  C = 2 cannot have one (2 N_rb_dl is even), so there
    # the nearest property is asserted: lanes past the last populated one stay empty (fewer than 64 populated)
    rbs = {C: {c.n_rb for c in dc.dl_cases() if dc.lanes_class(c.n_rb) == C} for C in (2, 3, 4)}
    assert any((2 * n) % 3 for n in rbs[3]) and 65 in rbs[3]
    assert any((2 * n) % 4 for n in rbs[4])
    assert any(n < 64 for n in rbs[2]) and 64 in rbs[2]  # (C = 2: 2 N_rb_dl / 2 = N_rb_dl populated lanes)


def test_coverage_of_subframes_cells_delays_formats_and_batches():
    dl = dc.dl_cases()
    for n_ant in (1, 2, 4):
        sfs = {u.sf for c in dl if c.n_ant == n_ant for u in c.units}
        assert {0, 9} <= sfs, n_ant
        assert any(u.d == 0 for c in dl if c.n_ant == n_ant for u in c.units)
        assert any(u.d == 100 for c in dl if c.n_ant == n_ant and c.n_rb == 100 and c.fft == 2048 for u in c.units), n_ant
    assert {u.sf for c in dl for u in c.units} == set(range(10))
    assert {0, 503} <= {u.cell for c in dl for u in c.units}
    f32 = [c for c in dl if c.fmt == "f32"]
    assert {(c.fft == 2048, c.scale) for c in f32} == {(True, 1e-3), (True, 1e3), (False, 1e-3), (False, 1e3)}
    for c in f32:  # non-integer samples
        buf, _ = dc.samples(c.name)
        x = buf[0].astype(np.float64) / c.scale
        assert np.abs(x - np.rint(x)).max() > 0.4
    assert any(c.all_rows and c.n_ant == 1 for c in dl) and any(c.all_rows and c.n_ant == 2 for c in dl)
    b = dc.by_name("batch_1024")
    _, starts = dc.samples(b.name)
    assert len(b.units) >= 4 and len({(u.sf, u.cell) for u in b.units}) == len(b.units)
    assert not (np.diff(starts.astype(np.int64)) > 0).all() and (starts % 2 == 1).any()
    odd = sum(int(dc.samples(c.name)[1][k]) % 2 for c in dl[:20] for k in range(len(c.units)))
    assert odd > 0


def test_steep_ramp_has_40_wraps_at_100_rb():
    """the model's own unwrapped phase of port 0, symbol 0: at least 40 turns from the first to the last sub-carrier, and every step between
    neighbouring pilots short of pi by more than the margin (that is the 0.05 rad condition, asserted for all units below)"""
    for name in ("c4_3_rb100", "c4_7_rb100", "c4_15_rb100"):
        c = dc.by_name(name)
        assert c.n_rb == 100 and c.units[0].d == 100
        a = dc.expected(name, 0).ang[0][0]
        assert abs(a[-1] - a[0]) / (2 * np.pi) >= 40, (name, abs(a[-1] - a[0]) / (2 * np.pi))
    assert {dc.by_name(n).n_ant for n in ("c4_3_rb100", "c4_7_rb100", "c4_15_rb100")} == {1, 2, 4}


def test_every_wrap_decision_is_clear_of_pi():
    worst = (np.pi, None)
    for c, k in all_dl_units():
        m = dc.expected(c.name, k).margin
        if m < worst[0]:
            worst = (m, (c.name, k))
        assert m >= dc.MARGIN, (c.name, k, m)
    print("least distance of a wrap decision from +-pi: %.3f rad at %s" % worst)


def test_model_against_the_oracle():
    """Symbol rows to 1e-6 rel-L2 (the oracle rounds a float64 transform to float32: ~4e-8); estimates to the project's hard gates; the
    frequency-direction rows: magnitude rows to 1e-5 rel-L2, phase rows to 1e-3 rad absolute (64 float32 ulp of 100 rad; a wrong wrap is
    6.28)."""
    worst = {"symb": (0, None), "ce_l2": (0, None), "ce_el": (0, None), "mag_l2": (0, None), "ang": (0, None)}
    for c, k in all_dl_units():
        e, o = dc.expected(c.name, k), dc.oracle(c.name, k)
        s = float(dc.rel_l2_rows(o.symb, e.symb).max())
        f = dict(dc.floors(c.name, k), symb=s)
        for q in worst:
            if f[q] > worst[q][0]:
                worst[q] = (f[q], (c.name, k))
        assert s < 1e-6 and f["ce_l2"] < dc.TOL_CE and f["ce_el"] < dc.TOL_EL and f["mag_l2"] < 1e-5 and f["ang"] < 1e-3, (c.name, k, f)
    for q, (v, where) in worst.items():
        print("oracle against model, %-6s worst %.3g at %s" % (q, v, where))


def test_uplink_model_against_a_direct_dft():
    """the uplink rows are the odd bins of a 2 N-point transform of the zero-padded samples (the reference's formulation)"""
    c = dc.by_name("ul_128_rb6")
    i, q = dc.unit_iq(c.name, 1)
    x = i.astype(np.float64) + 1j * q.astype(np.float64)
    rows = dc.expected(c.name, 1).symb
    for s in (0, 6, 13):
        w = dm.window_start(128, s)
        X = np.fft.fft(np.concatenate([x[w:w + 128], np.zeros(128)]))[1::2]
        assert np.allclose(rows[s], np.concatenate([X[128 - 36:], X[:36]]), rtol=0, atol=1e-9 * np.abs(X).max())


def test_floors():
    """the floors of the GPU file's tight gates: printed, and checked to lie inside the hard gates with the factor applied somewhere"""
    sym, ce, el, mg, an = [], [], [], [], []
    for c, k in all_dl_units():
        f = dc.floors(c.name, k)
        sym.append((f["symb"], c.name, k)); ce.append((f["ce_l2"], c.name, k)); el.append((f["ce_el"], c.name, k))
        mg.append((f["mag_l2"], c.name, k)); an.append((f["ang"], c.name, k))
    ul = [(dc.symb_floor(c.name, k), c.name, k) for c in dc.ul_cases() for k in range(len(c.units))]
    for what, v in (("symbol rows (float32 Stockham)", sym), ("uplink rows (float32 Stockham)", ul), ("estimates rel-L2", ce),
                    ("estimates elementwise", el), ("magnitude rows rel-L2", mg), ("phase rows rad", an)):
        print("floor, %-32s least %.3g at %s/%d, median %.3g, worst %.3g at %s/%d"
              % ((what,) + min(v) + (float(np.median([x[0] for x in v])),) + max(v)))
    assert dc.GATE_FACTOR * max(sym)[0] < dc.TOL_SYMB and dc.GATE_FACTOR * max(ul)[0] < dc.TOL_SYMB
    assert min(sym)[0] > 1e-8 and min(ce)[0] > 1e-8


def test_forced_decision_moves_one_link_by_a_turn():
    c = dc.by_name("rb50")
    i, q = dc.unit_iq(c.name, 0)
    x = i.astype(np.float64) + 1j * q.astype(np.float64)
    u = c.units[0]
    a = dm.dl_frontend(x, c.fft, c.n_rb, c.n_ant, u.sf, u.cell)
    b = dm.dl_frontend(x, c.fft, c.n_rb, c.n_ant, u.sf, u.cell, forced=((0, 1, 40, 1),))
    off = dm.pilot_offset(0, 1, u.cell)
    d = b.ang[0] - a.ang[0]
    assert np.abs(d[[0, 2, 3, 4]]).max() == 0 and np.abs(d[1, :6 * 39 + off + 1]).max() == 0
    assert np.allclose(d[1, 6 * 40 + off:], 2 * np.pi)
    far = np.ones(12 * c.n_rb, bool)
    far[6 * 39 + off + 1:6 * 40 + off] = False
    assert np.abs(b.ce[0][:, far] - a.ce[0][:, far]).max() < 1e-9 * np.abs(a.ce[0]).max()


def test_tie_family_condition():
    """At least 64 single-port units, each CRS symbol used, the swept step finer than the float spacing of the unwrapped phase in front of
    the link -- and on at least 8 units the guess from raw neighbours does not verify against the serial rule, so that an implementation
    that guesses must fall back there.  Away from the swept link every wrap decision keeps the 0.05 rad margin."""
    assert dc.TIE_UNITS >= 64 and {dc.tie_unit(u)[0] for u in range(dc.TIE_UNITS)} == {0, 1, 2, 3, 4}
    spacing = float(np.spacing(np.float32(dc.TIE_THETA * (dc.TIE_J - 1))))
    assert dc.TIE_EPS_STEP < spacing and dc.TIE_THETA * (dc.TIE_J - 1) / (2 * np.pi) > 30
    n_bad, n_differ = 0, 0
    for u in range(dc.TIE_UNITS):
        i_star = dc.tie_unit(u)[0]
        a, _ = dc.tie_expected(u)
        mf = [m.copy() for m in a.margin_f]
        assert mf[0][i_star, dc.TIE_J - 1] < 1e-4  # the swept link itself
        mf[0][i_star, dc.TIE_J - 1] = np.pi
        assert min(float(mf[0].min()), float(a.margin_t[0].min())) >= dc.MARGIN, u
        serial, guessed, ok = dc.tie_routes(dc.tie_raw_phases(u))
        n_bad += not ok
        n_differ += serial.tobytes() != guessed.tobytes()
    print("tie family: the guess fails verification on %d of %d units, its values differ from the serial route's on %d" % (n_bad, dc.TIE_UNITS, n_differ))
    assert n_bad >= 8
