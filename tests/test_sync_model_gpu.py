"""GPU: the synchronisation searches of sync.hip (k_cp_corr, k_cp_accum, k_sync_fft, k_seq_corr and the host decisions behind them) against the
float64 model of tests/sync_model.py on the cases of tests/sync_cases.py, through the taps for tests (mi_lte_coarse_timing_tap,
mi_lte_find_pss_tap, mi_lte_find_sss_tap: the same device part as the _run entries, what the kernels wrote copied out, no verdicts).

What is asserted, per case:
  corr, acc, k_seq_corr's sums   bit-identical to the float32 restatement in the reference's serial order (sync.hip's header: "each in the
                                 reference's own summation order"), both sample formats, fractional floats included; k_seq_corr restated on
                                 the device's own rows and the library's host PSS table, so neither the transform's rounding nor libm enters
  the same against the model     rel-L2 per slot row / per correlation set under gate(floor, hard) = min(8 x the restatement's own deviation
                                 on the same case, hard); integer samples: corr EQUAL to the model
  rows against the model         TOL_SYMB hard, 8 x dl_frontend_cases.stockham_f32's floor tight, at odd and even window starts
  the _run entries               every output equal to the model's decision function applied to the tapped arrays (pss_thresh bit for bit;
                                 the coarse freq_offset within 8 x the float32 restatement's distance from float64: numpy's arctan2 is not atan2f)
  families d, e, f               through the _run entries: every cell found, every verdict as the MODEL's own; the exact tie of family f is the
                                 one place where the one-sample alternative of test_sync_gpu.compare is accepted
  output buffers                 pre-filled with NAN_BITS: every documented element written, nothing else touched (FFT 128, 256, 1024: part-filled
                                 and tail blocks of k_cp_corr)

"Reads exactly as far as the reference": argued, not probed.  k_cp_corr stages samples b0 + k and b0 + k + N for k < n_win + cp with
n_win = min(1024, n_slot - i0): the last block of the last slot reads up to start + N_slots n_slot + cp - 1 + N, the reference's last idx + N
(:5737) and less than mi_lte_coarse_timing_samples.  k_cp_accum and k_seq_corr read what the stage before them wrote.

Measured on the MI355X (rel-L2 against the model, worst over the cases; floor = the float32 restatement's own distance on the worst case,
tight gate = 8 x floor, never wider than the hard gate):
  quantity                          device      floor       tight gate   hard gate
  corr, fractional floats           2.41e-07    2.41e-07    1.93e-06     1e-5   (bit-identical to the restatement on every case)
  corr, int8                        0           0           0            --     (equal to the model)
  acc                               3.19e-07    3.19e-07    2.55e-06     1e-5   (bit-identical to the restatement)
  rows, PSS pass (84 per call)      1.43e-07    1.50e-07    1.20e-06     1e-5   (floor: dl_frontend_cases.stockham_f32)
  rows, fine pass (80 per call)     1.42e-07    1.35e-07    1.08e-06     1e-5
  rows, SSS symbol                  1.31e-07    1.12e-07    8.96e-07     1e-5
  PSS correlation sets [9]          3.0e-04     3.0e-04     1e-3 (hard)  1e-3   (the reference's float-phase PSS table against the standard's)
  fine correlation sets [80]        9.27e-05    9.27e-05    7.4e-04      1e-3
  SSS correlation sets [336]        2.12e-07    2.07e-07    1.66e-06     1e-4   (7.8e-08 on the single-symbol family)
  k_seq_corr's sums                 bit-identical to the restatement on the device's own rows in every call
  coarse freq_offset                |device - float64| at most 2.3 x |float32 restatement - float64| (gate 8 x), 5.1e-4 Hz at the worst
  fine-timing tie                   2 of 9 cases took the one-sample alternative
The header's promise holds: no exception to record.

Mutations, each tried once on a scratch copy of sync.hip (none can move an address); failing tests before = test_sync_gpu.py,
test_scan_batch_gpu.py and test_args_gpu.py (16 tests), after = this file (199 tests); details in profiles/sync_model_mutants.txt:
  mutation                                                        before   after
  k_cp_corr: neg_hi dropped                                       7        104
  k_cp_corr: a packed product's halves swapped                    7        109
  k_cp_corr: acc + t1 + t2 for acc + (t1 + t2)                    0        22    (bit identity on fractional samples alone)
  k_cp_accum: accumulation started at slot 1                      1        98
  k_seq_corr: the conjugate flipped                               0        31    (the tapped correlations alone: no verdict changes)
  gen_sss: m1 off by one                                          10       83
  gen_pss: roots 29 <-> 34                                        10       69
  blanking width halved                                           7        44
  the gate's '<=' as '<'                                          0        2     (case d_const alone: every window AT the mean)
  0.9 -> 0.95                                                     4        31
"""
import ctypes as C

import numpy as np
import pytest

import dl_frontend_model as dm
import sync_cases as sc
import sync_model as sm

pytestmark = pytest.mark.gpu

ALL = sc.names()
# (the stages behind the coarse search: every start of two shapes, start 0 of the others; not the constant capture, whose spectrum is all DC)
STAGES = [n for n in ALL if n != "d_const" and (not (n.startswith("a_") and not n.endswith("_s0")) or n.startswith("a_256") or n.startswith("a_2048_100"))]
ERR_INVALID_ARG = -1


def _cfg(c):
    import openlte_amd as m
    return m.DlCfg(c.fft, c.n_rb, 1, m.IQ_I8 if c.fmt == "i8" else m.IQ_F32_PLANAR)


class Dev:
    """device buffers of one case, uploaded once"""

    def __init__(self, ctx, name):
        self.c, self.b = sc.by_name(name), sc.build(name)
        self.cfg = _cfg(self.c)
        if self.c.fmt == "i8":
            self.a, self.q = ctx.to_device(self.b.buf), None
        else:
            self.a, self.q = ctx.to_device(self.b.buf[0]), ctx.to_device(self.b.buf[1])

    def free(self):
        self.a.free()
        if self.q is not None:
            self.q.free()


@pytest.fixture(scope="module")
def dev(ctx):
    cache = {}

    def get(name):
        if name not in cache:
            cache[name] = Dev(ctx, name)
        return cache[name]
    yield get
    for d in cache.values():
        d.free()


@pytest.fixture(scope="module")
def coarse(ctx, dev):
    """(corr, acc) of the coarse tap per case.  Cached: read-only."""
    cache = {}

    def get(name):
        if name not in cache:
            d = dev(name)
            cache[name] = ctx.coarse_timing_tap_dev(d.cfg, d.a, d.q, d.c.n_slots, start=d.c.start)
        return cache[name]
    return get


def default_starts(fft):
    """symb_starts for a case whose coarse search yields no peak: the symbols of a capture that begins on a slot"""
    N, cp0, cpe, _, _ = sm.geom(fft)
    return np.array([(cp0 - cpe) + j * (N + cpe) for j in range(7)], np.uint32)


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


# ---- the cyclic-prefix correlation and its accumulation

@pytest.mark.parametrize("name", ALL)
def test_corr_and_acc_bit_identical_to_the_restatement(coarse, name):
    corr, acc = coarse(name)
    corr32, acc32 = sc.restated(name)
    bad = np.nonzero(corr.view(np.uint32) != np.ascontiguousarray(corr32).view(np.uint32))
    assert same_bits(corr, corr32), "%d of %d sums differ, first at %s" % (len(bad[0]), corr.size * 2, [int(v[0]) for v in bad])
    assert same_bits(acc, sm.cp_accum_f32(corr)) and same_bits(acc, acc32)


@pytest.mark.parametrize("name", ALL)
def test_corr_and_acc_against_the_model(coarse, name):
    c, e = sc.by_name(name), sc.expected(name)
    corr, acc = coarse(name)
    corr32, acc32 = sc.restated(name)
    if c.fmt == "i8":
        assert (corr.astype(np.complex128) == e.corr).all()  # 144 * 2 * 127^2 < 2^24: every sum is an exact integer
    got, floor = sm.rel_l2(corr, e.corr), sm.rel_l2(corr32, e.corr)
    got_a, floor_a = float(sm.rel_l2(acc, e.acc)), float(sm.rel_l2(acc32, e.acc))
    print("%s: corr rel-L2 worst %.3g (floor %.3g, gate %.3g)  acc %.3g (floor %.3g, gate %.3g)" % (name, got.max(), floor.max(), sc.gate(floor.max(), sc.TOL_CORR),
                                                                                               got_a, floor_a, sc.gate(floor_a, sc.TOL_CORR)))
    for s in range(c.n_slots):
        assert got[s] <= sc.gate(floor[s], sc.TOL_CORR), (s, got[s], floor[s])
    assert got_a <= sc.gate(floor_a, sc.TOL_CORR)


# ---- the transform's rows and the sequence correlations

def stage_checks(ctx, d, ss, e_peak=None):
    """One PSS tap and one SSS tap at symb_starts ss: the rows against the model under the front end's gates, k_seq_corr bit-identical to its
    restatement on the device's own rows, the correlations against the model.  Returns the figures and the window parities met."""
    c, b = d.c, d.b
    n_sc = 12 * c.n_rb
    fig, parity = {}, set()
    run_ss, n2, ps, th, fo = ctx.find_pss_dev(d.cfg, d.a, d.q, ss, start=c.start)
    shift = int(round(fo / 15000.0))
    rows, corr, frows, fcorr = ctx.find_pss_tap_dev(d.cfg, d.a, d.q, ss, n2, ps, shift, start=c.start)
    seqs32, z0 = sc.pss_candidates_f32(c.n_rb)
    seqs64, _ = sm.pss_candidates(c.n_rb)
    q = 3 * n2 + shift + 1
    sets = [("pss", sm.pss_windows(ss, c.fft), rows, corr, seqs32, seqs64, z0, sc.TOL_PSS),
            ("fine", sm.fine_windows(ss, ps, c.fft), frows, fcorr[:, None], seqs32[q:q + 1], seqs64[q:q + 1], z0[q:q + 1], sc.TOL_PSS)]
    srow, scorr = ctx.find_sss_tap_dev(d.cfg, d.a, d.q, n2, run_ss, start=c.start)
    s32, sz0 = sc.sss_candidates_f32(n2, c.n_rb)
    sets.append(("sss", [sm.sss_window(run_ss, c.fft)], srow[None], scorr[None], s32, s32.astype(np.complex128), sz0, sc.TOL_SEQ))
    for what, wins, r, co, q32, q64, zz, hard in sets:
        parity |= {(c.start + w) % 2 for w in wins}
        re, im = sc.rows_f32(r, c.n_rb)
        want_rows = dm.rows_at(b.x, c.fft, c.n_rb, wins)
        live = np.abs(want_rows).sum(1) > 0  # (a window of silence: zero rows, zero correlations)
        assert not re[~live].any() and not im[~live].any() and not co[~live].any()
        assert same_bits(co, sm.seq_corr_f32(re, im, q32, zz)), what  # the header's promise, on the device's own rows
        if not live.any():
            continue
        wins_l = [w for w, l in zip(wins, live) if l]
        yr, yi = sc.stockham_rows(b, c.fft, c.n_rb, wins_l)
        stock = yr.astype(np.float64) + 1j * yi.astype(np.float64)
        floor_r = float(sm.rel_l2(stock, want_rows[live]).max())
        got_r = float(sm.rel_l2(re[live].astype(np.float64) + 1j * im[live], want_rows[live]).max())
        assert got_r <= sc.gate(floor_r, sc.TOL_SYMB), (what, got_r, floor_r)
        # a correlation SET: a row's nine PSS or 336 SSS candidates; the fine pass's 80 offsets against its one sequence
        as_set = (lambda v: v.T) if what == "fine" else (lambda v: v)
        want_c = as_set(sm.seq_corr(want_rows[live], q64, zz))
        floor_c = float(sm.rel_l2(as_set(sm.seq_corr_f32(yr, yi, q32, zz)), want_c).max())  # float32 transform, then the float32 sums
        got_c = float(sm.rel_l2(as_set(co[live]), want_c).max())
        assert got_c <= sc.gate(floor_c, hard), (what, got_c, floor_c)
        fig[what] = (got_r, floor_r, got_c, floor_c)
    return fig, parity


@pytest.mark.parametrize("name", STAGES)
def test_rows_and_sequence_correlations(ctx, dev, name):
    d, e = dev(name), sc.expected(name)
    ss = e.coarse.symb_starts[0] if e.coarse.n_peaks else default_starts(d.c.fft)
    parity = set()
    for k in (0, 1):  # every window once at an even and once at an odd sample index
        fig, p = stage_checks(ctx, d, ss + np.uint32(k))
        parity |= p
        for what, (got_r, floor_r, got_c, floor_c) in fig.items():
            print("%s +%d %-4s: rows rel-L2 %.3g (floor %.3g, gate %.3g)  correlations %.3g (floor %.3g)" % (name, k, what, got_r, floor_r,
                                                                                                           sc.gate(floor_r, sc.TOL_SYMB), got_c, floor_c))
    assert parity == {0, 1}


# ---- the _run entries: the model's decisions on the tapped arrays

def run_chain(ctx, d):
    """the scanner's sequence through the _run entries: (CoarseTiming, [(pss tuple, sss tuple)] per peak)"""
    c = d.c
    t = ctx.coarse_timing_dev(d.cfg, d.a, d.q, c.n_slots, start=c.start)
    peaks = []
    for p in range(t.n_corr_peaks):
        pss = ctx.find_pss_dev(d.cfg, d.a, d.q, list(t.symb_starts[p]), start=c.start)
        peaks.append((pss, ctx.find_sss_dev(d.cfg, d.a, d.q, pss[1], pss[0], pss[3], start=c.start)))
    return t, peaks


@pytest.mark.parametrize("name", ALL)
def test_run_outputs_equal_the_decisions_on_the_taps(ctx, dev, coarse, name):
    d = dev(name)
    c = d.c
    corr, acc = coarse(name)
    t, peaks = run_chain(ctx, d)
    w = sm.coarse_decide(acc, c.fft)
    assert t.n_corr_peaks == w.n_peaks
    assert np.array([list(t.symb_starts[i]) for i in range(5)], np.uint32).tolist() == w.symb_starts.tolist()
    if w.n_peaks:
        pk = corr[:, w.peaks].T
        f32, f64 = sm.coarse_freq(pk, c.fft), sm.coarse_freq(pk, c.fft, single=False)
        got = np.array(list(t.freq_offset), np.float32)[:w.n_peaks]
        floor, err = float(np.abs(f32 - f64).max()), float(np.abs(got - f64).max())
        print("%s: freq_offset |device - float64| %.3g, |float32 restatement - float64| %.3g" % (name, err, floor))
        assert err <= sc.GATE_FACTOR * floor
    assert list(t.freq_offset)[w.n_peaks:] == [0.0] * (5 - w.n_peaks)
    found = []
    for p, ((ss, n2, ps, th, fo), (ok, n1, fs, ss2)) in enumerate(peaks):
        ss_in = w.symb_starts[p]
        shift = int(round(fo / 15000.0))
        rows, pcorr, frows, fcorr = ctx.find_pss_tap_dev(d.cfg, d.a, d.q, ss_in, n2, ps, shift, start=c.start)
        assert sm.pss_decide(pcorr)[:3] == (n2, ps, shift) and fo == 15000.0 * shift
        _, thresh, ss_w = sm.fine_decide(fcorr, ss_in, ps, c.fft)
        assert np.float32(th).tobytes() == np.float32(thresh).tobytes() and ss.tolist() == ss_w.tolist()
        _, scorr = ctx.find_sss_tap_dev(d.cfg, d.a, d.q, n2, ss, start=c.start)
        assert sm.sss_decide(scorr, th, ss, c.fft)[:3] == (ok, n1, fs) and sm.sss_decide(scorr, th, ss, c.fft)[3].tolist() == ss2.tolist()
        if ok:
            found.append((3 * n1 + n2, fs))
    if c.find:
        assert sc.cell_hits(c, found), (c.cells, found)


@pytest.mark.parametrize("name", sc.names("d_") + ["c_exact"])
def test_edge_verdicts_as_the_model_says(ctx, dev, name):
    """family d (and the 160-slot case) through the _run entries: every verdict the MODEL's own, formed from its float64 numbers"""
    d, e = dev(name), sc.expected(name)
    t, peaks = run_chain(ctx, d)
    assert t.n_corr_peaks == e.coarse.n_peaks
    assert np.array([list(t.symb_starts[i]) for i in range(5)], np.uint32).tolist() == e.coarse.symb_starts.tolist()
    for ((ss, n2, ps, th, fo), (ok, n1, fs, ss2)), m in zip(peaks, e.peaks):
        assert (n2, ps, int(round(fo / 15000.0)), ss.tolist()) == (m.n_id_2, m.pss_symb, m.shift, m.symb_starts.tolist())
        assert abs(th - m.pss_thresh) <= 1e-4 * m.pss_thresh
        assert (ok, n1, fs, ss2.tolist()) == (m.found, m.n_id_1, m.frame_start, m.symb_starts_out.tolist())
    if d.c.edge is not None:
        assert list(t.symb_starts[0])[0] == (d.c.edge[0] - d.c.edge[1] * (d.c.fft + sm.geom(d.c.fft)[2])) + d.c.fft + sm.geom(d.c.fft)[2]


# ---- families e and f: single symbols through the _run entries

@pytest.fixture(scope="module")
def sym_cfg():
    import openlte_amd as m
    return m.DlCfg(sc.SYM_FFT, sc.SYM_RB, 1, m.IQ_F32_PLANAR)


@pytest.fixture(scope="module")
def sss_dev(ctx):
    i, q, symb5 = sc.sss_family()
    a, b = ctx.to_device(i), ctx.to_device(q)
    yield a, b, symb5
    a.free()
    b.free()


def test_every_sss_is_found_at_its_index(ctx, sym_cfg, sss_dev):
    """family e: the 1008 (N_id_1, N_id_2, half-frame), pss_thresh = the model's maximum, 62 x the symbol's amplitude"""
    a, b, symb5 = sss_dev
    corr, amp = sc.sss_family_model()
    for n, (i, k, h) in enumerate(sc.SSS_CASES):
        ss = np.zeros(7, np.uint32)
        ss[5] = symb5[n]
        th = np.float32(62 * amp[n])
        want = sm.sss_decide(corr[n], th, ss, sc.SYM_FFT)
        ok, n1, fs, ss2 = ctx.find_sss_dev(sym_cfg, a, b, k, ss, float(th))
        assert (ok, n1, fs, ss2.tolist()) == (True, i, want[2], want[3].tolist()), (n, i, k, h)
        back = (128 + 9) * 4 + 128 + 10 + (9600 if h else 0)
        assert (fs + back - int(symb5[n])) % 19200 == 0  # the half-frame verdict: subframe 5's sequence puts the frame ten slots earlier


def test_sss_correlations_of_the_family_against_the_model(ctx, sym_cfg, sss_dev):
    """every twelfth symbol's 336 correlations: bit-identical to the restatement on the device's row, and against the model"""
    a, b, symb5 = sss_dev
    corr, amp = sc.sss_family_model()
    worst = 0.0
    for n in range(0, len(sc.SSS_CASES), 12):
        i, k, h = sc.SSS_CASES[n]
        ss = np.zeros(7, np.uint32)
        ss[5] = symb5[n]
        row, co = ctx.find_sss_tap_dev(sym_cfg, a, b, k, ss)
        s32, z0 = sc.sss_candidates_f32(k, sc.SYM_RB)
        assert same_bits(co[None], sm.seq_corr_f32(row[None, 0, :72], row[None, 1, :72], s32, z0))
        assert int(np.abs(co).argmax()) == 2 * i + h and abs(np.abs(co).max() / (62 * amp[n]) - 1) <= 1e-5
        worst = max(worst, float(sm.rel_l2(co, corr[n])))
        assert worst <= sc.TOL_SEQ
    print("SSS family: worst rel-L2 of a set of 336 correlations against the model %.3g (hard gate %.3g)" % (worst, sc.TOL_SEQ))


def _pss_run(ctx, cfg, k, sft, tie):
    i, q, ss = sc.pss_family(k, sft, tie)
    a, b = ctx.to_device(i), ctx.to_device(q)
    try:
        return ctx.find_pss_dev(cfg, a, b, ss), (i, q, ss)
    finally:
        a.free()
        b.free()


def test_every_pss_root_and_shift_is_found(ctx, sym_cfg):
    """family e: 3 roots x 3 sub-carrier shifts, one symbol among 84"""
    for k, sft in sc.PSS_CASES:
        (ss, n2, ps, th, fo), (i, q, ss_in) = _pss_run(ctx, sym_cfg, k, sft, False)
        m = sm.pss_stage(i.astype(np.float64) + 1j * q.astype(np.float64), sc.SYM_FFT, sc.SYM_RB, ss_in)
        assert (n2, ps, fo, ss.tolist()) == (k, 7 * sc.PSS_SLOT + sc.PSS_SYMB, 15000.0 * sft, m.symb_starts.tolist()) and m.timing == 1
        assert abs(th - m.pss_thresh) <= 1e-4 * m.pss_thresh


def test_fine_timing_tie(ctx, sym_cfg):
    """family f: offsets +1 and +2 tie exactly.  The verdict is the model's, or -- here alone -- the one-sample alternative as
    test_sync_gpu.compare states it: every symbol start moved by the same one sample, everything else equal, the maxima within 1e-6"""
    table = [sc.lib_pss(k) for k in range(3)]
    alt = 0
    for k, sft in sc.PSS_CASES:
        (ss, n2, ps, th, fo), (i, q, ss_in) = _pss_run(ctx, sym_cfg, k, sft, True)
        m = sm.pss_stage(i.astype(np.float64) + 1j * q.astype(np.float64), sc.SYM_FFT, sc.SYM_RB, ss_in, table)
        assert (n2, ps, fo) == (m.n_id_2, m.pss_symb, 15000.0 * m.shift)
        delta = ss.astype(np.int64) - m.symb_starts.astype(np.int64)
        assert (delta == delta[0]).all() and abs(int(delta[0])) <= 1 and int(delta[0]) + m.timing in (1, 2)
        assert abs(th - m.pss_thresh) <= 1e-6 * m.pss_thresh
        alt += int(delta[0] != 0)
    print("fine-timing tie: %d of %d cases took the one-sample alternative" % (alt, len(sc.PSS_CASES)))


def test_sss_threshold_straddle(ctx, sym_cfg, sss_dev):
    """family f: the sent SSS 2 % above 0.9 pss_thresh is found, 2 % below it nothing is"""
    a, b, symb5 = sss_dev
    corr, _ = sc.sss_family_model()
    for n in (0, 501, 1007):
        i, k, h = sc.SSS_CASES[n]
        peak = float(sm.mag32(corr[n]).max())
        ss = np.zeros(7, np.uint32)
        ss[5] = symb5[n]
        ok, n1, fs, ss2 = ctx.find_sss_dev(sym_cfg, a, b, k, ss, peak / (0.9 * 0.98))
        assert (ok, n1, fs, ss2.tolist()) == (False, 0, 0, ss.tolist())
        ok, n1, fs, ss2 = ctx.find_sss_dev(sym_cfg, a, b, k, ss, peak / (0.9 * 1.02))
        assert (ok, n1) == (True, i)


# ---- output extents and arguments

def _filled(shape):
    a = np.empty(shape, np.uint32)
    a[...] = sc.NAN_BITS
    return a.view(np.float32)


@pytest.mark.parametrize("name", ["a_128_6_f32_s1", "a_256_6_i8_s12345", "a_1024_6_f32_s0"])
def test_output_extents(ctx, dev, name):
    """Outputs pre-filled with NAN_BITS: k_cp_corr's part-filled block (960 windows at FFT 128) and tail blocks (896 at 256, 512 at 1024) write
    every window of every slot; the row outputs are written in their first N_sc columns and nowhere else; the samples are not touched"""
    d = dev(name)
    c = d.c
    n_slot, n_sc = sm.geom(c.fft)[3], 12 * c.n_rb
    out = (_filled((c.n_slots, n_slot, 2)), _filled((n_slot,)))
    corr, acc = ctx.coarse_timing_tap_dev(d.cfg, d.a, d.q, c.n_slots, start=c.start, out=out)
    assert not (out[0].view(np.uint32) == sc.NAN_BITS).any() and not (out[1].view(np.uint32) == sc.NAN_BITS).any()
    assert same_bits(corr, sc.restated(name)[0])
    e = sc.expected(name)
    ss = e.coarse.symb_starts[0]
    out = (_filled((84, 2, 1200)), _filled((84, 9, 2)), _filled((80, 2, 1200)), _filled((80, 2)))
    ctx.find_pss_tap_dev(d.cfg, d.a, d.q, ss, 1, 10, 0, start=c.start, out=out)
    out2 = (_filled((2, 1200)), _filled((336, 2)))
    ctx.find_sss_tap_dev(d.cfg, d.a, d.q, 2, ss, start=c.start, out=out2)
    for rows in (out[0], out[2], out2[0][None]):
        bits = rows.view(np.uint32)
        assert not (bits[..., :n_sc] == sc.NAN_BITS).any() and (bits[..., n_sc:] == sc.NAN_BITS).all()
    for full in (out[1], out[3], out2[1]):
        assert not (full.view(np.uint32) == sc.NAN_BITS).any()
    if c.fmt == "i8":
        assert same_bits(d.a.download(np.int8).reshape(-1, 2), d.b.buf)
    else:
        assert same_bits(d.a.download(np.float32), d.b.buf[0]) and same_bits(d.q.download(np.float32), d.b.buf[1])


def test_tap_arguments(ctx, dev):
    """each tap returns MI_LTE_ERR_INVALID_ARG where its _run does, and for a NULL output"""
    import openlte_amd as m
    d = dev("a_128_6_i8_s0")
    L, h, cfg = ctx.L, ctx.h, C.byref(d.cfg)
    corr, acc = np.zeros((2, 960, 2), np.float32), np.zeros(960, np.float32)
    ok = [h, cfg, d.a.ptr, None, 0, 2, corr.ctypes.data, acc.ctypes.data]
    assert L.mi_lte_coarse_timing_tap(*ok) == 0
    for i in (0, 1, 2, 6, 7):
        assert L.mi_lte_coarse_timing_tap(*(ok[:i] + [None] + ok[i + 1:])) == ERR_INVALID_ARG, i
    assert L.mi_lte_coarse_timing_tap(*(ok[:5] + [0] + ok[6:])) == ERR_INVALID_ARG  # N_slots = 0
    assert L.mi_lte_coarse_timing_tap(h, C.byref(m.DlCfg(1000, 6, 1, m.IQ_I8)), *ok[2:]) == ERR_INVALID_ARG
    assert L.mi_lte_coarse_timing_tap(h, C.byref(m.DlCfg(128, 6, 1, m.IQ_F32_PLANAR)), *ok[2:]) == ERR_INVALID_ARG  # planar without the second array
    ss = np.arange(7, dtype=np.uint32) * 137 + 1
    bufs = [np.zeros(s, np.float32) for s in ((84, 2, 1200), (84, 9, 2), (80, 2, 1200), (80, 2))]
    ok = [h, cfg, d.a.ptr, None, 0, ss.ctypes.data, 0, 3, 0] + [b.ctypes.data for b in bufs]
    assert L.mi_lte_find_pss_tap(*ok) == 0
    for i in (0, 1, 2, 5, 9, 10, 11, 12):
        assert L.mi_lte_find_pss_tap(*(ok[:i] + [None] + ok[i + 1:])) == ERR_INVALID_ARG, i
    for i, v in ((6, 3), (7, 84), (8, 2), (8, -2)):  # the caller's verdict out of range
        assert L.mi_lte_find_pss_tap(*(ok[:i] + [v] + ok[i + 1:])) == ERR_INVALID_ARG, (i, v)
    row, co = np.zeros((2, 1200), np.float32), np.zeros((336, 2), np.float32)
    ok = [h, cfg, d.a.ptr, None, 0, 1, ss.ctypes.data, row.ctypes.data, co.ctypes.data]
    assert L.mi_lte_find_sss_tap(*ok) == 0
    for i in (0, 1, 2, 6, 7, 8):
        assert L.mi_lte_find_sss_tap(*(ok[:i] + [None] + ok[i + 1:])) == ERR_INVALID_ARG, i
    assert L.mi_lte_find_sss_tap(*(ok[:5] + [3] + ok[6:])) == ERR_INVALID_ARG  # N_id_2 > 2
