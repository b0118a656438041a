"""GPU: the PRACH detector's three kernels -- k_prach_fft (24 or 4 decimation phases, radix-4 Stockham FFTs with a radix-2 tail),
k_prach_bins (the P-term recombination of the kept bins), k_prach_corr (Bluestein inverse DFT of prime length 839 / 139, power, sum and
first arg-max) -- against a float64 model whose transforms are numpy's FFT (prach_model.model), through the detector's tap
(mi_lte_prach_detect_tap): the kept bins x_hat, the whole correlation power profiles and the per-root records the verdict is formed from.
The cases are prach_model_cases': every FFT shape in format 0 and format 4, formats 1-3, both ends of the carrier, both sample formats,
one / 64 / restricted root sets with the library's own and with given spectra, a single peak at every tested output offset of the
Bluestein, exact ties, the 50 x threshold straddled at +-2 %, all-zero samples; every occ_start odd.

Gates.  Hard: rel-L2 < 1e-5 and largest elementwise error < 1e-4 (of the occasion's RMS for x_hat, of the profile's maximum for the powers):
the project's FFT-stage figures.  Tight: 8 x the error of a float32 restatement of the kernels' own plan (prach_model.float32_floor) against
the model on these tests' own inputs, recomputed here (worst x_hat rel-L2 1.65e-7 at offset_2048_f32 / elementwise 6.08e-7 at
format1_128_f32, power rel-L2 5.16e-7 at peaks_fmt0 / elementwise 1.13e-6 at shape_fmt0_2048), so 1.32e-6 / 4.86e-6 for x_hat and
4.13e-6 / 9.05e-6 for the powers.  sum and max_val: relative error under the powers' elementwise gate.  max_off: equal, on every
(occasion, root) of every case -- test_prach_model_cpu.py holds the inputs to a 1e-4 margin between a profile's two largest powers, so no
case is left out.  Verdicts: prach_model.verdict on the tapped records, on the model's own records, mi_lte_prach_detect_run before and
after the tap, all equal.

Measured on an MI355X (x_hat rel-L2 / elementwise over RMS; power rel-L2 / elementwise over the maximum; each the worst, at its case):
  every FFT shape, format 0   1.57e-7 at fft 1024 / 5.25e-7 at fft 2048;  5.02e-7 at fft 1024 / 9.14e-7 at fft 2048
  every FFT shape, format 4   1.27e-7 at fft 2048 / 3.49e-7 at fft 2048;  3.05e-7 at fft 2048 / 6.29e-7 at fft 1024
  formats 1, 2, 3             1.43e-7 (format 2) / 5.88e-7 (format 2);    3.58e-7 (format 1) / 9.51e-7 (format 1)
  freq_offset N_rb - 6        1.62e-7 at fft 2048 / 5.07e-7 at fft 2048;  4.98e-7 at fft 256 / 1.01e-6 at fft 2048
  planar float32 samples      1.63e-7 at offset_2048_f32 / 6.08e-7 at format1_128_f32;  3.99e-7 at roots_one_own_f32 / 1.02e-6 at offset_2048_f32
  root sets, own spectra      1.44e-7 (one root) / 4.96e-7 (64 roots);    4.07e-7 (one root) / 8.75e-7 (64 roots)
  root sets, given spectra    the same figures to every digit: the library's spectra are the model's
  a peak at every offset      1.32e-7 / 5.36e-7;  5.16e-7 / 5.16e-7 (format 0, 124 offsets);  9.4e-8 / 2.9e-7;  4.74e-7 / 4.74e-7 (format 4, 139)
  ties                        1.40e-7 / 4.90e-7;  3.12e-7 / 4.38e-7        threshold straddle  1.60e-7 / 5.17e-7;  2.52e-7 / 2.19e-7
  all-zero samples            0 / 0;  0 / 0
  sum: 5.70e-7 at shape_fmt0_1024, max_val: 8.49e-7 at shape_fmt0_256 (gate 9.05e-6)
So the kernels sit at the float32 restatement (x_hat 1.63e-7 against its 1.65e-7, powers 5.16e-7 against 5.16e-7), an eighth of the tight
gates: worst 1.63e-7 against 1.32e-6.  Every max_off and every verdict equal, none left out.

Libraries with one defect each (new tests failed, of 15 / the 19 tests of test_prach_gpu.py failed):
  one FFT twiddle (entry 77 of 1024) off by 1e-4                     10 / 0
  the radix-2 tail's twiddle one table entry late                    12 / 0
  k_prach_bins' phase t formed without the % T_fft                    5 / 0
  the chirp's entry n = 838 conjugated                                9 / 0
  bspec built without the BL - n mirror for n = 300                  10 / 0
  the wave reduction preferring the larger offset among equals        2 / 0   (ties, all-zero samples)
  start off by one                                                   13 / 18
The verdict tests -- golden, live reference, 20 MHz batch, wrapped root set, launch / fetch -- saw only the last.
"""
import numpy as np
import pytest

import prach_model as pm
import prach_model_cases as pcs

pytestmark = pytest.mark.gpu

ERR_INVALID_ARG = -1  # MI_LTE_ERR_INVALID_ARG


class Run:
    """One plan over a case's batch: .before / .after = detect_run's verdicts around the tap, .x_hat .stats .power = the tap's"""

    def __init__(self, ctx, c, fetch=False):
        cfg, pc = c.cfgs()
        plan = ctx.prach_plan(cfg, pc, c.roots if c.given else None)
        try:
            assert plan.n_roots == c.roots[0].shape[0] and plan.occasion_samples == c.g.occasion_samples and plan.n_zc == c.g.N_zc
            n = len(c.occ_start)
            if c.is_float:
                d_a, d_b = ctx.to_device(np.ascontiguousarray(c.re, np.float32)), ctx.to_device(np.ascontiguousarray(c.im, np.float32))
            else:
                d_a, d_b = ctx.to_device(np.ascontiguousarray(np.stack([c.re, c.im], 1), np.int8)), None
            d_s = ctx.to_device(np.asarray(c.occ_start, np.uint64))
            try:
                self.before = np.stack(plan.detect_dev(d_a, d_b, d_s, n), 1)
                self.x_hat, self.stats, self.power = plan.tap_dev(d_a, d_b, d_s, n)
                assert ctx.last_kernels() == "k_prach_bins:1,k_prach_corr:1"
                self.after = np.stack(plan.detect_dev(d_a, d_b, d_s, n), 1)
                if fetch:
                    plan.launch_dev(d_a, d_b, d_s, n)
                    self.fetched = np.stack(plan.fetch(), 1)
            finally:
                d_a.free()
                d_s.free()
                if d_b is not None:
                    d_b.free()
        finally:
            plan.close()


class Worst:
    """the worst figures of a test and the cases they occurred at"""

    def __init__(self, what):
        self.what, self.fig, self.at, self.fail = what, [0.0] * 6, [None] * 6, []
        self.gates = pcs.gates()
        assert self.gates[0] <= pcs.TOL_L2 and self.gates[1] <= pcs.TOL_EL and self.gates[2] <= pcs.TOL_L2 and self.gates[3] <= pcs.TOL_EL

    def check(self, ctx, c, fetch=False):
        """one case through the library, every figure against the model"""
        e, r = pcs.expected(c.name), Run(ctx, c, fetch)
        n, nr, nz = len(c.occ_start), c.roots[0].shape[0], c.g.N_zc
        assert r.x_hat.shape == (n, nz) and r.power.shape == (n, nr, nz) and r.stats.shape == (n, nr)
        assert np.isfinite(r.x_hat).all() and np.isfinite(r.power).all() and (r.stats["pad"] == 0).all()
        figs = [np.max(v) for v in pm.xhat_errors(r.x_hat, e.x_hat) + pm.power_errors(r.power, e.power)]
        figs += [pm.scalar_errors(r.stats["sum"], e.stats[0]).max(), pm.scalar_errors(r.stats["max_val"], e.stats[1]).max()]
        for i, v in enumerate(figs):
            if v >= self.fig[i]:
                self.fig[i], self.at[i] = float(v), c.name
        g = self.gates
        ok = figs[0] < g[0] and figs[1] < g[1] and figs[2] < g[2] and figs[3] < g[3] and figs[4] < g[3] and figs[5] < g[3]
        if c.kind == "zeros":  # nothing to round: every figure is exactly 0
            ok = all(v == 0 for v in figs) and (r.power == 0).all() and (r.stats["sum"] == 0).all() and (r.stats["max_val"] == 0).all()
        if not ok:
            self.fail.append((c.name, "figures", ["%.3g" % v for v in figs]))
        # the records are the profile's own: the stored maximum is a stored power, at the stored offset
        if not (np.take_along_axis(r.power, r.stats["max_off"][..., None].astype(np.int64), -1)[..., 0] == r.stats["max_val"]).all() \
                or not (r.power.max(-1) == r.stats["max_val"]).all():
            self.fail.append((c.name, "max_val is not the profile's maximum at max_off"))
        if not (r.stats["max_off"] == e.stats[2]).all():
            bad = np.argwhere(r.stats["max_off"] != e.stats[2])[0]
            self.fail.append((c.name, "max_off", bad.tolist(), int(r.stats["max_off"][tuple(bad)]), int(e.stats[2][tuple(bad)])))
        tapped = pm.verdict((r.stats["sum"], r.stats["max_val"], r.stats["max_off"]), c.N_cs, c.v_max, nz)
        for what, v in (("verdict of the tapped records", tapped), ("the model's verdict", e.verdict), ("detect_run after the tap", r.after)) \
                + ((("launch / fetch", r.fetched),) if fetch else ()):
            if not (v == r.before).all():
                self.fail.append((c.name, what, v.tolist(), r.before.tolist()))
        if c.detect is not None and tuple(r.before[:, 0]) != c.detect:
            self.fail.append((c.name, "detection", r.before[:, 0].tolist()))
        return r

    def report_and_assert(self):
        """Print first, then assert, so a failing run still shows every figure."""
        print("%s: x_hat rel-L2 %.3g at %s, elementwise / RMS %.3g at %s; power rel-L2 %.3g at %s, elementwise / max %.3g at %s; "
              "sum %.3g at %s, max_val %.3g at %s (gates %.3g %.3g %.3g %.3g)"
              % ((self.what,) + tuple(v for p in zip(self.fig, self.at) for v in p) + tuple(self.gates)))
        assert not self.fail, self.fail


def check_group(ctx, what, cases, fetch=False):
    assert cases
    w = Worst(what)
    for c in cases:
        w.check(ctx, c, fetch)
    w.report_and_assert()


@pytest.mark.parametrize("fmt", [0, 4])
def test_every_fft_shape(ctx, fmt):
    """fft 128 ... 2048: N2 = 64, 128, 256, 512, 1024 (the radix-2 tail at 128 and 512, every twiddle stride) with 24 phases and with 4;
    a preamble at zero delay, one inside its window, noise only"""
    cases = pcs.group("shape%d" % fmt)
    assert [c.g.N2 for c in cases] == [64, 128, 256, 512, 1024] and {c.g.P for c in cases} == {24 if fmt == 0 else 4}
    check_group(ctx, "every FFT shape, format %d" % fmt, cases)


def test_formats_1_2_3(ctx):
    """other cyclic-prefix lengths, the sequence sent twice"""
    check_group(ctx, "formats 1, 2, 3 at fft 128", pcs.group("formats"))


def test_frequency_offsets(ctx):
    """freq_offset = N_rb - 6: start moves to the other end of the carrier, idx wraps modulo T_fft"""
    check_group(ctx, "freq_offset N_rb - 6", pcs.group("offsets"))


def test_planar_float_samples_through_the_device_entries(ctx):
    """Samp<float>: every fft-128 and fft-2048 case once more as planar float32 with non-integer values"""
    check_group(ctx, "planar float32 samples", pcs.group("float"))


def test_root_sets_with_the_library_s_own_spectra(ctx):
    """one root, 64 roots (N_cs = 0: the verdict's other branch), a restricted set; spectra from mi_lte_prach_plan_create"""
    check_group(ctx, "root sets, own spectra", pcs.group("roots_own"))


def test_root_sets_with_the_model_s_spectra(ctx):
    """the same with the model's spectra handed to mi_lte_prach_plan_create_roots"""
    check_group(ctx, "root sets, given spectra", pcs.group("roots_given"))


@pytest.mark.parametrize("fmt", [0, 4])
def test_a_single_peak_at_every_offset_of_the_bluestein(ctx, fmt):
    """crafted noiseless occasions, one per output offset (format 0: every seventh and both edges; format 4: all 139): max_off bin by bin"""
    c, = [c for c in pcs.group("peaks") if c.pc[1] == fmt]
    w = Worst("a peak at each of %d offsets, format %d" % (len(c.occ_start), fmt))
    r = w.check(ctx, c)
    w.report_and_assert()
    assert (r.stats["max_off"][:, 0] == np.array(pcs.bluestein_offsets(fmt))).all()


def test_ties_go_to_the_smaller_offset_and_the_lower_root(ctx):
    """roots [X_u, 0, X_u]: the zero row's 839 equal powers leave offset 0, the two equal rows leave root 0 (prach_model_cases.tie_case)"""
    c, = pcs.group("ties")
    w = Worst("ties")
    r = w.check(ctx, c)
    w.report_and_assert()
    assert (r.stats["max_off"][:, 1] == 0).all() and (r.power[:, 1] == 0).all()
    assert r.power[:, 0].tobytes() == r.power[:, 2].tobytes() and r.stats[:, 0].tobytes() == r.stats[:, 2].tobytes()
    assert (r.before[:2, 0] == 1).all() and (r.before[:2, 1] <= c.v_max).all()  # root 0's preambles


def test_threshold_straddle(ctx):
    """max / (50 ave) of the model at 1.02 and at 0.98: detected, not detected"""
    check_group(ctx, "threshold straddle", pcs.group("straddle"))


def test_all_zero_samples_are_refused(ctx):
    """max_val != 0: every power, sum and maximum exactly 0, nothing detected"""
    w = Worst("all-zero samples")
    for c in pcs.group("zeros"):
        r = w.check(ctx, c)
        assert (r.before == 0).all() and (r.x_hat == 0).all()
    w.report_and_assert()


def test_launch_and_fetch_on_three_occasions(ctx):
    """mi_lte_prach_detect_launch / _fetch at n_occ = 3 (the records copied into the plan's pinned block) against detect_run (the small-results
    route, written by the kernel into pinned memory) and the model"""
    cases = [pcs.all_cases()[n] for n in ("shape_fmt0_128", "shape_fmt4_2048", "offset_2048_f32", "roots_max_given")]
    assert all(len(c.occ_start) == 3 for c in cases)
    check_group(ctx, "launch / fetch, 3 occasions", cases, fetch=True)


def test_the_tap_leaves_nothing_behind(ctx):
    """one plan: plain run, tapped run, plain run -- identical verdicts; and two tapped runs give identical bytes (no atomics, no order that
    depends on timing)"""
    c = pcs.all_cases()["shape_fmt0_512"]
    a, b = Run(ctx, c), Run(ctx, c)
    assert (a.before == a.after).all() and (a.before == pcs.expected(c.name).verdict).all()
    assert a.x_hat.tobytes() == b.x_hat.tobytes() and a.power.tobytes() == b.power.tobytes() and a.stats.tobytes() == b.stats.tobytes()


def test_the_tap_rejects_what_detect_run_rejects(ctx):
    import openlte_amd as m
    c = pcs.all_cases()["shape_fmt0_128_f32"]
    cfg, pc = c.cfgs()
    plan = ctx.prach_plan(cfg, pc)
    d_a, d_s = ctx.to_device(c.re), ctx.to_device(c.occ_start)
    try:
        x, s, p = np.zeros((3, 839), np.complex64), np.zeros((3, plan.n_roots), plan.STAT), np.zeros((3, plan.n_roots, 839), np.float32)
        L, ok = ctx.L, (ctx.h, plan.h, d_a.ptr, d_a.ptr, d_s.ptr, 3, x.ctypes.data, s.ctypes.data, p.ctypes.data)
        assert L.mi_lte_prach_detect_tap(*ok) == 0
        for i in (0, 1, 2, 4, 5, 6, 7, 8):  # a NULL context, plan, first plane, start list, no occasion, a NULL output
            bad = list(ok)
            bad[i] = 0 if i == 5 else None
            assert L.mi_lte_prach_detect_tap(*bad) == ERR_INVALID_ARG, i
        bad = list(ok)
        bad[3] = None  # planar float samples without their second plane, as detect_run
        assert L.mi_lte_prach_detect_tap(*bad) == ERR_INVALID_ARG
        with pytest.raises(m.MiLteError):
            plan.detect_dev(d_a, None, d_s, 3)
    finally:
        d_a.free()
        d_s.free()
        plan.close()
