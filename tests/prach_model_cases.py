"""Cases for the PRACH detector's model tests (test_prach_model_cpu.py, test_prach_model_gpu.py): small batches that reach every code path of
k_prach_fft / k_prach_bins / k_prach_corr, their expectations from the float64 model (prach_model.model) and the error of the float32
restatement (prach_model.float32_floor) on the same inputs, which sets the GPU tests' tight gates.  Inputs come from the library's host
transmitter (openlte_amd.synth.prach_occasions) or are crafted here; seeds are fixed.  No kernel result enters anything here.

Every batch is packed the same way: the occasions follow each other without a gap, each cut to an even number of samples behind a lead of 13
samples, so every occ_start is odd and every occasion has the tail of the one before it in front (the first: the tail of the last) -- a
detector that read a wrong T_cp or start would transform other data.

The root sets: where a set would run past the logical root table the reference reads behind its table and the library wraps (prach_sets.hpp);
no case here uses such a set, so the library's documented choice and the reference's coincide on all of them."""
import ctypes as C
import functools

import numpy as np

import prach_model as pm

TOL_L2, TOL_EL = 1e-5, 1e-4  # the project's FFT-stage figures (pusch_demod_cases.TOL_SYMB and 10 x it): the hard gates
GATE_FACTOR = 8.0            # tight gate = GATE_FACTOR x the float32 restatement's worst error on these inputs (as the pre-decoder's tests)
LEAD = 13
N_RB = {128: 6, 256: 15, 512: 25, 1024: 50, 2048: 100}


class Case:
    """.name .group .fft .n_rb .pc = (root_seq_idx, format, zczc, hs_flag, freq_offset) .is_float .re .im (one buffer: int8 or float32 [total])
    .occ_start uint64 [n_occ] .given (the plan takes the model's spectra through plan_create_roots) .roots (re, im) float32 [n_roots, 839]
    .kind: plain | tie | straddle | zeros .detect (straddle: the verdicts the library must reach) .g .u (physical roots) .N_cs .v_max"""

    def cfgs(self):
        import openlte_amd as m
        return m.DlCfg(self.fft, self.n_rb, 1, m.IQ_F32_PLANAR if self.is_float else m.IQ_I8), m.PrachCfg(*self.pc)

    def x(self):
        return pm.occasions(self.re, self.im, self.occ_start, self.g)


def root_list(pc):
    """the physical roots of the configuration's 64 preambles (mi_lte_prach_root_set: host arithmetic of the library)"""
    import openlte_amd as m
    u, n, cfg = np.zeros(64, np.uint32), np.zeros(1, np.uint32), m.PrachCfg(*pc)
    # a prototype of this module's own: other tests set argtypes on the shared library object, each to its own taste
    fn = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_void_p)(("mi_lte_prach_root_set", m.load_library()))
    assert fn(C.addressof(cfg), u.ctypes.data, n.ctypes.data) == 0
    return [int(v) for v in u[:n[0]]]


def pack(occ, g):
    """occ: list of (re, im) arrays, each at least the occasion's length + 6 -> (re [total], im [total], occ_start): see the module's docstring"""
    lens = [g.occasion_samples + (g.occasion_samples & 1) + 2 * ((5 * o + 1) % 3) for o in range(len(occ))]
    assert all(len(r) >= n for (r, _), n in zip(occ, lens))
    parts_re = [occ[-1][0][lens[-1] - LEAD:lens[-1]]] + [r[:n] for (r, _), n in zip(occ, lens)]
    parts_im = [occ[-1][1][lens[-1] - LEAD:lens[-1]]] + [i[:n] for (_, i), n in zip(occ, lens)]
    start = LEAD + np.concatenate([[0], np.cumsum(lens[:-1])])
    assert (start % 2 == 1).all()
    return np.concatenate(parts_re), np.concatenate(parts_im), start.astype(np.uint64)


def make(name, group, fft, pc, occ, is_float=False, given=False, kind="plain", roots=None, detect=None):
    c = Case()
    c.name, c.group, c.fft, c.n_rb, c.pc, c.is_float, c.given, c.kind, c.detect = name, group, fft, N_RB[fft], tuple(pc), is_float, given, kind, detect
    c.g = pm.Geom(fft, c.n_rb, pc[1], pc[4])
    c.u = root_list(pc)
    c.N_cs, c.v_max = pm.sets(c.u[0], pc[2], pc[3], pc[1])
    c.roots = roots if roots is not None else pm.root_spectra(c.u, c.g.N_zc)
    c.re, c.im, c.occ_start = pack(occ, c.g)
    assert c.re.dtype == (np.float32 if is_float else np.int8)
    return c


def synth_occ(fft, pc, pre, dly, snr_db, seed):
    """[(re, im)] int8 occasions of the host transmitter"""
    import openlte_amd as m
    from openlte_amd import synth
    iq = synth.prach_occasions(m.DlCfg(fft, N_RB[fft], 1, 0), m.PrachCfg(*pc), pre, dly, snr_db=snr_db, seed=seed)
    return [(iq[o, :, 0].copy(), iq[o, :, 1].copy()) for o in range(iq.shape[0])]


def three_occasions(fft, pc, seed, pre=(5, 41), snr_db=8.0):
    """a preamble at zero delay, one inside its cyclic-shift window (as far as the transmitter's delay limit and the window allow), noise only"""
    mid = max(3, fft // 20) if pc[1] == 4 else fft // 4 + 5
    return synth_occ(fft, pc, list(pre), [0, mid], snr_db, seed) + synth_occ(fft, pc, [0], [0], -30.0, seed + 1000)


def float_twin(c, seed):
    """the same batch as planar float32 with non-integer values: the int8 capture x 0.37 + a dither from the fixed seed"""
    rng = np.random.default_rng(seed)
    t = Case()
    t.__dict__.update(c.__dict__)
    t.name, t.group, t.is_float = c.name + "_f32", "float", True
    t.re = (c.re.astype(np.float32) * np.float32(0.37) + rng.uniform(-0.5, 0.5, c.re.shape).astype(np.float32)).astype(np.float32)
    t.im = (c.im.astype(np.float32) * np.float32(0.37) + rng.uniform(-0.5, 0.5, c.im.shape).astype(np.float32)).astype(np.float32)
    return t


def crafted_occasion(x_hat, g, peak=60.0):
    """(re, im) float32: T_fft samples whose kept bins are x_hat (up to a real scale), behind their own cyclic prefix, and 6 samples more"""
    X = np.zeros(g.T_fft, np.complex128)
    X[g.bin_index()] = x_hat
    x = np.fft.ifft(X)
    x *= peak / max(np.abs(x.real).max(), np.abs(x.imag).max())
    full = np.concatenate([x[g.T_fft - g.T_cp:], x, x[:8]])
    return full.real.astype(np.float32), full.imag.astype(np.float32)


def bluestein_offsets(fmt):
    """the output offsets of the crafted single-peak batch: formats 0-3 every seventh and both edges, format 4 every one"""
    return list(range(139)) if fmt == 4 else sorted(set(range(0, 839, 7)) | {1, 2, 837, 838})


def peak_case(fmt):
    """fft 128, one root, noiseless: occasion i has x_hat = X_u exp(+2 pi i j m_i / N_zc), so that X_u conj(x_hat) transforms back to a single
    peak at offset m_i -- every chirp entry, both edges, and the m - j wrap of the convolution"""
    pc = (40, fmt, 0 if fmt == 4 else 1, 0, 0)
    g = pm.Geom(128, 6, fmt, 0)
    u = root_list(pc)[:1]
    roots = pm.root_spectra(u, g.N_zc)
    Xu = pm.spectra_complex(roots, g.N_zc)[0]
    j = np.arange(g.N_zc)
    occ = [crafted_occasion(Xu * np.exp(2j * np.pi * j * m / g.N_zc), g) for m in bluestein_offsets(fmt)]
    return make("peaks_fmt%d" % fmt, "peaks", 128, pc, occ, is_float=True, given=True, roots=roots)


def tie_case():
    """Ties.  Roots given as [X_u, 0, X_u]: rows 0 and 2 give bit-equal profiles, so equal maxima across roots, and the lower root must win
    the verdict's scan; row 1 gives a profile of 839 exact zeros, so every offset ties inside that root -- offsets 255 and 256 among them, lanes
    and wavefronts apart in k_prach_corr's reduction -- and offset 0 must win, as the reference's ascending scan leaves it.  A tie between two
    live offsets inside one root cannot be constructed from samples: x_hat reaches the correlation through the float32 transform of the samples
    (sincospif included), whose rounding the float32 restatement does not reproduce bit for bit, so no input pins two non-zero powers to the
    same float.  The zero row is the inside-a-root tie."""
    pc = (22, 0, 11, 0, 0)
    u = root_list(pc)
    r1 = pm.root_spectra([u[0]], 839)
    roots = (np.concatenate([r1[0], 0 * r1[0], r1[0]]), np.concatenate([r1[1], 0 * r1[1], r1[1]]))
    occ = synth_occ(128, pc, [2, 7], [0, 20], 10.0, 77) + synth_occ(128, pc, [0], [0], -30.0, 78)
    return make("ties", "ties", 128, pc, occ, given=True, kind="tie", roots=roots)


def straddle_case(fft):
    """Two occasions of one preamble plus fixed noise at two scales, found by bisection with the float64 model so that max / (50 ave) is
    1.02 +- 0.005 and 0.98 +- 0.005: the library must detect the first and not the second"""
    pc = (100, 0, 1, 0, 0)
    g = pm.Geom(fft, N_RB[fft], 0, 0)
    roots = pm.root_spectra(root_list(pc), g.N_zc)
    xu = pm.spectra_complex(roots, g.N_zc)
    (sr, si), = synth_occ(fft, pc, [9], [fft // 8], 40.0, 91)
    rng = np.random.default_rng(92 + fft)
    nr, ni = rng.standard_normal(len(sr)).astype(np.float32), rng.standard_normal(len(sr)).astype(np.float32)

    def samples(s):
        return (sr.astype(np.float32) + np.float32(s) * nr).astype(np.float32), (si.astype(np.float32) + np.float32(s) * ni).astype(np.float32)

    def ratio(s):
        re, im = samples(s)
        x = (re.astype(np.float64) + 1j * im.astype(np.float64))[None, :]
        return pm.threshold_ratio(pm.model(x, g, xu)[2], g.N_zc)[0]

    occ = []
    for target in (1.02, 0.98):
        lo, hi = 0.0, 4000.0
        assert ratio(lo) > target > ratio(hi)
        for _ in range(60):
            mid = 0.5 * (lo + hi)
            if ratio(mid) > target:
                lo = mid
            else:
                hi = mid
            if abs(ratio(0.5 * (lo + hi)) - target) < 0.002:
                break
        s = 0.5 * (lo + hi)
        assert abs(ratio(s) - target) < 0.005, (fft, target, s, ratio(s))
        occ.append(samples(s))
    return make("straddle_%d" % fft, "straddle", fft, pc, occ, is_float=True, kind="straddle", roots=roots, detect=(1, 0))


def zero_cases():
    pc = (22, 0, 11, 0, 0)
    n = pm.Geom(128, 6, 0, 0).occasion_samples + 8
    z8, zf = np.zeros(n, np.int8), np.zeros(n, np.float32)
    return [make("zeros_i8", "zeros", 128, pc, [(z8, z8)] * 2, kind="zeros"), make("zeros_f32", "zeros", 128, pc, [(zf, zf)] * 2, is_float=True, kind="zeros")]


@functools.lru_cache(maxsize=None)
def all_cases():
    """{name: Case}, built once and shared: treat every array as read-only"""
    out = []
    # every FFT shape: N2 = 64 ... 1024 with 24 phases (format 0) and with 4 (format 4); the radix-2 tail at N2 = 128 and 512
    for k, fft in enumerate((128, 256, 512, 1024, 2048)):
        out.append(make("shape_fmt0_%d" % fft, "shape0", fft, (30 + 100 * k, 0, 12, 0, 0), three_occasions(fft, (30 + 100 * k, 0, 12, 0, 0), 110 + k)))
        out.append(make("shape_fmt4_%d" % fft, "shape4", fft, (7 + 20 * k, 4, 3, 0, 0), three_occasions(fft, (7 + 20 * k, 4, 3, 0, 0), 200 + k)))
    # formats 1, 2, 3: other T_cp, the sequence sent twice
    for fmt in (1, 2, 3):
        pc = (50 + fmt, fmt, 11, 0, 0)
        out.append(make("format%d_128" % fmt, "formats", 128, pc, three_occasions(128, pc, 300 + fmt)))
    # frequency offsets: 0 is every case above; the other end N_rb - 6 (at 1.4 MHz that is 0 again: six resource blocks in all)
    for fft in (256, 512, 2048):
        pc = (400 + fft % 97, 0, 10, 0, N_RB[fft] - 6)
        out.append(make("offset_%d" % fft, "offsets", fft, pc, three_occasions(fft, pc, 400 + fft % 89)))
    pc = (11, 4, 5, 0, N_RB[2048] - 6)
    out.append(make("offset_fmt4_2048", "offsets", 2048, pc, three_occasions(2048, pc, 450)))
    # root sets: one root, the most a configuration yields (64: N_cs = 0), a restricted set; each with the library's spectra and with the model's
    for tag, pc, pre in (("one", (100, 0, 1, 0, 0), (5, 41)), ("max", (200, 0, 0, 0, 0), (5, 41)), ("restricted", (300, 0, 6, 1, 0), (2, 9))):
        occ = three_occasions(128, pc, 500 + len(tag), pre=pre)
        out.append(make("roots_%s_own" % tag, "roots_own", 128, pc, occ))
        out.append(make("roots_%s_given" % tag, "roots_given", 128, pc, occ, given=True))
    # both sample formats: every fft-128 and fft-2048 case above once more as planar float32
    out += [float_twin(c, 800 + i) for i, c in enumerate(list(out)) if c.fft in (128, 2048)]
    out += [peak_case(0), peak_case(4), tie_case(), straddle_case(128), straddle_case(512)] + zero_cases()
    assert len({c.name for c in out}) == len(out)
    return {c.name: c for c in out}


def group(name):
    return [c for c in all_cases().values() if c.group == name]


class Expect:
    """.x_hat .power .stats: the float64 model's; .verdict: prach_model.verdict on the model's stats; .ratio; .floor = (x_hat rel-L2, x_hat
    elementwise, power rel-L2, power elementwise): the float32 restatement's worst errors on this case"""


@functools.lru_cache(maxsize=None)
def expected(name):
    c = all_cases()[name]
    e = Expect()
    x = c.x()
    e.x_hat, e.power, e.stats = pm.model(x, c.g, pm.spectra_complex(c.roots, c.g.N_zc))
    e.verdict = pm.verdict(e.stats, c.N_cs, c.v_max, c.g.N_zc)
    e.ratio = pm.threshold_ratio(e.stats, c.g.N_zc)
    fx, fp, fs = pm.float32_floor(x, c.g, c.roots)
    e.floor_stats = fs
    (a, b), (p, q) = pm.xhat_errors(fx, e.x_hat), pm.power_errors(fp, e.power)
    e.floor = (float(a.max()), float(b.max()), float(p.max()), float(q.max()))
    for arr in (e.x_hat, e.power):
        arr.setflags(write=False)
    return e


@functools.lru_cache(maxsize=None)
def gates():
    """(x_hat rel-L2, x_hat elementwise, power rel-L2, power elementwise): GATE_FACTOR x the float32 restatement's worst figure over all
    cases, capped at the hard gates.  Why 8: the kernels' sincospif and the host tables are a few ulp from the restatement's correctly
    rounded values and the kernel sums in another order; each moves a float32 transform's error by a small factor, none by an order of
    magnitude (the pre-decoder's kernel sits at 1.4 x its restatement)."""
    fl = np.array([expected(n).floor for n in all_cases()])
    w = GATE_FACTOR * fl.max(0)
    return min(w[0], TOL_L2), min(w[1], TOL_EL), min(w[2], TOL_L2), min(w[3], TOL_EL)
