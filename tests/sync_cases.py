"""The cases of the synchronisation model tests (test_sync_model_cpu.py, test_sync_model_gpu.py): a deterministic list from fixed seeds.  The
captures are the host Transmitter's (signals, bch, samples: CRS, PSS, SSS and the PBCH of whole frames), delayed, rotated, mixed and noised
in numpy; the single-symbol families take one SSS or PSS symbol out of a Transmitter subframe.  Nothing comes from a reference tree and no
kernel result enters anything here.

Families (the letters of the case names):
  a  shapes       every FFT size at 6 RB and (2048, 100); int8 and planar float (fractional); start 0, 1, 12345; N_slots 2 .. 4
  b  fractional   planar float: Gaussian noise alone; a cell with 60 dB between the halves of every slot
  c  exactness    int8, N_slots = 160 at FFT 128 (every sum an exact integer below 2^24)
  d  edges        the strongest coarse peak at window 0, 1, n_blank / 2 - 1, n_slot - 1 and one symbol before the end; silence; noise with
                  fewer than five peaks; a constant (every window AT the mean); two cells
  e  sequences    one SSS symbol per (N_id_1, N_id_2, half-frame): 1008; one PSS symbol per root and sub-carrier shift: 9
  f  thresholds   the SSS magnitude 2 % above and below 0.9 pss_thresh; a fine-timing pair that ties
Float magnitudes lie within 1e-3 .. 1e3 (no product is subnormal); no NaN, no infinity."""
import functools

import numpy as np

import dl_frontend_model as dm
import sync_model as sm

NAN_BITS = 0x7FC5A5A5  # the pattern an output buffer is filled with before a call (dl_frontend_cases.NAN_BITS)
GATE_FACTOR = 8.0


def gate(floor, hard):
    """GATE_FACTOR x the floor, never wider than the hard gate (dl_frontend_cases.gate)"""
    return min(GATE_FACTOR * floor, hard)


TOL_SYMB = 1e-5   # the project's hard gate on symbol rows, rel-L2 (dl_frontend_cases.TOL_SYMB)
TOL_CORR = 1e-5   # hard gate on a cyclic-prefix correlation row and on acc: sums of at most 144 float32 products (rel-L2; the restatements sit near 1e-7)
TOL_SEQ = 1e-4    # hard gate on a set of SSS correlations against the model: behind the transform, and most of a set is cross-correlation, a sum
#                   of 62 terms that cancel to an eighth of their total (the restatement on the model's own rows sits near 2e-7)
TOL_PSS = 1e-3    # the same for a set of PSS correlations: the reference's table is cosf / sinf of a phase rounded to float (up to 6600 rad:
#                   2.45e-4 rad of rounding, test_sync_model_cpu.test_standard_tables), the model's is the standard's; 4 x that phase error


def slack(fft):
    """how far a frame start may lie from where the cell was put (test_sync_gpu: the fine timing lands a few samples inside the prefix)"""
    return 20 * fft // 2048 + 1


class Case:
    """.name .fft .n_rb .fmt ('i8' / 'f32') .n_slots .start .cells [(N_id_cell, delay, gain)] .snr_db .f_off .seed .kind .edge"""

    def __init__(self, name, fft, n_rb, fmt, n_slots, start=0, cells=(), snr_db=30.0, f_off=0.0, seed=1, kind="cell", edge=None, find=True):
        self.name, self.fft, self.n_rb, self.fmt, self.n_slots, self.start = name, fft, n_rb, fmt, n_slots, start
        self.cells, self.snr_db, self.f_off, self.seed, self.kind, self.edge, self.find = list(cells), snr_db, f_off, seed, kind, edge, find


SHAPES = ((128, 6), (256, 6), (512, 6), (1024, 6), (2048, 6), (2048, 100))
STARTS = (0, 1, 12345)
# Two to four slots are few for the coarse search (the scanner takes 160), and the first PSS pass is coherent over 62 sub-carriers: it loses the
# cell when the coarse peak stands N / 62 samples from a symbol's prefix (2 samples at FFT 128; a 6-RB cell on a wide transform is oversampled
# and its prefix peak broad).  Samples added to the delay of the shapes in whose first draw the MODEL did not find its cell:
DELAY_BUMP = {5: 49, 8: 1096}
# d: name: (window of the strongest peak, steps of the walk-back, blanking indices that wrap, cell, delay, noise seed) at FFT 128 (symbol 137,
# n_blank 13).  Which of a slot's seven prefix peaks is the strongest is the data's choice: cell and delay are those at which the MODEL's first
# peak stands at the window and its cell is found (a search over the model alone; test_sync_model_cpu asserts each edge is reached).
EDGES = {"d_win0": (0, 0, 0, 106, 823, 439), "d_win1": (1, 1, 5, 100, 412, 440), "d_win5": (5, 1, 1, 91, 827, 441), "d_win959": (959, 7, 0, 93, 273, 442),
         "d_win823": (823, 7, 5, 95, 274, 443)}


@functools.lru_cache(maxsize=None)
def case_list():
    cs = []
    for s, (fft, n_rb) in enumerate(SHAPES):
        for f, fmt in enumerate(("i8", "f32")):
            idx = 2 * s + f
            cell, delay = (37 * idx + 5) % 504, (977 * idx + 13) % (3 * sm.geom(fft)[3]) + DELAY_BUMP.get(idx, 0)
            for start in STARTS:
                cs.append(Case("a_%d_%d_%s_s%d" % (fft, n_rb, fmt, start), fft, n_rb, fmt, 2 + idx % 3, start, [(cell, delay, 1.0)], 20.0, 200.0 - 50.0 * idx,
                               100 + idx))
    cs.append(Case("b_gauss", 256, 15, "f32", 3, 1, kind="gauss", seed=201, find=False))
    cs.append(Case("b_60db", 128, 6, "f32", 4, 0, [(77, 333, 1.0)], 25.0, 0.0, 202, kind="60db", find=False))
    cs.append(Case("c_exact", 128, 6, "i8", 160, 0, [(301, 1300, 1.0)], 12.0, 700.0, 301))
    for name in EDGES:
        cs.append(Case(name, 128, 6, "i8", 3, 0, [(EDGES[name][3], EDGES[name][4], 1.0)], 40.0, 0.0, EDGES[name][5], edge=EDGES[name][:3]))
    cs.append(Case("d_silence_i8", 128, 6, "i8", 3, 1, kind="silence", find=False))
    cs.append(Case("d_silence_f32", 256, 6, "f32", 2, 0, kind="silence", find=False))
    cs.append(Case("d_few", 128, 6, "i8", 3, 0, kind="few", seed=410, find=False))
    cs.append(Case("d_const", 128, 6, "i8", 3, 0, kind="const", find=False))
    cs.append(Case("d_two_cells", 128, 6, "i8", 4, 0, [(150, 100, 1.0), (341, 344, 1.0)], 30.0, 0.0, 411))
    return tuple(cs)


def names(prefix=""):
    return [c.name for c in case_list() if c.name.startswith(prefix)]


def by_name(name):
    return next(c for c in case_list() if c.name == name)


def needed(fft, n_slots):
    """samples a capture must hold from its first one: the coarse search's, and a frame and two slots past the PSS stage for the SSS symbol"""
    N, _, cpe, n_slot, n_frame = sm.geom(fft)
    return max((n_slots + 1) * n_slot + cpe + N, n_frame + 3 * n_slot + N) + 64


@functools.lru_cache(maxsize=None)
def cell_signal(fft, n_rb, cell, n_sub):
    """complex128: n_sub subframes of the cell from frame 0, subframe 0: a fully loaded grid (unit-power QPSK on every resource element, as a
    busy cell's PDSCH leaves it: the coarse search multiplies the prefix correlations of a slot's two CRS symbols, which an otherwise empty grid
    leaves below the mean of its PSS / SSS symbols), then CRS everywhere, PSS / SSS in subframes 0 and 5, the PBCH in 0"""
    import openlte_amd as m
    t = m.Transmitter(fft, n_rb, cell)
    rng = np.random.default_rng(cell)
    mib = rng.integers(0, 2, 24).astype(np.uint8)
    out = []
    for s in range(n_sub):
        t.clear()
        t.re[0, :14, :12 * n_rb] = (1 - 2 * rng.integers(0, 2, (14, 12 * n_rb))) / np.sqrt(2.0)
        t.im[0, :14, :12 * n_rb] = (1 - 2 * rng.integers(0, 2, (14, 12 * n_rb))) / np.sqrt(2.0)
        t.signals(s % 10)
        if s % 10 == 0:
            t.bch(mib, s // 10)
        i, q = t.samples()
        out.append(i.astype(np.float64) + 1j * q.astype(np.float64))
    t.close()
    return np.concatenate(out)


def mix(c, cells, n, peak=90.0):
    """complex128 [n]: the case's cells, each `delay` samples late and rotated by f_off, with noise, the strongest sample near `peak`"""
    rng = np.random.default_rng(c.seed)
    sub = 30720 * c.fft // 2048
    z = np.zeros(n, np.complex128)
    rms = 0.0
    for cell, delay, gain in cells:
        s = cell_signal(c.fft, c.n_rb, cell, (n - delay + sub - 1) // sub)[:n - delay]
        rms = max(rms, float(np.sqrt(np.mean(np.abs(s) ** 2))))
        z[delay:] += gain * s
    z *= np.exp(2j * np.pi * c.f_off * np.arange(n) / (30.72e6 * c.fft / 2048))
    sig = rms * 10 ** (-c.snr_db / 20) / np.sqrt(2)
    z += sig * (rng.standard_normal(n) + 1j * rng.standard_normal(n))
    return z * (peak / np.abs(z).max())


def quantise(z, fmt):
    """(i, q) float32 as the device will see them: integers in -127 .. 127, or fractional floats with magnitudes in 1e-3 .. 1e3 (or zero)"""
    if fmt == "i8":
        return tuple(np.clip(np.round(v), -127, 127).astype(np.float32) for v in (z.real, z.imag))
    out = []
    for v in (z.real, z.imag):
        a = np.clip(np.abs(v), 1e-3, 1e3)
        out.append(np.where(v == 0, 0.0, np.sign(v) * a).astype(np.float32))
    return tuple(out)


class Built:
    """.case .i .q (float32, the capture from its first sample) .x (complex128 of them) .buf (what goes to the device: int8 [n, 2] or an
    (i, q) pair of float32 arrays, `start` other samples in front)"""


@functools.lru_cache(maxsize=None)
def build(name):
    c = by_name(name)
    n = needed(c.fft, c.n_slots)
    rng = np.random.default_rng(c.seed + 7)
    N, cp0, cpe, n_slot, _ = sm.geom(c.fft)
    if c.kind == "silence":
        z = np.zeros(n, np.complex128)
    elif c.kind == "const":  # every window's acc EQUALS the mean (3 x 9^2 = 243, 960 of them sum exactly): the gate's '<=' clears them all
        z = np.ones(n, np.complex128)
    elif c.kind == "gauss":
        z = 3.0 * (rng.standard_normal(n) + 1j * rng.standard_normal(n))
    elif c.kind == "few":  # weak noise, and in every slot, at a window and at its fourth-symbol partner, two neighbouring samples A, A repeated N
        # later as A, -A: the products +|A|^2 and -|A|^2 cancel in every window that holds both, so ONE window before and ONE after survive
        # the mean gate at either place -- four survivors, two peaks
        z = np.round(1.5 * (rng.standard_normal(n) + 1j * rng.standard_normal(n)))
        fourth = N + cp0 + (N + cpe) * 3
        for s in range(c.n_slots + 1):
            for p in (400, 400 + fourth):
                a = s * n_slot + p
                if a + 1 + N < n:
                    z[a] = z[a + 1] = z[a + N] = 100 + 60j
                    z[a + 1 + N] = -(100 + 60j)
    else:
        z = mix(c, c.cells, n)
        if c.kind == "60db":
            z = z * np.where((np.arange(n) % n_slot) < n_slot // 2, 5.0, 5e-3)
    b = Built()
    b.case = c
    b.i, b.q = quantise(z, c.fmt)
    b.x = b.i.astype(np.float64) + 1j * b.q.astype(np.float64)
    ji, jq = (rng.integers(-50, 51, c.start).astype(np.float32) + (0.25 if c.fmt == "f32" else 0.0) for _ in range(2))
    fi, fq = np.concatenate([ji, b.i]), np.concatenate([jq, b.q])
    b.buf = np.ascontiguousarray(np.stack([fi, fq], 1).astype(np.int8)) if c.fmt == "i8" else (np.ascontiguousarray(fi), np.ascontiguousarray(fq))
    return b


@functools.lru_cache(maxsize=None)
def expected(name):
    """the model's Search of a listed case.  Cached: read-only."""
    c, b = by_name(name), build(name)
    return sm.search(b.x, c.fft, c.n_rb, c.n_slots)


@functools.lru_cache(maxsize=None)
def restated(name):
    """(corr complex64 [n_slots, n_slot], acc float32 [n_slot]): the float32 restatements on the case's samples.  Cached: read-only."""
    c, b = by_name(name), build(name)
    corr = sm.cp_corr_f32(b.i, b.q, c.fft, c.n_slots)
    return corr, sm.cp_accum_f32(corr)


def cell_hits(c, found):
    """every cell of the case is among found [(N_id_cell, frame_start)], its frame start within slack(fft) of its delay modulo a frame"""
    n_frame = sm.geom(c.fft)[4]
    return all(any(cell == fc and min((fs - delay) % n_frame, (delay - fs) % n_frame) <= slack(c.fft) for fc, fs in found) for cell, delay, _ in c.cells)


# ---- the library's own float32 sequences (host code, no kernel): what k_seq_corr is restated with

@functools.lru_cache(maxsize=None)
def lib_pss(n_id_2, n_rb=6):
    """complex64 [62]: the PSS as the library's host transmitter writes it (cosf / sinf of the reference's expression, liblte_phy.cc:8342-8368)"""
    import openlte_amd as m
    t = m.Transmitter(128, n_rb, n_id_2)
    t.clear()
    assert t.L.mi_lte_map_pss(n_rb, 12, n_id_2, 1, t.re, t.im) == 0
    k = 6 * n_rb - 31
    out = (t.re[0, 6, k:k + 62] + 1j * t.im[0, 6, k:k + 62]).astype(np.complex64)
    t.close()
    return out


def pss_candidates_f32(n_rb):
    seqs, z0 = sm.pss_candidates(n_rb)
    return np.stack([lib_pss(q // 3) for q in range(9)]), z0


def sss_candidates_f32(n_id_2, n_rb):
    seqs, z0 = sm.sss_candidates(n_id_2, n_rb)
    return seqs.astype(np.complex64), z0  # +-1: exact


def rows_f32(rows, n_rb):
    """(re, im) float32 [n_rows, N_sc] of tapped rows [n_rows, 2, 1200]"""
    return rows[:, 0, :12 * n_rb], rows[:, 1, :12 * n_rb]


def stockham_rows(b, fft, n_rb, wins):
    """(re, im) float32 [len(wins), N_sc]: dl_frontend_cases.stockham_f32 on the windows of the float32 samples, in the grid's column order"""
    import dl_frontend_cases as dc
    half = 6 * n_rb
    yr, yi = dc.stockham_f32(np.stack([b.i[w:w + fft] for w in wins]), np.stack([b.q[w:w + fft] for w in wins]))
    return np.concatenate([yr[:, fft - half:], yr[:, 1:half + 1]], axis=1), np.concatenate([yi[:, fft - half:], yi[:, 1:half + 1]], axis=1)


def rows_floor(b, fft, n_rb, wins, want):
    """worst rel-L2 over `want` (the model's rows at the windows) of the float32 Stockham transform on the same windows"""
    yr, yi = stockham_rows(b, fft, n_rb, wins)
    return float(sm.rel_l2(yr.astype(np.float64) + 1j * yi.astype(np.float64), want).max())


# ---- e: single symbols.  FFT 128, 6 RB, planar float

SYM_FFT, SYM_RB, SYM_GAIN, SYM_LEAD = 128, 6, 8.0, 16
SYM_LEN = 137


def _symbol(grid_fn, sym, shift=0, half=False):
    """complex128 [137]: symbol `sym` (its 9-sample prefix and body) of a Transmitter subframe whose grid grid_fn(t) filled; shift: the grid
    row moved by so many columns first (a sub-carrier offset as the PSS search hypothesises it, :5360-5365); half: the row given the phase
    ramp of half a sample's delay, exp(-i pi k / N) at sub-carrier k"""
    import openlte_amd as m
    t = m.Transmitter(SYM_FFT, SYM_RB, 0)
    t.clear()
    grid_fn(t)
    if shift:
        t.re[0, sym], t.im[0, sym] = np.roll(t.re[0, sym], shift), np.roll(t.im[0, sym], shift)
    if half:
        n_sc = 12 * SYM_RB
        k = np.concatenate([np.arange(-n_sc // 2, 0), np.arange(1, n_sc // 2 + 1)])
        g = (t.re[0, sym, :n_sc] + 1j * t.im[0, sym, :n_sc]) * np.exp(-1j * np.pi * k / SYM_FFT)
        t.re[0, sym, :n_sc], t.im[0, sym, :n_sc] = g.real, g.imag
    i, q = t.samples()
    t.close()
    a = sym * SYM_LEN + (1 if sym else 0)  # the first symbol's prefix is one sample longer at this size
    return SYM_GAIN * (i[a:a + SYM_LEN].astype(np.float64) + 1j * q[a:a + SYM_LEN].astype(np.float64))


def sss_symbol(n_id_1, n_id_2, half):
    def fill(t):
        assert t.L.mi_lte_map_sss(SYM_RB, 12, 5 * half, n_id_1, n_id_2, 1, t.re, t.im) == 0
    return _symbol(fill, 5)


def pss_symbol(n_id_2, shift=0, half=False):
    def fill(t):
        assert t.L.mi_lte_map_pss(SYM_RB, 12, n_id_2, 1, t.re, t.im) == 0
    return _symbol(fill, 6, shift, half)


SSS_CASES = [(i, k, h) for k in range(3) for i in range(168) for h in range(2)]  # 1008: (N_id_1, N_id_2, half-frame)


@functools.lru_cache(maxsize=None)
def sss_family():
    """(i, q, symb5 [1008]): the 1008 symbols back to back behind SYM_LEAD zeros; symb5[n] is the symb_starts[5] whose window opens ON symbol
    n's body (one sample early already costs a third of the coherent sum at this size: sin(62 pi / 128) / (62 sin(pi / 128)) = 0.66)"""
    z = np.zeros(SYM_LEAD + len(SSS_CASES) * SYM_LEN + SYM_FFT, np.complex128)
    symb5 = np.zeros(len(SSS_CASES), np.uint32)
    for n, (i, k, h) in enumerate(SSS_CASES):
        a = SYM_LEAD + n * SYM_LEN
        z[a:a + SYM_LEN] = sss_symbol(i, k, h)
        symb5[n] = a + 9 - 9
    i, q = quantise(z, "f32")
    return i, q, symb5


@functools.lru_cache(maxsize=None)
def sss_family_model():
    """(corr complex128 [1008, 336], amplitude [1008]): the model's correlations of every symbol, and its mean magnitude on the 62 sub-carriers"""
    i, q, symb5 = sss_family()
    x = i.astype(np.float64) + 1j * q.astype(np.float64)
    rows = dm.rows_at(x, SYM_FFT, SYM_RB, [int(s) + 9 for s in symb5])
    corr = np.zeros((len(SSS_CASES), 336), np.complex128)
    for k in range(3):
        sel = [n for n, c in enumerate(SSS_CASES) if c[1] == k]
        seqs, z0 = sm.sss_candidates(k, SYM_RB)
        corr[sel] = sm.seq_corr(rows[sel], seqs, z0)
    return corr, np.abs(rows[:, 6 * SYM_RB - 31:6 * SYM_RB + 31]).mean(1)


PSS_CASES = [(k, sft) for k in range(3) for sft in (-1, 0, 1)]
PSS_SLOT, PSS_SYMB = 7, 3  # where the lone PSS symbol stands among the 84 searched


@functools.lru_cache(maxsize=None)
def pss_family(n_id_2, shift, tie=False):
    """(i, q, symb_starts [7]): 14 silent slots with one PSS symbol's body (no prefix) as symbol PSS_SYMB of slot PSS_SLOT of the given
    symb_starts: the first pass's window opens one sample before the body, the fine timing has ONE best offset, +1 (the window on the body).
    tie (family f): the symbol delayed by half a sample and followed by one sample of cyclic suffix, so that the windows at offsets +1 and +2
    see it half a sample late and half a sample early: the same magnitude but for rounding, 62 A sin(31 pi / 128) / (62 sin(pi / 256)) = 0.905 x 62 A."""
    N, cp0, cpe, n_slot, _ = sm.geom(SYM_FFT)
    ss = np.array([50 + j * SYM_LEN for j in range(7)], np.uint32)
    z = np.zeros(14 * n_slot, np.complex128)
    body = int(ss[PSS_SYMB]) + PSS_SLOT * n_slot + cp0  # the search's window opens at body - 1
    s = pss_symbol(n_id_2, shift, tie)
    z[body:body + N] = s[9:]
    if tie:
        z[body + N] = s[9]
    i, q = quantise(z, "f32")
    return i, q, ss
