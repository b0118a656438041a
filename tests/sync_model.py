"""A float64 model of the three synchronisation searches (mi_lte_coarse_timing_run, mi_lte_find_pss_run, mi_lte_find_sss_run), written from
36.211 6.11 and the reference's liblte_phy_dl_find_coarse_timing_and_freq_offset, liblte_phy_find_pss_and_fine_timing and
liblte_phy_find_sss (liblte_phy.cc:5697-5852, :5306-5510, :5578-5687).  Nothing here restates a kernel of sync.hip: the sequences come from
the standard's formulas, the transform is numpy's FFT on dl_frontend_model's row extraction, the sliding cyclic-prefix sums are differences
of one cumulative sum.

Three layers:
  the model         float64 / complex128: cp_corr, cp_accum, seq_corr, pss_seq, sss_seq
  the decisions     the reference's expressions in float32 and in its loop order, on an `acc` or correlation ARRAY given as an argument, so
                    that one function judges the model's numbers and a device's: coarse_decide, coarse_freq, pss_decide, fine_decide, sss_decide
  the restatements  float32 numpy, one array operation per term, nothing fused, the serial order of the reference's loops
                    (liblte_phy.cc:5735-5741 and its like): cp_corr_f32, cp_accum_f32, seq_corr_f32.  Their distance from the model is what
                    float32 costs on a case; a device that keeps the reference's order equals them bit for bit."""
import numpy as np

import dl_frontend_model as dm

PSS_ROOTS = (25, 29, 34)  # 36.211 table 6.11.1.1-1
N_PEAKS_MAX = 5           # LIBLTE_PHY_N_MAX_ROUGH_CORR_SEARCH_PEAKS
ABS_CORR_LEN = 2 * 15360  # dl_timing_abs_corr[LIBLTE_PHY_N_SAMPS_PER_SLOT_30_72MHZ * 2]


def geom(fft):
    """(N, cp0, cpe, n_slot, n_frame)"""
    sc = 2048 // fft
    return fft, 160 // sc, 144 // sc, 15360 // sc, 307200 // sc


# ---- 36.211 6.11: the sequences

def pss_seq(n_id_2):
    """complex128 [62]: d_u(n) of 6.11.1.1"""
    u = PSS_ROOTS[n_id_2]
    n = np.arange(62)
    return np.where(n < 31, np.exp(-1j * np.pi * u * n * (n + 1) / 63.0), np.exp(-1j * np.pi * u * (n + 1) * (n + 2) / 63.0))


def _m_seq(taps):
    """1 - 2 x(i), i = 0 .. 30, of x(i + 5) = sum of x(i + t) over taps mod 2 from x(0 .. 4) = 0, 0, 0, 0, 1"""
    x = [0, 0, 0, 0, 1]
    for i in range(26):
        x.append(sum(x[i + t] for t in taps) % 2)
    return 1 - 2 * np.array(x)


def sss_m0_m1(n_id_1):
    """(m0, m1) of 6.11.2.1 (table 6.11.2.1-1)"""
    qp = n_id_1 // 30
    q = (n_id_1 + qp * (qp + 1) // 2) // 30
    mp = n_id_1 + q * (q + 1) // 2
    m0 = mp % 31
    return m0, (m0 + mp // 31 + 1) % 31


def sss_seq(n_id_1, n_id_2):
    """(d in subframe 0, d in subframe 5), float64 [62] each: 6.11.2.1"""
    s, c, z = _m_seq((2, 0)), _m_seq((3, 0)), _m_seq((4, 2, 1, 0))
    m0, m1 = sss_m0_m1(n_id_1)
    n = np.arange(31)
    s0, s1 = s[(n + m0) % 31], s[(n + m1) % 31]
    c0, c1 = c[(n + n_id_2) % 31], c[(n + n_id_2 + 3) % 31]
    z0, z1 = z[(n + m0 % 8) % 31], z[(n + m1 % 8) % 31]
    d0, d5 = np.zeros(62), np.zeros(62)
    d0[0::2], d0[1::2] = s0 * c0, s1 * c1 * z0
    d5[0::2], d5[1::2] = s1 * c0, s0 * c1 * z1
    return d0, d5


def pss_candidates(n_rb):
    """(seqs complex128 [9, 62], z0 [9]): PSS k one sub-carrier down, in place, one up -- column 3 k + sft, first grid column of each
    (liblte_phy.cc:5357-5366)"""
    return np.stack([pss_seq(k) for k in range(3) for _ in range(3)]), np.array([6 * n_rb - 31 + sft - 1 for _ in range(3) for sft in range(3)])


def sss_candidates(n_id_2, n_rb):
    """(seqs float64 [336, 62], z0 [336]): N_id_1 i in subframe 0 at 2 i, in subframe 5 at 2 i + 1"""
    return np.stack([d for i in range(168) for d in sss_seq(i, n_id_2)]), np.full(336, 6 * n_rb - 31)


# ---- the model's sums

def cp_corr(x, fft, n_slots, start=0):
    """complex128 [n_slots, n_slot]: sum over j < cp of conj(x[b + j]) x[b + j + N], b = start + slot n_slot + i (:5731-5742: re = i i' + q q',
    im = i q' - q i').  One cumulative sum (in long double: a capture may span 120 dB in power), a difference per window."""
    N, _, cp, n_slot, _ = geom(fft)
    n = n_slots * n_slot + cp
    x = np.asarray(x[start:start + n + N], np.complex128)
    p = np.conj(x[:n]) * x[N:N + n]
    out = []
    for part in (p.real, p.imag):
        cs = np.concatenate([[0], np.cumsum(part.astype(np.longdouble))])
        out.append((cs[cp:cp + n_slots * n_slot] - cs[:n_slots * n_slot]).astype(np.float64))
    return (out[0] + 1j * out[1]).reshape(n_slots, n_slot)


def cp_accum(corr):
    """float64 [n_slot]: sum over the slots of |corr|^2 (:5741)"""
    return (np.abs(np.asarray(corr, np.complex128)) ** 2).sum(0)


def seq_corr(rows, seqs, z0):
    """complex128 [n_rows, n_seq]: sum over t < 62 of conj(rows[r, z0[q] + t]) seqs[q, t] -- the reference's re = r_re s_re + r_im s_im,
    im = r_re s_im - r_im s_re (:5394-5405; its sum runs over every sub-carrier, the sequence is zero on the others)"""
    rows, seqs, z0 = np.asarray(rows, np.complex128), np.asarray(seqs, np.complex128), np.asarray(z0)
    out = np.zeros((rows.shape[0], len(z0)), np.complex128)
    for z in np.unique(z0):
        out[:, z0 == z] = np.conj(rows[:, z:z + 62]) @ seqs[z0 == z].T
    return out


# ---- window starts (sample indices from the capture's first sample)

def pss_windows(symb_starts, fft):
    """[84]: row 7 i + j is symbol j of slot i, one sample inside the end of a first-symbol prefix (samples_to_symbols_dl, :8592-8634)"""
    _, cp0, _, n_slot, _ = geom(fft)
    return [int(symb_starts[j]) + n_slot * i + cp0 - 1 for i in range(12) for j in range(7)]


def fine_windows(symb_starts, pss_symb, fft):
    """[80]: offsets -40 .. 39 around symbol pss_symb; a negative offset that would pass sample 0 is not applied (:5454-5465)"""
    _, cp0, _, n_slot, _ = geom(fft)
    base = int(symb_starts[pss_symb % 7]) + n_slot * (pss_symb // 7)
    return [(base + i if (i >= 0 or base >= -i) else base) + cp0 - 1 for i in range(-40, 40)]


def sss_window(symb_starts, fft):
    return int(symb_starts[5]) + geom(fft)[1] - 1


# ---- the reference's decisions, float32, in its loop order

def _f32(x):
    return np.asarray(x, np.float32)


def mag32(c):
    """abs_corr = sqrt(re*re + im*im): a float expression, the double sqrt, stored as float"""
    re, im = _f32(np.real(c)), _f32(np.imag(c))
    return np.sqrt(_f32(_f32(re * re) + _f32(im * im)).astype(np.float64)).astype(np.float32)


class Coarse:
    """.n_peaks .peaks [n_peaks] .symb_starts uint32 [5, 7] (zero rows past n_peaks) .mean float32 .survivors (windows above the mean)
    .walk [n_peaks] (steps of `while (tmp_idx > 0)`) .wrapped [n_peaks] (blanking indices that wrapped below zero and were skipped)"""


def coarse_decide(acc, fft):
    """The mean gate, first x fourth symbol, five rounds of arg-max and blanking, symbol starts (:5745-5806, :5835-5846) on acc float [n_slot]"""
    N, cp0, cpe, ns, _ = geom(fft)
    sym_else = N + cpe
    n_blank = sym_else // 10
    a = _f32(acc).copy()
    assert a.shape == (ns,)
    c = np.zeros(ABS_CORR_LEN + 1, np.float32)
    r = Coarse()
    r.mean = np.float32(np.cumsum(a, dtype=np.float32)[-1] / np.float32(ns))  # a serial float sum, then float / float
    low = a <= r.mean
    a[low] = 0
    c[:ns], c[ns:2 * ns] = a, a
    r.survivors = int((~low).sum())
    fourth = N + cp0 + sym_else * 3
    c[:ns] = _f32(c[:ns] * c[fourth:fourth + ns].copy())  # (ascending i reads fourth + i > i before it is overwritten)
    r.peaks, r.walk, r.wrapped, r.n_peaks = [], [], [], N_PEAKS_MAX
    for i in range(N_PEAKS_MAX):
        j = int(np.argmax(c[:ns]))  # first maximum: strict '>' in ascending order from abs_corr_max = 0
        if not c[j] > 0:
            r.n_peaks = i
            break
        t, walk, wrapped = j, 0, 0
        while t > 0:
            t, walk = t - sym_else, walk + 1
        for _ in range(7):
            t += sym_else
            idx = (t - n_blank // 2 + np.arange(n_blank)) % (1 << 32)  # uint32 idx: a position below zero wraps and fails the bound
            wrapped += int((idx >= ABS_CORR_LEN + 1).sum())
            c[idx[idx < ABS_CORR_LEN]] = 0  # (the reference's '<=' also clears one float past its array, which nothing reads)
        r.peaks.append(j)
        r.walk.append(walk)
        r.wrapped.append(wrapped)
    r.symb_starts = np.zeros((5, 7), np.uint32)
    for i, j in enumerate(r.peaks):
        t = j - sym_else * r.walk[i]
        r.symb_starts[i] = [(t + (k + 1) * sym_else) % (1 << 32) for k in range(7)]
    return r


def coarse_freq(pk, fft, single=True):
    """freq_offset [n_peaks] from pk complex64 [n_peaks, n_slots], the cyclic-prefix sums at the peaks (:5814-5833): per slot, in slot order,
    freq_err (float) += atan2f(im, re) / (double); then / N_slots.  single=False: the same in float64 throughout."""
    N, _, _, n_slot, _ = geom(fft)
    den = N * 2 * np.pi * (0.0005 / n_slot)
    pk = np.asarray(pk, np.complex64)
    if not single:
        return (np.arctan2(pk.imag.astype(np.float64), pk.real.astype(np.float64)) / den).sum(1) / pk.shape[1]
    err = np.zeros(pk.shape[0], np.float32)
    for s in range(pk.shape[1]):
        err = (err.astype(np.float64) + np.arctan2(pk[:, s].imag, pk[:, s].real).astype(np.float32).astype(np.float64) / den).astype(np.float32)
    return _f32(err / np.float32(pk.shape[1]))


def pss_decide(corr, n_id_2=0, pss_symb=0):
    """(N_id_2, pss_symb, shift, corr_max) from corr [84, 9]: strict '>' over symbols, roots, shifts -1 0 +1 in that order (:5370-5433).  Where
    nothing exceeds 0 the reference leaves the caller's N_id_2 and pss_symb (and its own shift unset: 0 here, as in the library)."""
    m = mag32(corr).reshape(-1)
    assert m.shape == (84 * 9,)
    j = int(np.argmax(m))
    if not m[j] > 0:
        return n_id_2, pss_symb, 0, np.float32(0)
    return (j % 9) // 3, j // 9, j % 3 - 1, m[j]


def fine_decide(fcorr, symb_starts, pss_symb, fft):
    """(timing, pss_thresh float32, symb_starts uint32 [7] rewritten) from fcorr [80] (:5449-5504), the arithmetic in uint32 as there"""
    N, cp0, cpe, n_slot, n_frame = geom(fft)
    m = mag32(fcorr)
    assert m.shape == (80,)
    j = int(np.argmax(m))
    timing, thresh = (j - 40, m[j]) if m[j] > 0 else (0, np.float32(0))
    M = 1 << 32
    t = (int(symb_starts[pss_symb % 7]) + n_slot * (pss_symb // 7) + timing) % M
    while (t + N + cpe) % M < n_slot:
        t = (t + n_frame) % M
    out = [(t + (N + cpe) - n_slot) % M] + [(t + (N + cpe) * i + N + cp0 - n_slot) % M for i in range(1, 7)]
    return timing, thresh, np.array(out, np.uint32)


def sss_decide(corr, pss_thresh, symb_starts, fft):
    """(found, N_id_1, frame_start, symb_starts uint32 [7]) from corr [336]: the FIRST of subframe 0's then subframe 5's sequence of
    N_id_1 = 0, 1, ... above float(pss_thresh * 0.9) (:5626-5682); not found: zeros, symb_starts as given"""
    N, cp0, cpe, n_slot, n_frame = geom(fft)
    thresh = np.float32(np.float64(np.float32(pss_thresh)) * 0.9)
    m = mag32(corr)
    assert m.shape == (336,)
    ss = np.array(symb_starts, np.uint32)
    hit = np.nonzero(m > thresh)[0]
    if len(hit) == 0:
        return False, 0, 0, ss
    i, h = int(hit[0]) // 2, int(hit[0]) % 2
    back = (N + cpe) * 4 + N + cp0 + (n_slot * 10 if h else 0)
    s5 = int(ss[5])
    while s5 < back:
        s5 = (s5 + n_frame) % (1 << 32)
    ss[5] = s5
    return True, i, s5 - back, ss


# ---- the float32 restatements

def cp_corr_f32(i, q, fft, n_slots, start=0):
    """complex64 [n_slots, n_slot] of float32 samples i, q: corr_re += i i' + q q', corr_im += i q' - q i', j ascending (:5735-5740), every
    product and every sum rounded to float32"""
    N, _, cp, n_slot, _ = geom(fft)
    i, q = _f32(i), _f32(q)
    n = n_slots * n_slot
    re, im = np.zeros(n, np.float32), np.zeros(n, np.float32)
    for j in range(cp):
        a, b = start + j, start + j + N
        xi, xq, yi, yq = i[a:a + n], q[a:a + n], i[b:b + n], q[b:b + n]
        re = _f32(re + _f32(_f32(xi * yi) + _f32(xq * yq)))
        im = _f32(im + _f32(_f32(xi * yq) - _f32(xq * yi)))
    return (re + 1j * im).astype(np.complex64).reshape(n_slots, n_slot)


def cp_accum_f32(corr):
    """float32 [n_slot]: abs_corr[i] += re*re + im*im, slot by slot (:5741)"""
    corr = np.asarray(corr, np.complex64)
    acc = np.zeros(corr.shape[1], np.float32)
    for s in range(corr.shape[0]):
        re, im = corr[s].real, corr[s].imag
        acc = _f32(acc + _f32(_f32(re * re) + _f32(im * im)))
    return acc


def seq_corr_f32(rows_re, rows_im, seqs, z0):
    """complex64 [n_rows, n_seq] of float32 rows [n_rows, N_sc] and seqs complex64 [n_seq, 62]: re += r_re s_re + r_im s_im,
    im += r_re s_im - r_im s_re over the 62 sub-carriers in ascending order (:5392-5405; the zero sub-carriers add +0)"""
    rows_re, rows_im, seqs = _f32(rows_re), _f32(rows_im), np.asarray(seqs, np.complex64)
    z0 = np.asarray(z0)
    re, im = np.zeros((rows_re.shape[0], len(z0)), np.float32), np.zeros((rows_re.shape[0], len(z0)), np.float32)
    for t in range(62):
        rr, ri = rows_re[:, z0 + t], rows_im[:, z0 + t]
        sr, si = seqs[:, t].real[None, :], seqs[:, t].imag[None, :]
        re = _f32(re + _f32(_f32(rr * sr) + _f32(ri * si)))
        im = _f32(im + _f32(_f32(rr * si) - _f32(ri * sr)))
    return (re + 1j * im).astype(np.complex64)


# ---- the whole search on the model's own numbers

class Peak:
    """.symb_starts_in .rows .corr .n_id_2 .pss_symb .shift .fine_rows .fine_corr .timing .pss_thresh .symb_starts .sss_row .sss_corr .found
    .n_id_1 .frame_start .symb_starts_out"""


def pss_stage(x, fft, n_rb, symb_starts, pss_table=None):
    """the PSS search and fine timing of one coarse peak on complex samples x (from the capture's first sample).  pss_table [3, 62]: the three
    sequences to correlate with in place of the standard's -- the reference evaluates cosf / sinf of the phase ROUNDED TO FLOAT (up to 6600 rad:
    2.4e-4 rad of rounding), which moves a correlation by 1e-5 of itself; the exact tie of family f is a tie only with the sent table."""
    p = Peak()
    p.symb_starts_in = np.array(symb_starts, np.uint32)
    seqs, z0 = pss_candidates(n_rb)
    if pss_table is not None:
        seqs = np.stack([np.asarray(pss_table[q // 3], np.complex128) for q in range(9)])
    p.rows = dm.rows_at(x, fft, n_rb, pss_windows(symb_starts, fft))
    p.corr = seq_corr(p.rows, seqs, z0)
    p.n_id_2, p.pss_symb, p.shift, _ = pss_decide(p.corr)
    q = 3 * p.n_id_2 + p.shift + 1
    p.fine_rows = dm.rows_at(x, fft, n_rb, fine_windows(symb_starts, p.pss_symb, fft))
    p.fine_corr = seq_corr(p.fine_rows, seqs[q:q + 1], z0[q:q + 1])[:, 0]
    p.timing, p.pss_thresh, p.symb_starts = fine_decide(p.fine_corr, symb_starts, p.pss_symb, fft)
    return p


def sss_stage(x, fft, n_rb, p):
    seqs, z0 = sss_candidates(p.n_id_2, n_rb)
    p.sss_row = dm.rows_at(x, fft, n_rb, [sss_window(p.symb_starts, fft)])
    p.sss_corr = seq_corr(p.sss_row, seqs, z0)[0]
    p.found, p.n_id_1, p.frame_start, p.symb_starts_out = sss_decide(p.sss_corr, p.pss_thresh, p.symb_starts, fft)
    return p


class Search:
    """.corr complex128 [n_slots, n_slot] .acc float64 [n_slot] .coarse (Coarse) .freq_offset float32 [n_peaks] .peaks [n_peaks] of Peak"""


def search(x, fft, n_rb, n_slots, stages=True):
    """The scanner's sequence on complex samples x from the capture's first sample: coarse timing, then PSS and SSS per coarse peak"""
    r = Search()
    r.corr = cp_corr(x, fft, n_slots)
    r.acc = cp_accum(r.corr)
    r.coarse = coarse_decide(r.acc, fft)
    r.freq_offset = coarse_freq(r.corr[:, r.coarse.peaks].T, fft) if r.coarse.n_peaks else np.zeros(0, np.float32)
    r.peaks = [sss_stage(x, fft, n_rb, pss_stage(x, fft, n_rb, r.coarse.symb_starts[i])) for i in range(r.coarse.n_peaks)] if stages else []
    return r


def cells_found(r):
    """[(N_id_cell, frame_start)] of a Search"""
    return [(3 * p.n_id_1 + p.n_id_2, p.frame_start) for p in r.peaks if p.found]


def rel_l2(got, want):
    """rel-L2 over the last axis"""
    got, want = np.asarray(got, np.complex128), np.asarray(want, np.complex128)
    return np.sqrt((np.abs(got - want) ** 2).sum(-1) / np.maximum((np.abs(want) ** 2).sum(-1), 1e-300))
