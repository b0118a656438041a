"""float64 numpy model of MI_LTE_DEMAP_MAXLOG on a transmit-diversity plan (include/mi_lte.h, "PDSCH, 3GPP mode: transmit diversity on 2 or 4
ports"): the resource elements of an allocation of a 2- or 4-port cell in the demodulator's order, their grouping into element pairs by index
alone, the pair's ports, z / w / t of the header's text, the automatic gain, the rounding and the descrambling.  The LLR arithmetic, the soft
byte, the guard band and the scrambling sequence are tests/demap_llr_model.py's, by import.  tests/test_txdiv_gpu.py compares the kernel's
bytes and gains with it; tests/test_txdiv_cpu.py checks the combiner itself."""
import numpy as np

from demap_llr_model import A_LIT, FOUR_A2, N_SC, QM, Demapped, gold, in_guard, llr_axis, soft_byte, sync_window  # noqa: F401

RS2 = 0.70710678118654752  # 1 / sqrt 2, the kernel's literal


def pdsch_res(al, sf, cell, n_rb, cfi, n_ant):
    """Plane indices L * 1200 + sub-carrier of the allocation's resource elements, in the demodulator's order, for a cell of n_ant ports
    (36.211 6.10.1.2: ports 0 / 1 take sub-carriers k = cell mod 3 (mod 3) in symbols 0 and 4 of a slot, ports 2 / 3 the same in symbol 1)."""
    first, last = sync_window(n_rb)
    cfi = al.n_pdcch_symbs if al.n_pdcch_symbs else cfi
    out = []
    j = np.arange(12)
    for L in range(cfi, 14):
        l7 = L % 7
        win = (sf == 0 and 7 <= L <= 10) or (sf in (0, 5) and L in (5, 6))
        for i in range(al.N_prb):
            sc = al.prb[1 if L >= 7 else 0][i] * 12 + j
            keep = np.ones(12, bool)
            if n_ant == 1:
                if l7 == 0:
                    keep &= (j % 6) != cell % 6
                elif l7 == 4:
                    keep &= (j % 6) != (cell + 3) % 6
            elif l7 in (0, 4) or (n_ant == 4 and l7 == 1):
                keep &= (j % 3) != cell % 3
            if win:
                keep &= (sc < first) | (sc > last)
            out.append(L * N_SC + sc[keep])
    return np.concatenate(out) if out else np.zeros(0, np.int64)


def pair_ports(n_pairs, n_ant):
    """(pa, pb) per element pair n: (0, 1) on two ports; on four, (0, 2) for even n and (1, 3) for odd n"""
    n = np.arange(n_pairs)
    if n_ant == 2:
        return np.zeros(n_pairs, np.int64), np.ones(n_pairs, np.int64)
    return n % 2, n % 2 + 2


def combine(ya, yb, ha_a, hb_b, ha_b, hb_a):
    """The header's combiner for arrays of element pairs (complex128): (t0, w0, t1, w1).  ha_a = h_pa(a), hb_b = h_pb(b), ha_b = h_pa(b),
    hb_a = h_pb(a).  Real arithmetic in the kernel's order of operations."""
    ar, ai, br, bi = ya.real, ya.imag, yb.real, yb.imag
    h0r, h0i, h1r, h1i, h2r, h2i, h3r, h3i = ha_a.real, ha_a.imag, hb_b.real, hb_b.imag, ha_b.real, ha_b.imag, hb_a.real, hb_a.imag
    z0r = ((h0r * ar + h0i * ai) + h1r * br) + h1i * bi
    z0i = ((h0r * ai - h0i * ar) + h1i * br) - h1r * bi
    z1r = ((h2r * br + h2i * bi) - h3r * ar) - h3i * ai
    z1i = ((h2r * bi - h2i * br) - h3i * ar) + h3r * ai
    w0 = ((h0r * h0r + h0i * h0i) + (h1r * h1r + h1i * h1i)) * 0.5
    w1 = ((h2r * h2r + h2i * h2i) + (h3r * h3r + h3i * h3i)) * 0.5
    return (z0r + 1j * z0i) * RS2, w0, (z1r + 1j * z1i) * RS2, w1


def symbols(planes, re, n_ant):
    """(t complex128 [M_symb], w [M_symb]) of one allocation: planes float64 [2 + 2 n_ant, 16 * 1200] (y_re, y_im, h_re of every port, h_im of
    every port), re its resource elements."""
    m = len(re) // n_ant * n_ant
    a, b = re[0:m:2], re[1:m:2]
    pa, pb = pair_ports(m // 2, n_ant)
    y = planes[0] + 1j * planes[1]
    h = planes[2:2 + n_ant] + 1j * planes[2 + n_ant:2 + 2 * n_ant]
    t0, w0, t1, w1 = combine(y[a], y[b], h[pa, a], h[pb, b], h[pa, b], h[pb, a])
    t, w = np.zeros(m, np.complex128), np.zeros(m)
    t[0::2], t[1::2], w[0::2], w[1::2] = t0, t1, w0, w1
    return t, w


def llr_symbols(t, w, mod):
    """[n, Q_m] LLRs from (t, w): bit 2k on the real axis, 2k + 1 on the imaginary (demap_llr_model.llr_axis, unchanged)"""
    out = np.zeros((len(t), QM[mod]))
    with np.errstate(all="ignore"):
        out[:, 0::2] = np.stack(llr_axis(t.real, w, mod), 1)
        out[:, 1::2] = np.stack(llr_axis(t.imag, w, mod), 1)
    return out


def auto_gain(w, mod, T):
    """T / (4 A^2 wbar) as the float the kernel scales with; 0 for a wbar that is 0 or not finite.  (the float value, the unrounded one)"""
    with np.errstate(all="ignore"):
        wbar = w.sum() / len(w) if len(w) else np.nan
        g = T / (FOUR_A2[mod] * wbar)
        ok = np.isfinite(wbar) and wbar > 0 and np.isfinite(np.float32(g))
    return (float(np.float32(g)), float(g)) if ok else (0.0, 0.0)


def demap(planes, allocs, sf, cell, n_rb, cfi, n_ant, gain=0.0, T=16):
    """planes: one unit's float32 [2 + 2 n_ant, 16, 1200]; allocs: its allocations; gain 0: automatic.  One demap_llr_model.Demapped each."""
    p = np.asarray(planes, np.float32).reshape(2 + 2 * n_ant, -1).astype(np.float64)
    out = []
    for al in allocs:
        mod = al.mod_type
        t, w = symbols(p, pdsch_res(al, sf, cell, n_rb, cfi, n_ant), n_ant)
        if gain == 0:
            g_used, g_tap = auto_gain(w, mod, T)
        else:
            g_used = g_tap = float(np.float32(gain))
        with np.errstate(all="ignore"):
            x = (g_used * llr_symbols(t, w, mod)).reshape(-1)
        c = gold(((al.rnti << 14) | (sf << 9) | cell) & 0x7FFFFFFF, len(x))
        x = np.where(c == 1, -x, x)
        out.append(Demapped(soft_byte(x), g_tap, x, c))
    return out
