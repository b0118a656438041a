"""float64 numpy model of MI_LTE_DEMAP_MAXLOG (include/mi_lte.h, "PDSCH, 3GPP mode: max-log soft-decision demapping"): the resource elements
of every allocation of one single-port unit in the demodulator's order (symbol -> PRB -> sub-carrier, CRS and, in subframes 0 and 5, the PBCH /
PSS / SSS window left out), the max-log LLRs in their piecewise-linear form from z = y conj(h) and w = |h|^2, the gain, the rounding and the
descrambling.  The tests compare the kernel's bytes and gains with it (tests/test_demap_llr_gpu.py) and the piecewise form with the brute-force
minimum over the whole constellation (tests/test_demap_llr_cpu.py)."""
import numpy as np

N_SC = 1200
A = {1: 1 / np.sqrt(2.0), 2: 1 / np.sqrt(10.0), 3: 1 / np.sqrt(42.0)}
A_LIT = {1: 0.70710678118654752, 2: 0.31622776601683794, 3: 0.15430334996209191}  # the kernel's literals
FOUR_A2 = {1: 2.0, 2: 4.0 / 10, 3: 4.0 / 42}
QM = {1: 2, 2: 4, 3: 6}
GUARD = 2.0 ** -16


def gold(c_init, n):
    """36.211 7.2: c(i) = x1(i + 1600) ^ x2(i + 1600), 28 steps of the two recurrences per numpy operation"""
    N = 1600 + n
    x1, x2 = np.zeros(N + 62, np.uint8), np.zeros(N + 62, np.uint8)
    x1[0] = 1
    x2[:31] = [(c_init >> i) & 1 for i in range(31)]
    for i in range(0, N, 28):
        x1[i + 31:i + 59] = x1[i + 3:i + 31] ^ x1[i:i + 28]
        x2[i + 31:i + 59] = x2[i + 3:i + 31] ^ x2[i + 2:i + 30] ^ x2[i + 1:i + 29] ^ x2[i:i + 28]
    return x1[1600:N] ^ x2[1600:N]


def sync_window(n_rb):
    return {6: (0, 71), 15: (54, 125), 25: (114, 185), 50: (264, 335), 75: (414, 485)}.get(n_rb, (564, 635))


def pdsch_res(al, sf, cell, n_rb, cfi):
    """Plane indices L * 1200 + sub-carrier of the allocation's resource elements, in the demodulator's order (single port)."""
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
            if l7 == 0:
                keep &= (j % 6) != cell % 6
            elif l7 == 4:
                keep &= (j % 6) != (cell + 3) % 6
            if win:
                keep &= (sc < first) | (sc > last)
            out.append(L * N_SC + sc[keep])
    return np.concatenate(out) if out else np.zeros(0, np.int64)


def llr_axis(t, w, mod):
    """The max-log LLRs of one axis, piecewise linear in t = Re or Im of y conj(h) for w = |h|^2: a list of mod arrays (the sign bit, then the
    amplitude bits), operation for operation what the kernel computes."""
    a4 = 4 * A_LIT[mod]
    a8 = 8 * A_LIT[mod]
    a, D = np.abs(t), A_LIT[mod] * w
    if mod == 1:
        return [a4 * t]
    if mod == 2:
        return [np.where(a <= 2 * D, a4 * t, np.copysign(a8 * (a - D), t)), a4 * (2 * D - a)]
    k = np.where(a < 2 * D, 0.0, np.where(a < 4 * D, 1.0, np.where(a < 6 * D, 2.0, 3.0)))
    return [np.copysign(a4 * (k + 1) * (a - k * D), t),
            np.where(a < 2 * D, a8 * (3 * D - a), np.where(a < 6 * D, a4 * (4 * D - a), a8 * (5 * D - a))),
            np.where(a < 4 * D, a4 * (a - 2 * D), a4 * (6 * D - a))]


def llr_symbols(y, h, mod):
    """[n, Q_m] LLRs L_k of n received symbols y (complex128) over channel h: bit 2k on the real axis, 2k + 1 on the imaginary."""
    w = h.real * h.real + h.imag * h.imag
    zr = y.real * h.real + y.imag * h.imag
    zi = y.imag * h.real - y.real * h.imag
    out = np.zeros((len(y), QM[mod]))
    with np.errstate(all="ignore"):
        out[:, 0::2] = np.stack(llr_axis(zr, w, mod), 1)
        out[:, 1::2] = np.stack(llr_axis(zi, w, mod), 1)
    return out


def axis_levels(mod):
    """{axis bits (sign, amplitude bits..) -> level in units of A}: 36.211 7.1.2-7.1.4 per axis"""
    if mod == 1:
        return {(0,): 1, (1,): -1}
    if mod == 2:
        return {(s, m): (1 - 2 * s) * (1 if m == 0 else 3) for s in (0, 1) for m in (0, 1)}
    mag = {(0, 0): 3, (0, 1): 1, (1, 0): 5, (1, 1): 7}
    return {(s, m, n): (1 - 2 * s) * mag[(m, n)] for s in (0, 1) for m in (0, 1) for n in (0, 1)}


def constellation(mod):
    """(points complex128 [2^Q_m], labels uint8 [2^Q_m, Q_m]): bit string b0 b1 .. -> symbol"""
    lv, q = axis_levels(mod), QM[mod]
    pts, labels = [], []
    for v in range(1 << q):
        b = [(v >> (q - 1 - k)) & 1 for k in range(q)]
        pts.append(A[mod] * complex(lv[tuple(b[0::2])], lv[tuple(b[1::2])]))
        labels.append(b)
    return np.array(pts), np.array(labels, np.uint8)


def brute_llr(x, w, mod):
    """w (min over the symbols with bit k = 1 of |x - s|^2 - min over those with bit k = 0), over the full 2-D constellation"""
    pts, labels = constellation(mod)
    d = np.abs(x[:, None] - pts[None, :]) ** 2
    out = np.zeros((len(x), QM[mod]))
    for k in range(QM[mod]):
        out[:, k] = d[:, labels[:, k] == 1].min(1) - d[:, labels[:, k] == 0].min(1)
    return w[:, None] * out


def soft_byte(x):
    """clamp(rint(x), -127, 127), ties to even; 0 where x is not finite"""
    with np.errstate(all="ignore"):
        return np.where(np.isfinite(x), np.clip(np.rint(x), -127, 127), 0).astype(np.int8)


def in_guard(x):
    """|x - boundary| <= 2^-16 (1 + |x|) for a rounding or clamp boundary (the half-integers up to +-127.5)"""
    ax = np.abs(x)
    d = np.abs(ax - (np.floor(ax) + 0.5))
    return np.isfinite(x) & (d <= GUARD * (1 + ax)) & (ax <= 127.5 + GUARD * 129)


def auto_gain(w, mod, T):
    """T / (4 A^2 wbar) as the float the kernel scales with; 0 for a wbar that is 0 or not finite.  Returns (the float value, the unrounded one)."""
    with np.errstate(all="ignore"):
        wbar = w.sum() / len(w) if len(w) else np.nan
        g = T / (FOUR_A2[mod] * wbar)
        ok = np.isfinite(wbar) and wbar > 0 and np.isfinite(np.float32(g))
    return (float(np.float32(g)), float(g)) if ok else (0.0, 0.0)


class Demapped:
    """One allocation: bytes (int8, descrambled), gain (what the tap must hold: the argument, or the automatic gain before its rounding to
    float), x (the unrounded g L, descrambled), c (the scrambling bits)"""

    def __init__(self, bytes_, gain, x, c):
        self.bytes, self.gain, self.x, self.c = bytes_, gain, x, c


def demap(planes, allocs, sf, cell, n_rb, cfi, gain=0.0, T=16):
    """planes: one unit's float32 [4, 16, 1200] (y_re, y_im, h_re, h_im); allocs: its allocations; gain 0: automatic.  One Demapped each."""
    p = np.asarray(planes, np.float32).reshape(4, -1).astype(np.float64)
    out = []
    for al in allocs:
        mod = al.mod_type
        re = pdsch_res(al, sf, cell, n_rb, cfi)
        y, h = p[0, re] + 1j * p[1, re], p[2, re] + 1j * p[3, re]
        if gain == 0:
            g_used, g_tap = auto_gain(h.real * h.real + h.imag * h.imag, mod, T)
        else:
            g_used = g_tap = float(np.float32(gain))
        with np.errstate(all="ignore"):
            x = (g_used * llr_symbols(y, h, mod)).reshape(-1)
        c = gold(((al.rnti << 14) | (sf << 9) | cell) & 0x7FFFFFFF, len(x))
        x = np.where(c == 1, -x, x)
        out.append(Demapped(soft_byte(x), g_tap, x, c))
    return out
