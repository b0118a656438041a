"""float64 numpy model of MI_LTE_DEMAP_MAXLOG (include/mi_lte.h, "PDSCH, 3GPP mode: max-log soft-decision demapping" and "transmit diversity on
2 or 4 ports"): the resource elements of every allocation of one unit of a 1-, 2- or 4-port cell in the demodulator's order (symbol -> PRB ->
sub-carrier, CRS and, in subframes 0 and 5, the PBCH / PSS / SSS window left out), each symbol's (t, w) of the header's text, the max-log LLRs in
their piecewise-linear form, the gain, the rounding and the descrambling.  The GPU tests compare the kernel's bytes and gains with it
(tests/test_demap_llr_gpu.py, tests/test_txdiv_gpu.py); tests/test_demap_llr_cpu.py and tests/test_txdiv_cpu.py check the model itself."""
import numpy as np

N_SC = 1200
RS2 = 0.70710678118654752  # 1 / sqrt 2, the kernel's literal
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


def pdsch_res(al, sf, cell, n_rb, cfi, n_ant=1):
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


def one_port(y, h):
    """(t, w) of received symbols y (complex128) over channel h on one port: t = y conj(h), w = |h|^2, in the kernel's order of operations"""
    w = h.real * h.real + h.imag * h.imag
    t = (y.real * h.real + y.imag * h.imag).astype(np.complex128)
    t.imag = y.imag * h.real - y.real * h.imag
    return t, w


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
    y = planes[0] + 1j * planes[1]
    h = planes[2:2 + n_ant] + 1j * planes[2 + n_ant:2 + 2 * n_ant]
    if n_ant == 1:
        return one_port(y[re], h[0, re])
    m = len(re) // n_ant * n_ant
    a, b = re[0:m:2], re[1:m:2]
    pa, pb = pair_ports(m // 2, n_ant)
    t0, w0, t1, w1 = combine(y[a], y[b], h[pa, a], h[pb, b], h[pa, b], h[pb, a])
    t, w = np.zeros(m, np.complex128), np.zeros(m)
    t[0::2], t[1::2], w[0::2], w[1::2] = t0, t1, w0, w1
    return t, w


def llr_tw(t, w, mod):
    """[n, Q_m] LLRs L_k from (t, w): bit 2k on the real axis, 2k + 1 on the imaginary."""
    out = np.zeros((len(t), QM[mod]))
    with np.errstate(all="ignore"):
        out[:, 0::2] = np.stack(llr_axis(t.real, w, mod), 1)
        out[:, 1::2] = np.stack(llr_axis(t.imag, w, mod), 1)
    return out


def llr_symbols(y, h, mod):
    """[n, Q_m] LLRs L_k of n received symbols y (complex128) over channel h on one port."""
    return llr_tw(*one_port(y, h), mod)


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


def demap(planes, allocs, sf, cell, n_rb, cfi, n_ant=1, gain=0.0, T=16):
    """planes: one unit's float32 [2 + 2 n_ant, 16, 1200] (symbols' order); allocs: its allocations; gain 0: automatic.  One Demapped each."""
    p = np.asarray(planes, np.float32).reshape(2 + 2 * n_ant, -1).astype(np.float64)
    out = []
    for al in allocs:
        mod = al.mod_type
        t, w = symbols(p, pdsch_res(al, sf, cell, n_rb, cfi, n_ant), n_ant)
        g_used, g_tap = auto_gain(w, mod, T) if gain == 0 else (float(np.float32(gain)),) * 2
        with np.errstate(all="ignore"):
            x = (g_used * llr_tw(t, w, mod)).reshape(-1)
        c = gold(((al.rnti << 14) | (sf << 9) | cell) & 0x7FFFFFFF, len(x))
        x = np.where(c == 1, -x, x)
        out.append(Demapped(soft_byte(x), g_tap, x, c))
    return out
