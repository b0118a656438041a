"""GPU: k_pucch2_decode (PUCCH formats 2 / 2a / 2b) against a float64 numpy model written from the definition in include/mi_lte.h, not from
the kernel: the correlations, the HARQ-ACK decision, the slot estimates, the soft bits (tapped inside the record), the exhaustive
search over the (20, A) code, and what comes back of what was sent.  The reference leaves these formats empty, so there is nothing of
it to compare with; the transmitter is the library's host modulator, which test_pucch2_cpu pins to the specification.

Scenarios (one decode call each, shared by the tests): N_rb_ul = 6 (PRB 0 and 5: the band edges), 25, 100; per call 3 units with subframe
numbers 0, 9, 0 and 67 UEs spread over them on n2 of the first block (m = 0), the second (m = 1: slot 0 at the top edge) and the mixed
block -- up to 12 UEs on the cyclic shifts of one block -- with A from {1, 4, 9, 10, 11, 13}, formats 2, 2a, 2b with every ACK value, a random
complex gain per slot, and noise-free, 20 dB or 0 dB.  Units 0 and 2 share the subframe number, so their UEs share table indices."""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ERR_INVALID = -1
U = 2.0 ** -24  # float32 unit round-off
COLS = [0xFFFFF, 0x5A933, 0x10E5A, 0x6339C, 0x7C3E0, 0xFFC00, 0xD8E64, 0x4F5B0, 0x218EC, 0x1B746, 0x0FFFF, 0x33FFF, 0x3FFFC]  # 36.212 table 5.2.3.3-1
DATA_L = [7 * (n // 5) + [0, 2, 3, 4, 6][n % 5] for n in range(10)]  # the symbol of d(n)
FORMATS = [(0, ()), (1, (0,)), (1, (1,)), (2, (0, 0)), (2, (0, 1)), (2, (1, 0)), (2, (1, 1))]
Z_OF = {(): 1, (0,): 1, (1,): -1, (0, 0): 1, (0, 1): -1j, (1, 0): 1j, (1, 1): -1}
N_RB_2, N_CS_1 = 2, 3
A_SET = (1, 4, 11, 13, 9, 10)  # 9 | 10: where the search changes from cosets one by one to the transform (pucch2.hip)
N2_POOL = list(range(12)) + list(range(12, 24)) + list(range(24, 31))  # m = 0, m = 1, the mixed block (m = 2)


@functools.lru_cache(maxsize=None)
def signs(A):
    """[2^A, 20]: 1 - 2 b_i(w)"""
    w = np.zeros(1 << A, np.int64)
    for n in range(A):
        w ^= np.where((np.arange(1 << A) >> n) & 1, COLS[n], 0)
    return 1 - 2 * ((w[:, None] >> np.arange(20)) & 1)


# ---- the model (include/mi_lte.h, "The decoder, k_pucch2_decode")

def correlations(y, tab):
    """step 1 in float64 on the float32 inputs: c[14], and a[14] = sum_k |y| |r|, what the float32 sums' rounding is relative to"""
    r = tab.r.astype(np.complex128)
    c, a = np.zeros(14, np.complex128), np.zeros(14)
    for L in range(14):
        k = slice(12 * tab.prb[L // 7], 12 * tab.prb[L // 7] + 12)
        c[L] = (y[L, k] * np.conj(r[L])).sum()
        a[L] = (np.abs(y[L, k]) * np.abs(r[L])).sum()
    return c, a


def ack_rule(fmt, D_re, D_im):
    """step 2: (ack bits, z)"""
    if fmt == 0:
        return (), 1
    if fmt == 1:
        return ((1,), -1) if D_re < 0 else ((0,), 1)
    cand = [D_re, -D_im, D_im, -D_re]
    ack = [(0, 0), (0, 1), (1, 0), (1, 1)][int(np.argmax(cand))]  # the first maximum
    return ack, Z_OF[ack]


def soft_model(c, z, c_scr):
    """steps 3 and 4: (P, the 20 values before rounding, the soft bits)"""
    h = [(c[7 * s + 1] + np.conj(z) * c[7 * s + 5]) / 24 for s in range(2)]
    P = (abs(h[0]) ** 2 + abs(h[1]) ** 2) / 2
    if not (P > 0 and np.isfinite(P)):
        return P, np.zeros(20), np.zeros(20, np.int64)
    g = 32 * np.sqrt(2) / P
    x = np.zeros(20)
    for n in range(10):
        v = c[DATA_L[n]] / 12 * np.conj(h[n // 5])
        x[2 * n], x[2 * n + 1] = g * v.real, g * v.imag
    x = x * (1 - 2 * ((c_scr >> np.arange(20)) & 1))
    return P, x, np.clip(np.rint(x), -127, 127).astype(np.int64)


def search_model(e, A):
    """step 5 on the tapped soft bits: (bits, metric, energy)"""
    metric = signs(A) @ np.asarray(e, np.int64)
    w = int(np.argmax(metric))  # the first maximum: the smallest w
    return w, int(metric[w]), int(np.abs(np.asarray(e, np.int64)).sum())


# ---- scenarios

def ue_grid(m, tab, fmt, ack, A, a_bits, gains):
    """complex128 [14, 1200]: one UE's subframe through a complex gain per slot"""
    g = m.pucch2_modulate(tab, fmt, m.pucch2_encode(A, a_bits), ack if fmt else None)
    y = g[0].astype(np.complex128) + 1j * g[1]
    y[:7] *= gains[0]
    y[7:] *= gains[1]
    return y


def to_units(grids):
    sub = np.zeros((len(grids), 2, 16, 1200), np.float32)
    for u, y in enumerate(grids):
        sub[u, 0, :14], sub[u, 1, :14] = y.real, y.imag
    return sub


_CACHE = {}


def scenario(ctx, n_rb_ul, snr_db, n_res=67):
    """One decode call and everything the tests compare it with, made once per (N_rb_ul, SNR, size)."""
    key = (n_rb_ul, snr_db, n_res)
    if key in _CACHE:
        return _CACHE[key]
    import openlte_amd as m
    rng = np.random.default_rng(1000 * n_rb_ul + (0 if snr_db is None else int(snr_db) + 100) + n_res)
    ul, cell, sfs = m.UlCfg(0, 0, 0, 0, 0), 17 + n_rb_ul, (0, 9, 0)
    n_units = 3 if n_res > 1 else 1
    grids = [np.zeros((14, 1200), np.complex128) for _ in range(n_units)]
    tabs, tab_of, res, sent = [], {}, [], []
    per_unit = [list(rng.permutation(N2_POOL)) for _ in range(n_units)]
    if n_units == 3:
        per_unit[2] = list(per_unit[0])  # the same subframe number, n2 and RNTI order as unit 0: its UEs share unit 0's tables
    for r in range(n_res):
        u = r % n_units
        n2, rnti = int(per_unit[u].pop()), 0x100 + (r // n_units)
        tk = (sfs[u], n2, rnti)
        if tk not in tab_of:
            tab_of[tk] = len(tabs)
            tabs.append(m.pucch2_table(ul, cell, sfs[u], n_rb_ul, n2, N_RB_2, N_CS_1, rnti))
        fmt, ack = FORMATS[r % 7]
        A = A_SET[(r // 7 + r) % len(A_SET)]
        a_bits = rng.integers(0, 2, A)
        gains = rng.uniform(0.5, 1.5, 2) * np.exp(1j * rng.uniform(-np.pi, np.pi, 2))
        grids[u] += ue_grid(m, tabs[tab_of[tk]], fmt, ack, A, a_bits, gains)
        res.append((u, fmt, tab_of[tk], A))
        sent.append((int(a_bits @ (1 << np.arange(A))), ack))
    if snr_db is not None:  # per element, against a UE of unit gain
        sig = 10 ** (-snr_db / 20) / np.sqrt(2)
        grids = [y + sig * (rng.standard_normal(y.shape) + 1j * rng.standard_normal(y.shape)) for y in grids]
    sub = to_units(grids)
    d_sub = ctx.to_device(sub)
    rec = ctx.pucch2_decode_dev(n_rb_ul, d_sub, n_units, res, tabs)
    assert ctx.last_kernels() == "k_pucch2_decode:1"
    d_sub.free()
    y32 = [sub[u, 0, :14].astype(np.complex128) + 1j * sub[u, 1, :14] for u in range(n_units)]  # what the device read
    _CACHE[key] = dict(res=res, tabs=tabs, sent=sent, rec=rec, y=y32, n_tab=len(tabs))
    return _CACHE[key]


CASES = [(6, None), (6, 20.0), (6, 0.0), (25, None), (25, 0.0), (100, 20.0), (100, 0.0)]


# ---- tests

@pytest.mark.parametrize("n_rb_ul,snr_db", CASES)
def test_soft_bits_against_the_float64_model(ctx, n_rb_ul, snr_db):
    """Steps 1-4.  With a[L] = sum_k |y| |r| of symbol L and u = 2^-24:
    c[L] in float32 -- a product rounding and at most 8 additions (6 in the lane, 2 butterflies) per component -- is within 9 u a[L] per
    component, 13 u a[L] in modulus (14 u with r's own rounding).  D = sum_s c5 conj(c1): 14 u (a5 |c1| + |c5| a1) from the c's plus
    4 roundings per component on sum |c5| |c1|, with |c| <= a and a5 a1 <= (a5^2 + a1^2) / 2: |dD| <= 17 u sum_L a[L]^2.
    h_s = (c1 + conj(z) c5) / 24 adds two roundings, |h|^2 three, the mean two: 576 |dP| <= 37 u sum_L a[L]^2.
    Relative to sum_L |c[L]|^2, with kappa = sum a^2 / sum |c|^2 from the model (1 where a block holds one UE without noise; up to the number
    of UEs on the block's cyclic shifts otherwise, since the correlation cancels what the sums were rounded in):
    |dD| / sum |c|^2 <= 20 u kappa and 576 |dP| / sum |c|^2 <= 40 u kappa are asserted.
    Soft bits: about 40 float32 operations on values <= 127 stay below 3e-4 of a step, so the tapped e equals the model's rounding
    unless the model's value before rounding lies within 2^-8 of a half-integer (that set is computed here from the model), and is
    within 1 of it always.  z is taken from the record's ACK bits, which test_integer_stage_exact ties to the tapped D."""
    sc = scenario(ctx, n_rb_ul, snr_db)
    worst_D = worst_P = worst_k = 0.0
    n_excused = n_bits = 0
    for (u, fmt, t, A), rec in zip(sc["res"], sc["rec"]):
        tab = sc["tabs"][t]
        c, a = correlations(sc["y"][u], tab)
        D = sum(c[7 * s + 5] * np.conj(c[7 * s + 1]) for s in range(2))
        sum_c2 = (np.abs(c) ** 2).sum()
        kappa = (a ** 2).sum() / sum_c2 if sum_c2 > 0 else 0.0  # how much larger than the correlations the sums they were rounded in are
        assert abs(complex(rec["D_re"], rec["D_im"]) - D) <= 20 * U * kappa * sum_c2
        z = Z_OF[tuple(int(b) for b in rec["ack"][:rec["n_ack"]])]
        P, x, e = soft_model(c, z, tab.c_scr)
        assert 576 * abs(float(rec["P"]) - P) <= 40 * U * kappa * sum_c2
        worst_D = max(worst_D, abs(complex(rec["D_re"], rec["D_im"]) - D) / sum_c2)
        worst_P = max(worst_P, 576 * abs(float(rec["P"]) - P) / sum_c2)
        worst_k = max(worst_k, kappa)
        got = rec["e"].astype(np.int64)
        assert (np.abs(got - e) <= 1).all(), (got, e)
        near_half = np.abs(np.abs(x - np.floor(x)) - 0.5) <= 2.0 ** -8
        assert (got[~near_half] == e[~near_half]).all(), (got, e, x)
        n_excused += int(near_half.sum())
        n_bits += 20
    print("N_rb_ul %d, %s dB: |dD| / sum|c|^2 <= %.3g, 576 |dP| / sum|c|^2 <= %.3g (u = %.3g, kappa <= %.1f); %d of %d soft bits within 2^-8 of a half-integer"
          % (n_rb_ul, snr_db, worst_D, worst_P, U, worst_k, n_excused, n_bits))


@pytest.mark.parametrize("n_rb_ul,snr_db", CASES)
def test_integer_stage_exact(ctx, n_rb_ul, snr_db):
    """Step 5 on the tapped soft bits and step 2's rule on the tapped D: every record equals the numpy search, the first maximum included."""
    sc = scenario(ctx, n_rb_ul, snr_db)
    assert sc["n_tab"] < len(sc["res"])  # tables are shared
    for (u, fmt, t, A), rec in zip(sc["res"], sc["rec"]):
        assert (int(rec["bits"]), int(rec["metric"]), int(rec["energy"])) == search_model(rec["e"], A) and rec["A"] == A
        ack, _ = ack_rule(fmt, np.float32(rec["D_re"]), np.float32(rec["D_im"]))
        assert rec["n_ack"] == len(ack) == (0, 1, 2)[fmt] and tuple(int(b) for b in rec["ack"][:len(ack)]) == ack and not rec["ack"][len(ack):].any()


@pytest.mark.parametrize("n_rb_ul,snr_db", [c for c in CASES if c[1] != 0.0])
def test_round_trip(ctx, n_rb_ul, snr_db):
    """Noise-free and at 20 dB every report and every ACK value sent comes back; without noise the metric is the whole energy."""
    sc = scenario(ctx, n_rb_ul, snr_db)
    assert {(r[1], s[1]) for r, s in zip(sc["res"], sc["sent"])} == set(FORMATS) and {r[3] for r in sc["res"]} == set(A_SET)
    for (u, fmt, t, A), (w, ack), rec in zip(sc["res"], sc["sent"], sc["rec"]):
        assert int(rec["bits"]) == w and tuple(int(b) for b in rec["ack"][:rec["n_ack"]]) == ack, (fmt, A)
        if snr_db is None:
            assert rec["metric"] == rec["energy"] > 0  # (every soft bit has its word's sign; a slot's weight is |h_s|^2 / P)


def test_single_resource_batch(ctx):
    """A batch of one resource on one unit (N_rb_ul = 25, 20 dB): the same checks."""
    sc = scenario(ctx, 25, 20.0, n_res=1)
    (u, fmt, t, A), rec, (w, ack) = sc["res"][0], sc["rec"][0], sc["sent"][0]
    c, _ = correlations(sc["y"][u], sc["tabs"][t])
    _, x, e = soft_model(c, Z_OF[ack], sc["tabs"][t].c_scr)
    near_half = np.abs(np.abs(x - np.floor(x)) - 0.5) <= 2.0 ** -8
    got = rec["e"].astype(np.int64)
    assert (np.abs(got - e) <= 1).all() and (got[~near_half] == e[~near_half]).all()
    assert (int(rec["bits"]), int(rec["metric"]), int(rec["energy"])) == search_model(rec["e"], A) and int(rec["bits"]) == w


@pytest.mark.parametrize("n_ue", [2, 4])
def test_code_division_multiplexing(ctx, n_ue):
    """Two and four UEs with different n2 on one resource block, superposed noise-free with different gains: each one's soft bits are
    within 1 of its single-UE run and every report and ACK comes back.  Only the correlation over the 12 sub-carriers separates them."""
    import openlte_amd as m
    rng = np.random.default_rng(n_ue)
    ul, n_rb_ul = m.UlCfg(0, 1, 0, 0, 0), 25
    n2s = [13, 22, 17, 12][:n_ue]  # all m = 1: PRB 24 then 0
    tabs, grids, res, sent = [], [], [], []
    for i, n2 in enumerate(n2s):
        tabs.append(m.pucch2_table(ul, 301, 9, n_rb_ul, n2, N_RB_2, N_CS_1, 0x200 + i))
        assert list(tabs[-1].prb) == [24, 0]
        fmt, ack = FORMATS[(2 * i + 3) % 7]
        A = (13, 11, 4, 13)[i]
        a_bits = rng.integers(0, 2, A)
        gains = (0.4 + 0.5 * i) * np.exp(1j * rng.uniform(-np.pi, np.pi, 2))
        grids.append(ue_grid(m, tabs[-1], fmt, ack, A, a_bits, gains))
        sent.append((int(a_bits @ (1 << np.arange(A))), ack))
        res.append((i, fmt, i, A))
    grids.append(sum(grids))
    res += [(n_ue, fmt, t, A) for (_, fmt, t, A) in res]
    d_sub = ctx.to_device(to_units(grids))
    rec = ctx.pucch2_decode_dev(n_rb_ul, d_sub, n_ue + 1, res, tabs)
    d_sub.free()
    for i in range(n_ue):
        alone, together = rec[i], rec[n_ue + i]
        assert np.abs(alone["e"].astype(np.int64)).min() >= 31
        assert (np.abs(alone["e"].astype(np.int64) - together["e"].astype(np.int64)) <= 1).all(), i
        for r in (alone, together):
            assert int(r["bits"]) == sent[i][0] and tuple(int(b) for b in r["ack"][:r["n_ack"]]) == sent[i][1], i


def test_edges(ctx):
    """An all-zero grid: e = 0, metric = energy = 0, bits = 0, P = 0.  Data symbols at 8 x the reference symbols' amplitude: every soft bit
    on a rail, +-127.  A grid whose soft bits leave two words with equal maxima -- the QPSK symbols that hold the bits in which the words of
    w1 > w2 differ are blanked, so e is exactly 0 there: the smaller w is decided."""
    import openlte_amd as m
    n_rb_ul, A = 6, 13
    tab = m.pucch2_table(m.UlCfg(0, 0, 0, 0, 0), 44, 0, n_rb_ul, 5, N_RB_2, N_CS_1, 0x77)
    sg = signs(A)
    w1 = 0x1ABC
    others = np.nonzero((sg != sg[w1]).sum(axis=1) == 4)[0]  # the nearest words (d_min = 4)
    w2 = int(others[others < w1][0])
    differ = np.nonzero(sg[w1] != sg[w2])[0]
    a1 = (w1 >> np.arange(A)) & 1
    rails = ue_grid(m, tab, 2, (1, 0), A, a1, (0.7j, -1.1))
    for L in DATA_L:
        rails[L] *= 8
    tie = ue_grid(m, tab, 0, (), A, a1, (1.0, 1.0))
    for n in sorted({int(i) // 2 for i in differ}):
        tie[DATA_L[n]] = 0
    d_sub = ctx.to_device(to_units([np.zeros((14, 1200), np.complex128), rails, tie]))
    rec = ctx.pucch2_decode_dev(n_rb_ul, d_sub, 3, [(0, 0, 0, A), (0, 2, 0, 4), (1, 2, 0, A), (2, 0, 0, A)], [tab])
    d_sub.free()
    for r in rec[:2]:
        assert not r["e"].any() and r["metric"] == r["energy"] == r["bits"] == 0 and r["P"] == 0 and not r["ack"].any()
    assert (np.abs(rec[2]["e"].astype(np.int64)) == 127).all() and rec[2]["bits"] == w1 and tuple(rec[2]["ack"]) == (1, 0) and rec[2]["energy"] == 20 * 127
    e = rec[3]["e"].astype(np.int64)
    metric = sg @ e
    assert not e[differ].any() and metric[w1] == metric[w2] == metric.max() and (metric == metric.max()).sum() >= 2
    assert rec[3]["bits"] == int(np.argmax(metric)) <= w2 < w1 and rec[3]["metric"] == metric.max()


def test_refusals_leave_the_context_usable(ctx):
    import ctypes as C
    import openlte_amd as m
    n_rb_ul = 25
    tab = m.pucch2_table(m.UlCfg(0, 0, 0, 0, 0), 44, 3, n_rb_ul, 17, N_RB_2, N_CS_1, 0x77)
    a_bits = np.array([1, 0, 1, 1])
    d_sub = ctx.to_device(to_units([ue_grid(m, tab, 1, (1,), 4, a_bits, (1.0, 1j))]))
    good = ctx.pucch2_decode_dev(n_rb_ul, d_sub, 1, [(0, 1, 0, 4)], [tab])
    assert good[0]["bits"] == 13 and good[0]["ack"][0] == 1 and good[0]["n_ack"] == 1
    wide = m.Pucch2Tab.from_buffer_copy(tab)
    wide.prb[0] = n_rb_ul
    bad = [dict(res=[(0, 3, 0, 4)]), dict(res=[(0, 1, 0, 0)]), dict(res=[(0, 1, 0, 14)]), dict(res=[(1, 1, 0, 4)]), dict(res=[(0, 1, 1, 4)]),
           dict(tabs=[wide]), dict(res=[]), dict(res=[(0, 1, 0, 4), (0, 1, 0, 4), (0, 1, 2, 4)], tabs=[tab, tab]), dict(n_rb_ul=5), dict(n_rb_ul=101)]
    for kw in bad:
        a = dict(dict(n_rb_ul=n_rb_ul, res=[(0, 1, 0, 4)], tabs=[tab]), **kw)
        with pytest.raises(m.MiLteError):
            ctx.pucch2_decode_dev(a["n_rb_ul"], d_sub, 1, a["res"], a["tabs"])
        again = ctx.pucch2_decode_dev(n_rb_ul, d_sub, 1, [(0, 1, 0, 4)], [tab])
        assert again.tobytes() == good.tobytes(), kw
    # null pointers, straight at the C entry point
    L, arr, tarr, d_out = ctx.L, (m.Pucch2Res * 1)(m.Pucch2Res(0, 1, 0, 4)), (m.Pucch2Tab * 1)(tab), ctx.alloc(64)
    assert L.mi_lte_pucch2_decode_run(ctx.h, n_rb_ul, None, 1, arr, 1, tarr, 1, d_out.ptr) == ERR_INVALID
    assert L.mi_lte_pucch2_decode_run(ctx.h, n_rb_ul, d_sub.ptr, 1, None, 1, tarr, 1, d_out.ptr) == ERR_INVALID
    assert L.mi_lte_pucch2_decode_run(ctx.h, n_rb_ul, d_sub.ptr, 1, arr, 1, None, 1, d_out.ptr) == ERR_INVALID
    assert L.mi_lte_pucch2_decode_run(ctx.h, n_rb_ul, d_sub.ptr, 1, arr, 1, tarr, 1, None) == ERR_INVALID
    assert L.mi_lte_pucch2_decode_run(None, n_rb_ul, d_sub.ptr, 1, arr, 1, tarr, 1, d_out.ptr) == ERR_INVALID
    # the no-wait form: the caller's device buffer
    assert ctx.pucch2_decode_dev(n_rb_ul, d_sub, 1, [(0, 1, 0, 4)], [tab], d_out=d_out) is None
    assert d_out.download(np.uint8, 64).tobytes() == good.tobytes()
    d_out.free()
    d_sub.free()
