"""CPU: PUCCH formats 2 / 2a / 2b on the host -- the (20, A) code of 36.212 5.2.3.3, the tables of 36.211 5.4.2 / 5.4.3 (n', the cyclic
shifts, the resource-block pair, the scrambling bits) and the modulator, each against a numpy restatement written here from the
specification as include/mi_lte.h quotes it.  The base sequences are compared with mi_lte_ul_pucch_tables', which other tests pin to the
compiled reference.  No GPU."""
import ctypes as C
from collections import Counter

import numpy as np
import pytest

ERR_INVALID = -1

# table 5.2.3.3-1, row i = M_i,0 .. M_i,12 (columns 0 .. 10: the first 20 rows of table 5.2.2.6.4-1)
TABLE = """1100000000110 1110000001110 1001001011111 1011000010111 1111000100111 1100101110111 1010101011111 1001100110111
           1101100101111 1011101001111 1010011101111 1110011010111 1001010111111 1101010101111 1000110100101 1100111101101
           1110111001011 1001110010011 1101111100000 1000011000000"""
M_TAB = np.array([[int(ch) for ch in row] for row in TABLE.split()], np.int64)  # [20, 13]
# the same as column words (bit i = M_i,n): what openlte_amd/csrc/pucch2_code.h holds
COLS = [0xFFFFF, 0x5A933, 0x10E5A, 0x6339C, 0x7C3E0, 0xFFC00, 0xD8E64, 0x4F5B0, 0x218EC, 0x1B746, 0x0FFFF, 0x33FFF, 0x3FFFC]
DATA_SYMB = [0, 2, 3, 4, 6]


def words(A):
    """[2^A, 20] from the column words: row w is the code word of a_n = bit n of w"""
    w = np.zeros(1 << A, np.int64)
    for n in range(A):
        w ^= np.where((np.arange(1 << A) >> n) & 1, COLS[n], 0)
    return (w[:, None] >> np.arange(20)) & 1


def gold(c_init, n):
    """36.211 7.2: c(i), i < n"""
    x1 = [1] + [0] * 30
    x2 = [(c_init >> i) & 1 for i in range(31)]
    for i in range(1600 + n - 31):
        x1.append(x1[i + 3] ^ x1[i])
        x2.append(x2[i + 3] ^ x2[i + 2] ^ x2[i + 1] ^ x2[i])
    return np.array([x1[i + 1600] ^ x2[i + 1600] for i in range(n)], np.int64)


def n_cs_cell(cell, n_s):
    """36.211 5.4: n_cs^cell(n_s, l), l < 7 = sum_i c(8 * 7 * n_s + 8 l + i) 2^i with c_init = N_id_cell"""
    c = gold(cell, 8 * 7 * (n_s + 1))
    return [int(c[8 * 7 * n_s + 8 * l:8 * 7 * n_s + 8 * l + 8] @ (1 << np.arange(8))) for l in range(7)]


def valid_n2(n_rb_2, n_cs_1):
    return list(range(12 * n_rb_2)) + (list(range(12 * n_rb_2, 12 * n_rb_2 + 10 - n_cs_1)) if n_cs_1 > 0 else [])


def n_prime(n2, n_rb_2, n_cs_1):
    """5.4.2: (n'(even slot), n'(odd slot)); python's % is the mathematical modulo"""
    if n2 < 12 * n_rb_2:
        n0 = n2 % 12
        return n0, (12 * (n0 + 1)) % 13 - 1
    return (n2 + n_cs_1 + 1) % 12, (12 - 2 - n2) % 12


def prbs(n2, n_rb_ul):
    m = n2 // 12
    return [m // 2 if (m + s) % 2 == 0 else n_rb_ul - 1 - m // 2 for s in range(2)]


def shift_bound(n_cs, k):
    """How far a float32 row r(k) = base(k) exp(j alpha k) can lie from the exact one, per element: alpha = 2 pi n_cs / 12 is rounded to float32
    (half a spacing of alpha, times k), alpha * k is a float32 product (half a spacing of the product), cosf / sinf are within one spacing of a
    value <= 1 (2^-23 each, both components), and the complex product rounds two products and one sum per component
    (3 * 2^-24 * sqrt 2 on a unit-modulus value); the base values themselves are float32 roundings of cos / sin (2^-24 sqrt 2).
    For alpha k < 64 this is at most 11 * 2^-22 + 2^-19 + about 8 * 2^-24: some 40 spacings of 1.0 at the largest shift, a few at the small ones."""
    alpha = np.float32(2 * np.pi * n_cs / 12)
    return k * np.spacing(alpha) / 2 + np.spacing(np.float32(alpha) * k.astype(np.float32)) / 2 + (2 * 2.0 ** -23 + 4 * 2.0 ** -24) * np.sqrt(2)


def base_from_format1(m, ul, cell, sf):
    """The slot's base sequence r_u,v(k) [2, 12] complex128 out of mi_lte_ul_pucch_tables (N_cs_an = 0, delta_shift = 1, n1 = 0: n' = 0 in the
    even slot and 2 in the odd one, n_oc = 0, so n_cs = (n_cs^cell + n') mod 12 on data symbols 0, 1, 5, 6), with the element-wise bound."""
    t = np.zeros(352, np.float32)
    assert m.load_library().mi_lte_ul_pucch_tables(C.byref(ul), cell, sf, 0, 0, 1, 1, C.c_void_p(t.ctypes.data)) == 0
    ruv = (t[144:240].astype(np.float64) + 1j * t[240:336]).reshape(2, 4, 12)
    k = np.arange(12)
    base, bound = np.zeros((2, 12), np.complex128), np.zeros((2, 12))
    for s in range(2):
        cs = n_cs_cell(cell, 2 * sf + s)
        per = []
        for i, l in enumerate([0, 1, 5, 6]):
            n_cs = (cs[l] + (0, 2)[s]) % 12
            per.append((ruv[s, i] * np.exp(-2j * np.pi * n_cs * k / 12), shift_bound(n_cs, k)))
        for b, bd in per[1:]:  # the four symbols of a slot carry one base sequence
            assert (np.abs(b - per[0][0]) <= bd + per[0][1]).all()
        base[s], bound[s] = per[0]
    assert np.allclose(np.abs(base), 1, atol=1e-6) and np.allclose((np.angle(base) * 4 / np.pi) % 2, 1, atol=1e-4)  # QPSK: odd multiples of pi / 4
    return base, bound


# ---- the code

def test_code_words_weights_and_distances():
    """Every code word of every A against the column words; the column words against the table as text and, columns 0 .. 10, against the low
    20 bits of the (32, O) code's words; the weight distributions and minimum distances, which a wrong bit in any column would change."""
    import openlte_amd as m
    assert [int(M_TAB[:, n] @ (1 << np.arange(20))) for n in range(13)] == COLS
    for n in range(11):
        assert int(m.cqi_encode(11, np.eye(11, dtype=np.uint8)[n], 32)[:20] @ (1 << np.arange(20))) == COLS[n], n
    want = {6: {0: 1, 8: 15, 10: 32, 12: 15, 20: 1},
            10: {0: 1, 6: 94, 8: 239, 10: 356, 12: 239, 14: 94, 20: 1},
            11: {0: 1, 4: 10, 6: 170, 8: 485, 10: 716, 12: 485, 14: 170, 16: 10, 20: 1},
            13: {0: 1, 4: 77, 6: 608, 8: 1970, 10: 2880, 12: 1970, 14: 608, 16: 77, 20: 1}}
    d_min = []
    for A in range(1, 14):
        got = np.stack([m.pucch2_encode(A, (w >> np.arange(A)) & 1) for w in range(1 << A)])
        assert (got == words(A)).all() and (got == ((np.arange(1 << A)[:, None] >> np.arange(A)) & 1) @ M_TAB[:, :A].T % 2).all(), A
        weights = got.sum(axis=1)
        d_min.append(int(weights[1:].min()))  # (a linear code: the minimum distance is the minimum non-zero weight)
        assert len({r.tobytes() for r in got}) == 1 << A, A
        if A in want:
            assert dict(Counter(weights.tolist())) == want[A], A
    assert d_min == [20, 10, 8, 8, 8, 8, 6, 6, 6, 6, 4, 4, 4]


def test_encoder_refusals():
    import openlte_amd as m
    L = m.load_library()
    a, b = np.zeros(16, np.uint8), np.zeros(20, np.uint8)
    for A in (0, 14, 1 << 31):
        assert L.mi_lte_pucch2_encode(A, a.ctypes.data, b.ctypes.data) == ERR_INVALID
    with pytest.raises(m.MiLteError) as e:
        m.pucch2_encode(14, a)
    assert e.value.args[1] == ERR_INVALID
    assert L.mi_lte_pucch2_encode(4, None, b.ctypes.data) == ERR_INVALID and L.mi_lte_pucch2_encode(4, a.ctypes.data, None) == ERR_INVALID
    assert L.mi_lte_pucch2_encode(13, a.ctypes.data, b.ctypes.data) == 0 and L.mi_lte_pucch2_encode(1, a.ctypes.data, b.ctypes.data) == 0


# ---- the tables

@pytest.mark.parametrize("cell,hop,sf", [(17, 0, 0), (17, 0, 9), (301, 1, 0), (301, 1, 9)])
def test_n_prime_prb_and_cyclic_shift(cell, hop, sf):
    """Every valid n2 for N_rb_2 in {1, 2, 3} x N_cs_1 in {0, 3, 7} x N_rb_ul in {6, 25, 100}: prb equals 5.4.3's, and every row of the
    table is the slot's base sequence (taken from mi_lte_ul_pucch_tables: another function's output) times exp(j 2 pi n_cs k / 12) with
    n_cs = (n_cs^cell + n') mod 12 from the numpy restatement, within shift_bound -- a wrong n' or n_cs^cell is off by the order of 1."""
    import openlte_amd as m
    ul = m.UlCfg(3, hop, 0, 0, 0)
    base, base_bound = base_from_format1(m, ul, cell, sf)
    cs = [n_cs_cell(cell, 2 * sf + s) for s in range(2)]
    k, n = np.arange(12), 0
    for n_rb_2 in (1, 2, 3):
        for n_cs_1 in (0, 3, 7):
            for n2 in valid_n2(n_rb_2, n_cs_1):
                npr = n_prime(n2, n_rb_2, n_cs_1)
                assert 0 <= npr[0] < 12 and 0 <= npr[1] < 12
                for n_rb_ul in (6, 25, 100):
                    t = m.pucch2_table(ul, cell, sf, n_rb_ul, n2, n_rb_2, n_cs_1, 0x1234)
                    assert list(t.prb) == prbs(n2, n_rb_ul), (n2, n_rb_ul)
                    if n_rb_ul != 25:
                        continue  # (the sequences do not depend on the bandwidth: compared once)
                    r = t.r.astype(np.complex128)
                    for s in range(2):
                        for l in range(7):
                            n_cs = (cs[s][l] + npr[s]) % 12
                            err = np.abs(r[7 * s + l] - base[s] * np.exp(2j * np.pi * n_cs * k / 12))
                            assert (err <= shift_bound(n_cs, k) + base_bound[s]).all(), (n2, n_rb_2, n_cs_1, s, l, float(err.max()))
                            n += 1
    assert n == 14 * sum(len(valid_n2(a, b)) for a in (1, 2, 3) for b in (0, 3, 7))


def test_slot_hopping_of_n_prime_is_a_permutation():
    """5.4.2's odd-slot rule maps the 12 values of the even slot onto 12 different ones (what keeps two UEs of one block apart in both slots);
    the band edges: m = 0 sits on PRB 0 then N_rb_ul - 1, m = 1 the other way round."""
    assert sorted(n_prime(n2, 1, 0)[1] for n2 in range(12)) == list(range(12))
    assert prbs(5, 6) == [0, 5] and prbs(17, 6) == [5, 0] and prbs(26, 25) == [1, 23] and prbs(40, 100) == [98, 1]


@pytest.mark.parametrize("cell,sf,rnti", [(0, 0, 0), (17, 3, 0x1234), (503, 9, 65535)])
def test_scrambling_bits(cell, sf, rnti):
    import openlte_amd as m
    t = m.pucch2_table(m.UlCfg(0, 0, 0, 0, 0), cell, sf, 25, 0, 1, 0, rnti)
    assert t.c_scr == int(gold((sf + 1) * (2 * cell + 1) * 65536 + rnti, 20) @ (1 << np.arange(20)))


def test_table_refusals():
    import openlte_amd as m
    L = m.load_library()
    ul, out = m.UlCfg(0, 0, 0, 0, 0), m.Pucch2Tab()
    good = dict(cell=17, sf=3, n_rb_ul=25, n2=5, n_rb_2=2, n_cs_1=3, rnti=0x1234)

    def rc(ul_=ul, out_=out, **kw):
        a = dict(good, **kw)
        return L.mi_lte_ul_pucch2_table(C.byref(ul_) if ul_ is not None else None, a["cell"], a["sf"], a["n_rb_ul"], a["n2"], a["n_rb_2"], a["n_cs_1"], a["rnti"],
                                        C.byref(out_) if out_ is not None else None)

    assert rc() == 0
    assert rc(sf=10) == rc(cell=504) == rc(n_cs_1=8) == rc(rnti=65536) == ERR_INVALID
    assert rc(ul_=None) == rc(out_=None) == ERR_INVALID
    # n2: the last valid and the first invalid value of each interval
    assert rc(n2=23, n_cs_1=0) == 0 and rc(n2=24, n_cs_1=0) == ERR_INVALID  # no mixed block without N_cs_1
    assert rc(n2=24) == 0 and rc(n2=30) == 0 and rc(n2=31) == ERR_INVALID       # 12 N_rb_2 + 10 - N_cs_1 = 31
    assert rc(n2=26, n_cs_1=7) == 0 and rc(n2=27, n_cs_1=7) == ERR_INVALID
    assert rc(n2=0xFFFFFFFF) == ERR_INVALID
    # floor(m / 2) >= N_rb_ul / 2: m = 6 in six resource blocks; m = 5 still fits (PRB 3 and 2)
    assert rc(n_rb_ul=6, n_rb_2=7, n2=72) == ERR_INVALID and rc(n_rb_ul=6, n_rb_2=7, n2=71) == 0
    with pytest.raises(m.MiLteError) as e:
        m.pucch2_table(ul, 17, 10, 25, 5, 2, 3, 1)
    assert e.value.args[1] == ERR_INVALID


# ---- the modulator

@pytest.mark.parametrize("n_rb_ul,n2,fmt,ack", [(6, 5, 0, None), (6, 17, 1, (0,)), (25, 17, 1, (1,)), (25, 26, 2, (0, 0)), (100, 30, 2, (0, 1)), (100, 3, 2, (1, 0)),
                                               (25, 12, 2, (1, 1))])
def test_modulator_against_numpy(n_rb_ul, n2, fmt, ack):
    """d(n) r on the data symbols, r on symbol 1, z r on symbol 5 of each slot; nothing outside the UE's two blocks.  The products are
    float32 products of float32 factors: equal to the float64 restatement within two roundings (2^-23 on values of modulus <= 1)."""
    import openlte_amd as m
    rng = np.random.default_rng(n2 + fmt)
    t = m.pucch2_table(m.UlCfg(0, 0, 0, 0, 0), 44, 9, n_rb_ul, n2, 2, 3, 0x4321)
    a = rng.integers(0, 2, 7)
    b = m.pucch2_encode(7, a)
    g = m.pucch2_modulate(t, fmt, b, ack)
    got = g[0].astype(np.complex128) + 1j * g[1]
    bs = b ^ ((t.c_scr >> np.arange(20)) & 1)
    d = ((1 - 2.0 * bs[0::2]) + 1j * (1 - 2.0 * bs[1::2])) / np.sqrt(2)
    z = 1 if fmt == 0 else (1 - 2 * ack[0]) if fmt == 1 else {(0, 0): 1, (0, 1): -1j, (1, 0): 1j, (1, 1): -1}[tuple(ack)]
    want, r = np.zeros((14, 1200), np.complex128), t.r.astype(np.complex128)
    for s in range(2):
        k = slice(12 * t.prb[s], 12 * t.prb[s] + 12)
        for n in range(5):
            want[7 * s + DATA_SYMB[n], k] = d[5 * s + n] * r[7 * s + DATA_SYMB[n]]
        want[7 * s + 1, k] = r[7 * s + 1]
        want[7 * s + 5, k] = z * r[7 * s + 5]
    assert np.abs(got - want).max() <= 2.0 ** -22
    assert (got[want == 0] == 0).all() and np.count_nonzero(np.abs(got).sum(axis=0)) == 24
    # written, not added: a second call over the same grid leaves the same values
    assert (m.pucch2_modulate(t, fmt, b, ack, g.copy()) == g).all()


def test_modulator_refusals():
    import openlte_amd as m
    L = m.load_library()
    t = m.pucch2_table(m.UlCfg(0, 0, 0, 0, 0), 44, 9, 25, 5, 2, 3, 1)
    b, ack, g = np.zeros(20, np.uint8), np.zeros(2, np.uint8), np.zeros((2, 14, 1200), np.float32)
    args = [C.byref(t), 0, b.ctypes.data, ack.ctypes.data, g[0].ctypes.data, g[1].ctypes.data]
    assert L.mi_lte_pucch2_modulate(*args) == 0
    for i in (0, 2, 4, 5):
        bad = list(args)
        bad[i] = None
        assert L.mi_lte_pucch2_modulate(*bad) == ERR_INVALID, i
    assert L.mi_lte_pucch2_modulate(args[0], 3, *args[2:]) == ERR_INVALID
    assert L.mi_lte_pucch2_modulate(args[0], 0, args[2], None, *args[4:]) == 0 and L.mi_lte_pucch2_modulate(args[0], 1, args[2], None, *args[4:]) == ERR_INVALID
    off = m.Pucch2Tab.from_buffer_copy(t)
    off.prb[1] = 100  # past the 1200-sub-carrier grid
    before = g.copy()
    assert L.mi_lte_pucch2_modulate(C.byref(off), *args[1:]) == ERR_INVALID and (g == before).all()
