"""CPU: CQI channel coding on PUSCH (36.212 5.2.2.6.4).  The host encoder mi_lte_cqi_encode against numpy restatements written here from the
specification -- table 5.2.2.6.4-1 as text, CRC8, the tail-biting convolutional code of 5.1.3.1 and the rate matching of 5.1.4.2 -- and the
numpy decoder model that test_ulsch_cqi_gpu pins k_ulsch_cqi_decode to (the combining, decision and tie rules of include/mi_lte.h), itself
checked against a brute-force maximum-likelihood search over all 2^20 tail-biting words.  No GPU."""
from collections import Counter

import numpy as np
import pytest

ERR_INVALID = -1
NONE, NO_CRC, CRC_OK, CRC_FAIL = range(4)
BLOCK_MAX, MAX_BITS, MAX_Q = 11, 128, 6 * 12 * 1320

# table 5.2.2.6.4-1, row i = M_i,0 .. M_i,10
TABLE = """11000000001 11100000011 10010010111 10110000101 11110001001 11001011101 10101010111 10011001101
           11011001011 10111010011 10100111011 11100110101 10010101111 11010101011 10001101001 11001111011
           11101110010 10011100100 11011111000 10000110000 10100010001 11010000011 10001001101 11101000111
           11111011110 11000111001 10110100110 11110101110 10101110100 10111111100 11111111111 10000000000"""
M_TAB = np.array([[int(ch) for ch in row] for row in TABLE.split()], np.int64)  # [32, 11]
# sub-block interleaver column permutation of 5.1.4.2.1 (table 5.1.4-2)
P_CONV = [1, 17, 9, 25, 5, 21, 13, 29, 3, 19, 11, 27, 7, 23, 15, 31, 0, 16, 8, 24, 4, 20, 12, 28, 2, 18, 10, 26, 6, 22, 14, 30]
G_TAPS = [[j for j in range(7) if (g >> (6 - j)) & 1] for g in (0o133, 0o171, 0o165)]  # delays j of c_(k-j) in each generator


# ---- the specification, restated

def block_words(O):
    """[2^O, 32]: row w is the code word of o_n = bit n of w"""
    o = (np.arange(1 << O)[:, None] >> np.arange(O)) & 1
    return (o @ M_TAB[:, :O].T) % 2


def crc8(bits):
    """gCRC8 = D^8 + D^7 + D^4 + D^3 + D + 1, register 0: the 8 parity bits, first the most significant"""
    rem = 0
    for b in list(bits) + [0] * 8:
        rem = (rem << 1) | int(b)
        if rem & 0x100:
            rem ^= 0x19B
    return [(rem >> (7 - i)) & 1 for i in range(8)]


def conv_tb(c):
    """5.1.3.1 on [.., L] bits: [.., 3 L], d[3 k + x] = sum over generator x's taps of c_(k - j), the register starting on the last six bits"""
    c = np.asarray(c)
    L = c.shape[-1]
    d = np.zeros(c.shape[:-1] + (3 * L,), np.int64)
    for x, taps in enumerate(G_TAPS):
        d[..., x::3] = sum(np.roll(c, j, axis=-1) for j in taps) % 2
    return d


def circular_buffer(L):
    """5.1.4.2.1-2: the index into d[3 L] of every entry of w (K_w = 3 K_pi), -1 for a dummy"""
    R = -(-L // 32)
    n_dummy = 32 * R - L
    w = []
    for x in range(3):
        y = np.concatenate([np.full(n_dummy, -1), 3 * np.arange(L) + x]).reshape(R, 32)
        w.append(y[:, P_CONV].T.reshape(-1))  # columns permuted, read column by column
    return np.concatenate(w)


def rm_index(L, E):
    """5.1.4.2.2: the index into d of transmitted bit k = 0 .. E - 1"""
    w = circular_buffer(L)
    sent = w[w >= 0]
    assert len(sent) == 3 * L
    return sent[np.arange(E) % (3 * L)]


def encode_py(o, Q):
    o = np.asarray(o, np.int64)
    if len(o) <= BLOCK_MAX:
        b = (M_TAB[:, :len(o)] @ o) % 2
        return b[np.arange(Q) % 32].astype(np.uint8)
    c = np.concatenate([o, crc8(o)])
    return conv_tb(c)[rm_index(len(c), Q)].astype(np.uint8)


# ---- the decoder model (include/mi_lte.h: the CQI section)

def pack_bits(bits):
    words = [0, 0, 0, 0]
    for n, b in enumerate(bits):
        words[n >> 5] |= int(b) << (n & 31)
    return words


def model_block(e, O):
    e = np.asarray(e, np.int64)
    r = np.bincount(np.arange(len(e)) % 32, weights=e, minlength=32).astype(np.int64)
    metric = (1 - 2 * block_words(O)) @ r
    w = int(np.argmax(metric))  # the first maximum: the smallest w
    return {"O": O, "crc": NO_CRC, "metric": int(metric[w]), "energy": int(np.abs(r).sum()), "bits": [w, 0, 0, 0]}


def unmatch(e, L):
    d = np.zeros(3 * L, np.int64)
    np.add.at(d, rm_index(L, len(e)), np.asarray(e, np.int64))
    return d


def viterbi3(d):
    """d [n, 3 L] int64 -> bits [n, L]: three laps, read from the middle one"""
    n, L = d.shape[0], d.shape[1] // 3
    st = np.arange(64)
    pred = [2 * (st & 31), 2 * (st & 31) + 1]
    sign = []  # [64, 3] per predecessor: 1 - 2 label of the register (input bit | predecessor state)
    for p in pred:
        reg = ((st >> 5) << 6) | p
        sign.append(np.array([[1 - 2 * (bin(r & g).count("1") & 1) for g in (0o133, 0o171, 0o165)] for r in reg], np.int64))
    pm, surv, rows = np.zeros((n, 64), np.int64), [], np.arange(n)
    for t in range(3 * L):
        tri = d[:, 3 * (t % L):3 * (t % L) + 3]
        c0, c1 = pm[:, pred[0]] + tri @ sign[0].T, pm[:, pred[1]] + tri @ sign[1].T
        odd = c1 > c0  # a tie keeps the even predecessor
        surv.append(odd)
        pm = np.where(odd, c1, c0)
    cur, c = np.argmax(pm, axis=1), np.zeros((n, L), np.int64)  # the first maximum in state order
    for t in range(3 * L - 1, -1, -1):
        if L <= t < 2 * L:
            c[:, t - L] = cur >> 5
        cur = 2 * (cur & 31) + surv[t][rows, cur]
    return c


def model_conv(es, O):
    """the records of several runs of one O (any lengths)"""
    L = O + 8
    d = np.stack([unmatch(e, L) for e in es])
    c = viterbi3(d)
    metric = ((1 - 2 * conv_tb(c)) * d).sum(axis=1)
    return [{"O": O, "crc": CRC_OK if list(c[k, O:]) == crc8(c[k, :O]) else CRC_FAIL, "metric": int(metric[k]), "energy": int(np.abs(d[k]).sum()),
             "bits": pack_bits(c[k, :O])} for k in range(len(es))]


ZERO = {"O": 0, "crc": NONE, "metric": 0, "energy": 0, "bits": [0, 0, 0, 0]}


def model(runs):
    """runs: [(e int8 [Q], O)] -> the records k_ulsch_cqi_decode must give, the convolutional ones vectorised over runs of equal O"""
    out, by_O = [None] * len(runs), {}
    for k, (e, O) in enumerate(runs):
        if not (1 <= O <= MAX_BITS and 1 <= len(e) <= MAX_Q):
            out[k] = dict(ZERO)
        elif O <= BLOCK_MAX:
            out[k] = model_block(e, O)
        else:
            by_O.setdefault(O, []).append(k)
    for O, ks in by_O.items():
        for k, rec in zip(ks, model_conv([runs[k][0] for k in ks], O)):
            out[k] = rec
    return out


def noisy(q, sigma, rng):
    """coded bits -> int8 soft bits round(24 y), y = (1 - 2 q) + sigma n, clipped to +-127"""
    return np.clip(np.rint(24 * ((1 - 2 * q.astype(np.float64)) + sigma * rng.standard_normal(len(q)))), -127, 127).astype(np.int8)


CONV_O = (12, 24, 25, 56, 64, 128)


def conv_Q(O):
    L = O + 8
    return [q + (q & 1) for q in (2 * L, 3 * L, 3 * L + 2, 7 * L + 4)]


# ---- tests

def test_table_weight_distributions_and_words():
    """The weights of all 2^O words of cqi_encode(O, ., 32) for O = 10, 11 have exactly the distributions of the (32, O) code; for every O
    the words equal the numpy product with the table as text; columns 1-5 take every 5-bit pattern once."""
    import openlte_amd as m
    assert sorted((M_TAB[:, 1:6] @ (1 << np.arange(5))).tolist()) == list(range(32)) and M_TAB[:, 0].all()
    want = {10: {0: 1, 12: 240, 16: 542, 20: 240, 32: 1}, 11: {0: 1, 10: 64, 12: 240, 14: 448, 16: 542, 18: 448, 20: 240, 22: 64, 32: 1}}
    for O in range(1, 12):
        got = np.stack([m.cqi_encode(O, (w >> np.arange(O)) & 1, 32) for w in range(1 << O)])
        assert (got == block_words(O)).all(), O
        if O in want:
            assert dict(Counter(got.sum(axis=1).tolist())) == want[O], O


@pytest.mark.parametrize("Q", [20, 32, 44, 1200])
def test_block_code_repetition(Q):
    import openlte_amd as m
    rng = np.random.default_rng(Q)
    for O in range(1, 12):
        o = rng.integers(0, 2, O)
        q, b = m.cqi_encode(O, o, Q), m.cqi_encode(O, o, 32)
        assert (q == b[np.arange(Q) % 32]).all() and (q == encode_py(o, Q)).all(), (O, Q)


def test_convolutional_path_against_the_specification():
    """CRC8's check value; the interleaver's rows and dummies at the sizes named; cqi_encode against the numpy restatement."""
    import openlte_amd as m
    msg = [(ord(ch) >> (7 - i)) & 1 for ch in "123456789" for i in range(8)]
    assert crc8(msg) == [(0xEA >> (7 - i)) & 1 for i in range(8)]
    shape = {O: (O + 8, -(-(O + 8) // 32), int((circular_buffer(O + 8) < 0).sum()) // 3) for O in CONV_O}
    assert shape == {12: (20, 1, 12), 24: (32, 1, 0), 25: (33, 2, 31), 56: (64, 2, 0), 64: (72, 3, 24), 128: (136, 5, 24)}
    rng = np.random.default_rng(7)
    for O in CONV_O:
        for Q in conv_Q(O):
            for o in (rng.integers(0, 2, O), np.ones(O, np.int64), rng.integers(0, 2, O)):
                assert (m.cqi_encode(O, o, Q) == encode_py(o, Q)).all(), (O, Q)


def test_encoder_refusals():
    import openlte_amd as m
    L = m.load_library()
    o, q = np.zeros(129, np.uint8), np.zeros(64, np.uint8)
    for O, Q in ((0, 32), (129, 32), (4, 0), (4, MAX_Q + 1), (64, MAX_Q + 1)):
        assert L.mi_lte_cqi_encode(O, o.ctypes.data, Q, q.ctypes.data) == ERR_INVALID, (O, Q)
        with pytest.raises(m.MiLteError) as e:
            m.cqi_encode(O, o, Q)
        assert e.value.args[1] == ERR_INVALID
    assert L.mi_lte_cqi_encode(4, None, 32, q.ctypes.data) == ERR_INVALID and L.mi_lte_cqi_encode(4, o.ctypes.data, 32, None) == ERR_INVALID
    assert L.mi_lte_cqi_encode(128, o.ctypes.data, 64, q.ctypes.data) == 0 and L.mi_lte_cqi_encode(1, o.ctypes.data, 1, q.ctypes.data) == 0


def test_model_roundtrip_without_noise():
    """The model gives back what the encoder sent, with the full correlation, at every O of the tests (block and convolutional)."""
    import openlte_amd as m
    rng = np.random.default_rng(11)
    runs, sent = [], []
    for O in list(range(1, 12)) + list(CONV_O):
        o = rng.integers(0, 2, O)
        Q = 44 if O <= BLOCK_MAX else conv_Q(O)[2]
        runs.append((noisy(m.cqi_encode(O, o, Q), 0.0, rng), O))
        sent.append(o)
    for (e, O), o, rec in zip(runs, sent, model(runs)):
        assert rec["bits"] == pack_bits(o) and rec["crc"] == (NO_CRC if O <= BLOCK_MAX else CRC_OK), O
        assert rec["metric"] == rec["energy"] == 24 * len(e), O


def test_model_against_brute_force_maximum_likelihood():
    """O = 12 (L = 20), Q_cqi = 3 L, sigma = 0.8 on round(24 y): the three-lap model's word has the maximum correlation over all 2^20
    tail-biting words in at least 98 of 100 seeded cases (a cap, not a tolerance; measured with this seed: 100 of 100)."""
    import openlte_amd as m
    O, L, n, rng = 12, 20, 100, np.random.default_rng(2026)
    es = [noisy(m.cqi_encode(O, rng.integers(0, 2, O), 3 * L), 0.8, rng) for _ in range(n)]
    d = np.stack([unmatch(e, L) for e in es])
    best = np.full(n, -1 << 40, np.int64)
    for w0 in range(0, 1 << L, 1 << 16):  # (sums of 60 values of magnitude <= 127: exact in float32)
        words = (np.arange(w0, w0 + (1 << 16))[:, None] >> np.arange(L)) & 1
        best = np.maximum(best, ((1 - 2 * conv_tb(words)).astype(np.float32) @ d.T.astype(np.float32)).max(axis=0).astype(np.int64))
    c = viterbi3(d)
    got = ((1 - 2 * conv_tb(c)) * d).sum(axis=1)
    assert (got <= best).all()
    differ = int((got < best).sum())
    print("three-lap model against maximum likelihood: %d of %d differ" % (differ, n))
    assert differ <= 2
