"""CPU: HARQ-ACK, RI and CQI multiplexed on PUSCH in the 3GPP transport-block mode (36.212 5.2.2.6-5.2.2.8, scrambling 36.211 5.3.1): the host
arithmetic.  Nothing in the reference does this, so the yardstick is a numpy restatement of the placement rules written here from their
statement (include/mi_lte.h), not from the library's map: mi_lte_ulsch_uci_map, _G and _qprime against it and against Python integers, the
transmitter's multiplexer and scrambler (mi_lte_ulsch_mux_3gpp) against it, the unit generator with all-zero descriptors against the plain
3GPP generator, and every refusal.  No GPU."""
import itertools

import numpy as np
import pytest

DATA, CQI, RI, ACK_DATA, ACK_CQI = range(5)
RI_WALK, ACK_WALK = (1, 10, 7, 4), (2, 9, 8, 3)  # column sets {1, 4, 7, 10} / {2, 3, 8, 9}, j <- (j + 3) mod 4 from j = 0
X, Y = 2, 3  # placeholders
ERR_INVALID, ERR_UNSUPPORTED = -1, -4
NONE = 0xFFFFFFFF


def uci(O_ack=0, Qp_ack=0, O_ri=0, Qp_ri=0, Q_cqi=0):
    import openlte_amd as m
    return m.UlschUci(O_ack, O_ri, Qp_ack, Qp_ri, Q_cqi)


# ---- the rules, restated

def walk_cells(M, Qp, walk):
    """rules 1 / 3: (row, column) of control symbol i = 0 .. Qp - 1"""
    i = np.arange(Qp)
    return M - 1 - i // 4, np.asarray(walk)[i % 4]


def place(n_prb, Qm, Qp_ack, Qp_ri, Q_cqi):
    """Rules 1-3 on the M x 12 matrix.  Returns kind [M, 12], own [M, 12] (a cell's symbol number in its own stream), under [M, 12] (for an
    ACK cell the CQI / data symbol it overwrote, NONE elsewhere), stream [12 M - Qp_ri] (the flat cell r * 12 + c of every symbol of
    CQI | data, in sequence order) and G."""
    M, n_cqi = 12 * n_prb, Q_cqi // Qm
    kind, own, under = np.zeros((M, 12), np.int64), np.zeros((M, 12), np.int64), np.full((M, 12), NONE, np.int64)
    r, c = walk_cells(M, Qp_ri, RI_WALK)
    kind[r, c], own[r, c] = RI, np.arange(Qp_ri)
    stream = np.flatnonzero(kind.reshape(-1) != RI)  # row by row, r ascending, c ascending, RI cells skipped
    t = np.arange(len(stream))
    kind.reshape(-1)[stream] = np.where(t < n_cqi, CQI, DATA)
    own.reshape(-1)[stream] = np.where(t < n_cqi, t, t - n_cqi)
    r, c = walk_cells(M, Qp_ack, ACK_WALK)
    under[r, c] = own[r, c]
    kind[r, c] = np.where(kind[r, c] == CQI, ACK_CQI, ACK_DATA)
    own[r, c] = np.arange(Qp_ack)
    return kind, own, under, stream, Qm * (12 * M - Qp_ri) - Q_cqi


def control_symbols(O, bits, Qp, Qm):
    """rule 4: [Qp, Qm] values of the coded ACK / RI symbols"""
    s = np.full((Qp, Qm), X, np.uint8)
    n = np.arange(Qp)
    if O == 1:
        s[:, 0], s[:, 1] = bits[0], Y
    elif O == 2:
        w = np.array([bits[0], bits[1], bits[0] ^ bits[1]], np.uint8)
        s[:, 0], s[:, 1] = w[(2 * n) % 3], w[(2 * n + 1) % 3]
    return s


def mux_py(n_prb, Qm, u, f, ack, ri, cqi):
    """rules 1-4: the values (0 / 1 / X / Y) in transmit order, bit (c * M + r) * Qm + q"""
    M = 12 * n_prb
    kind, own, under, stream, G = place(n_prb, Qm, u.Qp_ack, u.Qp_ri, u.Q_cqi)
    assert len(f) == G and len(cqi) == u.Q_cqi
    v = np.zeros((M * 12, Qm), np.uint8)
    v[stream] = np.concatenate([np.asarray(cqi, np.uint8), np.asarray(f, np.uint8)]).reshape(-1, Qm)
    v = v.reshape(M, 12, Qm)
    r, c = walk_cells(M, u.Qp_ri, RI_WALK)
    v[r, c] = control_symbols(u.O_ri, ri, u.Qp_ri, Qm)
    r, c = walk_cells(M, u.Qp_ack, ACK_WALK)
    v[r, c] = control_symbols(u.O_ack, ack, u.Qp_ack, Qm)
    return v.transpose(1, 0, 2).reshape(-1)


def gold(c_init, n):
    """36.211 7.2: c(i) = x1(i + 1600) ^ x2(i + 1600)"""
    N = 1600 + n
    x1, x2 = [0] * (N + 31), [0] * (N + 31)
    x1[0] = 1
    for i in range(31):
        x2[i] = (c_init >> i) & 1
    for i in range(N):
        x1[i + 31] = x1[i + 3] ^ x1[i]
        x2[i + 31] = x2[i + 3] ^ x2[i + 2] ^ x2[i + 1] ^ x2[i]
    return np.array([x1[i + 1600] ^ x2[i + 1600] for i in range(n)], np.uint8)


def scramble_py(v, c):
    """rule 5"""
    out = np.zeros(len(v), np.uint8)
    for i, b in enumerate(v):
        out[i] = 1 if b == X else out[i - 1] if b == Y else b ^ c[i]
    return out


# ---- map

@pytest.mark.parametrize("n_prb", [1, 2, 3, 5])
def test_map_equals_the_restated_rules(n_prb):
    """N_prb x Q_m 2/4/6 x every Qp_ri 0 .. 4 M x Qp_ack {0 .. 5, 4 M - 1, 4 M} x Q_cqi {0, Q_m, 20 Q_m, all but two stream cells}: classes,
    own indices, the overwritten positions, the class counts and G; ACK over CQI appears once the CQI reaches the last rows."""
    import openlte_amd as m
    M = 12 * n_prb
    seen = set()
    for Qm in (2, 4, 6):
        for Qp_ri in range(4 * M + 1):
            for Qp_ack in (0, 1, 2, 3, 4, 5, 4 * M - 1, 4 * M):
                for n_cqi in (0, 1, 20, 12 * M - Qp_ri - 2):
                    u = uci(1 if Qp_ack else 0, Qp_ack, 2 if Qp_ri else 0, Qp_ri, n_cqi * Qm)
                    kind, own, under, stream, G = place(n_prb, Qm, Qp_ack, Qp_ri, n_cqi * Qm)
                    assert G == Qm * (12 * M - Qp_ri) - n_cqi * Qm and G > 0
                    assert m.ulsch_uci_G(n_prb, Qm, u) == G
                    got_kind, got_index = m.ulsch_uci_map(n_prb, Qm, u)
                    key = (Qm, Qp_ri, Qp_ack, n_cqi)
                    assert (got_kind == kind).all(), key
                    assert (got_index[:, :, 0] == own).all() and (got_index[:, :, 1] == under).all(), key
                    cnt = np.bincount(got_kind.reshape(-1), minlength=5)
                    assert cnt.sum() == 12 * M and cnt[RI] == Qp_ri and cnt[ACK_DATA] + cnt[ACK_CQI] == Qp_ack
                    assert cnt[CQI] + cnt[ACK_CQI] == n_cqi and (cnt[DATA] + cnt[ACK_DATA]) * Qm == G
                    if n_cqi == 12 * M - Qp_ri - 2 and Qp_ack:
                        assert cnt[ACK_CQI] > 0, key
                    seen |= set(np.flatnonzero(cnt))
    assert seen == {DATA, CQI, RI, ACK_DATA, ACK_CQI}


def test_map_known_cells():
    """One matrix by hand: N_prb 1, QPSK, Qp_ri 5, Qp_ack 3, two CQI symbols."""
    import openlte_amd as m
    kind, index = m.ulsch_uci_map(1, 2, uci(1, 3, 1, 5, 4))
    assert kind[11].tolist() == [0, RI, ACK_DATA, 0, RI, 0, 0, RI, ACK_DATA, ACK_DATA, RI, 0]
    assert kind[10].tolist() == [0, RI, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0]
    assert kind[0].tolist() == [CQI, CQI] + [0] * 10
    assert index[11, :, 0].tolist()[1] == 0 and index[11, 10, 0] == 1 and index[11, 7, 0] == 2 and index[11, 4, 0] == 3 and index[10, 1, 0] == 4
    assert (index[11, 2].tolist(), index[11, 9].tolist(), index[11, 8].tolist()) == ([0, 130], [1, 135], [2, 134])
    # (rows 0-9 hold 120 stream cells, row 10 eleven: 131, less two of CQI -> column 0 of row 11 is data symbol 129, then columns 2, 3, 5, 6, 8, 9, 11)
    assert m.ulsch_uci_G(1, 2, uci(1, 3, 1, 5, 4)) == 2 * (144 - 5) - 4


# ---- symbol counts

def test_qprime_equals_integer_arithmetic():
    """O x beta (eighths) x M_sc_initial x sum K_r x N_prb: Q' = min(ceil(O' M_sc N_symb beta / sum K_r), cap), O' = O + 8 for a CQI above
    11 bits, cap 4 M (ACK, RI) or 12 M - Qp_ri (CQI) -- both caps reached."""
    import openlte_amd as m
    capped = {k: 0 for k in (m.UCI_ACK, m.UCI_RI, m.UCI_CQI)}
    free = dict(capped)
    for kind, O, beta8, msc, n_symb, sum_k, n_prb, qp_ri in itertools.product(
            (m.UCI_ACK, m.UCI_RI, m.UCI_CQI), (0, 1, 2, 4, 11, 12, 64), (10, 16, 20, 101, 1008), (12, 72, 300, 1200), (12, 11),
            (40, 1064, 6144, 13 * 5696), (1, 6, 25, 100), (0, 7)):
        Oe = O + 8 if kind == m.UCI_CQI and O > 11 else O
        M = 12 * n_prb
        cap = 12 * M - qp_ri if kind == m.UCI_CQI else 4 * M
        q = -((-Oe * msc * n_symb * beta8) // (8 * sum_k))
        assert m.ulsch_uci_qprime(kind, O, beta8, msc, n_symb, sum_k, n_prb, qp_ri) == min(q, cap), (kind, O, beta8, msc, n_symb, sum_k, n_prb, qp_ri)
        capped[kind] += q > cap
        free[kind] += 0 < q < cap
    assert all(capped.values()) and all(free.values())
    for bad in ((3, 1, 16, 72, 12, 1064, 6, 0), (0, 1, 16, 72, 12, 0, 6, 0), (0, 1, 16, 72, 12, 1064, 0, 0), (0, 1, 16, 72, 12, 1064, 111, 0),
                (2, 1, 16, 72, 12, 1064, 1, 49)):  # kind, no code block, N_prb 0 / 111, Qp_ri past 4 M
        with pytest.raises(m.MiLteError) as e:
            m.ulsch_uci_qprime(*bad)
        assert e.value.args[1] == ERR_INVALID


# ---- transmitter

def units_case():
    import openlte_amd as m
    cfg, ul = m.DlCfg(512, 25, 1, 0), m.UlCfg(3, 0, 0, 2, 1)
    allocs = [m.make_alloc(0, 1, 1096, list(range(0, 6)), 0x40), m.make_alloc(0, 2, 6200, list(range(6, 16)), 0x41, rv_idx=1),
              m.make_alloc(1, 3, 3240, list(range(2, 8)), 0x42, rv_idx=2), m.make_alloc(1, 1, 208, [9, 10], 0x43)]
    return cfg, ul, [1, 6], [21, 21], allocs


def test_units_with_all_zero_descriptors_are_the_plain_generators_bytes():
    from openlte_amd import synth
    cfg, ul, sfs, cells, allocs = units_case()
    iq_a, tx_a = synth.ul_units_3gpp(cfg, ul, sfs, cells, allocs, 2, snr_db=14.0, seed=11)
    iq_b, tx_b = synth.ul_units_3gpp(cfg, ul, sfs, cells, allocs, 2, uci=[uci()] * 4, snr_db=14.0, seed=11)
    assert iq_a.any() and iq_a.tobytes() == iq_b.tobytes() and tx_a.tobytes() == tx_b.tobytes()


def test_units_control_values_draw_nothing_from_the_generator():
    """With control information the payload bits are the ones the plain generator draws on the same seed (the control values are the
    caller's), and the samples differ."""
    from openlte_amd import synth
    cfg, ul, sfs, cells, allocs = units_case()
    us = [uci(1, 4, 0, 0, 0), uci(2, 6, 1, 3, 40), uci(), uci(0, 0, 2, 8, 0)]
    iq_a, tx_a = synth.ul_units_3gpp(cfg, ul, sfs, cells, allocs, 2, snr_db=14.0, seed=11)
    iq_b, tx_b = synth.ul_units_3gpp(cfg, ul, sfs, cells, allocs, 2, uci=us, ack=[[1], [0, 1], [], []], ri=[[], [1], [], [1, 1]],
                                     cqi=[[], np.arange(40) % 2, [], []], snr_db=14.0, seed=11)
    assert (tx_a == tx_b).all() and (iq_a != iq_b).any()


MUX_CASES = [(n_prb, mod, O) for n_prb in (1, 2) for mod in (1, 2, 3) for O in (1, 2)]


@pytest.mark.parametrize("n_prb,mod,O", MUX_CASES)
def test_multiplexer_and_scrambler_equal_the_restated_rules(n_prb, mod, O):
    """One allocation each of QPSK / 16QAM / 64QAM at N_prb 1 and 2, O = 1 and 2 for both ACK and RI, a partial RI row, CQI that the ACK
    reaches at N_prb 1: the values before scrambling = the numpy multiplexer over ulsch_encode_3gpp(bits, G, ..), the coded control symbols
    and the CQI bits; after scrambling x is 1, y repeats the bit before it, every other bit is b ^ c(i)."""
    import openlte_amd as m
    from openlte_amd import synth
    Qm, M = 2 * mod, 12 * n_prb
    rng = np.random.default_rng(100 * n_prb + 10 * mod + O)
    tbs = {1: 72, 2: 208}[n_prb]
    n_cqi = 12 * M - 9 - 30 if n_prb == 1 else 20  # N_prb 1: the CQI ends 30 cells before the matrix does, under the ACK's last rows
    u = uci(O, 4 * M - 1 if n_prb == 1 else 7, O, 9, n_cqi * Qm)
    G = m.ulsch_uci_G(n_prb, Qm, u)
    bits = rng.integers(0, 2, tbs).astype(np.uint8)
    ack, ri, cqi = rng.integers(0, 2, O).astype(np.uint8), rng.integers(0, 2, O).astype(np.uint8), rng.integers(0, 2, n_cqi * Qm).astype(np.uint8)
    f = synth.ulsch_encode_3gpp(bits, G, Qm, 0)
    c_init = (0x1234 << 14) | (7 << 9) | 301
    mux, scr = synth.ulsch_mux_3gpp(n_prb, Qm, u, f, ack, ri, cqi, c_init)
    want = mux_py(n_prb, Qm, u, f, ack, ri, cqi)
    assert (mux == want).all()
    assert ((want == X).sum() > 0) == (Qm > 2) and ((want == Y).sum() > 0) == (O == 1)
    c = gold(c_init, len(want))
    assert (scr == scramble_py(want, c)).all()
    assert (scr[want == X] == 1).all() and (scr[want == Y] == scr[np.flatnonzero(want == Y) - 1]).all()
    plain = want < 2
    assert (scr[plain] == want[plain] ^ c[plain]).all()
    if n_prb == 1:
        kind = m.ulsch_uci_map(n_prb, Qm, u)[0]
        assert (kind == ACK_CQI).any() and (kind == ACK_DATA).any()


# ---- refusals

def test_refusals_of_the_host_functions():
    """O > 2, Q' > 4 M, O without Q' and Q' without O, Q_cqi not a multiple of Q_m, G <= 0; a Q_m or N_prb outside the mode; and a transport
    block that the remaining G cannot carry (mi_lte_ulsch_layout) at the generator."""
    import openlte_amd as m
    from openlte_amd import synth
    M = 12
    bad = [uci(3, 4), uci(0, 0, 3, 4), uci(1, 4 * M + 1), uci(0, 0, 1, 4 * M + 1), uci(0, 4), uci(1, 0), uci(0, 0, 0, 4), uci(0, 0, 2, 0),
           uci(Q_cqi=3), uci(Q_cqi=2 * 144), uci(0, 0, 1, 48, 2 * 96)]
    for u in bad:
        for fn in (m.ulsch_uci_G, m.ulsch_uci_map):
            with pytest.raises(m.MiLteError) as e:
                fn(1, 2, u)
            assert e.value.args[1] == ERR_INVALID, (fn.__name__, u.O_ack, u.Qp_ack, u.O_ri, u.Qp_ri, u.Q_cqi)
        with pytest.raises(m.MiLteError):
            synth.ulsch_mux_3gpp(1, 2, u, np.zeros(288, np.uint8), [0, 0], [0, 0], np.zeros(max(u.Q_cqi, 1), np.uint8))
    assert m.ulsch_uci_G(1, 2, uci(Q_cqi=2 * 143)) == 2 and m.ulsch_uci_G(1, 2, uci(2, 48, 2, 48, 2 * 95)) == 2
    for n_prb, Qm in ((1, 1), (1, 3), (1, 8), (0, 2), (111, 2)):
        with pytest.raises(m.MiLteError) as e:
            m.ulsch_uci_G(n_prb, Qm, uci())
        assert e.value.args[1] == ERR_INVALID
    cfg, ul = m.DlCfg(512, 25, 1, 0), m.UlCfg(3, 0, 0, 2, 1)
    two = [m.make_alloc(0, 3, 6200, list(range(10)), 0x50)]  # two code blocks
    ok = synth.ul_units_3gpp(cfg, ul, [0], [21], two, 1, uci=[uci(1, 12)], ack=[[1]])
    assert ok[0].any()
    with pytest.raises(m.MiLteError):  # G = 6: one symbol for two code blocks
        synth.ul_units_3gpp(cfg, ul, [0], [21], two, 1, uci=[uci(Q_cqi=6 * (1440 - 1))], cqi=[np.zeros(6 * 1439, np.uint8)])
    for u in bad:
        with pytest.raises(m.MiLteError):
            synth.ul_units_3gpp(cfg, ul, [0], [21], [m.make_alloc(0, 1, 72, [0], 0x51)], 1, uci=[u], ack=[[0] * u.O_ack], ri=[[0] * u.O_ri],
                                cqi=[np.zeros(u.Q_cqi, np.uint8)])
