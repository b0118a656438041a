"""GPU: k_ulsch_cqi_decode (36.212 5.2.2.6.4 on the receiving side) through mi_lte_cqi_decode_batch and through a PUSCH plan with control
information (mi_lte_pusch_plan_set_cqi_decode).  The kernel is integer work, so every field of every record is compared exactly: the block
code against the exhaustive numpy search, the convolutional code against the numpy three-lap model (test_ulsch_cqi_cpu, where the model is
itself checked against brute-force maximum likelihood), the plan against the batch entry point on its own taps and against the sent bits."""
import numpy as np
import pytest

from test_ulsch_cqi_cpu import (BLOCK_MAX, CONV_O, CRC_OK, MAX_Q, NO_CRC, ZERO, block_words, conv_Q, encode_py, model, noisy, pack_bits)
from test_ulsch_uci_cpu import uci
from test_ulsch_uci_gpu import QM, Grant, UciUnits, tbs_at_most

pytestmark = pytest.mark.gpu

ERR_INVALID = -1
PLAN_HEAD = "k_pusch_demod:1,k_ulsch_uci_gather:1,k_ulsch_uci_decide:1,"


def decode(ctx, runs, pad=0):
    """the runs [(e, O)] back to back (pad bytes in front of each) through one cqi_decode_batch"""
    parts, descs, at = [], [], 0
    for e, O in runs:
        parts += [np.zeros(pad, np.int8), e]
        descs.append((at + pad, len(e), O))
        at += pad + len(e)
    assert all(d[0] % 2 == 0 for d in descs)
    return ctx.cqi_decode_batch(np.concatenate(parts), descs), descs


def check(ctx, runs, pad=0):
    got, _ = decode(ctx, runs, pad)
    want = model(runs)
    for k, (g, w) in enumerate(zip(got, want)):
        assert g == w, (k, runs[k][1], len(runs[k][0]), g, w)
    return got


def inputs(O, Q, rng, sigmas):
    """code word plus noise at each sigma, uniform random int8, all zero"""
    q = encode_py(rng.integers(0, 2, O), Q)
    return [noisy(q, s, rng) for s in sigmas] + [rng.integers(-128, 128, Q).astype(np.int8), np.zeros(Q, np.int8)]


def rails(O, Q, rng):
    """+-127 everywhere: a code word, and one sign for all"""
    q = encode_py(rng.integers(0, 2, O), Q)
    return [(127 * (1 - 2 * q.astype(np.int64))).astype(np.int8), np.full(Q, -127, np.int8)]


@pytest.mark.parametrize("Q", [20, 32, 44, 1200, MAX_Q])
def test_block_code_equals_the_exhaustive_search(ctx, Q):
    """Every O in 1 .. 11: sigma 0.8, sigma 1.6 (wrong decisions must be the same wrong decisions), random int8, all zero (word 0, metric
    0); at the largest Q also the +-127 rails (the int32 sums)."""
    rng = np.random.default_rng(100 + Q)
    runs = [(e, O) for O in range(1, 12) for e in inputs(O, Q, rng, (0.8, 1.6)) + (rails(O, Q, rng) if Q == MAX_Q else [])]
    got = check(ctx, runs)
    per = len(runs) // 11
    for O in range(1, 12):
        z = got[(O - 1) * per + 3]
        assert z == {"O": O, "crc": NO_CRC, "metric": 0, "energy": 0, "bits": [0, 0, 0, 0]}
    if Q == MAX_Q:
        assert max(g["energy"] for g in got) == 127 * MAX_Q


def test_block_code_ties_go_to_the_smaller_word(ctx):
    """r = 10 (s(w1) + s(w2)): both words reach the maximum.  The pairs lie in one lane and two cosets, in two lanes of one coset, and with
    the smaller word in the higher lane of the earlier coset."""
    words, runs = 1 - 2 * block_words(11), []
    for w1, w2 in ((5, 1029), (67, 70), (63, 64)):
        r = 10 * (words[w1] + words[w2])
        metric = words @ r
        assert (metric == metric.max()).sum() >= 2 and int(np.argmax(metric)) == w1 and metric[w2] == metric.max()
        runs.append((np.tile(r, 2).astype(np.int8), 11))
    got = check(ctx, runs)
    assert [g["bits"][0] for g in got] == [5, 67, 63]


def test_convolutional_code_equals_the_three_lap_model(ctx):
    """O in {12, 24, 25, 56, 64, 128} x Q_cqi in {2 L, 3 L, 3 L + 2, 7 L + 4}: sigma 0.8, sigma 1.3, random int8, all zero; and the largest
    Q_cqi on the +-127 rails."""
    rng = np.random.default_rng(200)
    runs = [(e, O) for O in CONV_O for Q in conv_Q(O) for e in inputs(O, Q, rng, (0.8, 1.3))]
    runs += [(e, O) for O in CONV_O for e in rails(O, MAX_Q, rng)]
    got = check(ctx, runs)
    n_ok = sum(g["crc"] == CRC_OK for g in got)
    print("%d runs, CRC8 passed on %d" % (len(got), n_ok))
    assert n_ok >= len(CONV_O) * 4  # (at least the sigma 0.8 runs with Q_cqi >= 3 L and the code-word rails)


def test_mixed_batch_odd_dword_offsets_and_unservable_descriptors(ctx):
    """Both codes in one batch at offsets that are 2 mod 4; a descriptor of each unservable kind (O = 0, O > 128, Q_cqi = 0, Q_cqi above the
    cap, odd offset) gives the zero record and leaves its neighbours alone."""
    rng = np.random.default_rng(300)
    runs = [(noisy(encode_py(rng.integers(0, 2, O), Q), 0.9, rng), O) for O, Q in ((3, 22), (64, 218), (11, 46), (12, 62), (128, 410), (7, 34), (25, 102))]
    want = model(runs)
    got, descs = decode(ctx, runs, pad=2)
    assert all(d[0] % 4 == 2 for d in descs) and got == want
    soft = np.concatenate([np.concatenate([np.zeros(2, np.int8), e]) for e, _ in runs])
    bad = [(descs[0][0], 22, 0), (descs[1][0], 218, 129), (descs[2][0], 0, 11), (descs[3][0], MAX_Q + 1, 12), (descs[4][0] + 1, 100, 12)]
    mixed, is_bad = [], []
    for k, d in enumerate(descs):
        mixed.append(d)
        is_bad.append(False)
        if k < len(bad):
            mixed.append(bad[k])
            is_bad.append(True)
    got = ctx.cqi_decode_batch(soft, mixed)
    assert [g for g, b in zip(got, is_bad) if b] == [ZERO] * len(bad)
    assert [g for g, b in zip(got, is_bad) if not b] == want
    assert ctx.last_kernels() == "k_ulsch_cqi_decode:1"


# ---- the plan

def cqi_grants():
    """1 PRB QPSK with 40 ACK symbols over rows 2 .. 11 of 12 and CQI in rows 0 .. 4 (erasures), O = 4; 6 PRB 16QAM, O = 11; 10 PRB 64QAM with
    RI, O = 64 (L = 72, Q_cqi = 5 L)"""
    import openlte_amd as m
    gr = [(Grant(1, 16, 1, 3, 0x201, uci(1, 40, 0, 0, 120), [1], seed=1), 4),
          (Grant(2, 0, 6, 5, 0x202, uci(1, 8, 1, 4, 120), [0], [1], rv=1, seed=2), 11),
          (Grant(3, 0, 10, 12, 0x203, uci(2, 12, 2, 7, 360), [1, 0], [0, 1], seed=3), 64)]
    rng = np.random.default_rng(400)
    for g, O in gr:
        if g.tbs == 0:
            left = m.ulsch_uci_G(g.n_prb, QM[g.mod], g.u) - QM[g.mod] * g.u.Qp_ack
            g.tbs = tbs_at_most(g.n_prb, int(0.6 * left) - 24)
        g.o = rng.integers(0, 2, O).astype(np.uint8)
        g.cqi = m.cqi_encode(O, g.o, g.u.Q_cqi)
    return [g for g, _ in gr], [O for _, O in gr]


@pytest.mark.parametrize("clean", [False, True])
def test_plan_decodes_cqi(ctx, clean):
    """30 dB and noiseless: the records equal cqi_decode_batch on the plan's own cqi_soft taps and the model, and carry the sent bits with
    _NO_CRC / _CRC_OK; ACK symbols erased CQI soft bits of the first grant; transport blocks, verdicts, cb_ok and the ACK / RI records are
    those of the same plan without the setter."""
    grants, Os = cqi_grants()
    un = UciUnits(ctx, 25, 91, grants, 30.0, seed=51, clean=clean)
    p0, p1 = un.plan(), un.plan()
    st0, bits0 = p0.run(un.d_sub)
    p1.set_cqi_decode(Os)
    st1, bits1 = p1.run(un.d_sub)
    assert st0.tobytes() == st1.tobytes() and all(a.tobytes() == b.tobytes() for a, b in zip(bits0, bits1))
    assert p0.cb_ok().tobytes() == p1.cb_ok().tobytes() and p0.uci_results() == p1.uci_results()
    assert all(st1[k] == 0 and (bits1[k] == un.sent(k)).all() for k in range(len(grants)))
    rec = p1.cqi_results()
    taps = [p1.cqi_soft(k) for k in range(len(grants))]
    assert all(t.tobytes() == p0.cqi_soft(k).tobytes() for k, t in enumerate(taps))
    assert (taps[0] == 0).sum() >= 24 and p0.cqi_results() == [ZERO] * len(grants)
    runs = list(zip(taps, Os))
    assert rec == decode(ctx, runs, pad=2)[0] == model(runs)
    for k, (g, O) in enumerate(zip(grants, Os)):
        print("alloc %d: O %d Q_cqi %d record %s" % (k, O, g.u.Q_cqi, rec[k]))
        assert rec[k]["O"] == O and rec[k]["bits"] == pack_bits(g.o) and rec[k]["crc"] == (NO_CRC if O <= BLOCK_MAX else CRC_OK), k
        assert 0 < rec[k]["metric"] <= rec[k]["energy"]
    p1.set_cqi_decode([0, 11, 0])  # the others left opaque: their records go back to zero
    p1.run(un.d_sub)
    assert p1.cqi_results() == [ZERO, rec[1], ZERO]
    for p in (p0, p1):
        p.close()
    un.free()


def small_units(ctx, seed):
    import openlte_amd as m
    g = Grant(2, tbs_at_most(6, 1000), 6, 0, 0x211, uci(1, 8, 1, 4, 40), [1], [1], seed=21)
    g.o = np.array([1, 0, 1, 1, 0], np.uint8)
    g.cqi = m.cqi_encode(5, g.o, 40)
    return UciUnits(ctx, 25, 5, [g], 30.0, seed=seed)


def test_last_kernels_with_and_without_the_setter(ctx):
    un = small_units(ctx, 52)
    plan = un.plan()
    plan.run(un.d_sub)
    lk = ctx.last_kernels()
    assert lk.startswith(PLAN_HEAD + "k_dl3_desc:1,") and "k_ulsch_cqi" not in lk
    plan.set_cqi_decode([5])
    plan.run(un.d_sub)
    assert ctx.last_kernels() == lk.replace(PLAN_HEAD, PLAN_HEAD + "k_ulsch_cqi_decode:1,")
    plan.set_cqi_decode(None)
    plan.run(un.d_sub)
    assert ctx.last_kernels() == lk
    plain = un.plan(with_uci=False)
    plain.run(un.d_sub)
    assert ctx.last_kernels().startswith("k_pusch_demod:1,k_dl3_desc:1,") and "k_ulsch" not in ctx.last_kernels()
    plain.close()
    plan.close()
    un.free()


def test_setter_refusals_leave_the_plan_as_it_was(ctx):
    """A plain 3GPP plan, a reference-mode plan, O > 128, O > 0 on an allocation without CQI: MI_LTE_ERR_INVALID_ARG, and the next run of the
    good plan decodes what it decoded before."""
    import ctypes as C
    import openlte_amd as m
    un = small_units(ctx, 53)
    g0 = Grant(2, tbs_at_most(6, 1000), 6, 0, 0x212, uci(1, 8), [0], seed=22)  # control information without CQI
    un0 = UciUnits(ctx, 25, 5, [g0], 30.0, seed=54)
    good, no_cqi, plain = un.plan(), un0.plan(), un.plan(with_uci=False)
    ref_mode = ctx.pusch_plan(un.cfg, un.ul, un.sfs, un.cells, [m.make_alloc(0, 1, 1544, list(range(10)), 0x213)])
    good.set_cqi_decode([5])

    def still_runs():
        st, bits = good.run(un.d_sub)
        rec = good.cqi_results()[0]
        assert st[0] == 0 and (bits[0] == un.sent(0)).all() and (rec["O"], rec["crc"], rec["bits"]) == (5, NO_CRC, pack_bits(un.g[0].o))
        assert PLAN_HEAD + "k_ulsch_cqi_decode:1," in ctx.last_kernels()

    still_runs()
    p = C.c_void_p()
    for plan, O in ((plain, [5]), (ref_mode, [5]), (good, [129]), (no_cqi, [4])):
        with pytest.raises(m.MiLteError) as e:
            plan.set_cqi_decode(O)
        assert e.value.args[1] == ERR_INVALID
        still_runs()
    for plan in (plain, ref_mode):
        assert ctx.L.mi_lte_pusch_plan_cqi_results(plan.h, C.byref(p)) == ERR_INVALID
    no_cqi.set_cqi_decode([0])  # nothing to decode is no refusal
    st, _ = no_cqi.run(un0.d_sub)
    assert st[0] == 0 and no_cqi.cqi_results() == [ZERO]
    for plan in (good, no_cqi, plain, ref_mode):
        plan.close()
    un.free()
    un0.free()


def test_records_are_zero_before_a_first_run(ctx):
    un = small_units(ctx, 55)
    plan = un.plan()
    assert plan.cqi_results() == [ZERO]
    plan.set_cqi_decode([5])
    assert plan.cqi_results() == [ZERO]
    plan.close()
    un.free()
