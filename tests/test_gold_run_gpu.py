"""The PDSCH demodulators' scrambling words by recurrence (openlte_amd/csrc/gold_run.h; mi_lte_set_gold_recurrence) and the compact loop's
trimmed loads (chain.hip).  Every plan runs with the recurrence and with the table method -- the method of every build before, which the
existing suites pin to the reference -- in ONE context: e_len, every soft-bit tap byte, every verdict and every decoded bit identical.  The
compact plans run against the full-estimate form of the same input, byte for byte, at every control-region size.  At most four subframes a
plan.  tests/test_gold_run_cpu.py holds the two word steps against the bitwise definition."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

FFT = {6: 128, 25: 512, 100: 2048}
QM = {0: 1, 1: 2, 2: 4, 3: 6}
RUNS = (2, 4, 8)  # the run lengths gold_fill_words was measured at; the kernels are built with one of them


def n_words(cfi, n_prb, mod):
    """the words a workgroup fills: 0 .. n_words_ub inclusive (k_pdsch_demod's prologue)"""
    return ((14 - cfi) * n_prb * 12 * QM[mod] + 31) // 32 + 1


# a case: (N_rb_dl, ports, plan CFI, [(subframe, cell, [(mod_type, tbs, first PRB, PRBs, rnti, own CFI or 0)])]); every unit the same number of allocations
# 1 PRB of QPSK on a 6-RB cell: 10 words with CFI 2 (subframe 0: the PBCH / PSS / SSS window over the whole band), next to 16QAM and 64QAM
SMALLEST = (6, 1, 2, [(0, 11, [(1, 16, 0, 1, 0x21, 0), (2, 16, 2, 1, 0x22, 0), (3, 16, 5, 1, 0x23, 0)]),
                      (3, 77, [(1, 16, 5, 1, 0x24, 0), (2, 16, 0, 1, 0x25, 0), (3, 16, 3, 1, 0x26, 0)])])
# 100 PRB of 64QAM with CFI 1: 2 926 words, more than the 192 lanes of waves 1-3 times any of the run lengths, so a lane takes several runs
LARGEST = (100, 1, 1, [(4, 503, [(3, 5160, 0, 100, 0x51, 0)])])
# QPSK with CFI 2 fills 9 N_prb + 1 words: 6, 7, 8 PRB are 55, 64, 73 -- one below, on and one above a multiple of 8, 4 and 2; 64QAM on 1, 3, 5
# PRB 28, 82, 136 (a multiple of 4 and of 2 / of 2 / of 8), 16QAM on 2 PRB 37 (a multiple of 4 plus 1), 16QAM on 1 PRB with CFI 1 21
RESIDUES = (100, 1, 2, [(1, 42, [(1, 328, 0, 6, 0x101, 0), (1, 328, 10, 7, 0x102, 0), (1, 328, 20, 8, 0x103, 0), (3, 328, 30, 1, 0x104, 0)]),
                        (6, 301, [(3, 1064, 40, 3, 0x105, 0), (3, 1064, 50, 5, 0x106, 0), (2, 328, 60, 2, 0x107, 0), (2, 208, 70, 1, 0x108, 1)])])
# c_init = rnti << 14 | subframe << 9 | cell at both ends: 26 set bits (four batches of table loads in the jump) and one
EXTREMES = (100, 1, 2, [(9, 503, [(3, 3240, 44, 12, 0xFFFF, 0), (1, 328, 0, 3, 0xFFFF, 0)]), (0, 0, [(3, 3240, 44, 12, 1, 0), (2, 1096, 10, 4, 1, 0)])])
TWO_PORT = (100, 2, 2, [(1, 11, [(2, 208, 0, 1, 0x111, 0), (3, 3240, 44, 12, 0x112, 0), (1, 328, 2, 3, 0x113, 0)])])
CASES = {"smallest": SMALLEST, "largest": LARGEST, "residues": RESIDUES, "extremes": EXTREMES}


def test_the_shapes_are_what_they_are_called():
    """(no kernel runs here; the word counts the cases above claim)"""
    assert n_words(2, 1, 1) == 10 and n_words(1, 100, 3) == 2926 > 192 * max(RUNS)
    got = [n_words(own or RESIDUES[2], n, mod) for (sf, cell, lst) in RESIDUES[3] for (mod, tbs, p0, n, rnti, own) in lst]
    assert got == [55, 64, 73, 28, 82, 136, 37, 21], got
    for R in RUNS:
        assert {0, 1, R - 1} <= {g % R for g in got}, (R, got)


def _allocs(m, case):
    return [m.make_alloc(u, mod, tbs, list(range(p0, p0 + n)), rnti, 0, 1, None, own) for u, (sf, cell, lst) in enumerate(case[3])
            for (mod, tbs, p0, n, rnti, own) in lst]


def _input(ctx, m, case, seed, synth_cfi=None):
    """The case's units from the synthesiser (one control-region size for the whole grid) on the device, before the front end"""
    from openlte_amd import synth
    n_rb, n_ant, cfi, units = case
    sfs, cells = [u[0] for u in units], [u[1] for u in units]
    iq, _ = synth.dl_units(m.DlCfg(FFT[n_rb], n_rb, 1, m.IQ_I8), sfs, cells, _allocs(m, case), len(units[0][2]), n_pdcch_symbs=synth_cfi or cfi, snr_db=28.0,
                           max_delay=4, seed=seed)
    return {"iq": ctx.to_device(iq.reshape(-1, 2)), "start": ctx.to_device((np.arange(len(units)) * iq.shape[1]).astype(np.uint64)),
            "sf": ctx.to_device(np.asarray(sfs, np.uint32)), "cell": ctx.to_device(np.asarray(cells, np.uint32)), "sfs": sfs, "cells": cells}


def _free(inp):
    for k in ("iq", "start", "sf", "cell"):
        inp[k].free()


def _plan(ctx, m, case, inp, fmt):
    """The input through the front end in the estimate form fmt, and the case's plan on it"""
    n_rb, n_ant, cfi, units = case
    cfg = m.DlCfg(FFT[n_rb], n_rb, n_ant, m.IQ_I8 | fmt)
    d_sub = ctx.alloc(len(units) * ctx.subframe_floats(n_ant) * 4)
    d_sub.zero()
    ctx.dl_frontend_dev(cfg, inp["iq"], None, inp["start"], inp["sf"], inp["cell"], len(units), d_sub)
    return ctx.pdsch_plan(cfg, cfi, _allocs(m, case)), d_sub


def _run(ctx, plan, d_sub, inp, recurrence):
    ctx.set_gold_recurrence(recurrence)
    st, bits = plan.run(d_sub, inp["sfs"], inp["cells"])
    return st.copy(), [b.copy() for b in bits], [plan.soft_bits(a).copy() for a in range(len(bits))]


def _same(x, y, what):
    assert (x[0] == y[0]).all(), (what, "status", x[0], y[0])
    assert len(x[1]) == len(y[1]) == len(x[2]) == len(y[2])
    for a in range(len(x[1])):
        assert len(x[2][a]) == len(y[2][a]) > 0, (what, "e_len of allocation", a, len(x[2][a]), len(y[2][a]))
        assert (x[2][a] == y[2][a]).all(), (what, "soft bits of allocation", a, int((x[2][a] != y[2][a]).sum()))
        assert x[1][a].shape == y[1][a].shape and (x[1][a] == y[1][a]).all(), (what, "bits of allocation", a)


def _both_methods(ctx, plan, d_sub, inp, what):
    """recurrence, table method, recurrence again: identical.  Returns the recurrence's results."""
    try:
        on = _run(ctx, plan, d_sub, inp, True)
        off = _run(ctx, plan, d_sub, inp, False)
        again = _run(ctx, plan, d_sub, inp, True)
    finally:
        ctx.set_gold_recurrence(True)
    _same(on, off, what)
    _same(again, off, what + " (second run)")
    return on


@pytest.mark.parametrize("fmt", ["full", "compact"])
@pytest.mark.parametrize("name", sorted(CASES))
def test_recurrence_and_table_method_agree(ctx, name, fmt):
    """k_pdsch_demod<true> on full estimate planes and k_pdsch_demod<true, true> on the compact form: the smallest and the largest allocation,
    word counts on, one above and one below a multiple of the run length, and the extremes of c_init."""
    import openlte_amd as m
    case = CASES[name]
    inp = _input(ctx, m, case, seed=1100 + len(name))
    plan, d_sub = _plan(ctx, m, case, inp, m.CE_COMPACT if fmt == "compact" else 0)
    on = _both_methods(ctx, plan, d_sub, inp, "%s %s" % (name, fmt))
    assert (on[0] == 0).any(), on[0]  # (the plans are no noise: something decodes)
    plan.close()
    d_sub.free()
    _free(inp)


def test_two_port_plan(ctx):
    """k_pdsch_demod<false>: the transmit-diversity combiner on a single-port capture -- whatever comes out, the same either way"""
    import openlte_amd as m
    inp = _input(ctx, m, TWO_PORT, seed=1200)
    plan, d_sub = _plan(ctx, m, TWO_PORT, inp, 0)
    _both_methods(ctx, plan, d_sub, inp, "two ports")
    plan.close()
    d_sub.free()
    _free(inp)


def test_maxlog_plan(ctx):
    """The second call site, k_pdsch_demod_llr: a 3GPP plan with MI_LTE_DEMAP_MAXLOG astride the 25-RB cell's PBCH / PSS / SSS window, control
    regions of 1, 2 and 3 symbols: soft bits, gains, verdicts, output rows and the code blocks' soft values identical."""
    import openlte_amd as m
    from test_demap_llr_gpu import N_SOFT, case
    from test_harq_gpu import Tx, decode
    n_rb, cfi, sfs, cells, per_unit, _ = case("25rb_window")
    t = Tx(ctx, n_rb, sfs, cells, per_unit, N_SOFT, cfi, 14.0, seed=1300)
    plan = t.plan(N_SOFT)
    plan.set_demapper(m.DEMAP_MAXLOG, 0.0)
    res = []
    try:
        for recurrence in (True, False, True):
            ctx.set_gold_recurrence(recurrence)
            out = decode(t, plan)
            assert ctx.last_kernels().startswith("k_pdsch_demod_llr:1,")
            res.append((out, [plan.soft_bits(a).copy() for a in range(plan.n_alloc)], plan.llr_gain().copy()))
    finally:
        ctx.set_gold_recurrence(True)
    (o0, e0, g0) = res[1]
    for (o, e, g) in (res[0], res[2]):
        assert (o["st"] == o0["st"]).all() and (o["rows"] == o0["rows"]).all() and (o["cb_ok"] == o0["cb_ok"]).all() and (g == g0).all()
        for a in range(plan.n_alloc):
            assert len(e[a]) == len(e0[a]) > 0 and (e[a] == e0[a]).all(), a
            assert (o["cb_soft"][a] == o0["cb_soft"][a]).all(), a
    assert (np.abs(e0[0]) < 127).any() and (o0["st"] == 0).any()
    plan.close()
    t.free()


# the compact loop requests a first-slot row only from the allocation's own control-region size on: plan CFI x own CFI, both ways round
def _cfi_case(n_rb, plan_cfi):
    if n_rb == 6:  # (a 6-RB cell's control region has 2 to 4 symbols)
        return (6, 1, plan_cfi, [(0, 12, [(1, 72, 0, 2, 0x31, 0), (3, 72, 2, 2, 0x32, 6 - plan_cfi), (2, 72, 4, 2, 0x33, 0)]),
                                 (7, 251, [(3, 72, 0, 2, 0x34, 0), (2, 72, 2, 2, 0x35, 2), (1, 72, 4, 2, 0x36, 0)])])
    other = {1: 3, 2: 1, 3: 2}[plan_cfi]
    return (100, 1, plan_cfi, [(5, 43, [(3, 3240, 42, 12, 0x121, 0), (3, 3240, 0, 12, 0x122, other), (1, 328, 20, 3, 0x123, 0), (2, 1096, 90, 4, 0x124, other)]),
                               (8, 300, [(3, 3240, 30, 12, 0x125, 0), (1, 680, 60, 8, 0x126, other), (2, 1096, 12, 4, 0x127, 0), (3, 1064, 96, 4, 0x128, 0)])])


@pytest.mark.parametrize("n_rb,plan_cfi", [(100, 1), (100, 2), (100, 3), (6, 4), (6, 2)])
def test_compact_loads_by_control_region_size(ctx, n_rb, plan_cfi):
    """The compact form against the full-estimate form of the same input (as tests/test_chain_gpu.py's
    test_compact_estimate_form_is_bit_identical): every soft bit, verdict and decoded bit.  The grid is synthesised with a one-symbol control
    region (two on the 6-RB cell), so every symbol an allocation may start at holds data, and an allocation whose own n_pdcch_symbs differs
    from the plan's reads the rows of ITS control-region size.  Both scrambling methods on the compact plan while it is there."""
    import openlte_amd as m
    case = _cfi_case(n_rb, plan_cfi)
    inp = _input(ctx, m, case, seed=1400 + plan_cfi, synth_cfi=2 if n_rb == 6 else 1)
    res = []
    for fmt in (0, m.CE_COMPACT):
        plan, d_sub = _plan(ctx, m, case, inp, fmt)
        res.append(_both_methods(ctx, plan, d_sub, inp, "cfi %d fmt %x" % (plan_cfi, fmt)) if fmt else _run(ctx, plan, d_sub, inp, True))
        plan.close()
        d_sub.free()
    _same(res[1], res[0], "compact against full, plan cfi %d" % plan_cfi)
    lens = [len(e) for e in res[1][2]]
    own = [o or plan_cfi for (sf, cell, lst) in case[3] for (*_x, o) in lst]
    assert len(set(own)) >= 2 and all(n > 0 for n in lens), (own, lens)
    _free(inp)
