"""The packed hand-over of 16QAM / 64QAM soft bits between k_pdsch_demod and k_turbo_prep (openlte_amd/csrc/soft_pack.h; mi_lte_set_soft_packed):
every case runs with the switch on and off in ONE context and compares status, decoded bits -- CRC failures included -- and the stage tap's
bytes of every allocation.  Where the compiled reference is there (oracle/_ref) and the allocations fit its 10 000-soft-bit scratch, status and
bits are the reference's too (its own received grid, as tests/test_mixed_gpu.py does).  20 MHz plans of one or two subframes."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

# a unit: (subframe, cell, CFI, [(mod_type, tbs, first PRB, PRBs, rnti, rv)])
ONE_PRB = [(1, 11, 1, [(2, 208, 0, 1, 0x101, 0), (3, 328, 1, 1, 0x102, 0), (1, 328, 2, 3, 0x103, 0), (3, 408, 99, 1, 0x104, 1)]),
           (6, 301, 3, [(2, 176, 7, 1, 0x201, 0), (3, 280, 8, 1, 0x202, 0), (1, 256, 20, 3, 0x203, 0), (2, 144, 50, 1, 0x204, 2)])]
# W4's code block (64QAM, 12 PRB, TBS 3240) on subframes 0 and 5: across the PSS / SSS / PBCH sub-carriers, which take soft bits away, and clear of
# them (9936 soft bits, just over one lap of K = 3264's 9804 positions: the `halving` path), next to a second size (the merged launches)
W4_SYNC = [(0, 42, 2, [(3, 3240, 44, 12, 0x111, 0), (3, 1064, 60, 4, 0x112, 0)]), (5, 43, 2, [(3, 3240, 42, 12, 0x121, 0), (3, 3240, 0, 12, 0x122, 0)])]
# 16QAM: 4 PRB behind TBS 328 (K = 352) is two laps, more than the lap and a quarter a merged launch stages at K <= 1024: lap by lap
REPEAT = [(2, 7, 2, [(2, 328, 0, 4, 0x131, 0), (2, 208, 4, 3, 0x132, 1), (2, 1096, 10, 4, 0x133, 0), (1, 328, 20, 3, 0x134, 0)])]
# 64QAM on 50 PRB, one code block: more than 32 768 soft bits (not through the demodulator's LDS block as bytes; beyond whole staging in prep)
LONG = [(3, 99, 2, [(3, 5160, 10, 50, 0x141, 0), (1, 328, 70, 3, 0x142, 0)])]
# K = 40 behind 13 PRB of 64QAM: more than 258 laps, so 32-bit sums in the per-size kernel, which stages the allocation whole (packed) ...
MANY_LAPS = [(4, 5, 2, [(3, 16, 0, 13, 0x151, 0), (3, 1064, 20, 4, 0x152, 0), (2, 1096, 30, 4, 0x153, 0)])]
# ... and behind 60 PRB: too long to stage, gathered straight from global memory -- the host keeps such a run in bytes
MANY_LAPS_GLOBAL = [(4, 5, 2, [(3, 16, 0, 60, 0x151, 0), (3, 1064, 60, 4, 0x152, 0), (2, 1096, 70, 4, 0x153, 0)])]
QPSK_ONLY = [(7, 9, 2, [(1, 328, 0, 3, 0x161, 0), (1, 256, 5, 3, 0x162, 0)])]


def _allocs(m, lists):
    return [m.make_alloc(u, mod, tbs, list(range(p0, p0 + n)), rnti, rv, 1, None, cfi) for u, (sf, cell, cfi, lst) in enumerate(lists)
            for (mod, tbs, p0, n, rnti, rv) in lst]


def _iq(m, lists, seed, snr_db):
    from openlte_amd import synth
    cfg = m.DlCfg(2048, 100, 1, m.IQ_I8)
    iq = []
    for u, (sf, cell, cfi, lst) in enumerate(lists):
        al = [m.make_alloc(0, mod, tbs, list(range(p0, p0 + n)), rnti, rv, 1, None, cfi) for (mod, tbs, p0, n, rnti, rv) in lst]
        iq.append(synth.dl_units(cfg, [sf], [cell], al, len(al), n_pdcch_symbs=cfi, snr_db=snr_db, max_delay=8, seed=seed + u)[0][0])
    return np.array(iq)


def _subframes(ctx, m, lists, iq, fmt, n_ant=1):
    """The units through the library's own front end in the estimate form `fmt` -> device subframes."""
    cfg, n = m.DlCfg(2048, 100, n_ant, m.IQ_I8 | fmt), len(lists)
    bufs = [ctx.to_device(iq.reshape(-1, 2)), ctx.to_device((np.arange(n) * iq.shape[1]).astype(np.uint64)),
            ctx.to_device(np.array([l[0] for l in lists], np.uint32)), ctx.to_device(np.array([l[1] for l in lists], np.uint32))]
    d_sub = ctx.alloc(n * ctx.subframe_floats(n_ant) * 4)
    ctx.dl_frontend_dev(cfg, bufs[0], None, bufs[1], bufs[2], bufs[3], n, d_sub)
    ctx.sync()
    for b in bufs:
        b.free()
    return cfg, d_sub


def _run(ctx, plan, d_sub, lists, packed):
    ctx.set_soft_packed(packed)
    st, bits = plan.run(d_sub, [l[0] for l in lists], [l[1] for l in lists])
    return st.copy(), [b.copy() for b in bits], [plan.soft_bits(a).copy() for a in range(sum(len(l[3]) for l in lists))]


def _same(x, y, what):
    assert (x[0] == y[0]).all(), (what, "status", x[0], y[0])
    for a in range(len(x[1])):
        assert x[1][a].shape == y[1][a].shape and (x[1][a] == y[1][a]).all(), (what, "bits of allocation", a)
        assert x[2][a].shape == y[2][a].shape and (x[2][a] == y[2][a]).all(), (what, "soft bits of allocation", a)


def _on_off(ctx, plan, d_sub, lists, what):
    """The plan with the packed hand-over and with bytes: identical.  Returns the packed run's results."""
    try:
        on = _run(ctx, plan, d_sub, lists, True)
        off = _run(ctx, plan, d_sub, lists, False)
        again = _run(ctx, plan, d_sub, lists, True)
    finally:
        ctx.set_soft_packed(True)
    _same(on, off, what)
    _same(again, off, what + " (second packed run)")
    for a, (mod, *_r) in enumerate(sum((l[3] for l in lists), [])):
        if mod >= 2:
            assert (np.abs(on[2][a]) == 127).all(), (what, a)
    return on


def _tap_ptr(ctx, plan, a):
    pe, pn = C.c_void_p(), C.c_void_p()
    ctx._check(ctx.L.mi_lte_pdsch_plan_soft_bits(plan.h, a, C.byref(pe), C.byref(pn)))
    return pe.value


def _raw(ctx, ptr, nbytes):
    out = np.empty(nbytes, np.uint8)
    ctx._check(ctx.L.mi_lte_memcpy_d2h(ctx.h, out.ctypes.data, ptr, nbytes))
    return out


def _case(ctx, lists, fmt, seed, snr_db=30.0, n_ant=1, ref_too=False):
    import openlte_amd as m
    from oracle import pyoracle as po
    iq = _iq(m, lists, seed, snr_db)
    ref = po.ref() if ref_too else None
    want = None
    if ref is not None:  # the reference's own grid and verdicts (single port, full estimate planes)
        import test_mixed_gpu as tm
        grids, want = tm._ref_decode_all(ref, po, lists, iq)
        cfg, d_sub = m.DlCfg(2048, 100, 1, m.IQ_I8), ctx.to_device(np.concatenate(grids))
    else:
        cfg, d_sub = _subframes(ctx, m, lists, iq, fmt, n_ant)
    plan = ctx.pdsch_plan(cfg, 2, _allocs(m, lists))
    on = _on_off(ctx, plan, d_sub, lists, "%s fmt %x" % (lists[0][3][0], fmt))
    if want is not None:
        for a, (rc, b) in enumerate(want):
            assert on[0][a] == rc and (on[1][a] == b).all(), ("against the reference", a, on[0][a], rc)
    return plan, d_sub, on


@pytest.mark.parametrize("fmt", ["full", "compact"])
def test_one_prb_allocations_next_to_qpsk(ctx, fmt):
    """16QAM and 64QAM on one PRB with CFI 1 and 3 (600 / 900 and 504 / 756 soft bits: no multiple of 32 or 16) and QPSK allocations in the
    same launch, from full estimate planes (the reference's grid where it is built) and from the compact form."""
    import openlte_amd as m
    plan, d_sub, on = _case(ctx, ONE_PRB, 0 if fmt == "full" else m.CE_COMPACT, 501, ref_too=fmt == "full")
    assert [len(s) for s in on[2]] == [600, 900, 900, 900, 504, 756, 756, 504], [len(s) for s in on[2]]
    plan.close()
    d_sub.free()


def test_w4_block_on_the_sync_subframes_and_the_slot_format(ctx):
    """W4's block across the PSS / SSS / PBCH window of subframes 0 and 5 (E just over one lap: the `halving` path), in a merged launch.  And
    the format itself: after a packed run the slot of a 64QAM allocation holds bit n of dword n / 32 = (soft bit n is -127), zeros from e_len to
    the end of the last dword; the tap then returns the bytes, twice the same, without touching the slot a second time."""
    import openlte_amd as m
    plan, d_sub, on = _case(ctx, W4_SYNC, m.CE_COMPACT, 502, ref_too=False)
    lens = [len(s) for s in on[2]]
    assert lens[0] < 9804 and lens[2] < 9804 and lens[3] == 9936, lens  # the window takes elements away (less than a lap is left); the last one is W4's
    assert on[0][3] == 0, on[0]
    ptrs = [_tap_ptr(ctx, plan, a) for a in range(4)]
    ctx.set_soft_packed(True)
    plan.run(d_sub, [l[0] for l in W4_SYNC], [l[1] for l in W4_SYNC])
    for a in range(4):
        n = lens[a]
        raw = _raw(ctx, ptrs[a], 4 * ((n + 31) // 32))
        want = np.packbits(np.concatenate([on[2][a] < 0, np.zeros(len(raw) * 8 - n, bool)]), bitorder="little")
        assert (raw == want).all(), ("packed slot of allocation", a)
    first = [plan.soft_bits(a).copy() for a in range(4)]
    second = [plan.soft_bits(a).copy() for a in range(4)]
    for a in range(4):
        assert (first[a] == on[2][a]).all() and (second[a] == on[2][a]).all(), a
        assert (_raw(ctx, ptrs[a], lens[a]).view(np.int8) == on[2][a]).all(), a
    plan.close()
    d_sub.free()


def test_w4_block_against_the_reference_on_a_sync_subframe(ctx):
    """The same units from the reference's received grid: status and bits are the reference's (skipped where the reference is not built)."""
    from oracle import pyoracle as po
    if po.ref() is None:
        pytest.skip("oracle/_ref not built")
    plan, d_sub, on = _case(ctx, W4_SYNC, 0, 502, ref_too=True)
    plan.close()
    d_sub.free()


def test_repetition_staged_lap_by_lap_in_a_merged_launch(ctx):
    """16QAM allocations of two laps at K = 352 and K = 232 in a merged launch (the lap-wise staging starts a lap at an arbitrary bit), also
    with the per-size launches, at an SNR where some blocks fail their CRC."""
    import openlte_amd as m
    ctx.set_turbo_small_batch(0)
    try:
        for snr, merged in ((30.0, True), (4.0, True), (30.0, False)):
            ctx.set_turbo_merged(merged)
            plan, d_sub, on = _case(ctx, REPEAT, m.CE_COMPACT, 503, snr_db=snr, ref_too=False)
            assert ("over all block sizes" in ctx.last_kernels()) == merged, ctx.last_kernels()
            assert len(on[2][0]) > 1.25 * 3 * 356 and (snr < 10 or (on[0][:2] == 0).all()), (snr, on[0], len(on[2][0]))  # (the two repeated ones)
            plan.close()
            d_sub.free()
    finally:
        ctx.set_turbo_small_batch(4096)
        ctx.set_turbo_merged(True)


def test_repetition_against_the_reference(ctx):
    from oracle import pyoracle as po
    if po.ref() is None:
        pytest.skip("oracle/_ref not built")
    plan, d_sub, on = _case(ctx, REPEAT, 0, 503, ref_too=True)
    plan.close()
    d_sub.free()


@pytest.mark.parametrize("merged", [True, False])
def test_long_allocation(ctx, merged):
    """64QAM on 50 PRB, one code block, more than 32 768 soft bits next to a QPSK allocation: as bytes it went straight to global memory in
    the demodulator and is staged lap by lap (merged) or not at all (per size) in prep; packed it goes through LDS in both."""
    import openlte_amd as m
    ctx.set_turbo_small_batch(0)
    ctx.set_turbo_merged(merged)
    try:
        plan, d_sub, on = _case(ctx, LONG, m.CE_COMPACT, 504)
        assert len(on[2][0]) > 32768 and on[0][0] == 0, (len(on[2][0]), on[0])
        plan.close()
        d_sub.free()
    finally:
        ctx.set_turbo_small_batch(4096)
        ctx.set_turbo_merged(True)


def test_two_port_plan(ctx):
    """k_pdsch_demod<false>: the transmit-diversity combiner on a single-port capture -- garbage in, the same garbage out either way."""
    import openlte_amd as m
    plan, d_sub, on = _case(ctx, ONE_PRB[:1] + W4_SYNC[:1], 0, 505, n_ant=2)
    plan.close()
    d_sub.free()


def test_run_with_a_group_gathered_from_global_memory_keeps_bytes(ctx):
    """K = 40 behind 13 PRB of 64QAM (more than 258 laps: the per-size kernel with 32-bit sums, staged whole): packed like any other.  Behind 60
    PRB the allocation is too long to stage and prep's gather from global memory reads bytes, so the host packs nothing in such a run -- the
    slots hold bytes right after it -- and everything decodes as with the switch off."""
    import openlte_amd as m
    for lists, packed in ((MANY_LAPS, True), (MANY_LAPS_GLOBAL, False)):
        plan, d_sub, on = _case(ctx, lists, m.CE_COMPACT, 506)
        ptr = _tap_ptr(ctx, plan, 1)
        ctx.set_soft_packed(True)
        plan.run(d_sub, [lists[0][0]], [lists[0][1]])
        n = len(on[2][1])
        assert ((_raw(ctx, ptr, n).view(np.int8) == on[2][1]).all()) == (not packed), packed
        if packed:
            assert (_raw(ctx, ptr, n // 8) == np.packbits(on[2][1] < 0, bitorder="little")[:n // 8]).all()
        plan.close()
        d_sub.free()


def test_dynamic_plan_reassigned_between_formats(ctx):
    """A dynamic plan from a 64QAM list to a QPSK list and back: every assignment decodes identically packed and in bytes, and the first
    list's results return."""
    import openlte_amd as m
    plan, res = ctx.pdsch_plan_dynamic(m.DlCfg(2048, 100, 1, m.IQ_I8 | m.CE_COMPACT), 16, 16 * 12 * 13 * 12 * 6), []
    for rnd, lists in enumerate((W4_SYNC, QPSK_ONLY, W4_SYNC)):
        cfg, d_sub = _subframes(ctx, m, lists, _iq(m, lists, 507, 30.0), m.CE_COMPACT)
        plan.assign(2, _allocs(m, lists))
        res.append(_on_off(ctx, plan, d_sub, lists, "assignment %d" % rnd))
        d_sub.free()
    _same(res[0], res[2], "first and third assignment")
    plan.close()


def test_tap_and_decoder_change(ctx):
    """soft_bits twice after one run: identical; a second run decodes identically; and the BCJR decoder on the same plan -- which takes bytes --
    gives what it gives with the switch off, its soft bits included."""
    import openlte_amd as m
    plan, d_sub, on = _case(ctx, W4_SYNC, 0, 508)
    sfs, cells = [l[0] for l in W4_SYNC], [l[1] for l in W4_SYNC]
    twice = [plan.soft_bits(a) for a in range(4)]
    assert all((twice[a] == on[2][a]).all() for a in range(4))
    try:
        plan.set_decoder(m.TURBO_BCJR, 8)
        b_on = _run(ctx, plan, d_sub, W4_SYNC, True)
        b_off = _run(ctx, plan, d_sub, W4_SYNC, False)
        _same(b_on, b_off, "BCJR")
        assert all((b_on[2][a] == on[2][a]).all() for a in range(4))
        plan.set_decoder(m.TURBO_REF)
        _same(_run(ctx, plan, d_sub, W4_SYNC, True), on, "REF again")
    finally:
        ctx.set_soft_packed(True)
    plan.close()
    d_sub.free()
