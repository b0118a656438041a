"""The trellis kernels' sign words, laid out per code block and by plane (turbo_swar.h, "the trellis kernels' sign words"): the REF decode
through Context.turbo_decode against the plain-C oracle's lo_turbo_decode_ref on the same float inputs, every bit of every block (failing
blocks too: there is no CRC in this path), at the smallest sizes that reach a distinct case of the addressing:

    K 40    one partial word, a last unit of 8 steps
    K 64    exactly one 64-step block
    K 72    unit 4: a halo out of the block before, an 8-step tail
    K 104   K % 16 == 8 inside the second block's second word
    K 136   a third block
    K 6144  384 units, the widest workgroup, 192 words per lane

with 130 code blocks (three tiles: an odd count, so pass 1 walks the last tile twice, and a last tile with two live lanes) and with one,
through the lock-step trellis kernel and the state-parallel one, merged and per-size launches, on hard inputs with 2 % flips (the
benchmark's kind) and on sigma = 1 AWGN inputs (many wrong and many zero-magnitude outputs: signs under magnitude 0).  One more case hands
sizes 40, 72 and 6144 to ONE merged decode through a PDSCH plan of three allocations."""
import ctypes as C

import numpy as np
import pytest

import lte_testdata as td

pytestmark = pytest.mark.gpu

SIZES = (40, 64, 72, 104, 136, 6144)
COUNTS = (130, 1)
_cache = {}


def _case(port, K, kind):
    """(float inputs [130, 3 (K + 4)], the oracle's bits [130, K]) of one size and input kind, computed once; the one-block case is its first row."""
    if (K, kind) not in _cache:
        from openlte_amd import synth
        if kind == "flip":
            _, soft = synth.turbo_soft_blocks(K, max(COUNTS), flip=0.02, seed=1000 + K)
        else:
            _, soft = synth.turbo_soft_blocks_awgn(K, max(COUNTS), sigma=1.0, seed=2000 + K)
        soft = np.ascontiguousarray(soft, dtype=np.float32)
        rows = td.parallel_map(lambda b: td.oracle_turbo_ref(port, soft[b:b + 1], K)[0], range(soft.shape[0]))
        want = np.stack(rows)
        soft.setflags(write=False)
        want.setflags(write=False)
        _cache[(K, kind)] = (soft, want)
    return _cache[(K, kind)]


@pytest.mark.parametrize("kind", ("flip", "awgn"))
@pytest.mark.parametrize("K", SIZES)
def test_ref_decode_equals_the_oracle_bit_for_bit(ctx, port, K, kind):
    soft, want = _case(port, K, kind)
    try:
        for n in COUNTS:
            for small, kernel in ((0, "k_turbo_siso"), (4096, "k_turbo_siso_small")):
                for merged in (True, False):
                    ctx.set_turbo_small_batch(small)
                    ctx.set_turbo_merged(merged)
                    got = ctx.turbo_decode(soft[:n], K)
                    bad = np.nonzero((got != want[:n]).any(axis=1))[0]
                    assert bad.size == 0, "K %d, %d blocks, %s, %s launches, %s inputs: %d blocks differ from the oracle, first %d at bits %s" % (
                        K, n, kernel, "merged" if merged else "per-size", kind, bad.size, bad[0], np.nonzero(got[bad[0]] != want[bad[0]])[0][:8])
    finally:
        ctx.set_turbo_small_batch(4096)
        ctx.set_turbo_merged(True)


def _oracle_allocation(port, lc, s, alloc, cell):
    """The oracle's verdict and the decoder's K hard bits of one allocation, whatever its CRC says: lo_pdsch_channel_decode gives the verdict
    and its demodulated soft bits, lo_dlsch_channel_decode on those (descrambled) the bits the decoder left."""
    out, n = np.zeros(6200, np.uint8), C.c_uint32()
    soft, ns = np.zeros(6 * 168 * alloc.N_prb + 64, np.int8), C.c_uint32()
    la = td.to_lo_alloc(alloc)
    err = port.lo_pdsch_channel_decode(C.byref(lc), C.byref(s), C.byref(la), 2, cell, 1, out, C.byref(n), soft.ctypes.data_as(C.c_void_p), C.byref(ns))
    c = np.zeros(ns.value, np.uint8)
    port.lo_prs_c((alloc.rnti << 14) | (s.num << 9) | cell, ns.value, c)
    desc = np.ascontiguousarray(soft[:ns.value].astype(np.float32) * (1 - 2 * c.astype(np.float32)))
    tap, out2, n2 = np.zeros(alloc.tbs + 24, np.uint8), np.zeros(6200, np.uint8), C.c_uint32()
    err2 = port.lo_dlsch_channel_decode(desc, ns.value, alloc.tbs, alloc.tx_mode, alloc.rv_idx, 8, 250368, out2, C.byref(n2), tap.ctypes.data_as(C.c_void_p))
    assert (err == 0) == (err2 == 0) and (err != 0 or (out[:n.value] == tap[:alloc.tbs]).all())
    return err, tap[:alloc.tbs].copy()


def test_sizes_40_72_6144_in_one_merged_decode(ctx, port):
    """One subframe with three allocations whose code blocks are K = 6144 (tbs 6120, 64QAM on 12 PRB: a code rate the decoder fails at, so
    its bits are those of a failing block), K = 40 (tbs 16) and K = 72 (tbs 48), from the oracle's front end: one merged decode over the three
    sizes through either trellis kernel, and the per-size launches.  Verdict and every bit of every allocation are the oracle's."""
    import openlte_amd as m
    from openlte_amd import synth
    cfg = m.DlCfg(2048, 100, 1, 0)
    sf, cell = 3, 42
    allocs = [m.make_alloc(0, 3, 6120, list(range(0, 12)), 0x100), m.make_alloc(0, 1, 16, [12], 0x101), m.make_alloc(0, 1, 48, [13], 0x102)]
    iq, tx = synth.dl_units(cfg, [sf], [cell], allocs, len(allocs), snr_db=30, max_delay=4, seed=11)
    lc, s = td.oracle_frontend(port, 2048, 100, 1, iq[0], sf, cell)
    want = [_oracle_allocation(port, lc, s, al, cell) for al in allocs]
    assert [w[0] for w in want[1:]] == [0, 0] and all((want[a][1] == tx[0, a, :allocs[a].tbs]).all() for a in (1, 2)), "the two short blocks are meant to decode"
    d_sub = ctx.to_device(np.concatenate([s.arr("rx_symb_re").ravel(), s.arr("rx_symb_im").ravel(), s.arr("rx_ce_re")[:1].ravel(),
                                          s.arr("rx_ce_im")[:1].ravel()]).astype(np.float32))
    plan = ctx.pdsch_plan(cfg, 2, allocs)
    try:
        for small, merged in ((0, True), (4096, True), (4096, False)):
            ctx.set_turbo_small_batch(small)
            ctx.set_turbo_merged(merged)
            st, bits = plan.run(d_sub, [sf], [cell])
            assert ("over all block sizes" in ctx.last_kernels()) == merged, (small, merged, ctx.last_kernels())
            for a, (err, b) in enumerate(want):
                assert st[a] == err and len(bits[a]) == len(b) and (bits[a] == b).all(), (small, merged, a, st[a], err)
    finally:
        ctx.set_turbo_small_batch(4096)
        ctx.set_turbo_merged(True)
        plan.close()
        d_sub.free()
