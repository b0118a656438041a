"""GPU parity of the sign-bit hand-over between the trellis kernels and k_turbo_perm / k_turbo_vote: the trellis kernels write one sign bit
per step (8 bytes per 64-step block and trellis), perm and vote join it with the magnitudes k_turbo_prep / k_turbo_perm computed.
ctx.turbo_decode against the oracle, bit for bit, at the shapes where that format can go wrong --

  block sizes   40 (one partial block), 64 and 72 (a block boundary; a last block of 8 steps, whose first unit takes its halo signs from
                the block before), 104 (K % 16 == 8), 528, 1088, 3264, 6144
  block counts  1, 65 and 130: two and three tiles, so the first pass (two tiles per lane) takes its last tile twice
  kernels       the lock-step and the state-parallel trellis kernel
  inputs        test_turbo_glue_gpu's kinds: sparse (magnitude 0 under a negative path sign), zero127, noise

and three of the sizes in one merged decode (a PDSCH plan) against the oracle's lo_pdsch_channel_decode."""
import ctypes as C
import functools

import numpy as np
import pytest

import lte_testdata as td
from test_turbo_glue_gpu import KINDS, glue_blocks

pytestmark = pytest.mark.gpu

KS = [40, 64, 72, 104, 528, 1088, 3264, 6144]
NS = [1, 65, 130]


@functools.lru_cache(maxsize=None)
def case(K, kind):
    """130 blocks (two draws of that file's 66) and the oracle's decisions, computed once and shared by the block counts and the kernels."""
    from oracle import pyoracle
    port = pyoracle.port()
    soft = np.concatenate([glue_blocks(K, kind, seed=977 * K + 2 * KINDS.index(kind) + i) for i in range(2)])[:max(NS)]
    want = np.concatenate(td.parallel_map(lambda b: td.oracle_turbo_ref(port, soft[b:b + 1], K), range(soft.shape[0])))
    soft.setflags(write=False)
    want.setflags(write=False)
    return soft, want


@pytest.fixture(params=[0, 4096], ids=["lockstep", "state-parallel"])
def siso(ctx, request):
    ctx.set_turbo_small_batch(request.param)
    yield request.param
    ctx.set_turbo_small_batch(4096)


@pytest.mark.parametrize("n", NS)
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("K", KS)
def test_turbo_sign_bits_bit_exact(ctx, siso, K, kind, n):
    soft, want = case(K, kind)
    got = ctx.turbo_decode(np.ascontiguousarray(soft[:n]), K)
    assert got.shape == (n, K)
    bad = np.nonzero((got != want[:n]).any(axis=1))[0]
    assert bad.size == 0, "blocks differing from the oracle: %s" % bad[:10]


def test_three_sizes_in_one_merged_decode(ctx, port, siso):
    """K = 528, 1088 and 3264 (TBS 504, 1064, 3240; 64QAM) in the allocations of two subframes through one PDSCH plan: one launch set over the
    three sizes' tiles, each size at its own offset of the byte, traceback and sign arrays.  Status and transport blocks against
    lo_pdsch_channel_decode, both fed the oracle's front end; the second subframe is noisy enough for both CRC verdicts to occur."""
    import openlte_amd as m
    from openlte_amd import synth
    cfg = m.DlCfg(2048, 100, 1, 0)
    sfs, cells = [3, 8], [42, 301]

    def unit_allocs(u):
        return [m.make_alloc(u, 3, 3240, list(range(0, 12)), 0x100), m.make_alloc(u, 3, 1064, list(range(12, 16)), 0x101),
                m.make_alloc(u, 3, 504, list(range(16, 19)), 0x102), m.make_alloc(u, 3, 3240, list(range(19, 31)), 0x103)]
    allocs = unit_allocs(0) + unit_allocs(1)
    n_a = len(unit_allocs(0))
    iq = np.concatenate([synth.dl_units(cfg, [sfs[u]], [cells[u]], unit_allocs(0), n_a, snr_db=snr, max_delay=4, seed=11 + u)[0] for u, snr in ((0, 30), (1, 19))])
    front = [td.oracle_frontend(port, 2048, 100, 1, iq[u], sfs[u], cells[u]) for u in range(2)]
    d_sub = ctx.to_device(np.concatenate([np.concatenate([s.arr("rx_symb_re").ravel(), s.arr("rx_symb_im").ravel(), s.arr("rx_ce_re")[:1].ravel(),
                                                          s.arr("rx_ce_im")[:1].ravel()]).astype(np.float32) for _, s in front]))
    plan = ctx.pdsch_plan(cfg, 2, allocs)
    st, bits = plan.run(d_sub, sfs, cells)
    assert "over all block sizes" in ctx.last_kernels(), ctx.last_kernels()  # the merged launches ran
    n_ok = 0
    for u in range(2):
        lc, s = front[u]
        for a in range(n_a):
            k = n_a * u + a
            out, n = np.zeros(6200, np.uint8), C.c_uint32()
            la = td.to_lo_alloc(allocs[k])
            err = port.lo_pdsch_channel_decode(C.byref(lc), C.byref(s), C.byref(la), 2, cells[u], 1, out, C.byref(n), None, None)
            assert st[k] == err, (k, st[k], err)
            if err == 0:  # (the oracle keeps the bits of a block that fails its CRC to itself)
                assert (out[:n.value] == bits[k]).all(), "allocation %d differs from the oracle" % k
                n_ok += 1
    assert n_ok >= n_a, (n_ok, list(st))  # the clean subframe decodes
    plan.close()
    d_sub.free()
