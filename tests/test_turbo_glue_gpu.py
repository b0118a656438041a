"""GPU parity of the turbo decoder's glue kernels (k_turbo_perm, k_turbo_vote) and of the sign-magnitude bytes the trellis kernels hand
them: ctx.turbo_decode against the oracle, bit for bit, on inputs that stress the byte-parallel soft re-encoder (turbo_swar.h) --

  sparse   mostly 0, some +-1 / +-2 (one +-127 per block keeps the scaling at 1): many trellis outputs have magnitude 0 on a path step
           of negative sign, the "-0" that sign-magnitude bytes must not leak into the next sign test;
  zero127  +-127 with random signs, one of the three streams 95 % zero;
  noise    full-range random int8.

None of them is a code word.  Block sizes: the smallest, one whose last 16-step unit holds eight steps (K % 16 == 8), the two W4 sizes
and the largest; 1 and 66 code blocks; both trellis kernels.  Then two W4 subframes through a PDSCH plan (the merged launches, CRC
verdict, status, both output forms) against the oracle's lo_pdsch_channel_decode."""
import ctypes as C
import functools

import numpy as np
import pytest

import lte_testdata as td

pytestmark = pytest.mark.gpu

KS = [40, 104, 1088, 3264, 6144]
KINDS = ["sparse", "zero127", "noise"]
N_BLOCKS = 66


def glue_blocks(K, kind, seed):
    """[N_BLOCKS, 3 (K + 4)] int8 soft values in the reference's interleaved layout (d0, d1, d2 per step)."""
    rng = np.random.default_rng(seed)
    D = K + 4
    if kind == "sparse":
        y = rng.choice(np.array([0, 1, -1, 2, -2], np.int8), (N_BLOCKS, D, 3), p=[0.6, 0.12, 0.12, 0.08, 0.08])
        for b in range(N_BLOCKS):  # the block's maximum: the reference scales by 127 / max, so the other values stay what they are
            y[b, rng.integers(0, K), 0] = 127 if b & 1 else -127
        assert ((y[:, :K, 0] == 0) & (y[:, :K, 1] == 0)).mean() > 0.3  # the first pass's outputs of magnitude 0, whatever their path's sign
    elif kind == "zero127":
        y = (127 * (1 - 2 * rng.integers(0, 2, (N_BLOCKS, D, 3)))).astype(np.int8)
        for b in range(N_BLOCKS):
            keep = y[b, rng.integers(0, K), b % 3]
            y[b, rng.random(D) < 0.95, b % 3] = 0
            y[b, rng.integers(0, K), b % 3] = keep  # (never all of it)
    elif kind == "noise":
        y = rng.integers(-127, 128, (N_BLOCKS, D, 3)).astype(np.int8)
    else:
        raise ValueError(kind)
    # the reference divides by the largest branch weight of each trellis pass, max |q(d1)| + |q(d0)|, max |q(d2)| + |q(d0)[pi]| and
    # max |q(d2)| + |I1|: a stream pair that is all zero would be a division by zero there.  A non-zero value in d0 and in d2 (inside
    # the K steps that count) keeps all three away from it.
    assert (np.abs(y[:, :K, 0]).max(axis=1) > 0).all() and (np.abs(y[:, :K, 2]).max(axis=1) > 0).all()
    return np.ascontiguousarray(y.reshape(N_BLOCKS, 3 * D))


@functools.lru_cache(maxsize=None)
def case(K, kind):
    """The input and the oracle's decisions, computed once and shared by the batch sizes and the two trellis kernels."""
    from oracle import pyoracle
    port = pyoracle.port()
    soft = glue_blocks(K, kind, seed=31 * K + KINDS.index(kind))
    want = np.concatenate(td.parallel_map(lambda b: td.oracle_turbo_ref(port, soft[b:b + 1], K), range(N_BLOCKS)))
    soft.setflags(write=False)
    want.setflags(write=False)
    return soft, want


@pytest.fixture(params=[0, 4096], ids=["lockstep", "state-parallel"])
def siso(ctx, request):
    ctx.set_turbo_small_batch(request.param)
    yield request.param
    ctx.set_turbo_small_batch(4096)


@pytest.mark.parametrize("n", [1, N_BLOCKS])
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("K", KS)
def test_turbo_glue_bit_exact(ctx, siso, K, kind, n):
    soft, want = case(K, kind)
    got = ctx.turbo_decode(np.ascontiguousarray(soft[:n]), K)
    assert got.shape == (n, K)
    bad = np.nonzero((got != want[:n]).any(axis=1))[0]
    assert bad.size == 0, "blocks differing from the oracle: %s" % bad[:10]


@pytest.mark.parametrize("packed", [False, True], ids=["bytes", "packed"])
def test_w4_plan_two_subframes_against_the_oracle(ctx, port, siso, packed):
    """Two 20 MHz subframes with W4's nine 64QAM allocations each through a PDSCH plan: the merged launches of perm and vote, vote's CRC
    verdict, the status words and the transport blocks in both output forms, against lo_pdsch_channel_decode, both fed the oracle's
    front end.  The second subframe is noisy enough for hard-decision 64QAM to fail, so both verdicts occur."""
    import openlte_amd as m
    from openlte_amd import synth
    cfg = m.DlCfg(2048, 100, 1, 0)
    sfs, cells = [3, 8], [42, 301]
    allocs = td.w4_allocs(0) + td.w4_allocs(1)
    iq = np.concatenate([synth.dl_units(cfg, [sfs[u]], [cells[u]], td.w4_allocs(0), 9, snr_db=snr, max_delay=4, seed=7 + u)[0] for u, snr in ((0, 30), (1, 19))])
    # the oracle's own received grid and channel estimate go to the device, so both sides demodulate the same numbers (test_chain_gpu.py)
    front = [td.oracle_frontend(port, 2048, 100, 1, iq[u], sfs[u], cells[u]) for u in range(2)]
    d_sub = ctx.to_device(np.concatenate([np.concatenate([s.arr("rx_symb_re").ravel(), s.arr("rx_symb_im").ravel(), s.arr("rx_ce_re")[:1].ravel(),
                                                          s.arr("rx_ce_im")[:1].ravel()]).astype(np.float32) for _, s in front]))
    plan = ctx.pdsch_plan(cfg, 2, allocs)
    if packed:
        plan.set_packed(True)
    st, bits = plan.run(d_sub, sfs, cells)
    verdicts = set()
    for u in range(2):
        lc, s = front[u]
        for a in range(9):
            k = 9 * u + a
            out, n = np.zeros(6200, np.uint8), C.c_uint32()
            la = td.to_lo_alloc(allocs[k])
            err = port.lo_pdsch_channel_decode(C.byref(lc), C.byref(s), C.byref(la), 2, cells[u], 1, out, C.byref(n), None, None)
            assert st[k] == err, (k, st[k], err)
            if err == 0:  # (the oracle keeps the bits of a block that fails its CRC to itself)
                assert (out[:n.value] == bits[k]).all(), "allocation %d differs from the oracle" % k
            verdicts.add(int(err))
    assert verdicts == {0, 2}, verdicts
    plan.close()
    d_sub.free()
